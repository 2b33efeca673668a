"""GPU: BASELINE.json configs at their REAL per-GPU sizes (VERDICT r01 "untested configs") and the one-call replay step
against the oracle.

  configs[2]  20-link DQN loop (simulator rollouts + replay) at batch 4096           -> test_cfg2_*
  configs[3]  100 links x 256 features x 3 layers, 8192 / 8 = 1024 graphs per GPU    -> test_cfg3_*
  configs[4]  8-128 links per graph (CSR offsets), 16384 / 8 = 2048 graphs per GPU   -> test_cfg4_*

Element-wise oracle parity at these sizes lives in test_gpu_fullsize.py (test_cfg3_share_vs_oracle,
test_cfg4_share_vs_oracle); here are the size-independent properties of the path at the same sizes: the loss is the Huber
mean of the engine's own forward output, the gradient is additive over shards taken with the global denominator (what the
data-parallel all-reduce relies on), hipGraph replay == eager.
"""
import contextlib
import os
import random

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine
from util import GOLDEN, ospec, f32_params, assert_close, assert_fwd_close, assert_grad_close
from oracle import compact as oc

pytestmark = pytest.mark.gpu


def _huber_mean(q, y, axis=None):
    ab = np.abs(q.astype(np.float64) - y)
    quad = np.minimum(ab, 1.0)
    return (0.5 * quad * quad + (ab - quad)).mean(axis=axis)


def _weights(spec, rng):
    return [rng.normal(0, 0.05, size=s).astype(np.float32) if len(s) == 1 else
            rng.uniform(-np.sqrt(6.0 / sum(s)), np.sqrt(6.0 / sum(s)), size=s).astype(np.float32)
            for s in v2xgnn.keras_list_shapes(spec)]


# ------------------------------------------------------------------------------------------------ v2x_dqn_step vs oracle
def _oracle_dqn_step(spec, w_online, w_target, x, e, adj, x2, e2, action, reward, gamma, nbr=None, nbr2=None):
    """Agent.replay (BS_brain.py:664-728) in float64: target forward on s', online forward on s, the target rule
    (:684-692), one fit step.  -> (y, per-output losses, weights after the step)
    nbr / nbr2 [B, N, F]: the Neighbor_Input of s / of s' (None: the reference's zeros)"""
    os_ = ospec(spec)
    B, N = x.shape[0], spec.n_nodes
    graph = oc.adj_to_csr(adj)
    online = oc.OracleModel(os_, oc.params_from_list(os_, w_online), dtype=np.float64)
    target = oc.OracleModel(os_, oc.params_from_list(os_, w_target), dtype=np.float64)
    flat = lambda a: a.reshape(B * N, -1).astype(np.float64)
    n1, n2 = (None if n is None else flat(n) for n in (nbr, nbr2))
    q = online.predict(flat(x), flat(e), graph, n1).reshape(B, N, -1)
    qn = target.predict(flat(x2), flat(e2), graph, n2).reshape(B, N, -1)           # same adjacency (:583)
    y = q.copy()
    tgt = reward[:, None] + gamma * qn.max(axis=2)
    y[np.arange(B)[:, None], np.arange(N)[None, :], action] = tgt
    _, g_ref, _ = online.loss_and_grads(flat(x), flat(e), graph, y.reshape(B * N, -1), n1)
    loss = online.train_step(flat(x), flat(e), graph, y.reshape(B * N, -1), n1)
    return y, loss, oc.params_to_list(online.params), oc.params_to_list(g_ref)


def _run_dqn_step(spec, w_online, w_target, x, e, adj, x2, e2, action, reward, gamma, nbr=None, nbr2=None, use_graph=False):
    import torch
    online, target = GnnEngine(spec, use_graph=use_graph), GnnEngine(spec, use_graph=use_graph)
    online.set_weights(w_online)
    target.set_weights(w_target)
    sb = online.to_device(PackedBatch.from_dense(x, e, adj, nbr))
    sn = online.to_device(PackedBatch.from_dense(x2, e2, adj, nbr2))
    B, N = x.shape[0], spec.n_nodes
    y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
    a_dev = torch.from_numpy(np.ascontiguousarray(action, np.int32)).cuda()
    r_dev = torch.from_numpy(np.ascontiguousarray(reward, np.float64)).cuda()
    with torch.cuda.stream(torch.cuda.Stream()) if use_graph else contextlib.nullcontext():    # (a capture needs a non-default stream)
        loss = online.dqn_step(target, sb, sn, a_dev, r_dev, gamma, y_out=y)
        if use_graph:
            torch.cuda.synchronize()
    out = y.cpu().numpy().reshape(B, N, 4), loss.cpu().numpy(), online.get_weights()
    online.close()
    target.close()
    return out


def _check_dqn_step(spec, w_online, w_target, x, e, adj, x2, e2, action, reward, gamma, nbr=None, nbr2=None):
    y, loss, w1 = _run_dqn_step(spec, w_online, w_target, x, e, adj, x2, e2, action, reward, gamma, nbr, nbr2)
    y_ref, loss_ref, w_ref, g_ref = _oracle_dqn_step(spec, w_online, w_target, x, e, adj, x2, e2, action, reward, gamma, nbr, nbr2)
    assert_fwd_close(y, y_ref, "training targets of the fused replay step")
    assert_close(loss, loss_ref, 5e-3, 1e-6, "per-output Huber losses")
    moved = 0
    for i, (a, b, c, g) in enumerate(zip(w1, w_ref, w_online, g_ref)):
        # Adam's first step is sign-like (m / sqrt(v) = +-1): where |g| is at rounding-noise level its direction is not
        # determined by fp32 arithmetic -- those entries are compared to within one full step (test_train_steps_vs_oracle)
        scale = np.abs(g).max() or 1.0
        tight = np.abs(g) > 1e-4 * scale
        err = np.abs(a.astype(np.float64) - b)
        assert (err[tight] <= 2e-5 + 2e-4 * np.abs(b[tight])).all(), ("weights", i, err[tight].max())
        assert (err[~tight] <= 1.1e-3).all(), ("weights (ill-conditioned)", i, err[~tight].max())
        moved += int(np.any(a != c))
    assert moved > len(w1) // 2
    return y, loss, w1


def test_dqn_step_vs_oracle_on_the_reference_agents_replay_memory():
    """s, a, r, s' = the 24 transitions the REFERENCE agent stored (golden_agent_n4.npz: reference Agent on the reference
    simulator, seed 1001)."""
    g = np.load(os.path.join(GOLDEN, "golden_agent_n4.npz"))
    n = 4
    s, s2 = g["mem_states"], g["mem_states_next"]
    B = s.shape[0]
    st, st2 = s[:, :n * 13].reshape(B, n, 13), s2[:, :n * 13].reshape(B, n, 13)
    adj = s[:, n * 13:].reshape(B, n, n)
    spec = GnnSpec(n_nodes=n, feat_dim=16)
    rng = np.random.default_rng(5)
    _check_dqn_step(spec, _weights(spec, rng), _weights(spec, rng), st[:, :, :9].astype(np.float32), st[:, :, 9:].astype(np.float32),
                    adj, st2[:, :, :9].astype(np.float32), st2[:, :, 9:].astype(np.float32), g["mem_actions"].astype(int),
                    g["mem_rewards"].astype(np.float64), float(g["gamma"]))


def test_dqn_step_vs_oracle_twenty_links():
    from util import random_inputs
    N, F, B = 20, 64, 40
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(6)
    x, e, adj = random_inputs(rng, B, N)
    x2, e2, _ = random_inputs(rng, B, N)
    _check_dqn_step(spec, _weights(spec, rng), _weights(spec, rng), x, e, adj, x2, e2, rng.integers(0, 4, size=(B, N)),
                    rng.normal(2.4, 0.3, size=B), 0.5)


# ------------------------------------------------------------------------------------------------ configs[2]
def _agent(seed, batch, device_replay):
    from v2xgnn.rl import Agent, RL_Config
    from test_rl_env import make_env
    random.seed(seed)
    np.random.seed(seed)
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, batch, 1, 0.1)
    env = make_env()
    env.new_random_game(20)
    return Agent(20, env.n_RB, env.n_Neighbor, 64, env, cfg, seed=seed, device_replay=device_replay)


def test_cfg2_dqn_loop_at_batch_4096():
    """BASELINE configs[2] at its real size: 20 links, 64 features, replay minibatch 4096, the HBM-resident replay
    memory; 10 train steps = 500 simulator steps, so the target network syncs once (BS_brain.py:846-847).  The first two
    steps are compared with the host-replay path (the reference's payload construction) on the same seed."""
    dev = _agent(31, 4096, True)
    loss, reward_step, reward_ep, q_mean, q_max, _, _ = dev.train(1, 10)
    assert loss.shape == (20, 1, 10) and np.all(np.isfinite(loss)) and np.all(loss >= 0)
    assert np.all(np.isfinite(reward_step)) and np.all(q_max >= q_mean - 1e-9)
    assert dev.num_step == 500 and len(dev.device_replay) == 500
    for a, b in zip(dev.brain.model.get_weights(), dev.brain.target_model.get_weights()):
        assert np.array_equal(a, b)                               # num_step % 500 == 0 after the 10th step
    host = _agent(31, 4096, False)
    host.num_Episodes, host.num_Train_Step, host.num_step = 1, 10, 0     # the same epsilon schedule as train(1, 10)
    host.env.new_random_game(host.num_D2D)                               # what train() does at the start of an episode
    for it in range(2):
        host.generate_d2d_transition(50)
        result, qm, qx, _, _ = host.replay()
        lh = np.array([result.history['D%d_Decide_Output_loss' % (k + 1)][0] for k in range(20)])
        assert np.allclose(lh, loss[:, 0, it], rtol=2e-3, atol=1e-6), it
        assert np.allclose(qm, q_mean[:, 0, it], rtol=1e-4, atol=1e-5) and np.allclose(qx, q_max[:, 0, it], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ configs[3], configs[4]
def _properties(spec, pb, y, n_global, rows_of_shard, per_output_axes, what):
    import torch
    rng = np.random.default_rng(77)
    w = _weights(spec, rng)
    eng = GnnEngine(spec)
    eng.set_weights(w)
    q = eng.forward(pb)
    assert np.all(np.isfinite(q))
    loss = eng.forward_backward(pb, y, n_global=n_global)
    assert_close(loss, per_output_axes(q, y), 5e-5, 1e-7, what + ": loss is the Huber mean of the forward output")
    g_full = eng.get_grad_flat().astype(np.float64)
    assert np.all(np.isfinite(g_full)) and np.abs(g_full).max() > 0
    acc = np.zeros_like(g_full)
    for r in range(2):
        sh, (r0, r1) = rows_of_shard(r)
        eng.forward_backward(sh, y[r0:r1], n_global=n_global)
        acc += eng.get_grad_flat()
    assert_grad_close(acc, g_full, what + ": sum of the two shards' gradients")
    # hipGraph replay == eager, bitwise, over three optimizer steps
    outs = []
    for use_graph in (False, True):
        e2 = GnnEngine(spec, use_graph=use_graph)
        e2.set_weights(w)
        with torch.cuda.stream(torch.cuda.Stream()):
            db = e2.to_device(pb)
            yd = torch.from_numpy(y).cuda()
            for _ in range(3):
                ls = e2.train_step(db, yd, n_global=n_global)
            torch.cuda.synchronize()
        outs.append((ls.cpu().numpy(), e2.get_flat()))
        e2.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.all(np.isfinite(outs[0][1]))
    eng.close()


def test_cfg3_hundred_links_256_features_3_layers_per_gpu_share():
    import bench
    N, F, L, B = 100, 256, 3, 1024
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    x, e, adj, y = bench.synth_batch(np.random.default_rng(41), B, N)
    pb = PackedBatch.from_dense(x, e, adj)
    assert pb.max_edges == N * (N - 2)
    _properties(spec, pb, y, B, lambda r: pb.shard(r, 2, with_rows=True),
                lambda q, yy: _huber_mean(q.reshape(B, N, 4), yy.reshape(B, N, 4), axis=(0, 2)), "configs[3]")


def test_cfg4_ragged_8_to_128_links_per_gpu_share():
    import bench
    B = 2048
    sizes, offs, row_ptr, col_idx, x, e, y = bench.synth_ragged(np.random.default_rng(42), B, 8, 128)
    spec = GnnSpec(n_nodes=1, feat_dim=64, share_weights=True, variable_graphs=True)
    pb = PackedBatch(B, 0, v2xgnn.pack_xe(x, e), row_ptr, col_idx, graph_off=offs)
    assert pb.max_nodes == sizes.max() and pb.n_rows == sizes.sum()
    shards = [pb.shard(r, 2, with_rows=True) for r in range(2)]
    cost = [s.n_rows + s.n_edges for s, _ in shards]
    assert abs(cost[0] - cost[1]) <= 128 * 127                   # balanced by edges + nodes to within one largest graph
    _properties(spec, pb, y, pb.n_rows, lambda r: shards[r], lambda q, yy: np.array([_huber_mean(q, yy)]), "configs[4]")


def test_dqn_step_hipgraph_replay_is_bitwise_eager():
    """The one-call replay step captured as a hipGraph (stable gather buffers, as rl/replay.py provides them): new
    contents in the same buffers, a target-network sync in between, three steps -- identical to eager launches."""
    import torch
    from util import random_inputs
    N, F, B = 20, 64, 64
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(8)
    w_on, w_tg = _weights(spec, rng), _weights(spec, rng)
    data = []
    for _ in range(3):
        x, e, adj = random_inputs(rng, B, N)
        x2, e2, _ = random_inputs(rng, B, N)
        data.append((PackedBatch.from_dense(x, e, adj), PackedBatch.from_dense(x2, e2, adj),
                     rng.integers(0, 4, size=(B, N)).astype(np.int32), rng.normal(2.4, 0.3, size=B)))
    res = []
    for use_graph in (False, True):
        online, target = GnnEngine(spec, use_graph=use_graph), GnnEngine(spec, use_graph=use_graph)
        online.set_weights(w_on)
        target.set_weights(w_tg)
        with torch.cuda.stream(torch.cuda.Stream()):
            sb, sn = online.to_device(data[0][0]), online.to_device(data[0][1])
            a_dev = torch.zeros((B, N), dtype=torch.int32, device="cuda")
            r_dev = torch.zeros(B, dtype=torch.float64, device="cuda")
            y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
            out = []
            for step, (pb, pb2, a, r) in enumerate(data):
                for dst, src in ((sb, pb), (sn, pb2)):                       # same device buffers, new contents
                    dst.xe.copy_(torch.from_numpy(src.xe))
                    dst.col_idx.copy_(torch.from_numpy(src.col_idx))
                a_dev.copy_(torch.from_numpy(a))
                r_dev.copy_(torch.from_numpy(r))
                loss = online.dqn_step(target, sb, sn, a_dev, r_dev, 0.5, y_out=y)
                out.append((loss.cpu().numpy(), y.cpu().numpy().copy()))
                if step == 1:
                    target.copy_weights_from(online)
            torch.cuda.synchronize()
        res.append((out, online.get_flat()))
        online.close()
        target.close()
    for (l0, y0), (l1, y1) in zip(res[0][0], res[1][0]):
        assert np.array_equal(l0, l1) and np.array_equal(y0, y1)
    assert np.array_equal(res[0][1], res[1][1])
