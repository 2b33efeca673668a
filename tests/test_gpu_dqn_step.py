"""GPU: the one-call DQN replay step (v2x_dqn_step, GnnEngine.dqn_step) against the float64 oracle -- targets, per-output
losses, the GRADIENT and the weights after Adam -- on every launch plan plan_batch can choose for it, with both branches of
the Huber loss in play.

test_gpu_configs.py checks the step's targets, losses and the weights after ONE Adam step (sign-like: lr * m / sqrt(v) = +-lr)
on draws whose |target - q[a]| has a median of 171: the size of the gradient was compared with nothing and the quadratic
branch of the loss carried 0.125 % of the replaced entries.  Here the gradient k_reduce_adam leaves in the gradient buffer
before it applies Adam (get_grad_flat) is compared element by element with the oracle's.

The draw (_draw; one seeded draw per case, nothing redrawn): f32_params for both networks; the last Dense layer of each is
divided by the standard deviation of the network's float64 output (q of order 1) and rounded to fp32; actions uniform in 0..3;
reward[b] = median over links of (q[b, k, a] - gamma max_c q'[b, k, c]) + U(-1, 1), gamma = 0.5: every graph has a reward of
its own and |target - q[a]| straddles the Huber delta.  Asserted in every case from the oracle's own numbers: at least 25 %
of the B x N replaced entries on either branch.  Checked on the CPU with this recipe: the quadratic share is 0.58-0.72 on
all fourteen draws below (each case prints its own).

A  one step per plan.  The case's path_info fields are asserted, so a case that silently runs another plan fails:

    #   N   F  L  weights   B   topology        switches                      pins
    1   20  64 2  per-node  48  reference       -                             fused(split5), edge-bitset-walk, fragment-major,
                                                                              dense0_dw=k_wgrad (the DQN loop's default form)
    2   20  64 2  per-node  48  reference       V2X_FUSED_SPLIT=0             fused, complement, fragment-major, k_wgrad
    3   20  64 2  per-node  48  reference       + V2X_MLP_WG0=1               fused, fragment-major, dense0_dw=k_mlp_train_wg
                                                                              (what batch 4096 runs)
    4   20  64 2  per-node  48  reference       V2X_FRAG_WITH_DENSE0_ROLE=0   row-major, k_wgrad
    5   20  64 2  per-node  17  reference       n_global = 51                 row-major, k_mlp_train_wg; one graph in the last
                                                                              tile, the denominator of 51 graphs
    6   20  64 2  shared    40  reference       -                             row-major (one 800-row index list); the launch
                                                                              that takes Dense-0 is printed
    7   4   16 2  per-node  32  reference       -                             fused, complement, fragment-major
    8   7   32 1  per-node  16  random 0.5      -                             fused, L = 1, F = 32
    9   20  64 4  per-node  16  reference       -                             fused on whole tiles (L > 3)
    10  20  16 3  per-node  32  reference       -                             fused; 1 embed tile over 3 stages: an embed role
                                                                              of its own (embed_rides needs L | F / 16)
    11  20  64 2  per-node  32  in-degree 2     -                             edge-bitset-walk on sparse rows (degree-aware)
    12  2   32 2  per-node  16  random, graphs  -                             fused; graphs 0, 5 and 15 have no edge at all
                                0, 5, 15 empty
    13  33  32 1  per-node  17  random 0.5      -                             layerwise, edge-gather, mlp=train_wg
    14  12  128 1 per-node  17  reference       -                             mlp=fwd+bwd, dense0_dw=k_wide_wgrad: full forward,
                                                                              k_dqn_targets, the ordinary training launch

   Every case: y (assert_fwd_close), per-output losses, the gradient (assert_grads_match_oracle with GRAD_RTOL,
   GRAD_ATOL_REL and MAX_GATE_FLIPS of util.py; the oracle differentiates at its own q and y -- clip is continuous, an fp32
   difference in q moves dq far below the tolerance), the weights after the oracle's Adam step, and a twin engine's
   forward_backward on the step's own y (the reference's predict-then-fit) under assert_grad_close.
   Loss bound: the fit-step tests' assert_close(loss, ref, 2e-4, 1e-6) (LOSS_RTOL / LOSS_ATOL) for all fourteen cases; each
   case prints its measured maximum relative error (6e-8 to 5e-7 on an MI355X: no case needed more than the starting
   bound).  The 5e-3 of test_gpu_configs.py is not needed at q of order 1.
B  the two target forms (k_dqn_tq inside k_mlp_train_wg / V2X_DQN_FUSED_TARGETS=0: forward, k_dqn_targets, training launch)
   on case 1's draw: replaced entries bit for bit, each form against the oracle, y_out=None bit for bit a call with a buffer.
C  three steps with new s, a, r, s' each and target.copy_weights_from(online) after the second, plans 1 and 6, by the
   scheme of test_gpu_launch_sizes._adam_steps.
D  the target rule on ties, signed zeros, +-inf, values near +-3e38 and NaN: numpy's np.float32(r + gamma *
   np.float64(np.amax(row))), where amax is NaN if any entry is -- through DeviceReplay.dqn_targets (k_dqn_targets),
   DeviceReplay.q_stats (k_q_stats) and dqn_step (k_dqn_tq).
"""
import functools

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch
from oracle import compact as oc
from util import (ospec, f32_params, random_inputs, fixed_indegree_adj, oracle_step, assert_close, assert_fwd_close,
                  assert_grad_close, assert_grads_match_oracle, assert_weights_after_adam_step)
from test_gpu_configs import _oracle_dqn_step
from test_gpu_launch_sizes import _engine

pytestmark = pytest.mark.gpu

GAMMA = 0.5
LOSS_RTOL, LOSS_ATOL = 2e-4, 1e-6        # the fit-step tests' bound (test_gpu_launch_sizes._parity)
MIN_BRANCH_SHARE = 0.25                  # of the replaced entries on either Huber branch: every draw of A and B
# C's later steps draw at whatever weights Adam has left: the head is no longer at unit scale (q std 0.5-30 after one or two
# steps of lr 1e-3 on every weight) and after the sync q' is the online network's own output, so the spread of target - q[a]
# moves.  The branch coverage is A's job; C is about the moments and the sync and only asks that neither branch is a handful
# of entries (a tenth of 800-960).
MIN_BRANCH_SHARE_LATER_STEPS = 0.10

SPLIT0 = dict(V2X_FUSED_SPLIT=0)
CASES = {  # number: (N, F, L, shared, B, topology, switches, n_global, path_info fields the case must show)
    1: (20, 64, 2, False, 48, "reference", {}, None,
        dict(graph_layers="fused(split5)", aggregation="edge-bitset-walk", handoff="fragment-major", dense0_dw="k_wgrad", mlp="train_wg")),
    2: (20, 64, 2, False, 48, "reference", SPLIT0, None,
        dict(graph_layers="fused", aggregation="complement", handoff="fragment-major", dense0_dw="k_wgrad")),
    3: (20, 64, 2, False, 48, "reference", dict(SPLIT0, V2X_MLP_WG0=1), None,
        dict(graph_layers="fused", aggregation="complement", handoff="fragment-major", dense0_dw="k_mlp_train_wg")),
    4: (20, 64, 2, False, 48, "reference", dict(V2X_FRAG_WITH_DENSE0_ROLE=0), None,
        dict(graph_layers="fused(split5)", handoff="row-major", dense0_dw="k_wgrad")),
    5: (20, 64, 2, False, 17, "reference", {}, 51, dict(handoff="row-major", dense0_dw="k_mlp_train_wg")),
    6: (20, 64, 2, True, 40, "reference", {}, None, dict(handoff="row-major", mlp="train_wg")),
    7: (4, 16, 2, False, 32, "reference", {}, None, dict(graph_layers="fused", aggregation="complement", handoff="fragment-major")),
    8: (7, 32, 1, False, 16, "random", {}, None, dict(graph_layers="fused")),
    9: (20, 64, 4, False, 16, "reference", {}, None, dict(graph_layers="fused")),
    10: (20, 16, 3, False, 32, "reference", {}, None, dict(graph_layers="fused(split5)")),
    11: (20, 64, 2, False, 32, "indegree2", {}, None, dict(graph_layers="fused(split5)", aggregation="edge-bitset-walk")),
    12: (2, 32, 2, False, 16, "some-empty", {}, None, dict(graph_layers="fused")),
    13: (33, 32, 1, False, 17, "random", {}, None, dict(graph_layers="layerwise", aggregation="edge-gather", mlp="train_wg")),
    14: (12, 128, 1, False, 17, "reference", {}, None, dict(mlp="fwd+bwd", dense0_dw="k_wide_wgrad")),
}


# ------------------------------------------------------------------------------------------------ the draw (host only)
def _spec(n):
    N, F, L, shared = CASES[n][:4]
    return GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)


def _flat(a):
    return np.asarray(a, np.float64).reshape(a.shape[0] * a.shape[1], -1)


def _graph(adj):
    return oc.adj_to_csr(adj)


def _oracle_q(spec, P, x, e, adj):
    """float64 forward of the oracle -> q [B, N, 4]"""
    B, N = x.shape[:2]
    M = oc.csr_to_matrix(*_graph(adj), dtype=np.float64)
    return oc.forward(ospec(spec), P, _flat(x), _flat(e), M)[0].reshape(B, N, -1)


def _inputs(spec, rng, B, topo):
    """s and s' of B transitions: node / edge features of both, one adjacency (BS_brain.py:583)"""
    N = spec.n_nodes
    if topo == "reference":
        x, e, adj = random_inputs(rng, B, N)
    else:
        x, e, adj = random_inputs(rng, B, N, ref_topology=False, density=0.5)
        if topo == "indegree2":
            adj = fixed_indegree_adj(rng, B, N, 2)
        elif topo == "some-empty":
            adj[[0, 5, B - 1]] = 0.0
        else:
            assert topo == "random", topo
    x2, e2, _ = random_inputs(rng, B, N)
    return x, e, adj, x2, e2


def _unit_scale_head(spec, P, x, e, adj):
    """P with W and b of the last Dense layer divided by the standard deviation of the network's output on (x, e, adj),
    rounded to fp32 (kept as float64) -> (P, the float64 q before the rounding)"""
    q = _oracle_q(spec, P, x, e, adj)
    s = q.std()
    d = P['dense'][3]
    P['dense'][3] = {k: (v / s).astype(np.float32).astype(np.float64) for k, v in d.items()}
    return P, q / s


def _actions_rewards(rng, q, qn):
    """actions uniform in 0..3; reward[b] = median_k (q[b, k, a] - gamma max_c q'[b, k, c]) + U(-1, 1)"""
    B, N = q.shape[:2]
    action = rng.integers(0, 4, size=(B, N))
    qa = np.take_along_axis(q, action[:, :, None], axis=2)[:, :, 0]
    reward = np.median(qa - GAMMA * qn.max(axis=2), axis=1) + rng.uniform(-1.0, 1.0, size=B)
    return action.astype(np.int32), reward.astype(np.float64)


def _draw(n):
    N, F, L, shared, B, topo = CASES[n][:6]
    spec = _spec(n)
    rng = np.random.default_rng(1000 + n)
    P_on, P_tg = f32_params(spec, rng), f32_params(spec, rng)
    x, e, adj, x2, e2 = _inputs(spec, rng, B, topo)
    P_on, q = _unit_scale_head(spec, P_on, x, e, adj)
    P_tg, qn = _unit_scale_head(spec, P_tg, x2, e2, adj)
    action, reward = _actions_rewards(rng, q, qn)
    return dict(spec=spec, P_on=P_on, P_tg=P_tg, x=x, e=e, adj=adj, x2=x2, e2=e2, action=action, reward=reward)


def _oracle_of(spec, P_on, P_tg, t, n_global, what, min_share=MIN_BRANCH_SHARE):
    """The oracle of one replay step on transitions t (x, e, adj, x2, e2, action, reward): the targets of _oracle_dqn_step,
    the fit step on them (util.oracle_step: loss, gradient, what the ReLU-gate resolution needs) and the Huber branch shares
    of the replaced entries, asserted."""
    B, N = t['x'].shape[:2]
    y, loss0, _, _ = _oracle_dqn_step(spec, oc.params_to_list(P_on), oc.params_to_list(P_tg), t['x'], t['e'], t['adj'],
                                      t['x2'], t['e2'], t['action'], t['reward'], GAMMA)
    step = oracle_step(spec, P_on, _flat(t['x']), _flat(t['e']), _graph(t['adj']), y.reshape(B * N, -1), n_denominator=n_global)
    if n_global is None:
        assert np.allclose(loss0, step['loss'], rtol=1e-12, atol=0)
    q = step['q'].reshape(B, N, -1)
    err = np.take_along_axis(y - q, t['action'][:, :, None].astype(np.int64), axis=2)[:, :, 0]
    untouched = np.ones(q.shape, bool)
    np.put_along_axis(untouched, t['action'][:, :, None].astype(np.int64), False, axis=2)
    assert np.array_equal(y[untouched], q[untouched])
    quad = float((np.abs(err) < 1.0).mean())
    print("%s: Huber branches of the %d replaced entries: quadratic %.3f, linear %.3f (|err| median %.3f, max %.3f; q std %.3f)"
          % (what, err.size, quad, 1.0 - quad, np.median(np.abs(err)), np.abs(err).max(), q.std()))
    assert quad >= min_share and 1.0 - quad >= min_share, (what, quad)
    return dict(y=y, step=step, untouched=untouched)


@functools.lru_cache(maxsize=None)
def _case(n):
    """(draw, oracle) of case n -- computed once, shared by the tests on that draw and never modified (cases 1-4 differ in their
    switches only, but each has a draw of its own; B runs on case 1's, C starts from the weights of case 1's and 6's)"""
    d = _draw(n)
    return d, _oracle_of(d['spec'], d['P_on'], d['P_tg'], d, CASES[n][7], "case %d" % n)


# ------------------------------------------------------------------------------------------------ the engines
def _run_step(spec, w_on, w_tg, t, switches, n_global=None, y_buffer=True, twin=False, want=None, what=""):
    """One dqn_step of a fresh engine pair created under `switches` -> dict(y, loss, grad, weights, info[, twin_grad])"""
    import torch
    online, target = _engine(spec, switches), _engine(spec, switches)
    online.set_weights(w_on)
    target.set_weights(w_tg)
    B, N = t['x'].shape[:2]
    sb = online.to_device(PackedBatch.from_dense(t['x'], t['e'], t['adj']))
    sn = online.to_device(PackedBatch.from_dense(t['x2'], t['e2'], t['adj']))
    info = online.path_info(sb)
    print("%s: N=%d F=%d L=%d %s B=%d %s  %s" % (what, N, spec.feat_dim, spec.n_mp_layers, "shared" if spec.share_weights else "per-node",
                                                  B, switches or "", " ".join("%s=%s" % kv for kv in sorted(info.items()))))
    for k, v in (want or {}).items():
        assert info[k] == v, (what, "the case must reach %s=%s" % (k, v), info)
    a_dev = torch.from_numpy(np.ascontiguousarray(t['action'], np.int32)).cuda()
    r_dev = torch.from_numpy(np.ascontiguousarray(t['reward'], np.float64)).cuda()
    y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda") if y_buffer else None
    loss = online.dqn_step(target, sb, sn, a_dev, r_dev, GAMMA, y_out=y, n_global=n_global)
    online.check_errors()
    out = dict(info=info, loss=loss.cpu().numpy(), grad=online.get_grad_flat(), weights=online.get_weights(),
               y=None if y is None else y.cpu().numpy().reshape(B, N, 4))
    assert online.get_optimizer_state()[2] == 1
    if twin:                      # the reference's predict-then-fit: an ordinary fit step's gradient on the step's own targets
        tw = _engine(spec, switches)
        tw.set_weights(w_on)
        out['twin_loss'] = tw.forward_backward(sb, y, n_global=n_global).cpu().numpy()
        out['twin_grad'] = tw.get_grad_flat()
        tw.close()
    online.close()
    target.close()
    return out


def _check_against_oracle(spec, P_on, ref, out, what):
    """y, losses, gradient and the weights after the oracle's Adam step -> the oracle gradient the check used (parameter structure)"""
    step = ref['step']
    assert_fwd_close(out['y'], ref['y'], what + ": training targets")
    rel = np.abs(out['loss'] - step['loss']) / np.abs(step['loss'])
    print("%s: per-output losses: max relative error %.3e (bound %.0e), loss mean %.4f" % (what, rel.max(), LOSS_RTOL, step['loss'].mean()))
    assert_close(out['loss'], step['loss'], LOSS_RTOL, LOSS_ATOL, what + ": per-output Huber losses")
    g_used, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, out['grad']), P_on, step, what + ": gradient")
    print("%s: %d ReLU gates at rounding distance of 0, %d taken the kernels' way" % (what, n_cand, n_flip))
    om = oc.OracleModel(ospec(spec), P_on, dtype=np.float64)
    om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_used))
    assert_weights_after_adam_step(out['weights'], oc.params_to_list(om.params), oc.params_to_list(g_used), 0, what)
    return g_used


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("n", sorted(CASES))
def test_a_one_step_per_plan_vs_oracle(n):
    N, F, L, shared, B, topo, switches, n_global, want = CASES[n]
    what = "A%d" % n
    d, ref = _case(n)
    spec = d['spec']
    if n == 10:
        assert (F // 16) % L != 0            # embed_rides: the embed tiles do not divide over the stages -> a role of its own
    if n == 12:
        assert not d['adj'][[0, 5, B - 1]].any() and d['adj'].any()
    if n == 11:
        assert (d['adj'].sum(axis=1) == 2).all()
    out = _run_step(spec, oc.params_to_list(d['P_on']), oc.params_to_list(d['P_tg']), d, switches, n_global, twin=True, want=want, what=what)
    if n == 6:
        print("A6: Dense-0's weight gradient is taken by %s" % out['info']['dense0_dw'])
    _check_against_oracle(spec, d['P_on'], ref, out, what)
    assert_grad_close(out['grad'], out['twin_grad'], what + ": gradient of the replay step against forward_backward on its targets")
    assert_close(out['loss'], out['twin_loss'], LOSS_RTOL, LOSS_ATOL, what + ": losses of the replay step against forward_backward")


# ---------------------------------------------------------------------------------------------------------------- B
def test_b_two_target_forms_agree():
    d, ref = _case(1)
    spec, want = d['spec'], CASES[1][8]
    w_on, w_tg = oc.params_to_list(d['P_on']), oc.params_to_list(d['P_tg'])
    outs = {}
    for form, sw in (("in-kernel", {}), ("k_dqn_targets", dict(V2X_DQN_FUSED_TARGETS=0))):
        outs[form] = _run_step(spec, w_on, w_tg, d, sw, want=want, what="B " + form)
        _check_against_oracle(spec, d['P_on'], ref, outs[form], "B " + form)
        nobuf = _run_step(spec, w_on, w_tg, d, sw, y_buffer=False, want=want, what="B %s, y_out=None" % form)
        assert np.array_equal(nobuf['loss'], outs[form]['loss']), form
        assert all(np.array_equal(a, b) for a, b in zip(nobuf['weights'], outs[form]['weights'])), form
        assert np.array_equal(nobuf['grad'], outs[form]['grad']), form
    ya, yb = outs["in-kernel"]['y'], outs["k_dqn_targets"]['y']
    replaced = ~ref['untouched']
    assert np.array_equal(ya[replaced].view(np.uint32), yb[replaced].view(np.uint32))
    assert_grad_close(outs["in-kernel"]['grad'], outs["k_dqn_targets"]['grad'], "B: gradients of the two forms")


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("n", [1, 6])
def test_c_three_steps_with_a_target_sync(n):
    """Every step: new transitions (rewards by the draw's rule at the engines' CURRENT weights, so that both Huber branches
    stay in play), the oracle's targets and gradient at the engines' weights of that step, the oracle's float64 Adam on that
    gradient, the weights against it with the gradient history.  The target network is synced after the second step: the
    third step's oracle takes the online engine's weights as read back after step two for its target network."""
    import torch
    N, F, L, shared, B, topo, switches, n_global, want = CASES[n]
    what = "C%d" % n
    d, _ = _case(n)
    spec, os_ = d['spec'], ospec(d['spec'])
    rng = np.random.default_rng(2000 + n)
    online, target = _engine(spec, switches), _engine(spec, switches)
    online.set_weights(oc.params_to_list(d['P_on']))
    target.set_weights(oc.params_to_list(d['P_tg']))
    om = oc.OracleModel(os_, d['P_on'], dtype=np.float64)
    w_tg = oc.params_to_list(d['P_tg'])
    history = []
    for step in range(3):
        P_eng = oc.params_from_list(os_, online.get_weights(), np.float64)
        P_tg = oc.params_from_list(os_, w_tg, np.float64)
        x, e, adj, x2, e2 = _inputs(spec, rng, B, topo)
        action, reward = _actions_rewards(rng, _oracle_q(spec, P_eng, x, e, adj), _oracle_q(spec, P_tg, x2, e2, adj))
        t = dict(x=x, e=e, adj=adj, x2=x2, e2=e2, action=action, reward=reward)
        ref = _oracle_of(spec, P_eng, P_tg, t, None, "%s step %d" % (what, step),
                         MIN_BRANCH_SHARE if step == 0 else MIN_BRANCH_SHARE_LATER_STEPS)
        sb = online.to_device(PackedBatch.from_dense(x, e, adj))
        sn = online.to_device(PackedBatch.from_dense(x2, e2, adj))
        info = online.path_info(sb)
        for k, v in want.items():
            assert info[k] == v, (what, info)
        y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
        loss = online.dqn_step(target, sb, sn, torch.from_numpy(action).cuda(), torch.from_numpy(reward).cuda(), GAMMA, y_out=y)
        assert_fwd_close(y.cpu().numpy().reshape(B, N, 4), ref['y'], "%s: targets of step %d" % (what, step))
        assert_close(loss.cpu().numpy(), ref['step']['loss'], LOSS_RTOL, LOSS_ATOL, "%s: losses of step %d" % (what, step))
        g_ref, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, online.get_grad_flat()), P_eng, ref['step'],
                                                          "%s: gradient of step %d" % (what, step))
        print("%s step %d: %d ReLU gates at rounding distance, %d taken the kernels' way" % (what, step, n_cand, n_flip))
        om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_ref))
        history.append(oc.params_to_list(g_ref))
        assert_weights_after_adam_step(online.get_weights(), oc.params_to_list(om.params), history, step, what)
        if step == 1:
            target.copy_weights_from(online)
            w_tg = online.get_weights()
            assert np.array_equal(target.get_flat(), online.get_flat())
    assert online.get_optimizer_state()[2] == 3
    assert target.get_optimizer_state()[2] == 0
    online.close()
    target.close()


# ---------------------------------------------------------------------------------------------------------------- D
INF, NAN, BIG = np.inf, np.nan, 3e38
SPECIAL_ROWS = np.array([
    [1.0, 3.0, 3.0, -2.0],            # the maximum tied at two positions
    [0.5, 0.5, 0.5, 0.5],             # ... at all four
    [-0.0, 0.0, -1.0, -2.0],          # -0.0 beside +0.0
    [0.0, -0.0, -0.0, -1.0],
    [INF, 1.0, 2.0, 3.0],
    [-INF, -INF, -5.0, -INF],
    [-INF, -INF, -INF, -INF],
    [1.0, -INF, 0.0, INF],
    [BIG, 2.9e38, -BIG, 0.0],         # near the ends of the fp32 range
    [-BIG, -3.1e38, -2.9e38, -3.2e38],
    [NAN, 1.0, 2.0, 3.0],             # a NaN at each position: np.amax is NaN
    [1.0, NAN, 2.0, 3.0],
    [3.0, 2.0, NAN, 1.0],
    [3.0, 2.0, 1.0, NAN],
    [NAN, NAN, NAN, NAN],
    [NAN, INF, 1.0, 2.0],             # NaN wins over +inf
], np.float32)
SPECIAL_REWARDS = np.array([-0.25, -1.5, -3.0, -1e-3, -7.75], np.float64)
SPECIAL_GAMMAS = (0.0, 0.5, 1.0)


def _numpy_targets(q, qn, action, reward, gamma):
    """BS_brain.py:684-692 row by row: y = q, y[row, a] = np.float32(r + gamma * np.float64(np.amax(q'[row])))"""
    n = action.shape[1]
    y = np.array(q, np.float32)
    act = action.reshape(-1)
    with np.errstate(all="ignore"):
        for row in range(y.shape[0]):
            y[row, act[row]] = np.float32(reward[row // n] + gamma * np.float64(np.amax(qn[row])))
    return y


def _assert_same_floats(got, want, what):
    """bit for bit, any NaN for a NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", np.argwhere(np.isnan(got) != nan)[:8].tolist())
    bad = got[~nan].view(np.uint32) != want[~nan].view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), got[~nan][bad][:8], want[~nan][bad][:8])


def test_d1_target_rule_on_special_values_k_dqn_targets_and_q_stats():
    import torch
    from v2xgnn.rl.replay import DeviceReplay
    n, B = len(SPECIAL_ROWS), len(SPECIAL_REWARDS)
    rng = np.random.default_rng(31)
    mem = DeviceReplay(64, n)
    qn = np.tile(SPECIAL_ROWS, (B, 1))                                   # link k of every graph carries row k
    q = rng.normal(0.0, 1.0, size=(B * n, 4)).astype(np.float32)
    action = rng.integers(0, 4, size=(B, n)).astype(np.int32)
    action[0] = np.arange(n) % 4
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for gamma in SPECIAL_GAMMAS:
        y = mem.dqn_targets(dev(q), dev(qn), dev(action), dev(SPECIAL_REWARDS), gamma).cpu().numpy()
        _assert_same_floats(y, _numpy_targets(q, qn, action, SPECIAL_REWARDS, gamma), "k_dqn_targets, gamma %g" % gamma)
    # the Q statistics of a minibatch (BS_brain.py:743-746): per link the sum of all entries and the sum of np.amax per sample
    with np.errstate(all="ignore"):
        y3 = qn.reshape(B, n, 4).astype(np.float64)
        want = np.stack([y3.sum(axis=(0, 2)), np.amax(y3, axis=2).sum(axis=0)])
    got = mem.q_stats(dev(qn), B, 4).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.allclose(got, want, rtol=1e-12, atol=0, equal_nan=True), (got, want)


def test_d2_target_rule_on_special_values_k_dqn_tq():
    """dqn_step at 4 links x 16 features: a target network of all-zero weights whose last Dense layer has the crafted rows as
    its per-link biases gives q' = those rows whatever s' is.  Only y_out (and that the call succeeds) is asserted: the step's
    loss is +-inf or NaN by construction."""
    import torch
    N, F, B = 4, 16, len(SPECIAL_REWARDS)
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(32)
    P_on = f32_params(spec, rng)
    x, e, adj, x2, e2 = _inputs(spec, rng, B, "reference")
    q_ref = _oracle_q(spec, P_on, x, e, adj).reshape(B * N, 4)
    online, target = _engine(spec, {}), _engine(spec, {})
    sb = online.to_device(PackedBatch.from_dense(x, e, adj))
    sn = online.to_device(PackedBatch.from_dense(x2, e2, adj))
    assert online.path_info(sb)["mlp"] == "train_wg"
    w_on = oc.params_to_list(P_on)
    zeros = np.zeros(online.n_params, np.float32)
    y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
    r_dev = torch.from_numpy(SPECIAL_REWARDS).cuda()
    for s in range(0, len(SPECIAL_ROWS), N):
        P_tg = oc.zeros_like_params(P_on)
        P_tg['dense'][3]['b'] = SPECIAL_ROWS[s:s + N].astype(np.float64)
        target.set_weights(oc.params_to_list(P_tg))
        qn = np.tile(SPECIAL_ROWS[s:s + N], (B, 1))
        for gamma in SPECIAL_GAMMAS:
            action = rng.integers(0, 4, size=(B, N)).astype(np.int32)
            online.set_weights(w_on)                                  # (the step before left NaN in the weights and the moments)
            online.set_optimizer_state(zeros, zeros, 0)
            online.dqn_step(target, sb, sn, torch.from_numpy(action).cuda(), r_dev, gamma, y_out=y, want_loss=False)
            online.check_errors()
            got = y.cpu().numpy()
            what = "k_dqn_tq, rows %d-%d, gamma %g" % (s, s + N - 1, gamma)
            want = _numpy_targets(q_ref, qn, action, SPECIAL_REWARDS, gamma)
            replaced = np.zeros(got.shape, bool)
            replaced[np.arange(B * N), action.reshape(-1)] = True
            _assert_same_floats(got[replaced], want[replaced], what)
            assert_fwd_close(got[~replaced], q_ref[~replaced], what + ": untouched entries")
    online.close()
    target.close()
