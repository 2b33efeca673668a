"""GPU: the whole model against the float64 oracle at 41 to 128 links -- forward, per-output Huber loss, every gradient
array, Keras Adam and the one-call DQN step.  Above 32 links a fixed-size model runs layer-wise (k_gemm_rows, k_agg /
k_agg_dense on the masks k_adj_masks builds into the model's own buffer, k_wgrad, k_mlp_train_wg); the other whole-model
suites stop at 40 links (tests/test_gpu_shapes.py, test_gpu_dqn_step.py case 13, test_gpu_launch_sizes.py) but for
100 links x 256 features.  Reached only here: mask rows of 3 words, a full last word (64, 96, 128 links), a single valid bit
in the last word (65, 97), a padded contraction tail (80 staged rows at 65 links), a whole staging pass (128 rows), two
feature groups (F = 128), the per-graph choice between the complement walk and the MFMA product and the per-row direct sum
with the backward's add / gate operands, own-receiver rows of in-degree n - 1, 41 to 128 weight slots in every per-slot
launch, the row-major Dense-0 roles of k_wgrad beside them, k_agg at F = 16 / 32 and on sparse graphs at F = 64.

The cases, their draws and the draws' conditions are in tests/test_links_41_128_host.py (CASES_A, CASES_B; one seeded draw
per case, nothing redrawn); that file checks them on the host with the oracle alone.  Every case prints its path_info and
asserts the fields of its table entry, so a case that silently takes another plan fails; it prints v2x_debug_layer_slabs,
the form each graph takes in k_agg_dense (from the rule n * n - n_edges <= 8 n and the edge counts) and its largest ratio of
error to bound.

A  fit step: forward, per-output loss and every gradient array as test_gpu_shapes._check (targets q + N(0, 1.2) around the
   kernels' own q, the loss differentiated at that q), then the weights after ONE fit call against the oracle's Keras Adam
   as test_gpu_fullsize.  Bounds: FWD_RTOL / FWD_ATOL, GRAD_RTOL / GRAD_ATOL_REL / MAX_GATE_FLIPS, assert_close(loss, ref,
   2e-4, 1e-6), assert_weights_after_adam_step.
A' cases 2, 4, 8 and 14 with V2X_AGG_DENSE_MIN_NODES=999: the same draws through the edge gather (k_agg) instead.
B  the one-call DQN step (cases 101-108) exactly as section A of test_gpu_dqn_step.py.
C  three DQN steps with a target sync, section C of test_gpu_dqn_step.py on cases 102 and 105, at learning rate 1e-5 (at
   1e-3 the later steps' draws are unusable at 128 links, shown from the oracle alone in the host file).
D  a replayed hipGraph whose batch tensors are overwritten in place, topology included (what the receiver replay does): the
   captured k_adj_masks must rebuild the masks on every replay.  Bit for bit an eager engine; the first call also against
   the oracle.
(E, sampled receiver batches at 65 and 128 links, is in tests/test_gpu_replay_receivers.py.)

Measured on an MI355X (every case graph_layers=layerwise, handoff=row-major; mlp=train_wg but for A7: fwd+bwd).  agg: D = dense
(k_agg_dense), G = edge-gather (k_agg); d0: which launch takes Dense-0's weight gradient; slabs: v2x_debug_layer_slabs as gnn /
dense / threads per column of the slab sum; then the largest error / bound of the forward (B: the targets), the loss and the
gradient; B: the quadratic share of the replaced entries.  No case needed a ReLU gate taken the kernels' way but B101 (1 of 4).

    A1   41 x  64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.054  0.000  0.019   all graphs complement
    A2   64 x  64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.062  0.001  0.035   complement
    A3   65 x  64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.124  0.001  0.027   all 16 graphs MFMA product
    A4   65 x  64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.129  0.000  0.067   complement (130 or 126 non-edges a graph)
    A5   96 x  32  G  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.067  0.001  0.055
    A6   97 x  64  D  k_mlp_train_wg  1,1,1,1 / 1,1,1,1 / 1    0.086  0.001  0.035   complement; max|q| 2.0e6
    A7  100 x 128  D  k_wide_wgrad    0,0,0 / 0,1,1,1 / 1      0.070  0.001  0.042   complement, two feature groups
    A8  128 x  64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.114  0.001  0.030   complement
    A9  128 x  64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.071  0.001  0.039   all 16 graphs MFMA product
    A10 128 x  64  D  k_wgrad         2,2,2 / 1,16,16,16 / 16  0.010  0.000  0.009   complement; shared weights
    A11 128 x  16  G  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.085  0.001  0.039
    A12 128 x  64  G  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.058  0.000  0.028
    A13 100 x  64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.080  0.001  0.058   complement; Neighbor_Input
    A14  80 x  64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.104  0.001  0.029   graphs 0 2 5 6 7 complement, 1 3 4 MFMA
    A' (edge gather) cases 2, 4, 8, 14: forward 0.059 0.142 0.113 0.104, gradient 0.032 0.043 0.049 0.049
    B101  64 x 64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.096  0.003  0.048   0.596
    B102 128 x 64  D  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.061  0.003  0.044   0.604
    B103  65 x 64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.048  0.003  0.025   0.618   MFMA product
    B104 100 x 32  G  k_mlp_train_wg  1,1 / 1,1,1,1 / 1        0.052  0.002  0.027   0.591
    B105 128 x 64  D  k_wgrad         2,2,2 / 1,16,16,16 / 16  0.110  0.005  0.004   0.555   shared weights
    B106  97 x 64  D  k_mlp_train_wg  1,1,1,1 / 1,1,1,1 / 1    0.051  0.003  0.098   0.579
    B107 128 x 16  G  k_mlp_train_wg  1,1,1 / 1,1,1,1 / 1      0.040  0.012  0.048   0.565
    B108  41 x 64  D  k_wgrad         1,1,1 / 1,1,1,1 / 1      0.103  0.001  0.019   0.620
    C102 / C105: gradient 0.034 0.058 0.063 / 0.005 0.019 0.027 of the bound at steps 0, 1, 2; the weights against Adam of the
    engine's own gradients reach 0.53 / 0.48 of _adam_of_own_gradient_bound after three steps

Every A and B case also held its bounds once with V2X_AGG_DENSE_MIN_NODES=999 (all aggregations edge-gather; only that pin
changed), with V2X_AGG_NO_SMALL=1 and with V2X_AGG_WORKERS_PER_GRAPH=1.  Arithmetic-only mutations of a scratch build, all
tests of this file and the receiver-batch test run against each:
  (a) the complement walk of k_agg_dense masks the last word to left - 1 bits: A1 4 6 7 13 14, B106 108, D and the 65-link
      receiver batch fail -- every complement-form case with a partial last word (41, 65, 80, 97, 100 links);
  (b) the complement rule as `<`: all pass (A14's graph 2 moves to the MFMA product, which is as right); the forward's
      complement walk reading the by-source masks: A1 2 4 6 7 8 10 13 14, B101 102 105 106 108, C, D and both receiver batches
      fail -- every dense case with a complement-form graph;
  (c) dense0_rides forced false: A1 3 9 and B101 103 108 fail on their dense0_dw pin, nothing else."""
import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch
from oracle import compact as oc
from util import (ospec, f32_params, random_inputs, oracle_step, assert_fwd_close, assert_close, assert_grad_close,
                  assert_grads_match_oracle, assert_weights_after_adam_step, FWD_RTOL, FWD_ATOL, GRAD_RTOL, GRAD_ATOL_REL)
from test_gpu_launch_sizes import _engine, _slabs
import test_gpu_dqn_step as T
from test_links_41_128_host import CASES_A, CASES_B, C_CASES, C_LR, DENSE, GATHER, draw_a, oracle_of_a, forms_of, rows

pytestmark = pytest.mark.gpu

LOSS_RTOL, LOSS_ATOL = T.LOSS_RTOL, T.LOSS_ATOL        # assert_close(loss, ref, 2e-4, 1e-6)


# ------------------------------------------------------------------------------------------------ what a case prints
def _ratio(got, ref, rtol, atol):
    """largest error / bound of assert_close(got, ref, rtol, atol)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def _fwd_ratio(got, ref):
    return _ratio(got, ref, FWD_RTOL, FWD_ATOL * max(1.0, float(np.abs(ref).max())))


def _grad_ratio(got_list, ref_list):
    return max(_ratio(a, b, GRAD_RTOL, GRAD_ATOL_REL * (float(np.abs(b).max()) or 1.0)) for a, b in zip(got_list, ref_list)
               if np.asarray(b).any() or np.asarray(a).any())


def _describe(what, spec, B, topo, switches, info, adj):
    print("%s: N=%d F=%d L=%d %s B=%d %s %s  %s" % (what, spec.n_nodes, spec.feat_dim, spec.n_mp_layers,
                                                    "shared" if spec.share_weights else "per-node", B, topo, switches or "",
                                                    " ".join("%s=%s" % kv for kv in sorted(info.items()))))
    if info["aggregation"] == DENSE:
        forms = forms_of(adj)
        print("%s: k_agg_dense form per graph: %s" % (what, " ".join("%d:%s" % gf for gf in enumerate(forms))))


def _assert_pins(what, info, want):
    for k, v in want.items():
        assert info[k] == v, (what, "the case must reach %s=%s" % (k, v), info)


# ---------------------------------------------------------------------------------------------------------------- A
def fit_case(n, switches=None, want_over=None):
    """one A case under `switches` (read when the engine is created); want_over: path_info fields the switches change"""
    N, F, L, shared, B, topo, n_global, want = CASES_A[n]
    switches = switches or {}
    want = dict(want, **(want_over or {}))
    what = "A%d" % n
    d = draw_a(n)
    spec, P = d['spec'], d['P']
    pb = PackedBatch.from_dense(d['x'], d['e'], d['adj'], d['nbr'])
    eng = _engine(spec, switches)
    w0 = oc.params_to_list(P)
    eng.set_weights(w0)
    info = eng.path_info(pb)
    _describe(what, spec, B, topo, switches, info, d['adj'])
    _assert_pins(what, info, want)
    q = eng.forward(pb)
    y, step = oracle_of_a(d, q)
    r_fwd = _fwd_ratio(q, step['q'])
    assert_fwd_close(q, step['q'], what + ": forward")
    loss = eng.forward_backward(pb, y, n_global=n_global)
    gnn, dense, groups = _slabs(eng)
    r_loss = _ratio(loss, step['loss'], LOSS_RTOL, LOSS_ATOL)
    assert_close(loss, step['loss'], LOSS_RTOL, LOSS_ATOL, what + ": per-output Huber loss")
    got = v2xgnn.flat_to_keras_list(spec, eng.get_grad_flat())
    g_used, n_cand, n_flip = assert_grads_match_oracle(got, P, step, what + ": gradient")
    r_grad = _grad_ratio(got, oc.params_to_list(g_used))
    # the weights after ONE fit call from the same start against the oracle's Keras Adam on the oracle's gradient
    assert eng.get_optimizer_state()[2] == 0
    loss_fit = eng.train_step(pb, y, n_global=n_global)
    assert_close(loss_fit, step['loss'], LOSS_RTOL, LOSS_ATOL, what + ": per-output Huber loss of the fit call")
    om = oc.OracleModel(ospec(spec), P, dtype=np.float64)
    om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_used))
    assert_weights_after_adam_step(eng.get_weights(), oc.params_to_list(om.params), oc.params_to_list(g_used), 0, what)
    assert eng.get_optimizer_state()[2] == 1
    eng.check_errors()
    eng.close()
    print("%s: slabs gnn %s dense %s groups %d; max|q| %.3g; error / bound: forward %.3f, loss %.3f, gradient %.3f; %d ReLU gates "
          "at rounding distance of 0, %d taken the kernels' way" % (what, gnn, dense, groups, np.abs(step['q']).max(), r_fwd, r_loss,
                                                                  r_grad, n_cand, n_flip))


@pytest.mark.parametrize("n", sorted(CASES_A))
def test_a_fit_step_vs_oracle(n):
    fit_case(n)


@pytest.mark.parametrize("n", [2, 4, 8, 14])
def test_a_fit_step_through_the_edge_gather(n):
    """V2X_AGG_DENSE_MIN_NODES=999: no batch is dense enough for k_agg_dense, every aggregation is k_agg's CSR gather -- at 64,
    65, 128 and 80 links with in-degrees of 0 to n - 1; only the `aggregation` pin changes"""
    assert CASES_A[n][7]["aggregation"] == DENSE
    fit_case(n, dict(V2X_AGG_DENSE_MIN_NODES=999), dict(aggregation=GATHER))


# ---------------------------------------------------------------------------------------------------------------- B
def _run_step_with_slabs(*args, **kw):
    """T._run_step, which closes its engines before it returns -> (its result, _slabs of the online engine as it closed)"""
    made, real = [], T._engine

    def engine(spec, switches, **k):
        eng = real(spec, switches, **k)
        rec = {}
        made.append(rec)
        close = eng.close

        def closing():
            if getattr(eng, "_h", None):
                rec['slabs'] = _slabs(eng)
            close()
        eng.close = closing
        return eng
    T._engine = engine
    try:
        out = T._run_step(*args, **kw)
    finally:
        T._engine = real
    return out, made[0]['slabs']                     # the online engine is the first one _run_step creates


def dqn_case(n, switches=None, want_over=None):
    N, F, L, shared, B, topo, sw, n_global, want = T.CASES[n]
    sw = dict(sw, **(switches or {}))
    want = dict(want, **(want_over or {}))
    what = "B%d" % n
    d, ref = T._case(n)
    spec = d['spec']
    out, (gnn, dense, groups) = _run_step_with_slabs(spec, oc.params_to_list(d['P_on']), oc.params_to_list(d['P_tg']), d, sw, n_global,
                                                     twin=True, want=want, what=what)
    if out['info']["aggregation"] == DENSE:
        print("%s: k_agg_dense form per graph: %s" % (what, " ".join("%d:%s" % gf for gf in enumerate(forms_of(d['adj'])))))
    g_used = T._check_against_oracle(spec, d['P_on'], ref, out, what)
    assert_grad_close(out['grad'], out['twin_grad'], what + ": gradient of the replay step against forward_backward on its targets")
    assert_close(out['loss'], out['twin_loss'], LOSS_RTOL, LOSS_ATOL, what + ": losses of the replay step against forward_backward")
    print("%s: slabs gnn %s dense %s groups %d; error / bound: targets %.3f, loss %.3f, gradient %.3f" % (
        what, gnn, dense, groups, _fwd_ratio(out['y'], ref['y']), _ratio(out['loss'], ref['step']['loss'], LOSS_RTOL, LOSS_ATOL),
        _grad_ratio(v2xgnn.flat_to_keras_list(spec, out['grad']), oc.params_to_list(g_used))))


@pytest.mark.parametrize("n", sorted(CASES_B))
def test_b_one_call_dqn_step_vs_oracle(n):
    dqn_case(n)


# ---------------------------------------------------------------------------------------------------------------- C
def _adam_of_own_gradient_bound(w, lr):
    """The engine's fp32 Adam against float64 Keras Adam on the SAME gradients: m, v and the update carry a relative error of a
    few fp32 roundings (3e-3 of a step is what test_gpu_fullsize allows, 3e-6 at lr 1e-3), and the stored weight is rounded to
    fp32 once per step (half an ulp, 6e-8 |w|, three steps)."""
    return 3e-3 * lr + 2e-7 * np.abs(w)


@pytest.mark.parametrize("n", C_CASES)
def test_c_three_dqn_steps_with_a_target_sync(n):
    """Section C of test_gpu_dqn_step.py at 128 links, per-node (102) and shared (105) weights, at learning rate C_LR: at the
    default 1e-3 one step takes q from a standard deviation of 1 to 114 / 5279 and the later steps' draws fail section C's own
    conditions from the oracle alone (tests/test_links_41_128_host.py, C).  Every step: new s, a, r, s' (rewards by the draw's
    rule at the engines' current weights), the oracle's targets, losses and gradient at those weights, the oracle's float64
    Adam on that gradient and the weights against it with the gradient history; target.copy_weights_from(online) after the
    second step.  assert_weights_after_adam_step's bounds are sized for steps of 1e-3, so the weights are ALSO held to
    float64 Keras Adam applied to the engine's own gradients, within _adam_of_own_gradient_bound: a skipped, doubled or
    wrong-sign update of 1e-5 fails there."""
    import torch
    from oracle.keras_semantics import KerasAdam
    N, F, L, shared, B, topo, switches, n_global, want = T.CASES[n]
    what = "C%d" % n
    d, _ = T._case(n)
    spec, os_ = d['spec'], ospec(d['spec'])
    rng = np.random.default_rng(2000 + n)
    online, target = _engine(spec, switches, lr=C_LR), _engine(spec, switches, lr=C_LR)
    online.set_weights(oc.params_to_list(d['P_on']))
    target.set_weights(oc.params_to_list(d['P_tg']))
    om = oc.OracleModel(os_, d['P_on'], dtype=np.float64)
    om.opt = KerasAdam(lr=C_LR)
    own, own_opt = oc.cast_params(d['P_on'], np.float64), KerasAdam(lr=C_LR)
    w_tg = oc.params_to_list(d['P_tg'])
    history, worst_own = [], 0.0
    for step in range(3):
        P_eng = oc.params_from_list(os_, online.get_weights(), np.float64)
        P_tg = oc.params_from_list(os_, w_tg, np.float64)
        x, e, adj, x2, e2 = T._inputs(spec, rng, B, topo)
        action, reward = T._actions_rewards(rng, T._oracle_q(spec, P_eng, x, e, adj), T._oracle_q(spec, P_tg, x2, e2, adj))
        t = dict(x=x, e=e, adj=adj, x2=x2, e2=e2, action=action, reward=reward)
        ref = T._oracle_of(spec, P_eng, P_tg, t, None, "%s step %d" % (what, step),
                           T.MIN_BRANCH_SHARE if step == 0 else T.MIN_BRANCH_SHARE_LATER_STEPS)
        sb = online.to_device(PackedBatch.from_dense(x, e, adj))
        sn = online.to_device(PackedBatch.from_dense(x2, e2, adj))
        _assert_pins(what, online.path_info(sb), want)
        y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
        loss = online.dqn_step(target, sb, sn, torch.from_numpy(action).cuda(), torch.from_numpy(reward).cuda(), T.GAMMA, y_out=y)
        assert_fwd_close(y.cpu().numpy().reshape(B, N, 4), ref['y'], "%s: targets of step %d" % (what, step))
        assert_close(loss.cpu().numpy(), ref['step']['loss'], LOSS_RTOL, LOSS_ATOL, "%s: losses of step %d" % (what, step))
        got = v2xgnn.flat_to_keras_list(spec, online.get_grad_flat())
        g_ref, n_cand, n_flip = assert_grads_match_oracle(got, P_eng, ref['step'], "%s: gradient of step %d" % (what, step))
        r_grad = _grad_ratio(got, oc.params_to_list(g_ref))
        om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_ref))
        history.append(oc.params_to_list(g_ref))
        w_now = online.get_weights()
        assert_weights_after_adam_step(w_now, oc.params_to_list(om.params), history, step, what)
        own_opt.step(oc.param_arrays(own), oc.param_arrays(oc.params_from_list(os_, got, np.float64)))
        for i, (a, b) in enumerate(zip(w_now, oc.params_to_list(own))):
            err = np.abs(a.astype(np.float64) - b)
            worst_own = max(worst_own, float((err / _adam_of_own_gradient_bound(b, C_LR)).max()))
            assert (err <= _adam_of_own_gradient_bound(b, C_LR)).all(), (what, "weights vs Adam of the engine's own gradients", step, i, err.max())
        print("%s step %d: gradient error / bound %.3f; %d ReLU gates at rounding distance, %d taken the kernels' way; weights against "
              "Adam of the engine's own gradients: error / bound %.3f so far" % (what, step, r_grad, n_cand, n_flip, worst_own))
        if step == 1:
            target.copy_weights_from(online)
            w_tg = online.get_weights()
            assert np.array_equal(target.get_flat(), online.get_flat())
    assert online.get_optimizer_state()[2] == 3
    assert target.get_optimizer_state()[2] == 0
    online.close()
    target.close()


# ---------------------------------------------------------------------------------------------------------------- D
def test_d_replayed_graph_rebuilds_its_masks_when_the_topology_changes_in_place():
    """65 links, F = 64, L = 2, per-node weights, 16 graphs; ONE device batch whose xe, row_ptr and col_idx are overwritten in
    place with draw X, then Y, then X (reference topology: the same edge count, other receivers), forward and train_step after
    each.  The second and third calls replay the graphs the first captured: q, losses and the weights after each step must be
    the bits of an eager engine on the same host batch -- masks left over from the call before would show.  The first call
    also holds the bounds of A."""
    import torch
    N, F, L, B = 65, 64, 2, 16
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(4200)
    P = f32_params(spec, rng)
    draws = []
    for _ in range(2):
        x, e, adj = random_inputs(rng, B, N)
        draws.append((x, e, adj, PackedBatch.from_dense(x, e, adj), rng.normal(0, 1.2, size=(B * N, 4))))
    (_, _, _, pbx, _), (_, _, _, pby, _) = draws
    assert pbx.n_edges == pby.n_edges == B * N * (N - 2) and not np.array_equal(pbx.col_idx, pby.col_idx)
    eager, graph = _engine(spec, {}), _engine(spec, {}, use_graph=True)
    for eng in (eager, graph):
        eng.set_weights(oc.params_to_list(P))
    info = graph.path_info(pbx)
    print("D: %s" % " ".join("%s=%s" % kv for kv in sorted(info.items())))
    assert info["graph_layers"] == "layerwise" and info["aggregation"] == DENSE, info
    db = graph.to_device(pbx)
    yd = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    for call, (x, e, adj, pb, noise) in enumerate((draws[0], draws[1], draws[0])):
        db.xe.copy_(torch.from_numpy(pb.xe))
        db.row_ptr.copy_(torch.from_numpy(pb.row_ptr))
        db.col_idx.copy_(torch.from_numpy(pb.col_idx))
        q_e = eager.forward(pb)
        y = (q_e + noise).astype(np.float32)
        yd.copy_(torch.from_numpy(y))
        torch.cuda.synchronize()                            # (the copies ran on the default stream)
        if call == 0:
            w0 = eager.get_weights()
            step = oracle_step(spec, P, rows(x), rows(e), oc.adj_to_csr(adj), y, q_at=q_e)
            assert_fwd_close(q_e, step['q'], "D: forward")
            loss_fb = eager.forward_backward(pb, y)
            assert_close(loss_fb, step['loss'], LOSS_RTOL, LOSS_ATOL, "D: per-output Huber loss")
            g_used, _, _ = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, eager.get_grad_flat()), P, step, "D: gradient")
        with torch.cuda.stream(stream):                     # graphs are only captured on a non-default stream
            q_g = graph.forward(db)
            loss_g = graph.train_step(db, yd)
        stream.synchronize()
        loss_e = eager.train_step(pb, y)
        assert np.array_equal(q_g.cpu().numpy(), q_e), ("q", call)
        assert np.array_equal(loss_g.cpu().numpy(), loss_e), ("losses", call)
        assert np.array_equal(graph.get_flat(), eager.get_flat()), ("weights", call)
        if call == 0:
            om = oc.OracleModel(ospec(spec), P, dtype=np.float64)
            om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_used))
            assert_weights_after_adam_step(graph.get_weights(), oc.params_to_list(om.params), oc.params_to_list(g_used), 0, "D")
            assert not all(np.array_equal(a, b) for a, b in zip(graph.get_weights(), w0))
    assert graph.get_optimizer_state()[2] == 3 and eager.get_optimizer_state()[2] == 3
    graph.check_errors()
    eager.close()
    graph.close()
