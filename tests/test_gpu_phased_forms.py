"""GPU: the phased step (v2x_forward_backward_phase), the mixed forward / backward forms of the fused graph layers and the
ranged Adam (v2x_apply_gradients_range) against the float64 oracle -- what every data-parallel run takes and the single-call
suites do not reach: ragged_fused_bwd(p, c) and dense0_out(p, c) of csrc/v2xgnn.hip are false in a phased call, so a ragged
batch runs the one-launch forward and a LAYER-WISE backward on what that forward left, and the plan's dense0_rides picks the
hand-over layout of a forward whose Dense-0 gradient then stays in the MLP launch.

The cases, their draws and the draws' conditions are in tests/test_phased_forms_host.py (CASES; one seeded draw per case,
nothing redrawn), which checks them on the host with the oracle alone.  Every case asserts the path_info fields and the launch
names of its table entry (profile_read of one eager step), so a case that silently takes another plan fails.

1  the phased step of every case on a device batch, default switches: q, the last phase's losses, bucket k final after phase
   k, buckets tiling the parameters, the gradient against the oracle; the same step as one forward_backward on a second
   engine: losses bit for bit, its gradient against the oracle, and between the two gradients bit equality for the arrays the
   case's table entry names (and why), 2e-5 of the array's scale where Dense-0 rides on k_wgrad in the single call only.
2  V2X_RAGGED_FUSED_BWD=0 in a single call (R1 to R3): fused forward, layer-wise backward; against the oracle, and bit for bit
   section 1's phased gradient (same launches, same order).
3  phases through a replayed hipGraph (F1, R1, A4): three rounds of phased step, apply_gradients, train_step, forward;
   everything bit for bit an eager engine.
4  mixed tile forms (F1, F6): default, V2X_FUSED_SPLIT_FWD=0, V2X_FUSED_SPLIT_BWD=0 and whole tiles in the edge form give q,
   losses and gradients bit for bit; V2X_FRAG_HANDOFF=0 against default on F1.
5  ranged Adam and the fragment-major weight copy in one process (F1, R1 under V2X_RAGGED_SMALL=1, A4): apply_gradients_range
   in half-buckets equals apply_gradients bit for bit, and so do two engines that each apply their own halves and copy the
   other's through param_tensor(); the next forward / forward_backward too.  Step 1 also against Keras Adam.
6  refusals: phase 1 and phases outside [0, n_buckets) on a fresh model; phase k > 0 after only a plain forward().

Measured on an MI355X (all with mlp=train_wg but A7: fwd+bwd).  Columns: graph_layers, aggregation (dense = k_agg_dense, gather =
k_agg, edge / compl = the fused kernels' edge-bitset walk / complement), handoff, dense0_dw of path_info; max|q|; error / bound
of the forward, the losses and the phased gradient; ReLU gates at rounding distance of 0 / taken the kernels' way; share of
residuals on Huber's linear branch; max|g_phased - g_single| / max|g| per array over the graph layers', Dense-0's and
Dense 1..3's arrays; which of them the test holds to bit equality (test_phased_forms_host.py: ALL, DENSE123, DENSE, WIDE).

    A1   layerwise      dense  row-major      k_wgrad        6.34e+03  0.054  0.000  0.019   0 / 0   0.405   0        2.46e-07 0   dense123
    A4   layerwise      dense  row-major      k_mlp_train_wg 1.4e+04   0.129  0.000  0.067   0 / 0   0.405   0        0        0   all
    A10  layerwise      dense  row-major      k_wgrad        4.43e+05  0.010  0.000  0.009   0 / 0   0.411   0        5.66e-07 0   dense123
    A11  layerwise      gather row-major      k_mlp_train_wg 2.63e+04  0.085  0.001  0.039   0 / 0   0.411   0        0        0   all
    A7   layerwise      dense  row-major      k_wide_wgrad   3.8e+04   0.070  0.001  0.042   0 / 0   0.427   0        0        0   wide
    F1   fused(split5)  edge   fragment-major k_wgrad        669       0.108  0.001  0.023   0 / 0   0.410   0        3.37e-07 0   dense123
    F2   fused(split5)  edge   row-major      k_mlp_train_wg 1.41e+03  0.073  0.001  0.017   0 / 0   0.407   0        0        0   all
    F3   fused(split3)  edge   fragment-major k_mlp_train_wg 83.6      0.051  0.000  0.018   0 / 0   0.402   0        0        0   all
    F4   fused(split2)  edge   fragment-major k_mlp_train_wg 63.8      0.054  0.000  0.014   0 / 0   0.416   0        0        0   all
    F5   fused(split5)  edge   row-major      k_wgrad        5.03e+03  0.007  0.000  0.008   0 / 0   0.408   0        1.89e-07 0   dense123
    F6   fused(split5)  edge   fragment-major k_wgrad        735       0.061  0.000  0.027   0 / 0   0.395   0        2.1e-07  0   dense123
    F7   fused          compl  fragment-major k_mlp_train_wg 42.6      0.093  0.000  0.012   0 / 0   0.393   0        0        0   all
    R1   fused(ragged)  dense  row-major      k_mlp_train_wg 3.49e+05  0.020  0.000  0.006   0 / 0   0.398   1.7e-07  0        0   dense
    R2   fused(ragged)  gather row-major      k_mlp_train_wg 985       0.007  0.001  0.008   0 / 0   0.387   1.41e-07 0        0   dense
    R3   fused(ragged)  gather row-major      k_mlp_train_wg 1.83e+05  0.005  0.000  0.013   0 / 0   0.410   1.15e-07 0        0   dense

Launches seen, phased / single call: the layer-wise narrow cases k_node_fwd_embed, k_node_fwd, k_agg_fwd, (k_adj_masks,)
k_mlp_train_wg, k_agg_bwd, k_node_dgrad, k_wgrad_gnn, two k_grad_reduce / one -- and k_mlp_train_wg123 + k_wgrad_gnn_d0 in the
single call of A1 and A10; A7 k_mlp_fwd, k_dense0_fwd, k_mlp_bwd, k_dense0_dgrad, k_wgrad_dense, then k_wgrad_dense0, two
k_wgrad_gnn and k_wgrad_embed phased against one k_wgrad_wide_all; the fused cases k_gnn_fwd_fused, k_mlp_train_wg, k_gnn_bwd_fused,
k_wgrad_gnn (F1, F5, F6 single call: k_mlp_train_wg123, k_wgrad_gnn_d0); the ragged cases k_adj_masks, k_gnn_fwd_ragged,
k_mlp_train_wg, k_wgrad_gnn with L + 1 k_agg_bwd and L k_node_dgrad phased (and in section 2) against one k_gnn_bwd_ragged.
Where the table allows 2e-5 (DENSE123) or leaves arrays to the oracle (WIDE), the graph layers' arrays came out bit for bit at
these sizes; that is measured, not claimed.  F4: the table of cases asked for whole tiles in the complement form at 8 links;
fused_split picks K = 2 there (4 K <= N), so F4 pins split2 in the edge form and F7 (7 links) is the whole-tile complement case.
Section 4, V2X_FRAG_HANDOFF=0 against default on F1: q, losses and every gradient array of the single call and of the phased
step came out bit for bit (max|dg| / max|g| = 0); asserted: q bit for bit, the rest against the oracle.

Mutations of a scratch build (host code of csrc/v2xgnn.hip only), this whole file against each:
  (1) the layer-wise backward (phased wide one included) passes nullptr for the ReLU gate h[s] of launch_agg: section 1 fails
      on A1 A4 A10 A11 A7 R1 R2 R3 and section 2 on R1 R2 R3 (gradient against the oracle, array 0 wholly out of tolerance);
  (2) dense0_out ignores BwdCall::phased: section 1 fails on A1 A10 F1 F5 F6, the cases whose plan says k_wgrad -- bucket 0 does
      keep its value after phase 0, but that value lacks Dense-0's gradient, which fails against the oracle;
  (3) bucket_begin of bucket 0 shifted by 4 floats: 25 tests fail, the tiling of the buckets first;
  (4) launch_reduce_adam fills AdamArgs::pack for a full-range call only: section 5 fails on F1 and R1, eager and graph, at
      `ranged`'s next forward (A4, no copy, passes);
  (5) v2x_param_ptr leaves pk_stale / raw_params alone: section 5 fails on F1 and R1 at rank0's next forward;
  (6) plan_batch keeps compl_sums when only one direction is split: section 4 fails on F1 and F6 -- q of the whole-tile
      forward is off by 3e-4 at |q| of 700 (and path_info shows the complement form, asserted after the values)."""
import types

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnEngine, lib
from oracle import compact as oc
from util import (ospec, assert_fwd_close, assert_close, assert_grads_match_oracle, assert_weights_after_adam_step, FWD_RTOL, FWD_ATOL,
                  GRAD_RTOL, GRAD_ATOL_REL)
from test_gpu_dense0_role import _env
from test_phased_forms_host import CASES, RAGGED_CASES, WIDE_CASE, ALL, DENSE123, DENSE, WIDE, draw, oracle_of

pytestmark = pytest.mark.gpu

LOSS_RTOL, LOSS_ATOL = 2e-4, 1e-6
DENSE0_ROLE_BOUND = 2e-5            # tests/test_gpu_dense0_role.py: another order of the sum over rows, of the array's scale


# ------------------------------------------------------------------------------------------------ helpers
def _engine(spec, switches=None, **kw):
    """an engine that read `switches` when it was created (csrc/knobs.hpp reads the environment once, at v2x_create)"""
    with _env(**(switches or {})):
        return GnnEngine(spec, **kw)


def _started(name, switches=None, **kw):
    d = draw(name)
    eng = _engine(d['spec'], switches, **kw)
    eng.set_weights(oc.params_to_list(d['P']))
    return eng


def _phased(eng, db, yd, n_global=None):
    """all len(grad_buckets()) phases -> ([flat gradient after phase k], losses of the last phase)"""
    nb = len(eng.grad_buckets())
    eng.grad_tensor().zero_()
    snaps, loss = [], None
    for k in range(nb):
        loss = eng.forward_backward_phase(db, yd, k, n_global=n_global)
        assert (loss is None) == (k < nb - 1)
        snaps.append(eng.get_grad_flat())
    return snaps, loss.cpu().numpy()


def _launches(eng, step):
    """{launch name: calls} of one eager `step()` of eng (a profiled engine never replays a graph)"""
    import torch
    torch.cuda.synchronize()
    eng.profile(True)
    step()
    torch.cuda.synchronize()
    names = {k: v[0] for k, v in eng.profile_read().items()}
    eng.profile(False)
    return names


def _assert_pins(what, info, want):
    for k, v in want.items():
        assert info[k] == v, (what, "the case must reach %s=%s" % (k, v), info)


def _assert_launches(what, names, shown, not_shown):
    for k in shown:
        assert names.get(k, 0) > 0, (what, "must launch", k, names)
    for k in not_shown:
        assert k not in names, (what, "must not launch", k, names)


def _ratio(got, ref, rtol, atol):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def _grad_ratio(got_list, ref_list):
    return max(_ratio(a, b, GRAD_RTOL, GRAD_ATOL_REL * (float(np.abs(b).max()) or 1.0)) for a, b in zip(got_list, ref_list)
               if np.asarray(b).any() or np.asarray(a).any())


def _groups(spec):
    """per array of the Keras-shaped list: 'graph' (embed and stages), 'dense0', 'dense123'"""
    n_slots = 1 if spec.share_weights else spec.n_nodes
    first_dense0 = 4 * n_slots * (spec.n_mp_layers + 1)
    n = len(v2xgnn.keras_list_shapes(spec))
    return ["graph" if i < first_dense0 else ("dense0" if i < first_dense0 + 2 * n_slots else "dense123") for i in range(n)]


def _between(spec, a_flat, b_flat):
    """largest |a - b| / max|b| per group of arrays, each array against its own scale -> dict(group: ratio)"""
    worst = dict(graph=0.0, dense0=0.0, dense123=0.0)
    for grp, a, b in zip(_groups(spec), v2xgnn.flat_to_keras_list(spec, a_flat), v2xgnn.flat_to_keras_list(spec, b_flat)):
        scale = max(float(np.abs(b).max()), 1e-30)
        worst[grp] = max(worst[grp], float(np.abs(a - b).max()) / scale)
    return worst


def _training_path_q(name, eng, db):
    """q of eng.forward(db) on the kernels the fit step runs.  A fixed-size batch of at most 256 rows (F4) takes the one-launch
    predict at default switches: its q is held to the oracle here, and the q the targets sit around comes from an engine with
    V2X_SMALL_PREDICT=0, a switch that only `forward` reads."""
    d = draw(name)
    q = eng.forward(db).cpu().numpy()
    spec = d['spec']
    if spec.variable_graphs or spec.n_nodes > 32 or d['pb'].n_rows > 256:
        return q
    step = oracle_of(d, q)[1]
    assert_fwd_close(q, step['q'], name + ": forward of the one-launch predict")
    qe = _started(name, dict(V2X_SMALL_PREDICT=0))
    q = qe.forward(qe.to_device(d['pb'])).cpu().numpy()
    qe.close()
    return q


BETWEEN = {  # same -> per group: 0 = bit for bit, a number = that share of the array's scale, None = through the oracle only
    ALL: dict(graph=0, dense0=0, dense123=0),
    DENSE123: dict(graph=DENSE0_ROLE_BOUND, dense0=DENSE0_ROLE_BOUND, dense123=0),
    DENSE: dict(graph=None, dense0=0, dense123=0),
    WIDE: dict(graph=None, dense0=None, dense123=0),
}


def _assert_between(what, spec, a_flat, b_flat, same):
    for i, (grp, a, b) in enumerate(zip(_groups(spec), v2xgnn.flat_to_keras_list(spec, a_flat), v2xgnn.flat_to_keras_list(spec, b_flat))):
        bound = BETWEEN[same][grp]
        if bound == 0:
            assert np.array_equal(a, b), (what, "array %d (%s) must be bit for bit" % (i, grp), float(np.abs(a - b).max()))
        elif bound is not None:
            scale = max(float(np.abs(b).max()), 1e-30)
            assert np.abs(a - b).max() <= bound * scale, (what, i, grp, float(np.abs(a - b).max()), scale)


def _tiles(buckets, n_params):
    off = 0
    for o, n in sorted(buckets):
        assert o == off and n > 0 and n % 4 == 0, buckets
        off += n
    assert off == n_params, (buckets, n_params)
    assert buckets[0][0] + buckets[0][1] == n_params and buckets[-1][0] == 0, buckets       # Dense layers first, embed last


# ------------------------------------------------------------------------------------------------ 1
_PHASED = {}


def phased_result(name):
    """section 1's phased step of a case, run once and shared (section 2 compares with its gradient): dict(q, y, step (the
    oracle's), yd, snaps, loss, buckets, names, info, g_used, flips)"""
    import torch
    if name in _PHASED:
        return _PHASED[name]
    kind, recipe, want, (shown, not_shown), same = CASES[name]
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    eng = _started(name)
    db = eng.to_device(d['pb'])
    info = eng.path_info(db)
    print("%s: %s" % (name, " ".join("%s=%s" % kv for kv in sorted(info.items()))))
    _assert_pins(name, info, want)
    q = _training_path_q(name, eng, db)
    y, step, share = oracle_of(d, q)
    r_fwd = _ratio(q, step['q'], FWD_RTOL, FWD_ATOL * max(1.0, float(np.abs(step['q']).max())))
    assert_fwd_close(q, step['q'], name + ": forward")
    yd = torch.from_numpy(y).cuda()
    buckets = eng.grad_buckets()
    _tiles(buckets, eng.n_params)
    snaps, loss = _phased(eng, db, yd, ng)
    for k, snap in enumerate(snaps):
        for o, n in buckets[:k + 1]:
            assert np.array_equal(snap[o:o + n], snaps[-1][o:o + n]), (name, "bucket changed after its phase", k, o, n)
    assert_close(loss, step['loss'], LOSS_RTOL, LOSS_ATOL, name + ": losses of the last phase")
    got = v2xgnn.flat_to_keras_list(spec, snaps[-1])
    g_used, n_cand, n_flip = assert_grads_match_oracle(got, P, step, name + ": phased gradient")
    names = _launches(eng, lambda: _phased(eng, db, yd, ng))
    print("%s phased launches: %s" % (name, " ".join("%s:%d" % kv for kv in sorted(names.items()))))
    _assert_launches(name + " phased", names, shown, not_shown)
    assert np.array_equal(eng.get_grad_flat(), snaps[-1]), (name, "the profiled phased step gave another gradient")
    eng.check_errors()
    eng.close()
    print("%s: max|q| %.3g, Huber share %.3f; error / bound: forward %.3f, loss %.3f, phased gradient %.3f; %d gates at rounding "
          "distance, %d taken the kernels' way" % (name, np.abs(step['q']).max(), share, r_fwd,
                                                   _ratio(loss, step['loss'], LOSS_RTOL, LOSS_ATOL),
                                                   _grad_ratio(got, oc.params_to_list(g_used)), n_cand, n_flip))
    _PHASED[name] = dict(q=q, y=y, step=step, snaps=snaps, loss=loss, buckets=buckets, names=names, info=info)
    return _PHASED[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_1_phased_step_vs_oracle_and_single_call(name):
    import torch
    kind, recipe, want, (shown, not_shown), same = CASES[name]
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    r = phased_result(name)
    one = _started(name)
    db = one.to_device(d['pb'])
    yd = torch.from_numpy(r['y']).cuda()
    loss1 = one.forward_backward(db, yd, n_global=ng).cpu().numpy()
    g1 = one.get_grad_flat()
    names1 = _launches(one, lambda: one.forward_backward(db, yd, n_global=ng))
    print("%s single-call launches: %s" % (name, " ".join("%s:%d" % kv for kv in sorted(names1.items()))))
    one.check_errors()
    one.close()
    if want.get("dense0_dw") == "k_wgrad":                      # the two calls differ in where Dense-0's weight gradient is summed
        _assert_launches(name + " single call", names1, ("k_mlp_train_wg123", "k_wgrad_gnn_d0"), ("k_mlp_train_wg",))
    if kind == "ragged":
        _assert_launches(name + " single call", names1, ("k_gnn_fwd_ragged", "k_gnn_bwd_ragged"), ("k_agg_bwd", "k_node_dgrad"))
    if name == WIDE_CASE:
        _assert_launches(name + " single call", names1, ("k_wgrad_wide_all",), ())
    diff = _between(spec, r['snaps'][-1], g1)
    print("%s: max|g_phased - g_single| / max|g| per array: graph layers %.3g, Dense-0 %.3g, Dense 1..3 %.3g (%s)"
          % (name, diff['graph'], diff['dense0'], diff['dense123'], same))
    assert np.array_equal(loss1, r['loss']), (name, "losses: the phased forward is the single call's")
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, g1), P, r['step'], name + ": single-call gradient")
    _assert_between(name + ": phased against single call", spec, r['snaps'][-1], g1, same)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", RAGGED_CASES)
def test_2_ragged_fused_forward_with_layerwise_backward_in_a_single_call(name):
    """V2X_RAGGED_FUSED_BWD=0: run_backward takes the pair of launches the phases take -- k_gnn_fwd_ragged's h[s] / gha / masks
    read by k_agg_bwd and k_node_dgrad -- so its gradient is the phased one bit for bit, bucket by bucket"""
    import torch
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    r = phased_result(name)
    eng = _started(name, dict(V2X_RAGGED_FUSED_BWD=0))
    db = eng.to_device(d['pb'])
    _assert_pins(name, eng.path_info(db), CASES[name][2])
    q = eng.forward(db).cpu().numpy()
    assert np.array_equal(q, r['q'])                            # the switch does not touch the forward: the same targets serve
    assert_fwd_close(q, r['step']['q'], name + ": forward")
    yd = torch.from_numpy(r['y']).cuda()
    loss = eng.forward_backward(db, yd, n_global=ng).cpu().numpy()
    g = eng.get_grad_flat()
    names = _launches(eng, lambda: eng.forward_backward(db, yd, n_global=ng))
    eng.check_errors()
    eng.close()
    _assert_launches(name, names, ("k_gnn_fwd_ragged", "k_agg_bwd", "k_node_dgrad"), ("k_gnn_bwd_ragged",))
    assert_close(loss, r['step']['loss'], LOSS_RTOL, LOSS_ATOL, name + ": loss")
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, g), P, r['step'], name + ": gradient, layer-wise backward in one call")
    assert np.array_equal(loss, r['loss'])
    for k, (o, n) in enumerate(r['buckets']):
        assert np.array_equal(g[o:o + n], r['snaps'][-1][o:o + n]), (name, "bucket %d differs from the phased step's" % k,
                                                                      float(np.abs(g[o:o + n] - r['snaps'][-1][o:o + n]).max()))


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["F1", "R1", "A4"])
def test_3_phases_through_a_replayed_graph_equal_eager(name):
    """keys 5 / 6 (20 + k: wide) of run_maybe_graph between calls of other kinds (train_step: 2, forward: 1): a replay must
    restore frag_live and the layers' slab counts as its capture left them"""
    import torch
    d = draw(name)
    spec, ng = d['spec'], d['n_global']
    eager, graph = _started(name), _started(name, use_graph=True)
    stream = torch.cuda.Stream()
    db_e, db_g = eager.to_device(d['pb']), graph.to_device(d['pb'])
    q0 = eager.forward(db_e).cpu().numpy()
    yd = torch.from_numpy((q0 + d['noise']).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    for rnd in range(3):
        out = []
        for eng, db in ((eager, db_e), (graph, db_g)):
            with torch.cuda.stream(stream):                     # graphs are only captured on a non-default stream
                snaps, loss = _phased(eng, db, yd, ng)
                eng.apply_gradients()
                w1 = eng.get_flat()
                loss_fit = eng.train_step(db, yd, n_global=ng).cpu().numpy()
                q = eng.forward(db).cpu().numpy()
            stream.synchronize()
            m, v, it = eng.get_optimizer_state()
            out.append(dict(snaps=snaps, loss=loss, w1=w1, loss_fit=loss_fit, q=q, w2=eng.get_flat(), m=m, v=v, it=it))
        e, g = out
        assert e['it'] == g['it'] == 2 * (rnd + 1)
        for k, (a, b) in enumerate(zip(e['snaps'], g['snaps'])):
            assert np.array_equal(a, b), (name, rnd, "gradient after phase %d" % k, float(np.abs(a - b).max()))
        for key in ("loss", "w1", "loss_fit", "q", "w2", "m", "v"):
            assert np.array_equal(e[key], g[key]), (name, rnd, key, float(np.abs(e[key] - g[key]).max()))
        assert np.all(np.isfinite(e['w2'])) and not np.array_equal(e['w1'], e['w2'])
    graph.check_errors()
    eager.close()
    graph.close()


# ------------------------------------------------------------------------------------------------ 4
MIXED = (("default", {}, "fused(split5)"),
         ("whole-tile forward", dict(V2X_FUSED_SPLIT_FWD=0), "fused(split5)"),
         ("whole-tile backward", dict(V2X_FUSED_SPLIT_BWD=0), "fused(split5)"),
         ("whole tiles, edge form", dict(V2X_FUSED_SPLIT=0, V2X_FUSED_COMPL=0), "fused"))


@pytest.mark.parametrize("name", ["F1", "F6"])
def test_4_mixed_tile_forms_are_bit_for_bit(name):
    """split tiles == whole tiles, also when only ONE direction is split: plan_batch then keeps both in the edge
    form, because the two kernels hand the rows' in-neighbour sets over"""
    import torch
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    res = []
    for what, switches, layers in MIXED:
        eng = _started(name, switches)
        db = eng.to_device(d['pb'])
        info = eng.path_info(db)
        q = eng.forward(db).cpu().numpy()
        if not res:
            y, step, _ = oracle_of(d, q)
            yd = torch.from_numpy(y).cuda()
        loss = eng.forward_backward(db, yd, n_global=ng).cpu().numpy()
        g = eng.get_grad_flat()
        snaps, loss_ph = _phased(eng, db, yd, ng)
        eng.check_errors()
        eng.close()
        res.append(dict(q=q, loss=loss, g=g, g_ph=snaps[-1], loss_ph=loss_ph, info=info))
    assert_fwd_close(res[0]['q'], step['q'], name + ": forward")
    assert_close(res[0]['loss'], step['loss'], LOSS_RTOL, LOSS_ATOL, name + ": loss")
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, res[0]['g']), P, step, name + ": gradient")
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, res[0]['g_ph']), P, step, name + ": phased gradient")
    for (what, _, _), r in zip(MIXED[1:], res[1:]):
        for key in ("q", "loss", "g", "loss_ph", "g_ph"):
            assert np.array_equal(r[key], res[0][key]), (name, what, key, float(np.abs(r[key] - res[0][key]).max()))
    for (what, _, layers), r in zip(MIXED, res):                # (after the values: a wrong form must show in them, not only here)
        info = r['info']
        assert info["graph_layers"] == layers and info["aggregation"] == "edge-bitset-walk" and info["handoff"] == "fragment-major", (what, info)


def test_4_row_major_hand_over_against_fragment_major():
    """V2X_FRAG_HANDOFF=0 on F1: h_L / a_L / gha cross between the fused kernels and the MLP launch row-major.  The layout
    cannot change a graph layer's forward value or q; the weight-gradient launches read other row chunks, so the gradients meet
    through the oracle"""
    import torch
    name = "F1"
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    res = []
    for switches, handoff in (({}, "fragment-major"), (dict(V2X_FRAG_HANDOFF=0), "row-major")):
        eng = _started(name, switches)
        db = eng.to_device(d['pb'])
        info = eng.path_info(db)
        assert info["handoff"] == handoff and info["graph_layers"] == "fused(split5)" and info["dense0_dw"] == "k_wgrad", info
        q = eng.forward(db).cpu().numpy()
        if not res:
            y, step, _ = oracle_of(d, q)
            yd = torch.from_numpy(y).cuda()
        loss = eng.forward_backward(db, yd, n_global=ng).cpu().numpy()
        g = eng.get_grad_flat()
        snaps, loss_ph = _phased(eng, db, yd, ng)
        eng.check_errors()
        eng.close()
        res.append(dict(q=q, loss=loss, g=g, g_ph=snaps[-1], loss_ph=loss_ph))
    frag, row = res
    d1, d2 = _between(spec, row['g'], frag['g']), _between(spec, row['g_ph'], frag['g_ph'])
    print("F1 row-major against fragment-major, max|dg| / max|g| per array: single call graph %.3g Dense-0 %.3g Dense 1..3 %.3g; "
          "phased graph %.3g Dense-0 %.3g Dense 1..3 %.3g; losses equal: %s / %s"
          % (d1['graph'], d1['dense0'], d1['dense123'], d2['graph'], d2['dense0'], d2['dense123'],
             np.array_equal(row['loss'], frag['loss']), np.array_equal(row['loss_ph'], frag['loss_ph'])))
    assert np.array_equal(row['q'], frag['q'])
    assert_fwd_close(row['q'], step['q'], "row-major: forward")
    for r, what in ((row, "row-major"), (frag, "fragment-major")):
        for key in ("loss", "loss_ph"):
            assert_close(r[key], step['loss'], LOSS_RTOL, LOSS_ATOL, "%s: %s" % (what, key))
        for key in ("g", "g_ph"):
            assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, r[key]), P, step, "%s: %s" % (what, key))


# ------------------------------------------------------------------------------------------------ 5
def _half_slices(eng):
    """per bucket, in bucket order: [(offset, count) of rank 0's part, of rank 1's part] by DataParallelTrainer._slice_of at
    world 2, or [(offset, count)] -- the whole bucket, which every rank updates -- where that returns None"""
    from v2xgnn.dp import DataParallelTrainer
    out = []
    for off, n in eng.grad_buckets():
        sl = [DataParallelTrainer._slice_of(types.SimpleNamespace(world=2, rank=r), n) for r in (0, 1)]
        out.append([(off, n)] if sl[0] is None else [(off + first, count) for first, count in sl])
    return out


RANGED = [("F1", {}, False), ("F1", {}, True), ("R1", dict(V2X_RAGGED_SMALL=1), False), ("R1", dict(V2X_RAGGED_SMALL=1), True), ("A4", {}, False)]


@pytest.mark.parametrize("name,switches,use_graph", RANGED)
def test_5_ranged_adam_keeps_the_fragment_major_copy(name, switches, use_graph):
    """plain: apply_gradients.  ranged: apply_gradients_range on every bucket's two halves, advance_iteration on the step's
    first call only.  rank0 / rank1: each its own halves, the other's copied in through param_tensor() (the all-gather).  Adam
    is element-wise and lr_t comes from the same host iteration: weights (all), moments (plain and ranged; a rank's on its own
    slices, untouched elsewhere) and the next forward / forward_backward bit for bit.  F1 and R1 (V2X_RAGGED_SMALL=1) read their
    graph-layer weights from the fragment-major copy pk_fwd / pk_bwd, which a ranged update has to write and a raw parameter
    write has to mark stale; A4 (layer-wise) has no copy.  use_graph: rank0 / rank1 and ranged replay captured steps."""
    import torch
    d = draw(name)
    spec, P, ng = d['spec'], d['P'], d['n_global']
    os_ = ospec(spec)
    plain = _started(name, switches)
    ranged, rank0, rank1 = (_started(name, switches, use_graph=use_graph) for _ in range(3))
    engines = (plain, ranged, rank0, rank1)
    slices = _half_slices(plain)
    assert sum(c for b in slices for _, c in b) == plain.n_params and any(len(b) == 2 for b in slices)
    own = [np.zeros(plain.n_params, bool), np.zeros(plain.n_params, bool)]
    for b in slices:
        for r in (0, 1):
            o, c = b[r] if len(b) == 2 else b[0]
            own[r][o:o + c] = True
    stream = torch.cuda.Stream()
    dbs = [eng.to_device(d['pb']) for eng in engines]
    info = plain.path_info(dbs[0])
    if name == "R1":
        assert info["graph_layers"] == "fused(ragged)", info
    else:
        _assert_pins(name, info, CASES[name][2])
    q0 = plain.forward(dbs[0]).cpu().numpy()
    yd = torch.from_numpy((q0 + d['noise']).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        p0, p1 = rank0.param_tensor(), rank1.param_tensor()
        for step in range(3):
            fb = []
            for eng, db in zip(engines, dbs):
                loss = eng.forward_backward(db, yd, n_global=ng).cpu().numpy()
                fb.append((loss, eng.get_grad_flat()))
            for (loss, g), who in zip(fb[1:], ("ranged", "rank0", "rank1")):
                assert np.array_equal(loss, fb[0][0]) and np.array_equal(g, fb[0][1]), (name, step, who, "forward_backward")
            w_before = plain.get_flat()
            plain.apply_gradients()
            first = True
            for b in slices:
                for o, c in b:
                    ranged.apply_gradients_range(o, c, first)
                    first = False
            first = True
            for b in slices:
                o0, c0 = b[0]
                o1, c1 = b[-1]
                rank0.apply_gradients_range(o0, c0, first)
                rank1.apply_gradients_range(o1, c1, first)
                first = False
                if len(b) == 2:                                 # the all-gather: each half travels to the other engine
                    p1[o0:o0 + c0].copy_(p0[o0:o0 + c0])
                    p0[o1:o1 + c1].copy_(p1[o1:o1 + c1])
            stream.synchronize()
            w = plain.get_flat()
            m, v, it = plain.get_optimizer_state()
            assert it == step + 1 and not np.array_equal(w, w_before)
            if step == 0:
                own_g = oc.params_from_list(os_, v2xgnn.flat_to_keras_list(spec, fb[0][1]), np.float64)
                om = oc.OracleModel(os_, P, dtype=np.float64)
                om.opt.step(oc.param_arrays(om.params), oc.param_arrays(own_g))
                assert_weights_after_adam_step(plain.get_weights(), oc.params_to_list(om.params), oc.params_to_list(own_g), 0, name)
            for eng, who in ((ranged, "ranged"), (rank0, "rank0"), (rank1, "rank1")):
                assert np.array_equal(eng.get_flat(), w), (name, step, who, "weights", float(np.abs(eng.get_flat() - w).max()))
                m2, v2, it2 = eng.get_optimizer_state()
                assert it2 == it, (name, step, who, it2)
                mine = np.ones_like(own[0]) if who == "ranged" else own[int(who[-1])]
                assert np.array_equal(m2[mine], m[mine]) and np.array_equal(v2[mine], v[mine]), (name, step, who, "moments")
                assert not m2[~mine].any() and not v2[~mine].any(), (name, step, who, "moments outside the rank's slices")
            qs = [eng.forward(db).cpu().numpy() for eng, db in zip(engines, dbs)]
            for q, who in zip(qs[1:], ("ranged", "rank0", "rank1")):
                assert np.array_equal(q, qs[0]), (name, step, who, "the next forward", float(np.abs(q - qs[0]).max()))
            assert not np.array_equal(qs[0], q0)
    for eng in engines:
        eng.check_errors()
        eng.close()


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", ["F1", WIDE_CASE])
def test_6_refusals(name):
    """a fresh model refuses phase 1 and a phase outside [0, n_buckets); a model that only ran a plain forward() refuses every
    phase k > 0 -- the activations are there, dz / gha of THIS step's phase 0 are not"""
    import torch
    d = draw(name)
    eng = _started(name)
    db = eng.to_device(d['pb'])
    yd = torch.zeros((d['pb'].n_rows, 4), dtype=torch.float32, device="cuda")
    nb = len(eng.grad_buckets())
    assert nb == (d['spec'].n_mp_layers + 2 if name == WIDE_CASE else 2)
    with pytest.raises(lib.V2XError, match="phase 1 before phase 0"):
        eng.forward_backward_phase(db, yd, 1)
    for k in (-1, nb):
        with pytest.raises(lib.V2XInvalidArgument, match=r"phase must be in \[0, %d\)" % nb):
            eng.forward_backward_phase(db, yd, k)
    eng.forward(db)
    for k in range(1, nb):
        with pytest.raises(lib.V2XError, match="phase %d before phase 0" % k):
            eng.forward_backward_phase(db, yd, k)
    # ... and after a whole single-call step, and after phase 0 followed by a forward
    eng.forward_backward(db, yd)
    with pytest.raises(lib.V2XError, match="phase 1 before phase 0"):
        eng.forward_backward_phase(db, yd, 1)
    assert eng.forward_backward_phase(db, yd, 0) is None
    eng.forward(db)
    with pytest.raises(lib.V2XError, match="phase 1 before phase 0"):
        eng.forward_backward_phase(db, yd, 1)
    # the phases in order still run
    snaps, loss = _phased(eng, db, yd)
    assert np.all(np.isfinite(loss)) and np.all(np.isfinite(snaps[-1]))
    eng.check_errors()
    eng.close()
