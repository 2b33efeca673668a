"""GPU: the model at 5 to 8 message-passing layers (v2x_create accepts 1..8) on every path whose plan changes with depth,
against the float64 oracle -- forward, per-output Huber loss and EVERY gradient array, judged as tests/test_gpu_shapes.py
judges (tests/util.py: plain fp32 tolerances, ReLU gates at rounding distance of 0 identified explicitly, nothing redrawn).

Every case first asserts the path it is meant to exercise (path_info, and launch counts from profile_read where the branch
is a launch count), then that its draw is informative: a deep ReLU stack with Glorot weights can die out, and a comparison
in which the deep stages' gradients are all zero proves nothing.

The branches (csrc/v2xgnn.hip):
  1. the graph-layer weight gradients that do not fit one launch (wgrad_gnn_all without embed_rides: WG_MAX_ROLES = 8
     stage roles per k_wgrad_gnn grid) -- one launch at L = 7, two at L = 8;
  2. the wide model (F >= 128) at L >= 5: no merged weight-gradient launch, no Adam in its epilogue, L + 2 phase buckets;
  3. the fused whole-tile graph layers at L = 5..8, complement and edge-bitset-walk aggregation, both hand-overs;
  4. k_predict_small at L = 8 (the top of the 4-bit stage field of its exchange tags);
  5. the ragged fused forward / backward at L = 6 and 8;
  6. the depth cut-offs of the default path: no split tiles above L = 3, Dense-0 as a k_wgrad role at L = 4."""
import contextlib
import os

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine
from oracle import compact as oc
from oracle.keras_semantics import KerasAdam
from util import (ospec, f32_params, random_inputs, oracle_step, assert_fwd_close, assert_close, assert_grads_match_oracle,
                  FWD_RTOL, FWD_ATOL)

pytestmark = pytest.mark.gpu

# An informative draw (asserted, never redrawn): at least LIVE_MIN of the units of the deepest ReLU of the graph layers
# (stage L - 1: stage L is linear) are live in the oracle's forward, and the embed stage's largest weight gradient is at
# least EMBED_MIN of the largest gradient of the model (the signal reaches the bottom of the stack).  Observed: 0.37-0.55 live,
# ratios 9e-3 .. 1.
LIVE_MIN = 0.10
EMBED_MIN = 1e-3
DQ_LIVE_MIN = 0.99      # ... and (nearly) every output carries a loss gradient


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _draw(N, F, L, shared, B, topo, seed, density=0.3, with_nbr=False):
    """-> spec, fp32-exact params, x, e, packed batch, graph (node-row CSR of the oracle), rng
    with_nbr: the batch carries a Neighbor_Input ~ N(0, 0.5) (test_gpu_kernels._setup's draw); its node rows are pb.nbr"""
    rng = np.random.default_rng(seed)
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    P = f32_params(spec, rng)
    x, e, adj = random_inputs(rng, B, N, ref_topology=topo, density=density)
    nbr = rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32) if with_nbr else None
    pb = PackedBatch.from_dense(x, e, adj, nbr)
    graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
    return spec, P, x.reshape(B * N, -1), e.reshape(B * N, -1), pb, graph, rng


def _engine(spec, P, **create_env):
    """V2X_SMALL_PREDICT=0: forward() on the training path's kernels (the loss is differentiated at its q)"""
    with _env(V2X_SMALL_PREDICT=0, **create_env):
        eng = GnnEngine(spec)
    eng.set_weights(oc.params_to_list(P))
    return eng


def _assert_informative(step, L, what):
    h = step['cache']['h']
    live = float((h[L - 1] > 0).mean())
    assert np.all(np.isfinite(step['q'])), (what, "q not finite")
    assert (step['dq'] != 0).mean() >= DQ_LIVE_MIN, (what, "%.3f of the outputs carry a loss gradient" % (step['dq'] != 0).mean())
    assert live >= LIVE_MIN, (what, "stage %d: %.3f of the ReLU units live" % (L - 1, live))
    g = step['grads']
    g_max = max(float(np.abs(a).max()) for a in oc.param_arrays(g))
    g_embed = max(float(np.abs(g['gnn'][0][k]).max()) for k in ('W1', 'W2', 'b'))
    assert g_embed >= EMBED_MIN * g_max, (what, "embed gradient %.3e vs largest %.3e" % (g_embed, g_max))
    return live, g_embed / g_max


def _parity(spec, P, x, e, pb, graph, rng, eng, what, n_global=None):
    """forward / loss / every gradient of one forward_backward against the oracle (with the batch's Neighbor_Input, if it
    carries one); -> names of the launches of that step"""
    L = spec.n_mp_layers
    q = eng.forward(pb)
    # targets around the kernels' own q as in test_gpu_shapes._check, the spread widened with |q|: deep stacks on dense
    # graphs reach |q| ~ 1e9, where q + N(0, 1.2) rounds back to q in fp32 and those rows would have no loss gradient
    y = (q + rng.normal(0, 1.2, size=q.shape) * np.maximum(1.0, 1e-3 * np.abs(q))).astype(np.float32)
    step = oracle_step(spec, P, x, e, graph, y, q_at=q, n_denominator=n_global, nbr=pb.nbr)
    live, ratio = _assert_informative(step, L, what)
    assert_fwd_close(q, step['q'], what + ": forward")
    eng.profile(True)
    loss = eng.forward_backward(pb, y, n_global=n_global)
    names = eng.profile_read()
    eng.profile(False)
    assert_close(loss, step['loss'], 2e-4, 1e-6, what + ": per-output Huber loss")
    _, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, eng.get_grad_flat()), P, step, what)
    print("%s: live(stage %d) %.3f  |g_embed|/|g|max %.2e  ReLU gates taken the kernels' way %d (candidates examined %d)"
          % (what, L - 1, live, ratio, n_flip, n_cand))
    return names


# ------------------------------------------------------------------------------------------------ 3. fused whole tiles
FUSED = [  # N, F, L, shared, B, reference topology (else random, density 0.3), aggregation, hand-over
    (20, 64, 8, False, 48, True, "complement", "fragment-major"),
    (20, 64, 8, False, 33, True, "complement", "row-major"),
    (12, 32, 6, False, 40, False, "edge-bitset-walk", None),
    (28, 16, 5, True, 17, False, "edge-bitset-walk", None),
    (4, 16, 8, False, 64, True, "complement", None),
]


@pytest.mark.parametrize("N,F,L,shared,B,topo,agg,handoff", FUSED)
def test_fused_whole_tiles_at_depth(N, F, L, shared, B, topo, agg, handoff):
    """k_gnn_fwd_fused / k_gnn_bwd_fused with L a runtime loop bound up to FZ_MAXL: stage pointers, ReLU' gate arrays and
    turn flags of FZ_MAXL + 1 stages."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, topo, seed=11 * N + F + L + B)
    eng = _engine(spec, P)
    info = eng.path_info(pb)
    assert info["graph_layers"] == "fused" and info["aggregation"] == agg, info
    if handoff:
        assert info["handoff"] == handoff, info
    names = _parity(spec, P, x, e, pb, graph, rng, eng, "fused N=%d F=%d L=%d B=%d" % (N, F, L, B))
    assert "k_gnn_fwd_fused" in names and "k_gnn_bwd_fused" in names, names
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. depth cut-offs
@pytest.mark.parametrize("L", [4, 5])
def test_no_split_tiles_above_three_layers(L):
    """fused_split takes K workgroups per 16-graph tile only for L <= 3: the batch that splits at L = 3 runs whole tiles at
    L = 4 and 5."""
    N, F, B = 20, 64, 48
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=500 + L)
    shallow = GnnEngine(GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=3))
    assert shallow.path_info(pb)["graph_layers"].startswith("fused(split"), shallow.path_info(pb)
    shallow.close()
    eng = _engine(spec, P)
    info = eng.path_info(pb)
    assert info["graph_layers"] == "fused" and info["aggregation"] == "complement", info
    _parity(spec, P, x, e, pb, graph, rng, eng, "no split L=%d" % L)
    eng.close()


def test_dense0_role_at_four_layers():
    """At F = 64, L = 4 divides the embed gradient's 4 output tiles (embed_rides), so Dense-0's weight gradient moves into
    k_wgrad as fragment-major roles (dense0_rides).  Equal to the in-kernel form (V2X_MLP_WG0=1) up to the order of the sums
    over rows, and both equal to the oracle."""
    from test_gpu_dense0_role import _grads
    N, F, L, B = 20, 64, 4, 64
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=904)
    weights = oc.params_to_list(P)
    probe = _engine(spec, P)
    q0 = probe.forward(pb)
    info = probe.path_info(pb)
    probe.close()
    assert info["handoff"] == "fragment-major" and info["dense0_dw"] == "k_wgrad", info
    y = (q0 + rng.normal(0, 1.2, size=q0.shape)).astype(np.float32)
    info_in, q_in, loss_in, g_in, names_in = _grads(spec, weights, pb, y, 1)
    info_out, q_out, loss_out, g_out, names_out = _grads(spec, weights, pb, y, 0)
    assert info_in["dense0_dw"] == "k_mlp_train_wg" and "k_mlp_train_wg" in names_in and "k_wgrad_gnn_d0" not in names_in, names_in
    assert info_out["dense0_dw"] == "k_wgrad" and {"k_mlp_train_wg123", "k_wgrad_gnn_d0"} <= names_out, (info_out, names_out)
    assert np.array_equal(q_in, q_out) and np.array_equal(loss_in, loss_out)
    li, lo = v2xgnn.flat_to_keras_list(spec, g_in), v2xgnn.flat_to_keras_list(spec, g_out)
    first_dense0 = 4 * N * (L + 1)
    for i, (a, b) in enumerate(zip(li, lo)):
        if i < first_dense0 + 2 * N:
            scale = max(np.abs(a).max(), 1e-30)
            assert np.abs(a - b).max() <= 2e-5 * scale, (i, np.abs(a - b).max(), scale)
        else:
            assert np.array_equal(a, b), i
    ref = oracle_step(spec, P, x, e, graph, y, q_at=q_out)
    _assert_informative(ref, L, "Dense-0 role")
    assert_fwd_close(q_out, ref['q'], "forward")
    assert_close(loss_out, ref['loss'], 2e-4, 1e-6, "loss")
    assert_grads_match_oracle(lo, P, ref, "Dense-0 as a k_wgrad role")
    assert_grads_match_oracle(li, P, ref, "Dense-0 in k_mlp_train_wg")


# ------------------------------------------------------------------------------------------------ 1. multi-launch weight gradients
LAYERWISE = [  # N, F, L, shared, B, reference topology, k_wgrad_gnn launches per step
    (33, 64, 7, False, 17, True, 1),      # L + 1 = 8 stage roles: the grid is full on the last stage
    (40, 32, 8, True, 130, False, 2),     # 9 roles: 8 + 1
    (30, 64, 8, False, 32, True, 2),
]


@pytest.mark.parametrize("N,F,L,shared,B,topo,n_launch", LAYERWISE)
def test_layerwise_multi_launch_weight_gradients(N, F, L, shared, B, topo, n_launch):
    """wgrad_gnn_all without embed_rides: at most WG_MAX_ROLES stage roles per k_wgrad_gnn grid, the row chunks of a launch
    sized by the work of the stages IN that launch."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, topo, seed=13 * N + F + L + B)
    eng = _engine(spec, P)
    assert eng.path_info(pb)["graph_layers"] == "layerwise", eng.path_info(pb)
    names = _parity(spec, P, x, e, pb, graph, rng, eng, "layerwise N=%d F=%d L=%d B=%d" % (N, F, L, B))
    assert names.get("k_wgrad_gnn", (0, 0))[0] == n_launch, names
    assert "k_wgrad_all" not in names and "k_wgrad_gnn_d0" not in names, names
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. few-graph predict
SMALL = [  # N, F, L, shared, B, reference topology
    (20, 64, 8, False, 12, True), (32, 16, 8, False, 8, False), (7, 32, 5, True, 5, False),
]


@pytest.mark.parametrize("N,F,L,shared,B,topo", SMALL)
def test_small_predict_at_depth(N, F, L, shared, B, topo):
    """k_predict_small: tag = 16 * epoch + stage + 1 (L = 8: the top of the stage field), hbuf slabs of L + 1 stages."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, topo, seed=17 * N + F + L + B)
    small = GnnEngine(spec)
    small.set_weights(oc.params_to_list(P))
    plain = _engine(spec, P)
    q_ref, cache = oc.forward(ospec(spec), P, x.astype(np.float64), e.astype(np.float64),
                              oc.csr_to_matrix(*graph, dtype=np.float64))
    live = float((cache['h'][L - 1] > 0).mean())
    assert np.all(np.isfinite(q_ref)) and live >= LIVE_MIN, live
    qp = plain.forward(pb)
    small.profile(True)
    q = small.forward(pb)
    names = small.profile_read()
    small.profile(False)
    assert "k_predict_small" in names and "k_gnn_fwd_fused" not in names, names
    scale = max(1.0, float(np.abs(q_ref).max()))
    assert_fwd_close(q, q_ref, "small predict vs oracle")
    assert np.all(np.abs(q - qp) <= FWD_RTOL * np.abs(qp) + FWD_ATOL * scale), "small predict vs training path"
    for rep in range(3):
        assert np.array_equal(small.forward(pb), q), "predict %d not bitwise repeatable" % rep
    small.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 2. wide, unmerged
WIDE = [  # N, F, L, shared, B, reference topology
    (12, 128, 5, False, 40, True), (16, 256, 8, True, 16, True),
]


@pytest.mark.parametrize("N,F,L,shared,B,topo", WIDE)
def test_wide_unmerged_weight_gradients(N, F, L, shared, B, topo):
    """L + 2 > WWM_ROLES: one k_wide_wgrad launch per layer instead of the merged k_wgrad_wide_all."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, topo, seed=19 * N + F + L + B)
    eng = _engine(spec, P)
    assert eng.path_info(pb)["graph_layers"] == "layerwise", eng.path_info(pb)
    names = _parity(spec, P, x, e, pb, graph, rng, eng, "wide N=%d F=%d L=%d B=%d" % (N, F, L, B))
    assert "k_wgrad_wide_all" not in names, names
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. ragged
@pytest.mark.parametrize("F,L,n_graphs", [(64, 8, 40), (32, 6, 60)])
def test_ragged_fused_at_depth(F, L, n_graphs):
    """kernels_ragged.hpp: stage weights, h / a / dpre pointers for FZ_MAXL + 1 stages; graph sizes 1..128."""
    from test_gpu_fused import _ragged_batch
    rng = np.random.default_rng(31 * F + L)
    sizes = [int(n) for n in rng.integers(1, 129, size=n_graphs)]
    spec = GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, sizes, 'mixed')
    P = f32_params(spec, rng)
    eng = GnnEngine(spec)
    eng.set_weights(oc.params_to_list(P))
    assert eng.path_info(pb)["graph_layers"] == "fused(ragged)", eng.path_info(pb)
    _parity(spec, P, x, e, pb, (offs, pb.row_ptr, pb.col_idx), rng, eng, "ragged F=%d L=%d" % (F, L), n_global=pb.n_rows)
    eng.check_errors()
    eng.close()


# ------------------------------------------------------------------------------------------------ fit steps and replay at depth
FIT = [  # N, F, L, shared, B, graph layers
    (20, 64, 8, False, 32, "fused"), (40, 32, 8, True, 17, "layerwise"), (12, 128, 6, False, 24, "layerwise"),
]


@pytest.mark.parametrize("N,F,L,shared,B,layers", FIT)
def test_fit_steps_at_depth_equal_keras_adam(N, F, L, shared, B, layers):
    """Three train_step calls equal (a) forward_backward + apply_gradients and (b) the oracle's Keras Adam applied to the
    engine's own gradients (as test_gpu_model.test_wide_fit_step_with_adam_in_the_weight_gradient_launch judges).  The wide
    model at L = 6 has no Adam in a weight-gradient epilogue: k_reduce_adam updates every parameter."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, True, seed=23 * N + F + L + B)
    y = rng.normal(0.0, 1.0, size=(B * N, 4)).astype(np.float32)
    fused, split = _engine(spec, P), _engine(spec, P)
    assert fused.path_info(pb)["graph_layers"] == layers, fused.path_info(pb)
    ref = oc.cast_params(P, np.float64)
    opt = KerasAdam()
    for step in range(3):
        if step == 0:
            fused.profile(True)
        lf = fused.train_step(pb, y)
        if step == 0:
            names = fused.profile_read()
            fused.profile(False)
            if F >= 128:
                assert "k_wgrad_wide_all" not in names and "k_reduce_adam" in names, names
        ls = split.forward_backward(pb, y)
        g = v2xgnn.flat_to_keras_list(spec, split.get_grad_flat())
        split.apply_gradients()
        assert np.allclose(lf, ls, rtol=1e-5, atol=1e-7), (step, lf, ls)
        err = np.abs(fused.get_flat() - split.get_flat())
        tol = 2e-6 if step == 0 else 1e-5
        assert (err > tol).mean() <= (0.0 if step == 0 else 1e-5), (step, err.max(), (err > tol).sum())
        opt.step(oc.param_arrays(ref), oc.param_arrays(oc.params_from_list(ospec(spec), g, np.float64)))
        for i, (a, b) in enumerate(zip(fused.get_weights(), oc.params_to_list(ref))):
            e2 = np.abs(a.astype(np.float64) - b)
            assert (e2 > 1e-5 * (step + 1)).mean() <= (0.0 if step == 0 else 1e-4), (step, i, e2.max())
    assert fused.get_optimizer_state()[2] == split.get_optimizer_state()[2] == 3
    fused.close()
    split.close()


def test_graph_replay_at_eight_layers_matches_eager_bitwise():
    """A captured fit step of the L = 8 layer-wise model holds two k_wgrad_gnn launches; its replays equal the eager steps
    bit for bit."""
    import torch
    N, F, L, B = 30, 64, 8, 32
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=808)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    res = []
    for use_graph in (False, True):
        eng = GnnEngine(spec, use_graph=use_graph)
        eng.set_weights(oc.params_to_list(P))
        db = eng.to_device(pb)
        yd = torch.from_numpy(y).cuda()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            if not use_graph:
                eng.profile(True)
            for i in range(4):
                loss = eng.train_step(db, yd)
                if i == 0 and not use_graph:
                    names = eng.profile_read()
                    eng.profile(False)
            q = eng.forward(db)
        st.synchronize()
        res.append((eng.get_flat(), loss.cpu().numpy(), q.cpu().numpy()))
        eng.close()
    assert names.get("k_wgrad_gnn", (0, 0))[0] == 2, names
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("N,F,L,shared,B", [(12, 128, 6, False, 24), (16, 256, 8, True, 16)])
def test_phased_step_of_the_wide_model_at_depth(N, F, L, shared, B):
    """forward_backward_phase over all L + 2 buckets ([Dense layers], [stage L], ..., [stage 1], [embed]): bucket k holds
    its final value after phase k and no later phase changes it; losses equal forward_backward's bit for bit, gradients
    as tightly as test_gpu_fused.test_two_phase_step_equals_single_call requires; the buckets tile the parameters."""
    import torch
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, True, seed=29 * N + F + L + B)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    one, two = _engine(spec, P), _engine(spec, P)
    buckets = two.grad_buckets()
    assert len(buckets) == L + 2, buckets
    off = 0
    for o, n in sorted(buckets):
        assert o == off and n > 0, buckets
        off += n
    assert off == two.n_params
    assert buckets[0][0] + buckets[0][1] == two.n_params and buckets[-1][0] == 0, buckets    # Dense first, embed last
    with torch.cuda.stream(torch.cuda.Stream()):
        db1, db2 = one.to_device(pb), two.to_device(pb)
        yd = torch.from_numpy(y).cuda()
        for _ in range(2):
            l1 = one.forward_backward(db1, yd)
            two.grad_tensor().zero_()
            snaps = []
            for k in range(L + 2):
                l2 = two.forward_backward_phase(db2, yd, k)
                assert (l2 is None) == (k < L + 1)
                snaps.append(two.get_grad_flat())
            torch.cuda.synchronize()
            g1, g2 = one.get_grad_flat(), snaps[-1]
            for k, snap in enumerate(snaps):
                for o, n in buckets[:k + 1]:
                    assert np.array_equal(snap[o:o + n], g2[o:o + n]), ("bucket changed after its phase", k, o, n)
            assert np.array_equal(l1.cpu().numpy(), l2.cpu().numpy())
            assert np.allclose(g1, g2, rtol=1e-5, atol=1e-9)
            one.apply_gradients()
            two.apply_gradients()
        torch.cuda.synchronize()
    assert np.allclose(one.get_flat(), two.get_flat(), rtol=1e-6, atol=1e-8)
    one.close()
    two.close()
