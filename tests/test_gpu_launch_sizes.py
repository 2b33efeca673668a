"""GPU: the multi-workgroup forms of the training step at small shapes.  At the batches of the other small suites every
weight-gradient role is one row chunk per slot, one partial-sum slab, and k_reduce_adam sums with one thread per column.  The
launch-size switches of csrc/knobs.hpp (read once, in v2x_create) bring the other forms down to a few thousand node rows:

  A  the embed gradient on the stage roles (WG_KIND_GNN_E1 / _E2 / _E4) with three chunks per slot, the last of 2 rows
  B  stage roles next to an embed role of its own; layer-wise graph layers; shared weights with 11 chunks and a 40-row tail
  C  roles with different chunk counts in one packed 1-D grid (WgradMulti::packed): the embed role, the Dense-0 halves
     fragment-major and row-major, the work-proportional branch of role_chunks
  D  the slab sum of k_reduce_adam with 16 and with 4 threads per column, also feeding Adam and pack_scatter
  E  a wide per-node model whose weight gradients take two row splits (wide_splits), merged launch and one launch per layer
  F  the persistent tile loops of k_gemm_rows and of k_mlp_fwd<0> / k_mlp_bwd<0> with one workgroup per slot
  G  slab counts carried from step to step: a smaller batch between two larger ones, and cached hipGraphs of both

Every parity case is `_check` of tests/test_gpu_shapes.py (one seeded draw, targets around the kernels' own q, the float64
oracle, the tolerances and MAX_GATE_FLIPS of tests/util.py) plus a look at v2x_debug_layer_slabs: the slabs the backward wrote
per layer and the threads per column of the slab sum.  A case that runs as one chunk after all fails."""
import ctypes as C
import os

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine
from oracle import compact as oc
from util import (ospec, f32_params, random_inputs, oracle_step, assert_fwd_close, assert_close, assert_grads_match_oracle,
                  assert_weights_after_adam_step)

pytestmark = pytest.mark.gpu


class _env(object):
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(spec, switches, **kw):
    """an engine that read `switches` (and V2X_SMALL_PREDICT=0: `forward` on the training path's kernels) when it was created"""
    with _env(V2X_SMALL_PREDICT=0, **switches):
        return GnnEngine(spec, **kw)


def _slabs(eng):
    """(slabs of gnn[0..L], slabs of dense[0..3], threads per column of the last slab sum) as the last backward left them"""
    L = eng.spec.n_mp_layers
    buf = (C.c_int32 * 32)()
    n = eng._lib.v2x_debug_layer_slabs(eng._h, buf, 32)
    assert n == L + 6, (n, eng._lib.v2x_last_error(eng._h))
    v = [int(t) for t in buf[:n]]
    return v[:L + 1], v[L + 1:L + 5], v[L + 5]


def _draw(spec, B, topo, seed):
    rng = np.random.default_rng(seed)
    N = spec.n_nodes
    P = f32_params(spec, rng)
    x, e, adj = random_inputs(rng, B, N, ref_topology=topo and N > 2)
    return rng, P, x, e, PackedBatch.from_dense(x, e, adj)


def _parity(N, F, L, shared, B, topo, switches, what):
    """-> (gnn slabs, dense slabs, groups, path_info, q) of one forward + forward_backward that matched the oracle"""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    rng, P, x, e, pb = _draw(spec, B, topo, seed=7 * N + F + L + B)
    eng = _engine(spec, switches)
    eng.set_weights(oc.params_to_list(P))
    info = eng.path_info(pb)
    graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
    q = eng.forward(pb)
    # targets around the kernels' own q (both Huber branches whatever the scale of q); the loss is differentiated at that q
    y = (q + rng.normal(0, 1.2, size=q.shape)).astype(np.float32)
    step = oracle_step(spec, P, x.reshape(B * N, -1), e.reshape(B * N, -1), graph, y, q_at=q)
    loss = eng.forward_backward(pb, y)
    gnn, dense, groups = _slabs(eng)
    print("%s: N=%d F=%d L=%d %s B=%d  slabs gnn %s dense %s groups %d  %s" % (
        what, N, F, L, "shared" if shared else "per-node", B, gnn, dense, groups, " ".join("%s=%s" % kv for kv in sorted(info.items()))))
    assert_fwd_close(q, step['q'], what + ": forward")
    assert_close(loss, step['loss'], 2e-4, 1e-6, what + ": per-output Huber loss")
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, eng.get_grad_flat()), P, step, "%s N=%d F=%d L=%d B=%d" % (what, N, F, L, B))
    eng.close()
    return gnn, dense, groups, info, q


def _adam_steps(N, F, L, shared, B, switches, what):
    """Three fit steps against the oracle's Keras Adam, as test_gpu_model.py::test_train_steps_vs_oracle -> slabs after the last.

    A ReLU gate at rounding distance of 0 in one of the steps moves a weight by a good part of an Adam step, and the moments
    carry it on: D2's draw has one in its second step (Dense-0 of link 2, unit 73 of graph 699: pre-activation 4.3e-6, 2.2e-8 of
    the terms it sums).  With that one gate taken the other way the float64 oracle's weight [104, 73] of that layer moves by
    2.79e-5 after the second step and 4.66e-5 after the third, against a bound of 3.6e-5 -- exactly what the kernels show, at
    64-row chunks, at the default launch sizes and with Dense-0 in the MLP launch alike.  So every step first compares the
    kernels' gradient with the oracle's as the parity cases do (assert_grads_match_oracle: the gates found at rounding distance
    that the kernels took the other way, at most MAX_GATE_FLIPS, are taken the kernels' way; nothing is redrawn, no tolerance
    is widened) -- the oracle's gradient taken at the engine's weights of that step, so that both sides look at the same
    pre-activations -- and the oracle's Adam, with its own float64 weights and moments, then steps on that gradient."""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    rng = np.random.default_rng(5 + N + B)
    P = f32_params(spec, rng)
    eng = _engine(spec, switches)
    eng.set_weights(oc.params_to_list(P))
    om = oc.OracleModel(ospec(spec), P, dtype=np.float64)
    for step in range(3):
        x, e, adj = random_inputs(rng, B, N)
        pb = PackedBatch.from_dense(x, e, adj)
        graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
        y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
        # (the gradient at the ENGINE's weights: a gate is only at rounding distance for both when both hold the same weights)
        P_eng = oc.params_from_list(ospec(spec), eng.get_weights(), np.float64)
        ref = oracle_step(spec, P_eng, x.reshape(B * N, -1), e.reshape(B * N, -1), graph, y)
        eng.forward_backward(pb, y)               # (leaves the weights and Adam's moments alone)
        g_ref, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, eng.get_grad_flat()), P_eng, ref,
                                                          "%s: gradient of step %d" % (what, step))
        print("%s step %d: %d ReLU gates at rounding distance, %d taken the kernels' way" % (what, step, n_cand, n_flip))
        om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_ref))
        loss = eng.train_step(pb, y)
        assert_close(loss, ref['loss'], 5e-4, 1e-6, "%s: loss at step %d" % (what, step))
        assert_weights_after_adam_step(eng.get_weights(), oc.params_to_list(om.params), oc.params_to_list(g_ref), step, what)
    assert eng.get_optimizer_state()[2] == 3
    out = _slabs(eng)
    eng.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- A
EMBED_RIDES = [  # N, F, L, reference topology: F / 16 embed tiles over L stages -> 1, 2 or 4 per stage role (WG_KIND_GNN_E1 / E2 / E4)
    (4, 16, 1, True), (7, 32, 2, False), (12, 32, 1, True), (20, 64, 1, True), (20, 64, 2, True), (20, 64, 4, True),
]


@pytest.mark.parametrize("N,F,L,topo", EMBED_RIDES)
def test_a_embed_gradient_on_stage_roles_in_three_chunks(N, F, L, topo):
    """V2X_WG_CHUNK_MERGED=64 at 130 graphs, per-node weights: chunks of 64, 64 and 2 rows per slot; every stage role also
    writes its columns of the embed layer's three slabs"""
    gnn, dense, groups, info, _ = _parity(N, F, L, False, 130, topo, dict(V2X_WG_CHUNK_MERGED=64), "A")
    assert gnn == [3] * (L + 1), (gnn, dense)
    assert groups == 1


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("N,F,L,shared,B,want,layers", [
    (20, 64, 3, False, 130, 3, "fused"),           # 4 embed tiles do not divide over 3 stages: the embed layer is a role of its own
    (33, 32, 2, False, 130, 3, "layerwise"),       # 33 links: layer-wise graph layers
    (40, 64, 2, True, 17, 11, "layerwise"),        # shared weights: 680 rows in one slot, 11 chunks, the last of 40 rows
])
def test_b_stage_roles_in_64_row_chunks(N, F, L, shared, B, want, layers):
    gnn, dense, groups, info, _ = _parity(N, F, L, shared, B, True, dict(V2X_WG_CHUNK_GNN=64), "B")
    assert gnn == [want] * (L + 1), (gnn, dense)
    assert info["graph_layers"].startswith(layers), info
    assert groups == 1


# ---------------------------------------------------------------------------------------------------------------- C
def test_c1_embed_role_with_fewer_chunks_than_the_stage_roles():
    """three chunks per stage role, two for the embed role: unequal counts -> the packed 1-D grid"""
    gnn, dense, groups, info, _ = _parity(20, 64, 2, False, 130, True,
                                          dict(V2X_WG_EMBED_MERGE=0, V2X_WG_CHUNK_GNN=64, V2X_WG_CHUNK_EMBED=128), "C1")
    assert gnn == [2, 3, 3], (gnn, dense)
    assert groups == 1


@pytest.mark.parametrize("shared,B,handoff", [(False, 272, "fragment-major"), (True, 16, "row-major")])
def test_c2_c3_dense0_halves_take_two_chunks_next_to_five(shared, B, handoff):
    """Dense-0's weight gradient as two roles of the graph layers' launch (V2X_MLP_WG0=0) at 272 / 320 rows per slot in 64-row
    chunks: five chunks for the stage roles, two for each half -- 192 + 80 rows read fragment-major (per-node weights, whole
    16-graph groups), 192 + 128 rows read row-major (shared weights)"""
    gnn, dense, groups, info, _ = _parity(20, 64, 2, shared, B, True, dict(V2X_MLP_WG0=0, V2X_WG_CHUNK_MERGED=64),
                                          "C3" if shared else "C2")
    assert info["dense0_dw"] == "k_wgrad" and info["handoff"] == handoff, info
    assert gnn == [5, 5, 5] and dense[0] == 2, (gnn, dense)
    assert groups == 1


def test_c4_work_proportional_chunk_counts():
    """V2X_WG_ROUNDS=1: the chunk count of a role follows its share of the launch's MFMA work and the number of CUs -- printed,
    not asserted; the slabs must have been pre-sized for them (no V2X_ESTATE) and the gradients must match"""
    gnn, dense, groups, info, _ = _parity(20, 64, 2, False, 130, True, dict(V2X_WG_ROUNDS=1, V2X_WG_EMBED_MERGE=0), "C4")
    assert min(gnn) >= 1 and min(dense) >= 1, (gnn, dense)


# ---------------------------------------------------------------------------------------------------------------- D
D1 = (20, 64, 2, True, 64, dict(V2X_WG_CHUNK=64))            # 1280 rows in one slot: 20 chunks; P / 4 = 9,588 < 64 Ki
D2 = (8, 64, 2, False, 1024, dict(V2X_WG_CHUNK_MERGED=64))   # 16 chunks per slot; P / 4 = 76,704: 64 Ki <= P / 4 < 256 Ki (N = 8 hits it)


def test_d1_slab_sum_with_16_threads_per_column():
    """Shared weights, 1280 rows, V2X_WG_CHUNK=64: at least 16 slabs and fewer than 64 Ki float4 columns -> 16 threads share a
    column of the slab sum.  Parity of the gradient, then three fit steps against Keras Adam (the slab sum feeding Adam and the
    fragment-major weight copy)."""
    N, F, L, shared, B, sw = D1
    gnn, dense, groups, info, _ = _parity(N, F, L, shared, B, True, sw, "D1")
    assert groups == 16, (groups, gnn, dense)
    assert max(gnn + dense) >= 16, (gnn, dense)
    gnn3, dense3, groups3 = _adam_steps(N, F, L, shared, B, sw, "D1")
    print("D1 after three fit steps: slabs gnn %s dense %s groups %d" % (gnn3, dense3, groups3))
    assert groups3 == 16 and (gnn3, dense3) == (gnn, dense)


def test_d1b_slab_sum_with_16_threads_per_column_and_slab_counts_that_differ():
    """D1's shape with the Dense-0 halves at half the graph layers' chunk count (V2X_WG_CHUNK_MERGED=64 cuts the stage roles
    into 20 chunks of 64 rows, the halves into 10 of 128; V2X_WG_CHUNK, D1's switch, sets one chunk size for EVERY role and
    k_mlp_train_wg runs 1280 rows as 20 workgroups, so D1 itself has 20 slabs for every layer): k_reduce_adam looks up the slab
    count per layer while 16 threads share a column"""
    N, F, L, shared, B, _ = D1
    sw = dict(V2X_WG_CHUNK_MERGED=64, V2X_MLP_WG0=0)
    gnn, dense, groups, info, _ = _parity(N, F, L, shared, B, True, sw, "D1b")
    assert groups == 16, (groups, gnn, dense)
    assert set(gnn) != set(dense) and max(gnn + dense) >= 16, (gnn, dense)
    assert gnn == [20] * (L + 1) and dense[0] == 10, (gnn, dense)
    gnn3, dense3, groups3 = _adam_steps(N, F, L, shared, B, sw, "D1b")
    assert groups3 == 16 and (gnn3, dense3) == (gnn, dense)


def test_d2_slab_sum_with_4_threads_per_column():
    """Per-node weights, 8 links x 1024 graphs, 64-row chunks: 16 slabs per graph layer, 8 per Dense-0 half, and between 64 Ki
    and 256 Ki float4 columns -> 4 threads share a column and the layers' slab counts differ"""
    N, F, L, shared, B, sw = D2
    n4 = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared).n_params // 4
    assert 64 * 1024 <= n4 < 256 * 1024, n4
    gnn, dense, groups, info, _ = _parity(N, F, L, shared, B, True, sw, "D2")
    assert groups == 4, (groups, gnn, dense)
    assert gnn == [16] * (L + 1) and dense[0] == 8, (gnn, dense)
    gnn3, dense3, groups3 = _adam_steps(N, F, L, shared, B, sw, "D2")
    print("D2 after three fit steps: slabs gnn %s dense %s groups %d" % (gnn3, dense3, groups3))
    assert groups3 == 4 and (gnn3, dense3) == (gnn, dense)


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("merge", [1, 0])
def test_e_wide_weight_gradients_in_two_row_splits(merge):
    """5 links x 300 graphs x 128 features, per-node weights: too few tiles x slots to fill the chip, so every wide weight
    gradient (graph layers, Dense-0) is cut into two row splits, each a slab -- as roles of the merged launch (E1) and with
    V2X_WIDE_MERGE=0 as one launch per layer (E2).  Adam cannot ride on a split weight gradient: the fit step sums the slabs
    and applies Adam in k_reduce_adam, bit for bit what forward_backward + apply_gradients give."""
    N, F, L, B = 5, 128, 2, 300
    sw = dict(V2X_WIDE_MERGE=merge)
    gnn, dense, groups, info, _ = _parity(N, F, L, False, B, True, sw, "E1" if merge else "E2")
    assert min(gnn) >= 2 and dense[0] >= 2, (gnn, dense)
    assert groups == 1
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng, P, x, e, pb = _draw(spec, B, True, seed=11)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    fit, split = _engine(spec, sw), _engine(spec, sw)
    for eng in (fit, split):
        eng.set_weights(oc.params_to_list(P))
    fit.profile(True)
    lf = fit.train_step(pb, y)
    names = set(fit.profile_read())
    fit.profile(False)
    gnn_f, dense_f, _ = _slabs(fit)
    ls = split.forward_backward(pb, y)
    split.apply_gradients()
    print("E%d fit step: launches %s  slabs gnn %s dense %s" % (1 if merge else 2, sorted(names), gnn_f, dense_f))
    assert "k_reduce_adam" in names, names
    if merge:
        assert "k_wgrad_wide_all" in names and "k_wgrad_gnn" not in names, names
    else:
        assert {"k_wgrad_gnn", "k_wgrad_embed", "k_wgrad_dense0"} <= names and "k_wgrad_wide_all" not in names, names
    assert min(gnn_f) >= 2 and dense_f[0] >= 2, (gnn_f, dense_f)          # (an Adam epilogue needs ONE split: 0 slabs)
    assert np.array_equal(lf, ls)
    assert np.array_equal(fit.get_flat(), split.get_flat())
    fit.close()
    split.close()


# ---------------------------------------------------------------------------------------------------------------- F
@pytest.mark.parametrize("N,F,L,B,switch", [
    (40, 32, 2, 130, "V2X_GEMM_WGS_PER_CU"),      # k_gemm_rows: 9 tiles per slot, one workgroup: rounds of 4, 4 and 1
    (5, 128, 2, 140, "V2X_MLP_WGS_PER_CU"),       # k_mlp_fwd<0> / k_mlp_bwd<0> of a wide model: 9 tiles per slot likewise
])
def test_f_persistent_tile_loops_with_one_workgroup_per_slot(N, F, L, B, switch):
    """the switch at 0 leaves one persistent workgroup per slot, which walks all of the slot's tiles; tiles are independent, so
    the forward is bit for bit that of an engine with the default two workgroups per CU"""
    gnn, dense, groups, info, q = _parity(N, F, L, False, B, True, {switch: 0}, "F " + switch)
    # the default decomposition of these batches: one chunk per role; a wide model's single row split writes in place
    assert gnn == ([0] * (L + 1) if F >= 128 else [1] * (L + 1)), (gnn, dense)
    assert groups == 1
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng, P, x, e, pb = _draw(spec, B, True, seed=7 * N + F + L + B)
    plain = _engine(spec, {})
    plain.set_weights(oc.params_to_list(P))
    assert np.array_equal(plain.forward(pb), q)
    plain.close()


# ---------------------------------------------------------------------------------------------------------------- G
G_SWITCHES = dict(V2X_WG_CHUNK_GNN=64, V2X_WG_EMBED_MERGE=0)
G_SPEC = (20, 64, 2)


def _g_batches(rng, sizes):
    N = G_SPEC[0]
    out = []
    for B in sizes:
        x, e, adj = random_inputs(rng, B, N, ref_topology=True)
        out.append((B, PackedBatch.from_dense(x, e, adj), rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)))
    return out


def test_g1_slabs_of_an_earlier_larger_batch_are_not_summed():
    """130, 48 and 130 graphs on one engine: 3, 1 and 3 slabs per graph layer.  The slab buffer still holds the first batch's
    slabs 1 and 2 when the second batch's gradient is summed: every gradient must be the bits a fresh engine gives"""
    N, F, L = G_SPEC
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(41)
    w = oc.params_to_list(f32_params(spec, rng))
    eng = _engine(spec, G_SWITCHES)
    eng.set_weights(w)
    for (B, pb, y), want in zip(_g_batches(rng, (130, 48, 130)), (3, 1, 3)):
        loss = eng.forward_backward(pb, y)
        g = eng.get_grad_flat()
        gnn, dense, groups = _slabs(eng)
        fresh = _engine(spec, G_SWITCHES)
        fresh.set_weights(w)
        loss_f = fresh.forward_backward(pb, y)
        g_f = fresh.get_grad_flat()
        fresh_slabs = _slabs(fresh)
        fresh.close()
        print("G1: B=%d slabs gnn %s dense %s groups %d" % (B, gnn, dense, groups))
        assert gnn == [want] * (L + 1), (B, gnn, dense)
        assert (gnn, dense, groups) == fresh_slabs, (B, gnn, dense, groups, fresh_slabs)
        assert np.array_equal(loss, loss_f), B
        assert np.array_equal(g, g_f), (B, np.abs(g - g_f).max())
    eng.close()


def test_g2_replayed_graphs_restore_their_slab_counts():
    """six fit steps alternating 130 and 48 graphs, captured and replayed hipGraphs next to eager launches: the slab sum and
    Adam run outside the graph with the slab counts the cached entry restores -- the weights are the same bits after every step"""
    import torch
    N, F, L = G_SPEC
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(43)
    w = oc.params_to_list(f32_params(spec, rng))
    eager, graph = _engine(spec, G_SWITCHES), _engine(spec, G_SWITCHES, use_graph=True)
    eager.set_weights(w)
    graph.set_weights(w)
    batches = [(B, pb, y, graph.to_device(pb), torch.from_numpy(y).cuda()) for B, pb, y in _g_batches(rng, (130, 48))]
    stream = torch.cuda.Stream()
    for step in range(6):
        B, pb, y, db, yd = batches[step % 2]
        with torch.cuda.stream(stream):
            lg = graph.train_step(db, yd)
        stream.synchronize()
        le = eager.train_step(pb, y)
        assert np.array_equal(lg.cpu().numpy(), le), (step, B)
        assert np.array_equal(graph.get_flat(), eager.get_flat()), (step, B)
        assert _slabs(eager)[0] == [3 if B == 130 else 1] * (L + 1), (step, B, _slabs(eager))
    print("G2: after step 6 eager %s graph %s" % (_slabs(eager), _slabs(graph)))
    assert _slabs(graph) == _slabs(eager)
    eager.close()
    graph.close()
