"""Host: the draws of tests/test_gpu_phased_forms.py (the phased step, the mixed forward / backward forms and the ranged Adam
against the float64 oracle) held to their conditions with the oracle alone, so that a draw is known to be usable before it
reaches a GPU.  This file owns the case table and the draws; the GPU file imports them.

CASES  name -> (kind, what the draw is made of, what path_info must show, launches the PHASED step must / must not show,
                which gradient arrays the phased step and the single call must give bit for bit).
  A*   layer-wise models at 41 to 128 links: draw_a of tests/test_links_41_128_host.py (cases 1, 4, 10, 11 and 7), imported,
       not drawn again.
  F*   fused graph layers (<= 32 links): ONE seeded draw, default_rng(4300 + number): f32_params, random_inputs, the N(0, 1.2)
       noise around the forward's own q.
  R*   ragged batches (shared weights, variable graphs): default_rng(4310 + number): _ragged_batch of tests/util.py, then
       f32_params, then the noise.
draw(name) is computed once, shared by every test on it and never modified:
  dict(spec, P, pb (host PackedBatch), x / e (node rows), nbr (node rows or None), graph (offsets, row_ptr, col_idx),
       noise [R, 4], n_global (the loss's denominator: graphs, node rows for a ragged batch)).

Asserted per case, the oracle alone (test_draw_is_usable): the fp32 restatement of oracle.compact -- the same functions with
parameters and inputs cast to float32 -- meets assert_fwd_close and, with targets around its own q and the float64 loss
differentiated at that q, assert_grads_match_oracle with at most MAX_GATE_FLIPS gates; every gradient array of the oracle
has a scale above 1e-12 but for stage 0's W3, which multiplies a Neighbor_Input no case here feeds and must be exactly zero;
the share of residuals with |q - y| > 1 lies in [0.2, 0.8] (both Huber branches carry weight; the draw gives about 0.40:
P(|N(0, 1.2)| > 1)); the wide case's buckets (oracle.engine) tile the parameters."""
import functools

import numpy as np
import pytest

from v2xgnn import GnnSpec, PackedBatch
from oracle import compact as oc
from util import (ospec, f32_params, random_inputs, oracle_step, assert_fwd_close, assert_grads_match_oracle, _ragged_batch,
                  FWD_RTOL, FWD_ATOL, MAX_GATE_FLIPS)
from test_links_41_128_host import CASES_A, draw_a, rows, MIN_GRAD_SCALE

HUBER_SHARE = (0.2, 0.8)

# which arrays the phased step and the single call give bit for bit ("same"):
#   ALL      both calls run the same launches in the same order on every array: the two reductions of the phased step
#            (Dense bucket, graph-layer bucket) are ranges of the single call's one column-wise slab sum
#   DENSE123 the single call's plan hands Dense-0's weight gradient to k_wgrad (k_mlp_train_wg123 + k_wgrad_gnn_d0) while the
#            phases keep it in the MLP launch (k_mlp_train_wg + k_wgrad_gnn): Dense 1..3 leave the MLP launch in the same
#            order either way; Dense-0's arrays and the graph layers' (their launch is cut into other row chunks when Dense-0
#            rides along) sum the rows in another order and are held to 2e-5 of the array's scale, the bound of
#            tests/test_gpu_dense0_role.py
#   DENSE    ragged: the MLP launch is the same, the graph layers' data chain is one launch in the single call and L + 1
#            transposed aggregations + L data gradients in the phased one -- another order of the aggregation sums; the graph
#            layers' arrays meet only through the oracle
#   WIDE     the wide model: the single call sums every layer's weight gradient in ONE merged launch, the phases in one launch
#            per layer (other row splits): Dense 1..3 (k_wgrad_dense either way) bit for bit, the rest through the oracle
ALL, DENSE123, DENSE, WIDE = "all", "dense123", "dense", "wide"

FUSED_WG = dict(mlp="train_wg")
RAGGED_INFO = dict(graph_layers="fused(ragged)", mlp="train_wg", handoff="row-major", dense0_dw="k_mlp_train_wg")
RAGGED_LAUNCHES = (("k_gnn_fwd_ragged", "k_agg_bwd", "k_node_dgrad", "k_mlp_train_wg"), ("k_gnn_bwd_ragged", "k_mlp_train_wg123"))

CASES = {  # name: (kind, recipe, path_info pins, (launches the phased step shows, launches it must not show), same)
    "A1": ("layerwise", 1, CASES_A[1][7], (("k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), DENSE123),
    "A4": ("layerwise", 4, CASES_A[4][7], (("k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), ALL),
    "A10": ("layerwise", 10, CASES_A[10][7], (("k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), DENSE123),
    "A11": ("layerwise", 11, CASES_A[11][7], (("k_mlp_train_wg", "k_agg_bwd", "k_node_dgrad"), ("k_mlp_train_wg123",)), ALL),
    "A7": ("layerwise", 7, CASES_A[7][7], (("k_mlp_bwd", "k_wgrad_dense", "k_agg_bwd"), ("k_mlp_train_wg", "k_wgrad_wide_all")), WIDE),
    # fused: (N, F, L, shared, B, reference topology, density)
    "F1": ("fused", (20, 64, 2, False, 48, True, None),
           dict(FUSED_WG, graph_layers="fused(split5)", aggregation="edge-bitset-walk", handoff="fragment-major", dense0_dw="k_wgrad"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), DENSE123),
    "F2": ("fused", (20, 64, 2, False, 44, True, None),
           dict(FUSED_WG, graph_layers="fused(split5)", aggregation="edge-bitset-walk", handoff="row-major", dense0_dw="k_mlp_train_wg"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg"), ("k_mlp_train_wg123",)), ALL),
    "F3": ("fused", (12, 64, 3, False, 32, False, 0.3),
           dict(FUSED_WG, graph_layers="fused(split3)", aggregation="edge-bitset-walk", handoff="fragment-major", dense0_dw="k_mlp_train_wg"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg"), ("k_mlp_train_wg123",)), ALL),
    # (8 links: fused_split of csrc/v2xgnn.hip picks K = 2 as soon as 4 K <= N, so the one tile of this batch is split in two
    #  and runs the edge form; F = 32: Dense-0 never rides.  Whole tiles in the complement form at default switches need
    #  N <= 7: case F7)
    "F4": ("fused", (8, 32, 2, False, 16, True, None),
           dict(FUSED_WG, graph_layers="fused(split2)", aggregation="edge-bitset-walk", handoff="fragment-major", dense0_dw="k_mlp_train_wg"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg"), ("k_mlp_train_wg123",)), ALL),
    "F7": ("fused", (7, 32, 2, False, 16, True, None),
           dict(FUSED_WG, graph_layers="fused", aggregation="complement", handoff="fragment-major", dense0_dw="k_mlp_train_wg"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg"), ("k_mlp_train_wg123",)), ALL),
    "F5": ("fused", (20, 64, 2, True, 48, True, None),
           dict(FUSED_WG, graph_layers="fused(split5)", aggregation="edge-bitset-walk", handoff="row-major", dense0_dw="k_wgrad"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), DENSE123),
    "F6": ("fused", (20, 64, 2, False, 32, True, None),                    # F1's forms on two tiles: the second batch of the mixed forms
           dict(FUSED_WG, graph_layers="fused(split5)", aggregation="edge-bitset-walk", handoff="fragment-major", dense0_dw="k_wgrad"),
           (("k_gnn_fwd_fused", "k_gnn_bwd_fused", "k_mlp_train_wg", "k_wgrad_gnn"), ("k_mlp_train_wg123", "k_wgrad_gnn_d0")), DENSE123),
    # ragged: (F, L, topology of _ragged_batch, sizes)
    "R1": ("ragged", (64, 2, 'mixed', [128, 1, 2, 17, 33, 64, 100, 127] + [8] * 20), RAGGED_INFO, RAGGED_LAUNCHES, DENSE),
    "R2": ("ragged", (16, 1, 'ref', [40, 33]), RAGGED_INFO, RAGGED_LAUNCHES, DENSE),
    "R3": ("ragged", (32, 3, 0.3, [int(n) for n in np.random.default_rng(5).integers(1, 65, size=30)]), RAGGED_INFO, RAGGED_LAUNCHES, DENSE),
}
SEED = {"F1": 4301, "F2": 4302, "F3": 4303, "F4": 4304, "F5": 4305, "F6": 4306, "F7": 4307, "R1": 4311, "R2": 4312, "R3": 4313}
RAGGED_CASES = ("R1", "R2", "R3")
WIDE_CASE = "A7"


@functools.lru_cache(maxsize=None)
def draw(name):
    kind, recipe = CASES[name][:2]
    if kind == "layerwise":
        a = draw_a(recipe)
        assert a['nbr'] is None
        return dict(spec=a['spec'], P=a['P'], pb=PackedBatch.from_dense(a['x'], a['e'], a['adj']), x=rows(a['x']), e=rows(a['e']),
                    nbr=None, graph=oc.adj_to_csr(a['adj']), noise=a['noise'], n_global=a['n_global'] or a['x'].shape[0])
    rng = np.random.default_rng(SEED[name])
    if kind == "fused":
        N, F, L, shared, B, ref, density = recipe
        spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
        P = f32_params(spec, rng)
        x, e, adj = random_inputs(rng, B, N, ref_topology=ref, density=density or 0.5)
        pb = PackedBatch.from_dense(x, e, adj)
        noise = rng.normal(0, 1.2, size=(B * N, 4))
        return dict(spec=spec, P=P, pb=pb, x=rows(x), e=rows(e), nbr=None, graph=oc.adj_to_csr(adj), noise=noise, n_global=B)
    F, L, topo, sizes = recipe
    spec = GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, list(sizes), topo)
    P = f32_params(spec, rng)
    noise = rng.normal(0, 1.2, size=(pb.n_rows, 4))
    return dict(spec=spec, P=P, pb=pb, x=x, e=e, nbr=None, graph=(offs, pb.row_ptr, pb.col_idx), noise=noise, n_global=pb.n_rows)


def oracle_of(d, q):
    """targets around q (the forward under test's own output) and the float64 oracle's step differentiated at that q
    -> (y float32 [R, 4], oracle_step(...), share of the residuals on Huber's linear branch); every gradient array's scale and
    the share asserted from the oracle alone"""
    y = (q + d['noise']).astype(np.float32)
    step = oracle_step(d['spec'], d['P'], d['x'], d['e'], d['graph'], y, q_at=q, n_denominator=d['n_global'])
    g = step['grads']
    for kind in ('gnn', 'dense'):
        for i, layer in enumerate(g[kind]):
            for name, arr in layer.items():
                if kind == 'gnn' and i == 0 and name == 'W3':
                    assert not arr.any()              # multiplies the Neighbor_Input, which no case here feeds
                    continue
                for k in range(arr.shape[0]):
                    assert np.abs(arr[k]).max() > MIN_GRAD_SCALE, ("unusable draw", kind, i, name, k, np.abs(arr[k]).max())
    share = float((np.abs(np.asarray(q, np.float64) - y) > 1.0).mean())
    assert HUBER_SHARE[0] <= share <= HUBER_SHARE[1], ("unusable draw: Huber branches", share)
    return y, step, share


def _fp32_restatement(d):
    """forward, Huber and reverse pass of oracle.compact in float32 -> (q, gradient as a Keras-shaped list)"""
    f4 = np.float32
    os_ = ospec(d['spec'])
    P4 = oc.cast_params(d['P'], f4)
    M = oc.csr_to_matrix(*d['graph'], dtype=f4)
    q, cache = oc.forward(os_, P4, d['x'].astype(f4), d['e'].astype(f4), M, None)
    assert q.dtype == f4
    y = (q + d['noise']).astype(f4)
    if d['spec'].variable_graphs:                   # one mean over (rows, C): oracle_step's expression, in float32
        dq = (np.clip(q - y, -1.0, 1.0) / f4(d['n_global'] * q.shape[1])).astype(f4)
    else:
        _, dq = oc.huber_loss_and_grad(os_, q, y, d['n_global'])
    g = oc.backward(os_, P4, cache, dq.astype(f4), probe={})
    return q, oc.params_to_list(oc.cast_params(g, np.float64))


def test_case_table_is_what_the_issue_of_this_file_names():
    assert sorted(CASES) == sorted(["A1", "A4", "A10", "A11", "A7", "F1", "F2", "F3", "F4", "F5", "F6", "F7", "R1", "R2", "R3"])
    assert [CASES_A[n][:5] for n in (1, 4, 10, 11, 7)] == [(41, 64, 2, False, 32), (65, 64, 2, False, 9), (128, 64, 2, True, 8),
                                                          (128, 16, 2, False, 3), (100, 128, 2, False, 5)]
    assert CASES_A[4][5] == "receivers" and CASES_A[1][7]["dense0_dw"] == "k_wgrad"
    assert len(CASES["R3"][1][3]) == 30 and min(CASES["R3"][1][3]) >= 1 and max(CASES["R3"][1][3]) <= 64
    assert CASES["R1"][1][3][:8] == [128, 1, 2, 17, 33, 64, 100, 127] and CASES["R1"][1][3][8:] == [8] * 20


@pytest.mark.parametrize("name", sorted(CASES))
def test_draw_is_usable(name):
    d = draw(name)
    assert draw(name) is d                                              # one draw, never redrawn
    spec, pb = d['spec'], d['pb']
    assert d['x'].shape == (pb.n_rows, 9) and d['e'].shape == (pb.n_rows, 4) and d['noise'].shape == (pb.n_rows, 4)
    kind, recipe = CASES[name][:2]
    if kind == "ragged":
        sizes = np.diff(d['graph'][0])
        assert list(sizes) == list(recipe[3]) and pb.max_nodes == max(recipe[3]) <= 128 and d['n_global'] == pb.n_rows
        if name == "R1":
            indeg = np.diff(pb.row_ptr)
            assert (indeg == 0).any() and (sizes == 1).any() and (sizes == 128).any()      # isolated rows, 1-node graphs, a full tile
            big = np.nonzero(sizes >= 16)[0]
            dense_rows = sum(int((indeg[d['graph'][0][g]:d['graph'][0][g + 1]] * 2 > sizes[g]).sum()) for g in big)
            assert dense_rows > 0                                       # rows with more edges than non-edges: the zero-bit walk
        if name == "R2":
            assert pb.n_rows < 256                                      # fewer rows than one workgroup has threads
    elif kind == "fused":
        N, F, L, shared, B, ref, density = recipe
        assert pb.n_graphs == B and pb.n_rows == B * N and N <= 32
        if density is not None:
            assert pb.n_edges < 0.5 * B * N * (N - 1)                   # sparse: below the complement form's density
    q32, g32 = _fp32_restatement(d)
    _, step, share = oracle_of(d, q32.astype(np.float64))
    ref = step['q']
    ratio = (np.abs(q32 - ref) / (FWD_RTOL * np.abs(ref) + FWD_ATOL * max(1.0, np.abs(ref).max()))).max()
    assert_fwd_close(q32, ref, "%s: fp32 restatement, forward" % name)
    _, n_cand, n_flip = assert_grads_match_oracle(g32, d['P'], step, "%s: fp32 restatement, gradient" % name)
    assert n_flip <= MAX_GATE_FLIPS
    print("%s: N=%d F=%d L=%d %s rows=%d: max|q| %.3g, fp32 restatement forward error / bound %.3f, %d gates flipped of %d "
          "candidates, share of residuals with |q - y| > 1: %.3f" % (name, spec.n_nodes, spec.feat_dim, spec.n_mp_layers,
                                                                   "shared" if spec.share_weights else "per-node", pb.n_rows,
                                                                   np.abs(ref).max(), ratio, n_flip, n_cand, share))


def test_wide_case_buckets_tile_the_parameters():
    from oracle.engine import OracleEngine
    d = draw(WIDE_CASE)
    eng = OracleEngine(d['spec'], d['P'])
    buckets = eng.grad_buckets()
    L = d['spec'].n_mp_layers
    assert len(buckets) == L + 2
    off = 0
    for o, n in sorted(buckets):
        assert o == off and n > 0 and n % 4 == 0, buckets
        off += n
    assert off == eng.n_params == d['spec'].n_params
    assert buckets[0][0] + buckets[0][1] == eng.n_params and buckets[-1][0] == 0        # Dense layers first, embed last
