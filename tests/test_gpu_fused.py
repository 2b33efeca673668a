"""GPU: the graph-major fused graph-layer kernels (csrc/kernels_fused.hpp) against the layer-by-layer kernels
(V2X_FUSED=0) and the oracle; the LDS tile guards and the batch contract checks."""
import os

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine
from util import (ospec, random_inputs, fixed_indegree_adj, f32_params, assert_fwd_close, assert_grad_close, assert_close, oracle_step,
                  assert_grads_match_oracle, _ragged_batch)
from oracle import compact as oc

pytestmark = pytest.mark.gpu


def _engine(spec, weights, fused, compl=False, split=None, **kw):
    """compl: let dense graphs aggregate through the complement (column sum minus the non-neighbours' rows; the default
    of the library) -- same values up to rounding, so the bitwise comparisons below switch it off.
    split: V2X_FUSED_SPLIT (None = the library's choice: K workgroups per 16-graph tile for batches that leave most of the
    chip idle, csrc/kernels_fused_split.hpp; 0 = whole-tile workgroups; K = forced)."""
    env = {"V2X_FUSED": "1" if fused else "0", "V2X_FUSED_COMPL": "1" if compl else "0"}     # read by v2x_create
    if split is not None:
        env["V2X_FUSED_SPLIT"] = str(split)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = GnnEngine(spec, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    eng.set_weights(weights)
    return eng


CASES = [  # N, F, L, B, share, reference topology
    (4, 16, 2, 64, False, True),
    (4, 16, 2, 7, False, True),          # one partial 16-graph tile
    (20, 64, 2, 33, False, True),        # two full tiles + one graph
    (20, 64, 2, 16, True, True),
    (6, 32, 3, 50, False, False),        # random topologies: ragged in-degrees, some nodes without in-edges
    (28, 64, 1, 20, False, True),        # largest tile that fits the LDS at F = 64
    (5, 64, 2, 1, False, True),          # batch 1 (the rollout predict)
]


@pytest.mark.parametrize("N,F,L,B,share,ref_topo", CASES)
def test_fused_equals_layerwise_bitwise_and_oracle(N, F, L, B, share, ref_topo):
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=share)
    rng = np.random.default_rng(100 + N + F + B)
    P = f32_params(spec, rng)
    weights = oc.params_to_list(P)
    x, e, adj = random_inputs(rng, B, N, ref_topology=ref_topo, density=0.4)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    fused, plain = _engine(spec, weights, True), _engine(spec, weights, False)
    qf, qp = fused.forward(pb), plain.forward(pb)
    assert np.array_equal(qf, qp), "fused forward differs from the layer-by-layer kernels"
    lf, lp = fused.forward_backward(pb, y), plain.forward_backward(pb, y)
    gf, gp = fused.get_grad_flat(), plain.get_grad_flat()
    assert np.array_equal(lf, lp)
    assert np.array_equal(gf, gp), "fused gradient differs: max %g" % np.abs(gf - gp).max()
    # and the oracle (float64 restatement of BS_brain.py:17-216); backward for the SAME q the kernels differentiate
    os_ = ospec(spec)
    M = oc.csr_to_matrix((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx, np.float64)
    q_ref, cache = oc.forward(os_, P, x.reshape(B * N, -1).astype(np.float64), e.reshape(B * N, -1).astype(np.float64), M)
    assert_fwd_close(qf, q_ref, "fused forward vs oracle")
    loss_ref, dq = oc.huber_loss_and_grad(os_, qf.astype(np.float64), y.astype(np.float64))
    g_ref = oc.backward(os_, P, cache, dq)
    assert_close(lf, loss_ref, 2e-4, 1e-6, "loss")
    for i, (a_, b_) in enumerate(zip(v2xgnn.flat_to_keras_list(spec, gf), oc.params_to_list(g_ref))):
        assert_grad_close(a_, b_, "fused gradient array %d vs oracle" % i)
    # three optimizer steps stay together
    for _ in range(3):
        fused.train_step(pb, y)
        plain.train_step(pb, y)
    assert np.array_equal(fused.get_flat(), plain.get_flat())
    fused.close()
    plain.close()


@pytest.mark.parametrize("N,F,L,B,share,ref_topo", CASES)
def test_complement_aggregation_matches_layerwise_and_oracle(N, F, L, B, share, ref_topo):
    """Dense graphs (the reference topology has in-degree N - 2): Agg through the column sum minus the non-neighbours.
    Equal to the edge-ordered gather up to fp32 rounding; sparse batches must not take that form at all (bitwise)."""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=share)
    rng = np.random.default_rng(100 + N + F + B)
    P = f32_params(spec, rng)
    weights = oc.params_to_list(P)
    x, e, adj = random_inputs(rng, B, N, ref_topology=ref_topo, density=0.4)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    fused, plain = _engine(spec, weights, True, compl=True, split=0), _engine(spec, weights, False)     # (split tiles: edge form only)
    qf, qp = fused.forward(pb), plain.forward(pb)
    lf, lp = fused.forward_backward(pb, y), plain.forward_backward(pb, y)
    gf, gp = fused.get_grad_flat(), plain.get_grad_flat()
    rowf = 4 * ((F // 16) | 1)                                 # fused_lds() of csrc/v2xgnn.hip with the partial column sums
    lds = 4 * 16 * N * rowf * 4 + (16 * N + 1) * 4 + 16 * pb.max_edges + 16 * N * 4 + 512 * rowf * 4
    dense = 2 * pb.col_idx.size > B * N * (N - 1) and N >= 4 and lds <= 160 * 1024
    if not dense:
        assert np.array_equal(qf, qp) and np.array_equal(gf, gp)
    else:
        assert not np.array_equal(gf, gp)                      # the complement form really ran
    assert np.allclose(qf, qp, rtol=1e-5, atol=1e-5 * np.abs(qp).max()), np.abs(qf - qp).max()
    assert np.allclose(lf, lp, rtol=1e-5, atol=1e-7)
    assert np.allclose(gf, gp, rtol=1e-3, atol=1e-4 * np.abs(gp).max()), np.abs(gf - gp).max()
    os_ = ospec(spec)
    M = oc.csr_to_matrix((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx, np.float64)
    q_ref, cache = oc.forward(os_, P, x.reshape(B * N, -1).astype(np.float64), e.reshape(B * N, -1).astype(np.float64), M)
    assert_fwd_close(qf, q_ref, "complement forward vs oracle")
    loss_ref, dq = oc.huber_loss_and_grad(os_, qf.astype(np.float64), y.astype(np.float64))
    g_ref = oc.backward(os_, P, cache, dq)
    assert_close(lf, loss_ref, 2e-4, 1e-6, "loss")
    for i, (a_, b_) in enumerate(zip(v2xgnn.flat_to_keras_list(spec, gf), oc.params_to_list(g_ref))):
        assert_grad_close(a_, b_, "complement gradient array %d vs oracle" % i)
    fused.close()
    plain.close()


@pytest.mark.parametrize("N,B,degree,split", [(20, 40, 2, 0), (20, 40, 4, 0), (28, 24, 2, 0), (28, 24, 4, 0), (20, 40, (1, 18), 0),
                                              (20, 40, 2, None), (20, 33, 4, None), (24, 20, (1, 22), None)])
def test_sparse_graphs_take_the_degree_aware_walk(N, B, degree, split):
    """graphs of in-degree 2 and 4 (and batches that mix sparse and dense graphs inside one wave): a lane
    whose slots hold fewer than N / 2 sources walks only those -- same sums in the same order, so still bitwise the
    layer-by-layer CSR gather (k_agg), and within tolerance of the oracle.  split: whole-tile (0) and split-tile (None: the
    library's choice at these batch sizes) kernels."""
    F, L = 64, 2
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(4000 + N + B)
    P = f32_params(spec, rng)
    weights = oc.params_to_list(P)
    x, e, _ = random_inputs(rng, B, N)
    if isinstance(degree, tuple):          # alternate sparse and dense graphs: lanes of one wave take different walks
        adj = np.concatenate([fixed_indegree_adj(rng, 1, N, degree[b % 2]) for b in range(B)])
    else:
        adj = fixed_indegree_adj(rng, B, N, degree)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    fused, plain = _engine(spec, weights, True, split=split), _engine(spec, weights, False)
    info = fused.path_info(pb)
    assert info["graph_layers"].startswith("fused(split" if split is None else "fused") and info["aggregation"] == "edge-bitset-walk", info
    assert plain.path_info(pb)["aggregation"] == "edge-gather"
    qf, qp = fused.forward(pb), plain.forward(pb)
    assert np.array_equal(qf, qp)
    lf, lp = fused.forward_backward(pb, y), plain.forward_backward(pb, y)
    gf, gp = fused.get_grad_flat(), plain.get_grad_flat()
    assert np.array_equal(lf, lp) and np.array_equal(gf, gp), np.abs(gf - gp).max()
    # the oracle; a ReLU whose float64 pre-activation lies within fp32 rounding of 0 may be gated the other way by the kernels
    # (sparse sums are small: it happens) -- resolved explicitly, as at the full sizes (tests/util.py, assert_grads_match_oracle)
    graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
    ref = oracle_step(spec, P, x.reshape(B * N, -1), e.reshape(B * N, -1), graph, y, q_at=qf)
    assert_fwd_close(qf, ref['q'], "sparse forward vs oracle")
    assert_close(lf, ref['loss'], 2e-4, 1e-6, "loss")
    _, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, gf), P, ref, "sparse gradients vs oracle")
    assert n_flip <= 8, (n_flip, n_cand)
    fused.close(); plain.close()


SPLIT_CASES = [  # N, F, L, B, share, reference topology, K
    (16, 64, 2, 33, False, True, 2),      # 8 slots per member: every wave owns one
    (20, 64, 2, 33, False, True, 4),      # the 1024-graph share's form: 5 slots per member
    (20, 64, 2, 48, False, True, 5),      # the 512-graph share's form: 4 slots per member
    (20, 64, 2, 130, True, True, 4),      # shared weights, 9 tiles (more than one tile per XCD column)
    (20, 64, 3, 20, False, False, 3),     # K does not divide N (members with 7 and 6 slots), random topologies, 3 layers
    (12, 32, 2, 40, False, False, 2),
    (8, 16, 1, 17, False, True, 4),       # two slots per member, one layer
    (24, 64, 1, 20, False, True, 4),
]


@pytest.mark.parametrize("N,F,L,B,share,ref_topo,K", SPLIT_CASES)
def test_split_tiles_equal_whole_tiles_bitwise(N, F, L, B, share, ref_topo, K):
    """K workgroups per 16-graph tile with tagged-word hand-overs of the stage rows (kernels_fused_split.hpp) against the
    whole-tile kernels and the layer-by-layer kernels: same arithmetic order, bitwise the same q, losses, gradients and
    weights -- eager and replayed, over several steps (the epoch of the exchange advances with every launch)."""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=share)
    rng = np.random.default_rng(900 + N + F + B + K)
    P = f32_params(spec, rng)
    weights = oc.params_to_list(P)
    x, e, adj = random_inputs(rng, B, N, ref_topology=ref_topo, density=0.4)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    split, whole, plain = _engine(spec, weights, True, split=K), _engine(spec, weights, True, split=0), _engine(spec, weights, False)
    assert split.path_info(pb)["graph_layers"] == "fused(split%d)" % K, split.path_info(pb)
    assert whole.path_info(pb)["graph_layers"] == "fused", whole.path_info(pb)
    qs, qw, qp = split.forward(pb), whole.forward(pb), plain.forward(pb)
    assert np.array_equal(qs, qw) and np.array_equal(qs, qp), "split forward differs: max %g" % np.abs(qs - qw).max()
    ls, lw = split.forward_backward(pb, y), whole.forward_backward(pb, y)
    gs, gw = split.get_grad_flat(), whole.get_grad_flat()
    assert np.array_equal(ls, lw)
    assert np.array_equal(gs, gw), "split gradient differs: max %g" % np.abs(gs - gw).max()
    for _ in range(5):
        split.train_step(pb, y)
        whole.train_step(pb, y)
    assert np.array_equal(split.get_flat(), whole.get_flat())
    assert np.array_equal(split.forward(pb), whole.forward(pb))
    split.close(); whole.close(); plain.close()


def test_split_tiles_hipgraph_replay_and_mixed_batch_sizes():
    """The exchange's epoch lives in device memory (departure counters), so a replayed graph -- frozen kernel arguments --
    keeps working; batches of different sizes share the buffer (tiles are addressed by capacity, not by batch)."""
    import torch
    N, F = 20, 64
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(17)
    weights = oc.params_to_list(f32_params(spec, rng))
    eager = _engine(spec, weights, True, split=0)
    graph = _engine(spec, weights, True, use_graph=True)            # the library's choice: split at these sizes
    batches = []
    for B in (48, 130, 16, 48):
        x, e, adj = random_inputs(rng, B, N)
        batches.append((PackedBatch.from_dense(x, e, adj), rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)))
    assert "split" in graph.path_info(batches[0][0])["graph_layers"]
    with torch.cuda.stream(torch.cuda.Stream()):
        for pb, y in batches:
            db, yd = graph.to_device(pb), torch.from_numpy(y).cuda()
            for _ in range(3):
                graph.train_step(db, yd)
        torch.cuda.synchronize()
    for pb, y in batches:
        for _ in range(3):
            eager.train_step(pb, y)
    assert np.array_equal(eager.get_flat(), graph.get_flat())
    # re-arming the exchange (v2x_reset_exchange: tags and departure counters back to zero) leaves a working exchange behind
    graph.reset_exchange()
    pb, y = batches[1]
    with torch.cuda.stream(torch.cuda.Stream()):
        graph.train_step(graph.to_device(pb), torch.from_numpy(y).cuda())
        torch.cuda.synchronize()
    eager.train_step(pb, y)
    assert np.array_equal(eager.get_flat(), graph.get_flat())
    eager.close(); graph.close()


def test_split_tiles_alternating_members_per_tile():
    """A tile that is visited by launches of DIFFERENT K (1200 graphs: 3 workgroups per tile, 300 graphs: 5) must never see
    an epoch twice: round 5's first exchange counted the members' departures and divided by K, which repeated an epoch in
    exactly this sequence and let a member take a stale row of the earlier launch for a fresh one (a 1-in-6 failure of
    test_graph_cache_survives_workspace_growth).  Forward + forward_backward alternate between the two sizes for many
    rounds; every q, loss and gradient bit for bit the whole-tile engine's."""
    import torch
    N, F = 20, 64
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(23)
    weights = oc.params_to_list(f32_params(spec, rng))
    split, whole = _engine(spec, weights, True, use_graph=True), _engine(spec, weights, True, split=0)
    data = {}
    for B in (1200, 300):
        x, e, adj = random_inputs(rng, B, N)
        y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
        pb = PackedBatch.from_dense(x, e, adj)
        data[B] = (pb, y, whole.forward(pb), whole.forward_backward(pb, y).copy(), whole.get_grad_flat().copy())
    assert split.path_info(data[1200][0])["graph_layers"] == "fused(split3)" and split.path_info(data[300][0])["graph_layers"] == "fused(split5)"
    with torch.cuda.stream(torch.cuda.Stream()):
        dev = {B: (split.to_device(data[B][0]), torch.from_numpy(data[B][1]).cuda()) for B in data}
        for it in range(60):
            B = (1200, 300)[it % 2] if it % 7 else 300
            db, yd = dev[B]
            q = split.forward(db)
            loss = split.forward_backward(db, yd)
            torch.cuda.synchronize()
            assert np.array_equal(q.cpu().numpy(), data[B][2]), (it, B)
            assert np.array_equal(loss.cpu().numpy(), data[B][3]) and np.array_equal(split.get_grad_flat(), data[B][4]), (it, B)
    split.close(); whole.close()


def test_split_tiles_out_of_step_exchange_times_out_instead_of_hanging():
    """The members of a tile poll for their partners' rows with BOUNDED polls.  Here the tiles' launch counters are bumped from
    another stream WHILE split-tile fit steps run, so that members of one launch read different epochs and wait for tags nobody
    writes: the launch must terminate, the call must report V2X_ESTATE ("timed out"), the library must re-arm the exchange by
    itself, and the following steps must be right again (bit-identical to a whole-tile engine from the same weights)."""
    import ctypes as C
    import time
    import torch
    N, F, B = 20, 64, 512                                           # 32 tiles x 5 members: many chances per launch
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(41)
    weights = oc.params_to_list(f32_params(spec, rng))
    split = _engine(spec, weights, True)        # ONE engine while the race runs: each engine owns streams, and HIP folds streams
    x, e, adj = random_inputs(rng, B, N)        # onto 4 hardware queues -- two streams of one queue would run in turn
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    assert split.path_info(pb)["graph_layers"] == "fused(split5)"
    split.forward_backward(pb, y)                                   # allocates the exchange
    n = C.c_int32(0)
    ptr = int(split._lib.v2x_debug_split_counters(split._h, C.byref(n)))
    assert ptr and n.value >= 3

    class _H(object):
        pass
    h = _H()
    h.__cuda_array_interface__ = {"shape": (n.value,), "typestr": "<i8", "data": (ptr, False), "version": 2, "strides": None}
    cnt = torch.as_tensor(h, device="cuda:%d" % split.device)
    side, main = torch.cuda.Stream(), torch.cuda.Stream()
    bumps = torch.cuda.CUDAGraph()
    with torch.cuda.graph(bumps, stream=side):
        for _ in range(2000):
            cnt.add_(3)
    seen, t_max = 0, 0.0
    for attempt in range(60):
        with torch.cuda.stream(side):
            bumps.replay()
        t0 = time.perf_counter()
        try:
            with torch.cuda.stream(main):
                loss = split.forward_backward(pb, y)
            assert loss.shape == (N,)
        except v2xgnn.lib.V2XError as exc:
            assert "timed out" in str(exc), str(exc)
            seen += 1
        t_max = max(t_max, time.perf_counter() - t0)
        torch.cuda.synchronize()
        if seen >= 2:
            break
    assert seen >= 1, "the bumps never met a running split-tile launch"
    assert t_max < 30.0, t_max                                      # bounded: a few poll caps, not a hang
    # recovery: the exchange was re-armed by the failing call; same weights in, same bits out as the whole-tile engine
    whole = _engine(spec, weights, True, split=0)
    split.set_weights(weights)
    for _ in range(3):
        ls, lw = split.forward_backward(pb, y), whole.forward_backward(pb, y)
        assert np.array_equal(ls, lw) and np.array_equal(split.get_grad_flat(), whole.get_grad_flat())
    split.close(); whole.close()


def test_fused_hipgraph_replay_is_bitwise_eager():
    import torch
    N, F, B = 20, 64, 48
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(7)
    weights = oc.params_to_list(f32_params(spec, rng))
    x, e, adj = random_inputs(rng, B, N)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    eager = _engine(spec, weights, True)
    graph = _engine(spec, weights, True, use_graph=True)
    with torch.cuda.stream(torch.cuda.Stream()):
        db = graph.to_device(pb)
        yd = torch.from_numpy(y).cuda()
        for _ in range(4):
            graph.train_step(db, yd)
        torch.cuda.synchronize()
    for _ in range(4):
        eager.train_step(pb, y)
    assert np.array_equal(eager.get_flat(), graph.get_flat())


def test_understated_max_edges_is_reported_not_corrupting():
    """A device batch whose max_edges understates the real edge count must not overrun the LDS tile: the kernels skip
    the tile and the next synchronising call reports V2X_EINVAL."""
    import torch
    for fused in (True, False):
        N, F, B = 20, 64, 32
        spec = GnnSpec(n_nodes=N, feat_dim=F)
        rng = np.random.default_rng(11)
        eng = _engine(spec, oc.params_to_list(f32_params(spec, rng)), fused)
        x, e, adj = random_inputs(rng, B, N)
        pb = PackedBatch.from_dense(x, e, adj)
        db = eng.to_device(pb)
        db.max_edges = pb.max_edges // 2
        eng.forward(db)
        with pytest.raises(ValueError, match="max_nodes / max_edges"):
            eng.check_errors()
        eng.check_errors()                       # flag was cleared
        with pytest.raises(ValueError, match="max_edges"):
            eng.validate(db)
        eng.close()


def test_host_batches_are_validated_before_any_copy():
    N, F, B = 6, 16, 9
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(12)
    eng = _engine(spec, oc.params_to_list(f32_params(spec, rng)), True)
    x, e, adj = random_inputs(rng, B, N)
    good = PackedBatch.from_dense(x, e, adj)
    eng.forward(good)

    def broken(**kw):
        pb = PackedBatch.from_dense(x, e, adj)
        for k, v in kw.items():
            setattr(pb, k, v)
        return pb
    with pytest.raises(ValueError, match="max_edges"):
        eng.forward(broken(max_edges=good.max_edges - 1))
    col = good.col_idx.copy()
    col[1] = col[0]                               # duplicate edge
    with pytest.raises(ValueError, match="ascending"):
        eng.forward(broken(col_idx=col))
    col = good.col_idx.copy()
    col[0] = N                                    # source outside the graph
    with pytest.raises(ValueError, match="outside"):
        eng.forward(broken(col_idx=col))
    # the device-side checker agrees
    db = eng.to_device(good)
    eng.validate(db)
    import torch
    db.col_idx = torch.from_numpy(col).cuda()
    with pytest.raises(ValueError, match="source id"):
        eng.validate(db)
    eng.close()


@pytest.mark.parametrize("N,F,B,use_graph", [(20, 64, 48, False), (20, 64, 48, True), (4, 16, 64, False)])
def test_two_phase_step_equals_single_call(N, F, B, use_graph, monkeypatch):
    """v2x_forward_backward_phase (data-parallel overlap: Dense bucket final after phase 0, graph-layer bucket after
    phase 1) leaves the same gradient and losses as v2x_forward_backward.  (V2X_MLP_WG0=1: at this batch size the single call
    would otherwise hand Dense-0's weight gradient to k_wgrad -- another summation order, tests/test_gpu_dense0_role.py -- while
    the phases keep it in the MLP launch, whose end completes the Dense bucket.)"""
    import torch
    monkeypatch.setenv("V2X_MLP_WG0", "1")
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(17)
    weights = oc.params_to_list(f32_params(spec, rng))
    x, e, adj = random_inputs(rng, B, N)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    pb = PackedBatch.from_dense(x, e, adj)
    one, two = _engine(spec, weights, True, use_graph=use_graph), _engine(spec, weights, True, use_graph=use_graph)
    (o0, n0), (o1, n1) = two.grad_buckets()
    assert o1 == 0 and o0 == n1 and n0 + n1 == two.n_params          # graph layers first, Dense layers behind them
    with torch.cuda.stream(torch.cuda.Stream()):
        db1, db2 = one.to_device(pb), two.to_device(pb)
        yd = torch.from_numpy(y).cuda()
        for _ in range(3):                                            # replays of the captured phases included
            l1 = one.forward_backward(db1, yd)
            two.grad_tensor().zero_()
            assert two.forward_backward_phase(db2, yd, 0) is None
            g_mid = two.get_grad_flat()
            l2 = two.forward_backward_phase(db2, yd, 1)
            torch.cuda.synchronize()
            g1, g2 = one.get_grad_flat(), two.get_grad_flat()
            assert np.array_equal(g_mid[o0:], g2[o0:]) and not g_mid[:o0].any()     # Dense bucket final after phase 0
            assert np.array_equal(l1.cpu().numpy(), l2.cpu().numpy())
            assert np.allclose(g1, g2, rtol=1e-5, atol=1e-9)
            one.apply_gradients()
            two.apply_gradients()
    assert np.allclose(one.get_flat(), two.get_flat(), rtol=1e-6, atol=1e-8)


RAGGED = [  # feat_dim, layers, topology, sizes
    (64, 2, 'ref', [128] * 3 + [8] * 40 + [127, 1, 2, 16, 15, 17, 64, 100]),         # tiles of one 128-node graph, > 16 tiny graphs per tile
    (64, 2, 'mixed', list(np.random.default_rng(1).integers(8, 129, size=70))),
    (32, 3, 'mixed', list(np.random.default_rng(2).integers(1, 129, size=90))),
    (16, 1, 'ref', list(np.random.default_rng(3).integers(8, 129, size=50))),
    (64, 2, 'ref', [40, 33]),                                                         # less than one workgroup of rows
    (64, 4, 'mixed', list(np.random.default_rng(4).integers(30, 129, size=24))),
    (64, 2, 'ref', [1] * 700 + [128, 64, 128] + [2] * 90),                            # runs of one-node graphs: a tile of 320 graphs
    (32, 2, 'ref', [64] * 25 + [128] * 5 + [32] * 30),                                # tiles that fill exactly (5 x 64 = 320 rows)
]


@pytest.mark.parametrize("F,L,kind,sizes", RAGGED[:4])
def test_ragged_small_tiles_equal_large_tiles_bitwise(F, L, kind, sizes):
    """csrc/kernels_ragged_small.hpp (round 5, opt-in: V2X_RAGGED_SMALL=1 -- measured slower, kept as the measured alternative):
    160-row tiles in 4-wave workgroups with the weights streamed from L2 as MFMA fragments against the 320-row tiles with the
    weight image in LDS.  A row's arithmetic does not depend on the tile it sits in: q, losses and gradients bit for bit."""
    rng = np.random.default_rng(70 * F + L + len(sizes))
    spec = GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, [int(n) for n in sizes], kind)
    P = f32_params(spec, rng)
    large = _engine(spec, oc.params_to_list(P), True)
    os.environ["V2X_RAGGED_SMALL"] = "1"
    try:
        small = _engine(spec, oc.params_to_list(P), True)
        ql, qs = large.forward(pb), small.forward(pb)
        assert np.array_equal(ql, qs), np.abs(ql - qs).max()
        y = (ql + rng.normal(0, 1.2, size=ql.shape)).astype(np.float32)
        ll, ls = large.forward_backward(pb, y, n_global=pb.n_rows), small.forward_backward(pb, y, n_global=pb.n_rows)
        assert np.array_equal(ll, ls) and np.array_equal(large.get_grad_flat(), small.get_grad_flat())
        for _ in range(3):                   # the fragment-major copy follows the parameters (Adam writes both)
            large.train_step(pb, y, n_global=pb.n_rows)
            small.train_step(pb, y, n_global=pb.n_rows)
        assert np.array_equal(large.get_flat(), small.get_flat()) and np.array_equal(large.forward(pb), small.forward(pb))
    finally:
        del os.environ["V2X_RAGGED_SMALL"]
    large.close(); small.close()


@pytest.mark.parametrize("F,L,kind,sizes", RAGGED)
def test_ragged_fused_layers_vs_layerwise_and_oracle(F, L, kind, sizes):
    """csrc/kernels_ragged.hpp: variable-size graphs with shared weights run embed + L stages + L + 1
    aggregations as ONE launch, and the L + 1 transposed aggregations + L data gradients as ONE.  Against the float64 oracle
    (forward, loss, every gradient array) and against the layer-wise kernels (V2X_RAGGED_FUSED=0: same arithmetic up to the
    fp32 order of the aggregation sums), over graph sizes 1..128, tiles made of one big graph or of dozens of tiny ones,
    the reference topology, half-dense and sparse graphs in one batch, isolated nodes."""
    rng = np.random.default_rng(7 * F + L + len(sizes))
    spec = GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, [int(n) for n in sizes], kind)
    P = f32_params(spec, rng)
    fused = _engine(spec, oc.params_to_list(P), True)
    os.environ["V2X_RAGGED_FUSED"] = "0"
    try:
        plain = _engine(spec, oc.params_to_list(P), True)
    finally:
        del os.environ["V2X_RAGGED_FUSED"]
    info = fused.path_info(pb)
    assert info["graph_layers"] == "fused(ragged)" and plain.path_info(pb)["graph_layers"] == "layerwise", info
    q, qp = fused.forward(pb), plain.forward(pb)
    y = (q + rng.normal(0, 1.2, size=q.shape)).astype(np.float32)
    step = oracle_step(spec, P, x, e, (offs, pb.row_ptr, pb.col_idx), y, q_at=q, n_denominator=pb.n_rows)
    assert_fwd_close(q, step['q'], "ragged fused forward vs oracle")
    assert_fwd_close(q, qp, "ragged fused forward vs layer-wise")
    loss = fused.forward_backward(pb, y, n_global=pb.n_rows)
    assert_close(loss, step['loss'], 2e-4, 1e-6, "loss vs oracle")
    # (the oracle is handed the fused path's q: the element-wise check of the backward.  The layer-wise path would
    #  differentiate the loss at ITS q, and with 126-neighbour sums |q| reaches 1e4: its fp32 rounding alone moves the
    #  unit-scale residuals q - y -- the two paths' gradients are not comparable, only their forwards are)
    g = fused.get_grad_flat()
    assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, g), P, step, "ragged fused F=%d L=%d %s" % (F, L, kind))
    # the tiles packed by k_ragged_plan (the default) against the row-interval plan of k_adj_masks: every row's arithmetic
    # is the same wherever its graph sits in a tile, so the two agree bit for bit
    os.environ["V2X_RAGGED_PACKED"] = "0"
    try:
        interval = _engine(spec, oc.params_to_list(P), True)
    finally:
        del os.environ["V2X_RAGGED_PACKED"]
    assert np.array_equal(interval.forward(pb), q), "packed plan vs interval plan: forward"
    interval.forward_backward(pb, y, n_global=pb.n_rows)
    assert np.array_equal(interval.get_grad_flat(), g), "packed plan vs interval plan: gradients"
    interval.close()
    for _ in range(3):
        fused.train_step(pb, y, n_global=pb.n_rows)
    assert np.all(np.isfinite(fused.get_flat())) and fused.get_optimizer_state()[2] == 3
    fused.check_errors()
    fused.close()
    plain.close()


def _greedy_plan(sizes, cap):
    """Runs of whole graphs of <= cap rows, each as long as it can be: the fewest runs a split into runs can have."""
    starts, rows = [0], 0
    for g, n in enumerate(sizes):
        if rows + n > cap:
            starts.append(g)
            rows = 0
        rows += n
    return starts + [len(sizes)]


@pytest.mark.parametrize("sizes", [
    list(np.random.default_rng(11).integers(8, 129, size=300)),           # the configs[4] mix
    [128] * 40, [1] * 1000, [64] * 25 + [128] * 5 + [32] * 30,            # tiles that fill exactly, 320 one-node graphs per tile
    [128, 1, 128, 1, 127, 66, 2] * 9, [100],
])
@pytest.mark.parametrize("fold", [1, 0])
def test_ragged_plan_is_the_greedy_packing(sizes, fold):
    """k_ragged_plan (csrc/kernels_ragged.hpp) resolves the chain "next run starts where the previous one stops fitting" by
    pointer doubling in one workgroup: its plan must be the sequential greedy packing exactly -- every graph once, no run over
    320 rows, and no split into runs with fewer workgroups -- with the launch's surplus workgroups pointing past the batch."""
    import ctypes as C
    sizes = [int(n) for n in sizes]
    rng = np.random.default_rng(len(sizes))
    spec = GnnSpec(n_nodes=1, feat_dim=64, n_mp_layers=2, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, sizes, 'ref')
    os.environ["V2X_RAGGED_PLAN_FOLD"] = str(fold)        # 1: a workgroup of the mask launch (16-bit tables), 0: k_ragged_plan
    try:
        eng = _engine(spec, oc.params_to_list(f32_params(spec, rng)), True)
    finally:
        del os.environ["V2X_RAGGED_PLAN_FOLD"]
    assert eng.path_info(pb)["graph_layers"] == "fused(ragged)"
    eng.forward(pb)
    buf = (C.c_int32 * 4096)()
    n = eng._lib.v2x_debug_ragged_plan(eng._h, buf, 4096)
    assert n > 0, eng.last_error() if hasattr(eng, "last_error") else n
    plan = list(buf[:n])
    want = _greedy_plan(sizes, 320)
    assert plan[:len(want)] == want, (plan[:len(want) + 2], want)
    assert all(v == len(sizes) for v in plan[len(want):]), plan[len(want):]
    assert n >= len(want)                                   # the launch (row-interval count) is an upper bound of the runs
    eng.check_errors()
    eng.close()
