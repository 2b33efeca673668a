"""GPU: every whole-model call on a batch that carries a NON-ZERO Neighbor_Input (v2x_batch.nbr_init, PackedBatch.nbr).

The reference always feeds zeros there, so every fast path is written for nbr == NULL: fused_path, small_path,
ragged_fused_path and embed_rides (csrc/v2xgnn.hip) return false on d.nbr, and with embed_rides false Dense-0 as a k_wgrad
role, the fragment-major hand-over and the one-launch weight gradient are off as well.  A batch with a neighbour input
therefore runs the layer-wise plan: the stage-0 term nbr . W3 in k_gemm_rows / k_wide_gemm, weight-gradient role
WG_KIND_EMBED with a real third K segment ([x | e | nbr] in the wide role), the un-merged loop of wgrad_gnn_all, host
batches staged through st_nbr, ptrs[1] of the hipGraph key, PackedBatch.shard cutting nbr, GnnQModel.fit taking nbr[sel].

Judged as tests/test_gpu_depth.py judges (its helpers; tests/util.py: plain fp32 tolerances, ReLU gates at rounding
distance of 0 identified explicitly, nothing redrawn).  Every case asserts the plan it is meant to exercise (path_info, the
launch names of the profile) and, from the oracle ALONE, that its draw is informative: the neighbour input moves (nearly)
every output by far more than the forward tolerance, so kernels that dropped or mis-strided it cannot pass."""
import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine, BS
from oracle import compact as oc, literal as ol
from oracle.keras_semantics import KerasAdam
from util import (ospec, f32_params, random_inputs, oracle_step, assert_close, assert_fwd_close, assert_grad_close,
                  assert_grads_match_oracle, assert_weights_after_adam_step, FWD_RTOL, FWD_ATOL)
from test_gpu_depth import _draw, _engine, _parity

pytestmark = pytest.mark.gpu

MOVED_MIN, MOVED_BY = 0.90, 10.0      # >= 90 % of the outputs move by > 10 x the forward bound when nbr is taken away
FUSED_LAUNCHES = ("k_gnn_fwd_", "k_gnn_bwd_", "k_predict_small", "k_wgrad_all", "k_wgrad_gnn_d0")      # what nbr == NULL may run


def _fwd_bound(q_ref):
    return FWD_RTOL * np.abs(q_ref) + FWD_ATOL * max(1.0, float(np.abs(q_ref).max()))


def _without_nbr(pb):
    return PackedBatch(pb.n_graphs, pb.n_nodes, pb.xe, pb.row_ptr, pb.col_idx, pb.max_edges, graph_off=pb.graph_off,
                       max_nodes=pb.max_nodes)


def _with_nbr(pb, nbr):
    return PackedBatch(pb.n_graphs, pb.n_nodes, pb.xe, pb.row_ptr, pb.col_idx, pb.max_edges, nbr=nbr, graph_off=pb.graph_off,
                       max_nodes=pb.max_nodes)


def _assert_nbr_informative(spec, P, x, e, graph, nbr, what, n_global=None):
    """From the oracle alone (before any GPU result is looked at).  -> (q_ref with nbr, q_ref without)"""
    M = oc.csr_to_matrix(*graph, dtype=np.float64)
    q0, _ = oc.forward(ospec(spec), P, np.asarray(x, np.float64), np.asarray(e, np.float64), M)
    y = np.random.default_rng(12345).normal(2.5, 1.0, size=q0.shape)
    step = oracle_step(spec, P, x, e, graph, y, n_denominator=n_global, nbr=nbr)
    q1 = step['q']
    moved = float((np.abs(q1 - q0) > MOVED_BY * _fwd_bound(q1)).mean())
    ratio = float(np.median(np.abs(q1 - q0) / _fwd_bound(q1)))
    g_w3 = float(np.abs(step['grads']['gnn'][0]['W3']).max())
    print("%s: %.3f of the outputs move by > %g x the forward bound without nbr (median %.0f x); max|d gnn[0].W3| %.3e"
          % (what, moved, MOVED_BY, ratio, g_w3))
    assert moved >= MOVED_MIN, (what, "only %.3f of the outputs depend visibly on the neighbour input" % moved)
    assert g_w3 > 0, (what, "the embed stage's W3 has no gradient")
    return q1, q0


def _no_fused_launch(names, what):
    bad = [n for n in names if n.startswith(FUSED_LAUNCHES)]
    assert not bad, (what, "launches of the nbr == NULL plan", bad, sorted(names))


def _forward_and_gradients(spec, P, x, e, pb, graph, rng, eng, what, n_global=None):
    """Test 1's calls on one engine: forward from the host batch and from the device batch, forward_backward.
    -> launch names of (forward, forward_backward)"""
    q_ref, _ = _assert_nbr_informative(spec, P, x, e, graph, pb.nbr, what, n_global)
    eng.profile(True)
    q = eng.forward(pb)
    names_f = eng.profile_read()
    eng.profile(False)
    assert_fwd_close(q, q_ref, what + ": forward from the host batch")
    assert np.array_equal(eng.forward(eng.to_device(pb)).cpu().numpy(), q), what + ": device batch != host batch"
    names_b = _parity(spec, P, x, e, pb, graph, rng, eng, what, n_global=n_global)
    _no_fused_launch(names_f, what + ": forward")
    _no_fused_launch(names_b, what + ": forward_backward")
    return names_f, names_b


# ------------------------------------------------------------------------------------------------ 1. forward and gradients
FIXED = [  # N, F, L, shared, B: the smallest batches at which each plan still has its structure
    (4, 16, 2, False, 37),       # odd B: row tail of k_gemm_rows and of the weight-gradient chunks
    (20, 64, 2, False, 48),      # without nbr: fused, fragment-major hand-over, Dense-0 as a k_wgrad role
    (20, 64, 2, True, 35),       # one slot, odd B
    (6, 32, 3, False, 50),       # F = 32, three stages
    (4, 16, 8, False, 16),       # nine stage roles: two k_wgrad_gnn launches (WG_MAX_ROLES = 8), the embed in the second
    (5, 128, 2, False, 40),      # k_wide_gemm, stage-0 K = 16 + 128
    (12, 256, 3, True, 16),      # K = 16 + 256: three 128-wide K tiles with a 16-row tail
]


@pytest.mark.parametrize("N,F,L,shared,B", FIXED)
def test_forward_and_gradients_vs_oracle(N, F, L, shared, B):
    what = "nbr N=%d F=%d L=%d %s B=%d" % (N, F, L, "shared" if shared else "per-node", B)
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, shared, B, True, seed=41 * N + F + L + B, with_nbr=True)
    eng = _engine(spec, P)
    info, info0 = eng.path_info(pb), eng.path_info(_without_nbr(pb))
    assert info["graph_layers"] == "layerwise", info
    if F < 128:
        assert info["dense0_dw"] != "k_wgrad" and info["handoff"] == "row-major", info
        assert info0["graph_layers"].startswith("fused"), info0          # the same batch without nbr: the other plan
        if (N, F, B) == (20, 64, 48):
            assert info0["handoff"] == "fragment-major" and info0["dense0_dw"] == "k_wgrad", info0
    names_f, names_b = _forward_and_gradients(spec, P, x, e, pb, graph, rng, eng, what)
    assert {"k_node_fwd_embed", "k_node_fwd"} <= set(names_f) and {"k_node_fwd_embed", "k_node_fwd"} <= set(names_b), (names_f, names_b)
    if F < 128:
        assert names_b.get("k_wgrad_gnn", (0, 0))[0] == (2 if L == 8 else 1), names_b       # the embed role inside it
    else:
        assert "k_wgrad_wide_all" in names_b or "k_wgrad_embed" in names_b, names_b
    eng.close()


# (topology None: the reference's, in-degree n - 2 -- every row has in-neighbours, so every output is large enough against
#  the batch-wide absolute part of the forward bound to show whether nbr reached it; a float: that edge density)
RAGGED = [  # F, L, sizes, topology, aggregation of the layer-wise path
    (32, 2, [2, 40, 7, 1, 33, 16, 5, 24] * 3, None, "edge-gather"),
    (64, 2, [33, 64, 8, 2, 40], 0.9, "dense(complement-or-mfma-per-graph)"),    # max_nodes >= 32, 4 max_edges >= max_nodes^2
]


def _ragged_draw(F, L, sizes, density):
    from test_gpu_fused import _ragged_batch
    rng = np.random.default_rng(37 * F + L + len(sizes))
    spec = GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)
    pb, x, e, offs = _ragged_batch(rng, sizes, 'ref' if density is None else density)
    P = f32_params(spec, rng)
    pb = _with_nbr(pb, rng.normal(0, 0.5, size=(pb.n_rows, F)).astype(np.float32))
    return spec, P, x, e, pb, (offs, pb.row_ptr, pb.col_idx), rng


@pytest.mark.parametrize("F,L,sizes,density,agg", RAGGED)
def test_ragged_forward_and_gradients_vs_oracle(F, L, sizes, density, agg):
    what = "nbr ragged F=%d L=%d %d graphs" % (F, L, len(sizes))
    spec, P, x, e, pb, graph, rng = _ragged_draw(F, L, sizes, density)
    eng = GnnEngine(spec)
    eng.set_weights(oc.params_to_list(P))
    info, info0 = eng.path_info(pb), eng.path_info(_without_nbr(pb))
    assert info["graph_layers"] == "layerwise" and info["aggregation"] == agg, info
    assert info0["graph_layers"] == "fused(ragged)", info0
    _forward_and_gradients(spec, P, x, e, pb, graph, rng, eng, what, n_global=pb.n_rows)
    eng.check_errors()
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. no few-graph shortcut
@pytest.mark.parametrize("N,F,L,B", [(4, 16, 2, 1), (20, 64, 2, 12)])
def test_few_graphs_with_nbr_do_not_take_the_one_launch_predict(N, F, L, B):
    """Host batch in, host q out, <= SMALL_ROWS rows: v2x_forward's pinned-window call.  k_predict_small has no nbr term."""
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=43 * N + F + B, with_nbr=True)
    q_ref, q_ref0 = _assert_nbr_informative(spec, P, x, e, graph, pb.nbr, "few graphs N=%d B=%d" % (N, B))
    eng = GnnEngine(spec)                                  # (V2X_SMALL_PREDICT at its default)
    eng.set_weights(oc.params_to_list(P))
    out = []
    for b in (pb, _without_nbr(pb)):
        eng.profile(True)
        out.append((eng.forward(b), eng.profile_read()))
        eng.profile(False)
    (q, names), (q0, names0) = out
    assert "k_predict_small" in names0, names0             # the same call without nbr is the shortcut
    _no_fused_launch(names, "few graphs")
    assert_fwd_close(q, q_ref, "few graphs with nbr vs oracle")
    assert_fwd_close(q0, q_ref0, "few graphs without nbr vs oracle")
    assert (np.abs(q - q0) > _fwd_bound(q_ref)).mean() >= MOVED_MIN, "the neighbour input did not reach the output"
    assert np.array_equal(eng.forward(pb), q), "not repeatable after the one-launch predict"
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. one model, alternating plans
@pytest.mark.parametrize("N,F,L,B", [(20, 64, 2, 48), (5, 128, 2, 40)])
def test_one_model_alternating_plans(N, F, L, B):
    """Five fit steps of ONE engine, nbr on steps 2 and 4 only: Adam writes every copy of the weights (the fused kernels' packed
    ones, the fragment-major ones) and both plans must see them; then forward_backward with nbr and without: no stale stage-0
    W3 slab may survive into the second gradient.

    Judged step by step (a) as test_gpu_model.test_train_steps_vs_oracle judges, against the oracle's own trajectory, with
    the history rule of util.assert_weights_after_adam_step: an entry is held to the tight bound unless its gradient was at
    rounding-noise level at a step at which its array had one (Adam's moments carry such a step forward); steps without nbr,
    where stage 0's W3 has no gradient at all, change nothing in that -- W3 is held tightly from the first step on; and (b)
    against float64 Keras Adam applied to the ENGINE's gradients (a second engine's forward_backward, each checked against
    the oracle at that engine's weights), every entry within 1e-5 per step taken as in test_gpu_depth: no ill-conditioned
    class, so a stale gradient that keeps feeding Adam cannot hide in it."""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(47 * N + F + B)
    P = f32_params(spec, rng)
    eng, split = GnnEngine(spec), GnnEngine(spec)
    eng.set_weights(oc.params_to_list(P))
    split.set_weights(oc.params_to_list(P))
    om = oc.OracleModel(ospec(spec), P, dtype=np.float64)
    adam64, opt = oc.cast_params(P, np.float64), KerasAdam()
    rows = lambda a: None if a is None else a.reshape(B * N, -1)
    plans, g_hist = [], []
    for step in range(5):
        x, e, adj = random_inputs(rng, B, N)
        nbr = rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32) if step in (1, 3) else None
        pb = PackedBatch.from_dense(x, e, adj, nbr)
        plans.append(eng.path_info(pb)["graph_layers"])
        graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
        y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
        _, g_ref, _ = om.loss_and_grads(rows(x), rows(e), graph, y, rows(nbr))
        if nbr is not None:
            assert np.abs(g_ref['gnn'][0]['W3']).max() > 0
        loss_ref = om.train_step(rows(x), rows(e), graph, y, rows(nbr))
        loss = eng.train_step(pb, y)
        assert_close(loss, loss_ref, 5e-4, 1e-6, "loss at step %d" % step)
        g_hist.append(oc.params_to_list(g_ref))
        assert_weights_after_adam_step(eng.get_weights(), oc.params_to_list(om.params), g_hist, step)
        # (b) the second engine's gradient at its own weights against the oracle, float64 Keras Adam on that gradient
        Ps = oc.params_from_list(ospec(spec), split.get_weights(), np.float64)
        qs = split.forward(pb)
        split.forward_backward(pb, y)
        gs = v2xgnn.flat_to_keras_list(spec, split.get_grad_flat())
        assert_grads_match_oracle(gs, Ps, oracle_step(spec, Ps, rows(x), rows(e), graph, y, q_at=qs, nbr=pb.nbr), "step %d" % step)
        w3 = np.stack([gs[4 * k + 2] for k in range(N)])
        assert w3.any() if nbr is not None else not w3.any(), ("stage-0 W3 gradient at step", step, np.abs(w3).max())
        split.apply_gradients()
        opt.step(oc.param_arrays(adam64), oc.param_arrays(oc.params_from_list(ospec(spec), gs, np.float64)))
        for i, (a, b) in enumerate(zip(eng.get_weights(), oc.params_to_list(adam64))):
            err = np.abs(a.astype(np.float64) - b)
            assert (err <= 1e-5 * (step + 1)).all(), ("train_step vs Keras Adam on the engine's gradients", step, i, err.max())
    split.close()
    if F < 128:
        assert [p.startswith("fused") for p in plans] == [True, False, True, False, True], plans
    assert eng.get_optimizer_state()[2] == 5
    # forward_backward with nbr, then without, at the weights the five steps left
    Pn = oc.params_from_list(ospec(spec), eng.get_weights(), np.float64)
    x, e, adj = random_inputs(rng, B, N)
    nbr = rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32)
    for with_nbr in (True, False):
        pb = PackedBatch.from_dense(x, e, adj, nbr if with_nbr else None)
        graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
        q = eng.forward(pb)
        y = (q + rng.normal(0, 1.2, size=q.shape)).astype(np.float32)
        ref = oracle_step(spec, Pn, rows(x), rows(e), graph, y, q_at=q, nbr=pb.nbr)
        assert_fwd_close(q, ref['q'], "forward, nbr %s" % with_nbr)
        loss = eng.forward_backward(pb, y)
        assert_close(loss, ref['loss'], 2e-4, 1e-6, "loss, nbr %s" % with_nbr)
        g = v2xgnn.flat_to_keras_list(spec, eng.get_grad_flat())
        w3 = np.stack([g[4 * k + 2] for k in range(spec.n_slots)])
        if with_nbr:
            assert np.abs(ref['grads']['gnn'][0]['W3']).max() > 0 and w3.any()
        else:
            assert not w3.any(), "stale stage-0 W3 gradient after a step with nbr: max %.3e in %d entries" % (
                np.abs(w3).max(), np.count_nonzero(w3))
        assert_grads_match_oracle(g, Pn, ref, "gradients, nbr %s" % with_nbr)
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. hipGraph
def test_graph_replay_with_and_without_nbr_matches_eager_bitwise():
    """d.nbr is ptrs[1] of the graph key: a step with nbr and a step without are two graphs of one model; host batches reach
    the kernels through st_nbr, which a larger batch re-allocates."""
    import torch
    N, F, L, B = 20, 64, 2, 48
    pattern = [True, True, False, True, False, False]
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=515, with_nbr=True)
    pb0 = _without_nbr(pb)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    x2, e2, adj2 = random_inputs(rng, 2 * B, N)
    big = PackedBatch.from_dense(x2, e2, adj2, rng.normal(0, 0.5, size=(2 * B, N, F)).astype(np.float32))
    y2 = rng.normal(2.5, 1.0, size=(2 * B * N, 4)).astype(np.float32)
    for on_device in (False, True):
        res = []
        for use_graph in (False, True):
            eng = GnnEngine(spec, use_graph=use_graph)
            eng.set_weights(oc.params_to_list(P))
            with torch.cuda.stream(torch.cuda.Stream()):
                if on_device:
                    b1, b0, b2 = eng.to_device(pb), eng.to_device(pb0), eng.to_device(big)
                    t1, t2 = torch.from_numpy(y).cuda(), torch.from_numpy(y2).cuda()
                else:
                    b1, b0, b2, t1, t2 = pb, pb0, big, y, y2
                losses = [eng.train_step(b1 if has else b0, t1) for has in pattern]
                losses.append(eng.train_step(b2, t2))                     # B = 96: st_nbr grows
                losses.append(eng.train_step(b1, t1))                     # ... and the first graph again
                torch.cuda.synchronize()
                losses = [np.asarray(l.cpu().numpy() if on_device else l) for l in losses]
            m, v, it = eng.get_optimizer_state()
            assert it == len(pattern) + 2
            res.append((eng.get_flat(), np.stack(losses), m, v))
            eng.close()
        for a, b, name in zip(res[0], res[1], ("weights", "losses", "Adam m", "Adam v")):
            assert np.all(np.isfinite(a)), name
            assert np.array_equal(a, b), ("device" if on_device else "host", name, np.abs(a - b).max())


# ------------------------------------------------------------------------------------------------ 6. phased step
@pytest.mark.parametrize("N,F,L,B", [(20, 64, 2, 48), (5, 128, 2, 40)])
def test_phased_step_with_nbr_equals_single_call(N, F, L, B):
    """v2x_forward_backward_phase (2 phases; L + 2 for the wide model) on a batch with nbr: bucket k final after phase k,
    losses and gradients those of v2x_forward_backward bit for bit, over three steps."""
    import torch
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=53 * N + F + B, with_nbr=True)
    y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
    one, two = _engine(spec, P), _engine(spec, P)
    buckets = two.grad_buckets()
    n_ph = L + 2 if F >= 128 else 2
    assert len(buckets) == n_ph and sum(n for _, n in buckets) == two.n_params, buckets
    with torch.cuda.stream(torch.cuda.Stream()):
        db1, db2 = one.to_device(pb), two.to_device(pb)
        yd = torch.from_numpy(y).cuda()
        for it in range(3):
            l1 = one.forward_backward(db1, yd)
            two.grad_tensor().zero_()
            snaps = []
            for k in range(n_ph):
                l2 = two.forward_backward_phase(db2, yd, k)
                assert (l2 is None) == (k < n_ph - 1)
                snaps.append(two.get_grad_flat())
            torch.cuda.synchronize()
            g1, g2 = one.get_grad_flat(), snaps[-1]
            for k, snap in enumerate(snaps):
                for o, n in buckets[:k + 1]:
                    assert np.array_equal(snap[o:o + n], g2[o:o + n]), ("bucket changed after its phase", k, o, n)
            w3 = np.stack([a for a in v2xgnn.flat_to_keras_list(spec, g2)[2:4 * spec.n_slots:4]])
            assert w3.any() and np.all(np.isfinite(g2))
            print("phased N=%d F=%d step %d: max|g_single - g_phased| = %.3e (max|g| %.3e)" % (N, F, it, np.abs(g1 - g2).max(), np.abs(g1).max()))
            assert np.array_equal(l1.cpu().numpy(), l2.cpu().numpy())
            assert np.array_equal(g1, g2), (it, np.abs(g1 - g2).max(), np.count_nonzero(g1 != g2))
            one.apply_gradients()
            two.apply_gradients()
        torch.cuda.synchronize()
    assert np.array_equal(one.get_flat(), two.get_flat())
    one.close()
    two.close()


# ------------------------------------------------------------------------------------------------ 7. shards
def _shards_sum(spec, P, pb, y, n_global, what):
    eng = GnnEngine(spec)
    eng.set_weights(oc.params_to_list(P))
    full_loss = eng.forward_backward(pb, y, n_global=n_global)
    g_full = eng.get_grad_flat().astype(np.float64)
    w3_rows = np.stack(v2xgnn.flat_to_keras_list(spec, g_full)[2:4 * spec.n_slots:4])
    assert np.all(np.isfinite(g_full)) and w3_rows.any()
    acc, loss_acc = np.zeros_like(g_full), np.zeros_like(np.asarray(full_loss, np.float64))
    for r in range(4):
        sh, (r0, r1) = pb.shard(r, 4, with_rows=True)
        assert sh.nbr is not None and np.array_equal(sh.nbr, pb.nbr[r0:r1]) and np.array_equal(sh.xe, pb.xe[r0:r1]), r
        assert eng.path_info(sh)["graph_layers"] == "layerwise"
        loss_acc += eng.forward_backward(sh, y[r0:r1], n_global=n_global)
        acc += eng.get_grad_flat()
    assert_grad_close(acc, g_full, what + ": sum of the four shards' gradients")
    assert_close(loss_acc, full_loss, 1e-5, 1e-7, what + ": sum of the four shards' losses")
    eng.close()


def test_gradient_shards_with_nbr_sum_to_global_gradient():
    N, F, L, B = 20, 64, 2, 64
    spec, P, x, e, pb, graph, rng = _draw(N, F, L, False, B, True, seed=707, with_nbr=True)
    _assert_nbr_informative(spec, P, x, e, graph, pb.nbr, "shards")
    _shards_sum(spec, P, pb, rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32), B, "fixed-size")


def test_ragged_gradient_shards_with_nbr_sum_to_global_gradient():
    F, L, sizes, density, _ = RAGGED[0]
    spec, P, x, e, pb, graph, rng = _ragged_draw(F, L, sizes, density)
    _assert_nbr_informative(spec, P, x, e, graph, pb.nbr, "ragged shards", n_global=pb.n_rows)
    _shards_sum(spec, P, pb, rng.normal(2.5, 1.0, size=(pb.n_rows, 4)).astype(np.float32), pb.n_rows, "ragged")


# ------------------------------------------------------------------------------------------------ 8. dqn_step
@pytest.mark.parametrize("N,F,L,B", [(4, 16, 2, 24), (20, 64, 2, 32)])
def test_dqn_step_with_nbr_vs_oracle(N, F, L, B):
    """v2x_dqn_step with a neighbour input of its own on s and on s': target forward, online forward, target rule, fit step
    against the oracle; the captured step equals the eager one bit for bit."""
    from test_gpu_configs import _check_dqn_step, _run_dqn_step
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(59 * N + F + B)
    w_online, w_target = (oc.params_to_list(oc.cast_params(f32_params(spec, rng), np.float32)) for _ in range(2))
    x, e, adj = random_inputs(rng, B, N)
    x2, e2, _ = random_inputs(rng, B, N)
    nbr, nbr2 = (rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32) for _ in range(2))
    graph = oc.adj_to_csr(adj)
    rows = lambda a: a.reshape(B * N, -1)
    os_ = ospec(spec)
    for w, xx, ee, nn, which in ((w_online, x, e, nbr, "s"), (w_target, x2, e2, nbr2, "s'")):
        _assert_nbr_informative(spec, oc.params_from_list(os_, w, np.float64), rows(xx), rows(ee), graph, rows(nn), "dqn " + which)
    args = (spec, w_online, w_target, x, e, adj, x2, e2, rng.integers(0, 4, size=(B, N)), rng.normal(2.4, 0.3, size=B), 0.5)
    y, loss, w1 = _check_dqn_step(*args, nbr=nbr, nbr2=nbr2)
    yg, lossg, wg = _run_dqn_step(*args, nbr=nbr, nbr2=nbr2, use_graph=True)
    assert np.array_equal(y, yg) and np.array_equal(loss, lossg)
    for i, (a, b) in enumerate(zip(w1, wg)):
        assert np.array_equal(a, b), ("captured dqn_step != eager: weight array", i)


# ------------------------------------------------------------------------------------------------ 9. dict payload
def test_dict_payload_with_nbr_through_fit():
    """The reference's dict payload with non-zero D{k}_Neighbor_Input: one fit step through v2x_pack_feed, then three
    minibatch steps through feed_to_arrays and nbr[sel]."""
    B = 24
    brain = BS(4, 3, 1, 16, 1, 4, seed=0)
    model = brain.model
    spec = model.spec
    N, F = spec.n_nodes, spec.feat_dim
    assert (N, F, spec.n_mp_layers) == (4, 16, 2)
    rng = np.random.default_rng(61)
    P = f32_params(spec, rng)
    model.set_weights(oc.params_to_list(P))
    x, e, adj = random_inputs(rng, B, N)
    nbr = rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32)
    yt = rng.normal(2.5, 1.0, size=(B, N, 4)).astype(np.float32)
    feed = ol.feed_from_compact(ospec(spec), x, e, adj, nbr)
    targets = {'D%d_Decide_Output' % (k + 1): yt[:, k, :] for k in range(N)}
    pb = model._pack_batch(feed)
    assert pb.nbr is not None and np.array_equal(pb.nbr, nbr.reshape(B * N, F))
    assert np.array_equal(model._pack(feed)[2], nbr)
    rows = lambda a: a.reshape(-1, a.shape[-1])
    _assert_nbr_informative(spec, P, rows(x), rows(e), oc.adj_to_csr(adj), rows(nbr), "dict payload")
    om = oc.OracleModel(ospec(spec), P, dtype=np.float64)

    def oracle(sel):
        graph = oc.adj_to_csr(adj[sel])
        a = (rows(x[sel]), rows(e[sel]), graph, rows(yt[sel]), rows(nbr[sel]))
        _, g, _ = om.loss_and_grads(*a)
        return om.train_step(*a), oc.params_to_list(g)

    def check_history(hist, loss_ref, what):
        got = np.array([hist.history['D%d_Decide_Output_loss' % (k + 1)][0] for k in range(N)])
        assert_close(got, loss_ref, 2e-4, 1e-6, what + ": per-output losses of the History")
        assert_close(hist.history['loss'][0], loss_ref.sum(), 2e-4, 1e-6, what + ": total loss of the History")

    loss_ref, g0 = oracle(np.arange(B))
    check_history(model.fit(feed, targets, batch_size=B), loss_ref, "one step")
    assert_weights_after_adam_step(model.get_weights(), oc.params_to_list(om.params), g0, 0, "one step")
    steps = [oracle(np.arange(s, s + 8)) for s in range(0, B, 8)]
    check_history(model.fit(feed, targets, batch_size=8, shuffle=False), np.mean([l for l, _ in steps], axis=0), "three minibatches")
    assert_weights_after_adam_step(model.get_weights(), oc.params_to_list(om.params), [g0] + [g for _, g in steps], 3, "three minibatches")
    assert model.engine.get_optimizer_state()[2] == 4
    brain.model.close()
    brain.target_model.close()
