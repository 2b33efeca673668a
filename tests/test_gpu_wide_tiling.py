"""GPU: the wide-feature GEMMs (feat_dim >= 128, csrc/kernels_wide.hpp) as 64-row half tiles, and the wide switches no other
suite sets.  launch_wide_gemm cuts the row blocks of an under-filled last round into two half tiles each -- wide_gemm_body<.., 1>,
the `half` branch of k_wide_gemm, wide_run_order over the half units -- by comparing the launch with the chip's 5 x CUs resident
slots, which no small shape reaches.  V2X_WIDE_SLOTS makes the rule plan for a handful of slots instead, and nothing else, so that
a few hundred rows reach it; v2x_debug_wide_tiling reports what every launch really was.

  a  half tiles are bit for bit whole tiles: forward, gradient, loss and the weights after a fit step, for several borders between
     whole and half tiles per shape -- a last row block of 12 rows (second half skipped), of 72 rows (second half 8 rows), three
     row blocks per weight slot with the plain-order remainder of wide_run_order, one shared weight slot, 4 and 8 column tiles,
     Dense-0's 5-tile strip, the V2X_WIDE_TAIL=2 rule
  b  one of them against the float64 oracle (the tolerances and MAX_GATE_FLIPS of tests/util.py)
  c  a captured and replayed hipGraph of the half-tiled fit step against eager whole tiles
  d  the chip's own slot count, no override: 99 links x 801 graphs
  e  V2X_WIDE_FOLD=0: the [x | e] segment as a K tile of its own in the merged weight-gradient launch, against the oracle
  f  V2X_WIDE_ADAM=0 where the default plan applies Adam in the weight-gradient epilogues

A tile's rows are independent and every output element sums its K chunks in the same order whichever tile it is in, so (a), (c)
and (d) compare with np.array_equal.  Each compared engine first runs another draw of the same shape: a tile that is never
written then shows that draw's values.  A case whose launches turn out to be whole tiles fails."""
import ctypes as C

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch, GnnEngine
from v2xgnn import lib as vlib
from oracle import compact as oc
from util import ospec, f32_params, random_inputs, oracle_step, assert_close, assert_grads_match_oracle, assert_weights_after_adam_step
import test_gpu_launch_sizes
from test_gpu_launch_sizes import _engine, _draw, _parity, _slabs

pytestmark = pytest.mark.gpu

H1 = 80          # Dense-0's output width (the 5-tile strip)


def _plan(n_idx, grid_z, n_out, slots, tail):
    out = (C.c_int32 * 4)()
    assert vlib.load_library().v2x_wide_tiling_plan(n_idx, grid_z, n_out, slots, tail, out) == 0
    return tuple(int(v) for v in out)


def _launches(spec, B, slots, tail, backward):
    """[(kind, expected tiling)] of the wide GEMM launches of a forward (and a backward) in launch order: the node updates of stages
    0 .. L, Dense-0; Dense-0's data gradient, the stages' data gradients L .. 1.  Per-node weights: B rows in each of N weight
    slots; shared weights: one slot of B x N rows."""
    N, F, L = spec.n_nodes, spec.feat_dim, spec.n_mp_layers
    n_idx, gz = (B * N, 1) if spec.share_weights else (B, N)
    p = lambda n_out: _plan(n_idx, gz, n_out, slots, tail)
    seq = [("stage", p(F))] * (L + 1) + [("dense0", p(H1))]
    if backward:
        seq += [("dense0_dgrad", p(2 * F))] + [("dgrad", p(2 * F))] * L
    return seq


def _halved(t):
    return t[2] < t[3]


def _weights_and_batches(spec, B, seed):
    """weights, the compared batch and targets, another draw of the same shape"""
    rng, P, x, e, pb = _draw(spec, B, True, seed)
    y = rng.normal(2.5, 1.0, size=(B * spec.n_nodes, 4)).astype(np.float32)
    rng2, _, _, _, pb2 = _draw(spec, B, True, seed + 1000)
    y2 = rng2.normal(-1.0, 2.0, size=y.shape).astype(np.float32)
    return oc.params_to_list(P), pb, y, pb2, y2


def _run(eng, w, pb, y, pb2, y2, fit=True):
    """-> the compared results and the tilings recorded by each compared call, after a pass over the other draw"""
    eng.set_weights(w)
    eng.forward_backward(pb2, y2)
    eng.wide_tiling()
    out, rec = {}, {}
    out["q"] = np.array(eng.forward(pb))
    rec["forward"] = eng.wide_tiling()[0]
    out["loss"] = np.array(eng.forward_backward(pb, y))
    out["grad"] = np.array(eng.get_grad_flat())
    rec["forward_backward"] = eng.wide_tiling()[0]
    if fit:
        out["fit_loss"] = np.array(eng.train_step(pb, y))
        out["weights"] = np.array(eng.get_flat())
        rec["train_step"] = eng.wide_tiling()[0]
    return out, rec


def _assert_recorded(rec, spec, B, slots, tail, what):
    for call, got in rec.items():
        want = [t for _, t in _launches(spec, B, slots, tail, call != "forward")]
        assert got == want, (what, call, got, want)


def _assert_same_bits(got, ref, what):
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].size > 0, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), float(np.abs(got[k] - ref[k]).max()))


# ---------------------------------------------------------------------------------------------------------------- a
# (N, F, L, shared, B), the (V2X_WIDE_TAIL, V2X_WIDE_SLOTS) of the compared engines, and the edge the shape is here for as a
# predicate over the {(kind, tiling)} the engines recorded.  T = n_rb x ny tiles against the planned slots (test_wide_tiling_host.py
# has the rule): e.g. 140 graphs x 5 slots x 128 features on 12 slots is 20 stage tiles, rem 8 -> row blocks 6 .. 9 as half tiles.
def _edge_last_block(rows):
    """per-node weights, two row blocks per slot, the second of `rows` rows: it is the last block of the enumeration, so any half
    region holds it"""
    def edge(seen, B):
        assert B % 128 == rows
        return any(k == "stage" and _halved(t) and t[1] == 2 for k, t in seen)
    return edge


def _edge_remainder_across_slots(seen, B):
    """three blocks per slot; a half region that starts in one weight slot and ends in the next, with a whole run of 8 half units
    and a plain-order remainder"""
    return any(k == "stage" and t[1] == 3 and t[2] // 3 < (t[3] - 1) // 3 and 2 * (t[3] - t[2]) > 8 and 2 * (t[3] - t[2]) % 8
               for k, t in seen)


def _edge_shared(seen, B):
    """one weight slot of 300 rows: the last row block (44 rows across graph borders) as half tiles, forward and transposed"""
    return {k for k, t in seen if t[3] == 3 and t[2] == 2} >= {"stage", "dgrad"}


def _edge_wide_columns(seen, B):
    """4 column tiles forward, 8 (512 columns) transposed"""
    return any(k == "stage" and t[0] == 4 and _halved(t) for k, t in seen) and any(k == "dgrad" and t[0] == 8 and _halved(t) for k, t in seen)


A_CASES = [
    ((5, 128, 1, False, 140), [(1, 8), (2, 8), (1, 12), (2, 12), (1, 16), (2, 16)], _edge_last_block(12)),
    ((5, 128, 2, False, 200), [(1, 6), (2, 6), (1, 12), (2, 12), (2, 16)], _edge_last_block(72)),
    ((5, 128, 1, False, 300), [(1, 18), (2, 18), (1, 20), (2, 22), (1, 24)], _edge_remainder_across_slots),
    ((12, 128, 1, True, 25), [(1, 4), (2, 4), (2, 5), (2, 7), (1, 8)], _edge_shared),
    ((5, 256, 1, False, 140), [(1, 12), (2, 12), (1, 16), (2, 18), (1, 24)], _edge_wide_columns),
]


@pytest.mark.parametrize("shape,engines,edge", A_CASES, ids=["%dx%dx%d-%s-B%d" % (s[0], s[1], s[2], "shared" if s[3] else "pernode", s[4])
                                                            for s, _, _ in A_CASES])
def test_a_half_tiles_are_bit_for_bit_whole_tiles(shape, engines, edge):
    N, F, L, shared, B = shape
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    w, pb, y, pb2, y2 = _weights_and_batches(spec, B, seed=3 * N + F + L + B)
    whole = _engine(spec, dict(V2X_WIDE_TAIL=0, V2X_WIDE_SLOTS=engines[0][1]))
    ref, rec = _run(whole, w, pb, y, pb2, y2)
    whole.close()
    _assert_recorded(rec, spec, B, engines[0][1], 0, "whole tiles")
    assert all(not _halved(t) for call in rec.values() for t in call), rec
    assert len(rec["forward"]) == L + 2 and len(rec["train_step"]) == 2 * L + 3, rec
    seen = set()
    for tail, slots in engines:
        what = "N=%d F=%d L=%d B=%d V2X_WIDE_TAIL=%d V2X_WIDE_SLOTS=%d" % (N, F, L, B, tail, slots)
        eng = _engine(spec, dict(V2X_WIDE_TAIL=tail, V2X_WIDE_SLOTS=slots))
        got, rec = _run(eng, w, pb, y, pb2, y2)
        eng.close()
        print("a %s: forward_backward %s" % (what, rec["forward_backward"]))
        _assert_recorded(rec, spec, B, slots, tail, what)
        assert rec["train_step"] == rec["forward_backward"]
        assert any(_halved(t) for t in rec["forward_backward"]), (what, "whole tiles after all", rec)
        seen |= {(k, t) for (k, _), t in zip(_launches(spec, B, slots, tail, True), rec["forward_backward"])}
        if tail == 2:
            seen |= {("dense0@2", rec["forward"][L + 1])}
        _assert_same_bits(got, ref, what)
    halved = {k for k, t in seen if _halved(t)}
    assert halved >= {"stage", "dgrad", "dense0_dgrad", "dense0@2"}, (halved, sorted(seen))
    assert any(k == "dense0@2" and t[2] == 0 for k, t in seen), sorted(seen)       # the V2X_WIDE_TAIL=2 rule: every block of the strip
    assert edge(seen, B), sorted(seen)


# ---------------------------------------------------------------------------------------------------------------- b
def _record_at_close(monkeypatch):
    """-> a list that receives eng.wide_tiling() of the engine _parity makes, read when _parity closes it after its checks"""
    recs = []

    def recording_engine(spec, switches, **kw):
        eng = _engine(spec, switches, **kw)
        close = eng.close

        def recording_close():
            if eng._h:
                recs.append(eng.wide_tiling())
            close()
        eng.close = recording_close
        return eng
    monkeypatch.setattr(test_gpu_launch_sizes, "_engine", recording_engine)
    return recs


def test_b_half_tiles_against_the_oracle(monkeypatch):
    """5 links x 200 graphs x 128 features, two stages, planned for 12 slots at V2X_WIDE_TAIL=2: row blocks 6 .. 9 of the node
    updates, block 9 of the data gradients and all of Dense-0's strip as half tiles, the last of each slot with 72 rows"""
    N, F, L, B = 5, 128, 2, 200
    recs = _record_at_close(monkeypatch)
    _parity(N, F, L, False, B, True, dict(V2X_WIDE_TAIL=2, V2X_WIDE_SLOTS=12), "half tiles")
    (tiles, roles), = recs
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    want = [t for _, t in _launches(spec, B, 12, 2, False) + _launches(spec, B, 12, 2, True)]
    print("b: %s" % (tiles,))
    assert tiles == want, (tiles, want)
    assert tiles[:L + 2] == [(2, 2, 6, 10)] * (L + 1) + [(1, 2, 0, 10)] and tiles[-1] == (4, 2, 9, 10), tiles
    assert len(roles) == L + 2, roles


# ---------------------------------------------------------------------------------------------------------------- c
def test_c_replayed_graph_of_half_tiled_fit_steps():
    """three fit steps of one batch: a captured hipGraph of the half-tiled step (planned for 18 slots, V2X_WIDE_TAIL=2), replayed
    twice, against eager whole tiles -- the same weights after every step; only the capture records its launches"""
    import torch
    N, F, L, B = 5, 128, 1, 300
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    w, pb, y, pb2, y2 = _weights_and_batches(spec, B, seed=77)
    eager = _engine(spec, dict(V2X_WIDE_TAIL=0))
    graph = _engine(spec, dict(V2X_WIDE_TAIL=2, V2X_WIDE_SLOTS=18), use_graph=True)
    for eng in (eager, graph):
        eng.set_weights(w)
    db, yd = graph.to_device(pb), torch.from_numpy(y).cuda()
    stream = torch.cuda.Stream()
    want = [t for _, t in _launches(spec, B, 18, 2, True)]
    assert sum(_halved(t) for t in want) == len(want), want
    for step in range(3):
        with torch.cuda.stream(stream):
            lg = graph.train_step(db, yd)
        stream.synchronize()
        le = eager.train_step(pb, y)
        tiles = graph.wide_tiling()[0]
        print("c step %d: recorded %s" % (step, tiles))
        assert tiles == (want if step == 0 else []), (step, tiles, want)
        assert np.array_equal(lg.cpu().numpy(), le), step
        assert np.array_equal(graph.get_flat(), eager.get_flat()), step
    assert all(not _halved(t) for t in eager.wide_tiling()[0])
    eager.close()
    graph.close()


# ---------------------------------------------------------------------------------------------------------------- d
def test_d_the_chips_own_slot_count():
    """99 links x 801 graphs x 128 features, one stage, per-node weights, no V2X_WIDE_SLOTS: on 256 CUs the node update is
    7 x 99 = 693 row blocks x 2 = 1386 tiles on 1280 slots, the last 53 blocks as 106 half units (13 runs of 8 and a remainder of 2),
    the last block of every slot with 33 rows"""
    import torch
    N, F, L, B = 99, 128, 1, 801
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    want = _launches(spec, B, 5 * cus, 1, True)
    if not _halved(want[0][1]):
        pytest.skip("%d CUs: the rule leaves the stage launch of %d x %d rows in whole tiles: %s" % (cus, N, B, want[0][1]))
    w, pb, y, pb2, y2 = _weights_and_batches(spec, B, seed=99)
    whole, default = _engine(spec, dict(V2X_WIDE_TAIL=0)), _engine(spec, {})
    ref, rec0 = _run(whole, w, pb, y, pb2, y2, fit=False)
    whole.close()
    got, rec = _run(default, w, pb, y, pb2, y2, fit=False)
    default.close()
    print("d: %d CUs, forward_backward %s" % (cus, rec["forward_backward"]))
    assert all(not _halved(t) for call in rec0.values() for t in call), rec0
    _assert_recorded(rec, spec, B, 5 * cus, 1, "default engine")
    assert _halved(rec["forward"][0]) and _halved(rec["forward_backward"][-1]), rec
    _assert_same_bits(got, ref, "default engine against V2X_WIDE_TAIL=0")


# ---------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("N,F,L,shared,B", [(5, 128, 2, False, 140), (12, 256, 1, True, 150)])
def test_e_xe_segment_as_a_k_tile_of_its_own_in_the_merged_launch(monkeypatch, N, F, L, shared, B):
    """V2X_WIDE_FOLD=0: every role with an [x | e] segment next to wide ones (the stages 1 .. L and Dense-0; not the embed layer,
    whose only segment it is) takes one K tile more, inside k_wgrad_wide_all -- against the oracle"""
    recs = _record_at_close(monkeypatch)
    _parity(N, F, L, shared, B, True, dict(V2X_WIDE_FOLD=0), "unfolded")
    (_, unfolded), = recs
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    w, pb, y, pb2, y2 = _weights_and_batches(spec, B, seed=5)
    plain = _engine(spec, {})
    plain.set_weights(w)
    plain.forward_backward(pb, y)
    _, folded = plain.wide_tiling()
    plain.close()
    print("e: default roles %s, V2X_WIDE_FOLD=0 roles %s" % (folded, unfolded))
    # the roles as they are planned: stages L .. 1, the embed layer, Dense-0
    assert [r[3] for r in folded] == [1] * L + [0, 1], folded
    assert [r[3] for r in unfolded] == [0] * (L + 2), unfolded
    assert [r[0] for r in folded] == [2 * F // 128] * L + [1, 2 * F // 128], folded
    for f, u in zip(folded, unfolded):
        assert u[0] == f[0] + f[3] and u[1] == f[1], (f, u)
    fit = _engine(spec, dict(V2X_WIDE_FOLD=0))
    fit.set_weights(w)
    fit.profile(True)
    loss = fit.train_step(pb, y)
    names = set(fit.profile_read())
    fit.profile(False)
    assert [r[3] for r in fit.wide_tiling()[1]] == [0] * (L + 2)
    fit.close()
    assert np.all(np.isfinite(loss))
    assert "k_wgrad_wide_all" in names and "k_wgrad_gnn" not in names, names


# ---------------------------------------------------------------------------------------------------------------- f
def test_f_adam_as_a_launch_of_its_own_on_the_wide_path():
    """100 links x 8 graphs x 256 features, per-node weights: 4 K tiles x 100 slots fill the chip, one row split per role
    (0 slabs), so the default fit step applies Adam to the stages 1 .. L and Dense-0 in the weight-gradient epilogues.  With
    V2X_WIDE_ADAM=0 k_reduce_adam does it for every layer from the gradient buffer: that buffer then holds the step's gradient,
    and the step is bit for bit forward_backward + apply_gradients of a default engine -- and Keras Adam."""
    N, F, L, B = 100, 256, 1, 8
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(5 + N + B)
    P = f32_params(spec, rng)
    own, split = _engine(spec, dict(V2X_WIDE_ADAM=0)), _engine(spec, {})
    for eng in (own, split):
        eng.set_weights(oc.params_to_list(P))
    om = oc.OracleModel(ospec(spec), P, dtype=np.float64)
    for step in range(2):
        x, e, adj = random_inputs(rng, B, N)
        pb = PackedBatch.from_dense(x, e, adj)
        y = rng.normal(2.5, 1.0, size=(B * N, 4)).astype(np.float32)
        if step == 0:
            graph = ((np.arange(B + 1) * N).astype(np.int32), pb.row_ptr, pb.col_idx)
            ref = oracle_step(spec, P, x.reshape(B * N, -1), e.reshape(B * N, -1), graph, y)
        ls = split.forward_backward(pb, y)
        grad = split.get_grad_flat().copy()
        gnn, dense, _ = _slabs(split)
        assert gnn[1:] == [0] * L and dense[0] == 0, (gnn, dense)            # one row split: the default plan fuses Adam
        if step == 0:
            g_ref, n_cand, n_flip = assert_grads_match_oracle(v2xgnn.flat_to_keras_list(spec, grad), P, ref, "f: gradient of step 0")
            om.opt.step(oc.param_arrays(om.params), oc.param_arrays(g_ref))
        split.apply_gradients()
        own.profile(True)
        lo = own.train_step(pb, y)
        names = set(own.profile_read())
        own.profile(False)
        print("f step %d: launches %s" % (step, sorted(names)))
        assert "k_reduce_adam" in names and "k_wgrad_wide_all" in names, names
        assert _slabs(own)[:2] == (gnn, dense)
        assert np.array_equal(lo, ls), step
        assert np.array_equal(own.get_grad_flat(), grad), step
        assert np.array_equal(own.get_flat(), split.get_flat()), step
        if step == 0:
            assert_close(lo, ref['loss'], 5e-4, 1e-6, "f: loss at step 0")
            assert_weights_after_adam_step(own.get_weights(), oc.params_to_list(om.params), oc.params_to_list(g_ref), 0, "f")
    assert own.get_optimizer_state()[2] == 2
    own.close()
    split.close()
