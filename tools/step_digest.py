#!/usr/bin/env python3
"""Digests of what the library computes on every branch of the training dispatcher, for a bitwise A/B of two builds.

    V2XGNN_LIB=/path/to/libv2xgnn.so python tools/step_digest.py > a.txt       (one fresh process per library)
    python tools/step_digest.py > b.txt && diff a.txt b.txt

Per case one line: path_info, then sha256 of forward's q, of the loss and get_grad_flat() after one forward_backward, and of
get_flat() after three train_steps -- all from fixed seeds.  The cases are the smallest shapes that reach each branch: fused split
tiles, whole tiles with Dense-0 in the MLP launch, shared weights, layer-wise graph layers, F = 16 / 32, eight layers (two
weight-gradient launches), the wide path (also with the profiler's events around every launch), ragged batches on both ragged
kernels and with each of their switches off, a replay step with and without in-kernel targets, the phased backward of a fixed-size,
a wide and a ragged model, the few-graph predict from a host and from a device batch, a non-zero Neighbor_Input, the MFMA
aggregation against bit masks, whole tiles in both aggregation forms or in one direction only, the row-major hand-off, and
V2X_MLP_WG0 forced either way.  Nothing here is a tolerance: two builds that compute the same print the same text."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import v2xgnn  # noqa: E402
from v2xgnn import GnnEngine, GnnSpec, PackedBatch  # noqa: E402


def sha(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def weights(spec, rng):
    return [rng.normal(0, 0.05, size=s).astype(np.float32) if len(s) == 1 else
            rng.uniform(-np.sqrt(6.0 / sum(s)), np.sqrt(6.0 / sum(s)), size=s).astype(np.float32)
            for s in v2xgnn.keras_list_shapes(spec)]


class env(object):
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


def info_text(eng, pb):
    return " ".join("%s=%s" % kv for kv in sorted(eng.path_info(pb).items()))


def fit_case(name, spec, pb, y, w, n_global=None, profile=False):
    eng = GnnEngine(spec)
    eng.set_weights(w)
    if profile:
        eng.profile(True)               # (HIP events around every launch: steps run eagerly, never as a replayed graph)
    info = info_text(eng, pb)
    q = eng.forward(pb)
    loss = eng.forward_backward(pb, y, n_global=n_global)
    g = eng.get_grad_flat()
    eng.set_weights(w)
    for _ in range(3):
        eng.train_step(pb, y, n_global=n_global)
    print("%-34s %s | q %s loss %s grad %s flat3 %s" % (name, info, sha(q), sha(loss), sha(g), sha(eng.get_flat())), flush=True)
    eng.close()


def dense_case(name, N, F, L, B, share=False, nbr=False, keep=1.0, profile=False, **switches):
    """nbr: a non-zero Neighbor_Input; keep < 1: only that share of the edges (too sparse for the complement form)"""
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=share)
    rng = np.random.default_rng(1000 + 7 * N + F + 3 * L + B)
    x, e, adj, y = bench.synth_batch(rng, B, N)
    w = weights(spec, rng)
    if keep < 1.0:
        adj = adj * (rng.random(adj.shape) < keep)
    nb = rng.normal(0.0, 0.5, size=(B, N, F)).astype(np.float32) if nbr else None
    with env(**switches):               # (set from before the engine exists until it is closed: read at create or per call)
        fit_case(name, spec, PackedBatch.from_dense(x, e, adj, nb), y, w, profile=profile)


def ragged_batch():
    spec = GnnSpec(n_nodes=1, feat_dim=64, n_mp_layers=2, share_weights=True, variable_graphs=True)
    rng = np.random.default_rng(77)
    sizes, offs, row_ptr, cols, x, e, y = bench.synth_ragged(rng, 24, 8, 40)
    pb = PackedBatch(len(sizes), 0, v2xgnn.pack_xe(x, e), row_ptr, cols, graph_off=offs)
    return spec, pb, y, weights(spec, rng), int(offs[-1])


def ragged_case(name, **switches):
    spec, pb, y, w, rows = ragged_batch()
    with env(**switches):
        fit_case(name, spec, pb, y, w, n_global=rows)


def predict_case(name, N, F, B):
    """the few-graph predict: the same batch from host memory (the pinned window) and from device memory; path_info describes a
    fit step of the batch, so the kernels a forward alone launches are read from the profiler afterwards"""
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(500 + N + F + B)
    x, e, adj, _ = bench.synth_batch(rng, B, N)
    pb = PackedBatch.from_dense(x, e, adj)
    eng = GnnEngine(spec)
    eng.set_weights(weights(spec, rng))
    db = eng.to_device(pb)
    q = [sha(eng.forward(b)) for b in (pb, db)]
    eng.profile(True)
    ran = []
    for b in (pb, db):
        eng.forward(b)
        ran.append(",".join("%s*%d" % (k, c) for k, (c, _) in sorted(eng.profile_read().items())))
    print("%-34s %s | q host %s device %s launches host %s device %s" % (name, info_text(eng, pb), q[0], q[1], ran[0], ran[1]), flush=True)
    eng.close()


def dqn_case(name, N, F, B, **switches):
    with env(**switches):
        dqn_run(name, N, F, B)


def dqn_run(name, N, F, B):
    import torch
    spec = GnnSpec(n_nodes=N, feat_dim=F)
    rng = np.random.default_rng(31)
    x, e, adj, _ = bench.synth_batch(rng, B, N)
    x2, e2, _, _ = bench.synth_batch(rng, B, N)
    online, target = GnnEngine(spec), GnnEngine(spec)
    online.set_weights(weights(spec, rng))
    target.set_weights(weights(spec, rng))
    sb, sn = online.to_device(PackedBatch.from_dense(x, e, adj)), online.to_device(PackedBatch.from_dense(x2, e2, adj))
    y = torch.empty((B * N, 4), dtype=torch.float32, device="cuda")
    action = torch.from_numpy(rng.integers(0, 4, size=(B, N)).astype(np.int32)).cuda()
    reward = torch.from_numpy(rng.normal(1.0, 0.5, size=B)).cuda()
    loss = online.dqn_step(target, sb, sn, action, reward, 0.5, y_out=y)
    torch.cuda.synchronize()
    print("%-34s %s | y %s loss %s flat1 %s" % (name, info_text(online, sb), sha(y), sha(loss), sha(online.get_flat())), flush=True)
    online.close()
    target.close()


def phase_case(name, N, F, L, B):
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L)
    rng = np.random.default_rng(2000 + N + F + B)
    x, e, adj, y = bench.synth_batch(rng, B, N)
    phase_run(name, spec, PackedBatch.from_dense(x, e, adj), y, weights(spec, rng))


def phase_run(name, spec, pb, y, w, n_global=None):
    import torch
    eng = GnnEngine(spec)
    eng.set_weights(w)
    db = eng.to_device(pb)
    yd = torch.from_numpy(y).cuda()
    eng.grad_tensor().zero_()
    out, loss = [], None
    for k in range(len(eng.grad_buckets())):
        loss = eng.forward_backward_phase(db, yd, k, n_global=n_global)
        torch.cuda.synchronize()
        out.append(sha(eng.get_grad_flat()))
    print("%-34s %s | loss %s grad after each phase %s" % (name, info_text(eng, db), sha(loss), " ".join(out)), flush=True)
    eng.close()


def main():
    print("library: %s" % os.environ.get("V2XGNN_LIB", "the tree's own"), file=sys.stderr)
    dense_case("n20 f64 l2 b64 per-node", 20, 64, 2, 64)
    dense_case("n20 f64 l2 b4096 per-node", 20, 64, 2, 4096)
    dense_case("n20 f64 l2 b16 shared", 20, 64, 2, 16, share=True)
    dense_case("n30 f64 l2 b32 layer-wise", 30, 64, 2, 32)
    dense_case("n4 f16 l2 b64", 4, 16, 2, 64)
    dense_case("n12 f32 l1 b40", 12, 32, 1, 40)
    dense_case("n40 f32 l8 b130 shared", 40, 32, 8, 130, share=True)
    dense_case("n24 f128 l2 b8 wide", 24, 128, 2, 8)
    ragged_case("ragged 24 graphs of 8-40")
    ragged_case("ragged, V2X_RAGGED_SMALL=1", V2X_RAGGED_SMALL=1)
    dqn_case("dqn_step n20 f64 b64", 20, 64, 64)
    phase_case("phases n20 f64 l2 b64", 20, 64, 2, 64)
    phase_case("phases n24 f128 l2 b8 wide", 24, 128, 2, 8)
    dense_case("n20 f64 l2 b64, V2X_MLP_WG0=1", 20, 64, 2, 64, V2X_MLP_WG0=1)
    dense_case("n20 f64 l2 b64, V2X_MLP_WG0=0", 20, 64, 2, 64, V2X_MLP_WG0=0)
    predict_case("predict n20 f64 b4", 20, 64, 4)
    dense_case("n20 f64 l2 b16 Neighbor_Input", 20, 64, 2, 16, nbr=True)
    dense_case("n100 f64 l2 b4 shared, dense", 100, 64, 2, 4, share=True)
    phase_run("phases ragged 24 graphs of 8-40", *ragged_batch())
    ragged_case("ragged, V2X_RAGGED_FUSED_BWD=0", V2X_RAGGED_FUSED_BWD=0)
    ragged_case("ragged, V2X_RAGGED_PACKED=0", V2X_RAGGED_PACKED=0)
    ragged_case("ragged, V2X_RAGGED_PLAN_FOLD=0", V2X_RAGGED_PLAN_FOLD=0)
    dense_case("n20 b64, V2X_FUSED_SPLIT=0", 20, 64, 2, 64, V2X_FUSED_SPLIT=0)
    dense_case("n20 b64 sparse, V2X_FUSED_SPLIT=0", 20, 64, 2, 64, keep=0.3, V2X_FUSED_SPLIT=0)
    dense_case("n20 b64, V2X_FUSED_SPLIT_FWD=0", 20, 64, 2, 64, V2X_FUSED_SPLIT_FWD=0)
    dense_case("n20 b64, V2X_FUSED_SPLIT_BWD=0", 20, 64, 2, 64, V2X_FUSED_SPLIT_BWD=0)
    dqn_case("dqn_step, V2X_DQN_FUSED_TARGETS=0", 20, 64, 64, V2X_DQN_FUSED_TARGETS=0)
    dense_case("n20 b64, V2X_FRAG_HANDOFF=0", 20, 64, 2, 64, V2X_FRAG_HANDOFF=0)
    dense_case("n24 f128 l2 b8 wide, profiled", 24, 128, 2, 8, profile=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
