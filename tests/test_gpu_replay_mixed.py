"""GPU: a replay minibatch of graphs of different sizes assembled in one launch (v2x_replay_gather_mixed, csrc/kernels.hpp
k_replay_gather_mixed) and rl/mixed.py's MixedReplay on top of it, against a numpy assembly -- bit for bit, all seven outputs.

Pools of 4, 12, 20 and 31 links at capacity 64 in the storage layout of rl/replay.py; slot lists that are non-monotone and
repeat slots; an empty pool; a one-pool call and an eight-pool call; output buffers pre-filled with a sentinel and one element
longer than needed, so that a store past the written extents shows; the assembled batch through GnnEngine.validate;
MixedReplay.sample on rings that have wrapped; an irregular transition counted and not stored.
"""
import ctypes as C

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec
from v2xgnn import lib as vlib
from v2xgnn.engine import DeviceBatch
from oracle import compact as oc

pytestmark = pytest.mark.gpu

CAP = 64
SENTINEL = -77


def _pool(rng, n, cap=CAP):
    """random storage of one link count: xe, xe_next [cap, n, 16], col [cap, n (n - 2)] (reference topology, graph-local
    ascending sources), action [cap, n], reward [cap]"""
    adj = oc.random_topology(rng, cap, n)
    _, _, ci = oc.adj_to_csr(adj)
    return dict(n=n, xe=rng.normal(size=(cap, n, 16)).astype(np.float32), xe_next=rng.normal(size=(cap, n, 16)).astype(np.float32),
                col=ci.reshape(cap, n * (n - 2)).astype(np.int32), action=rng.integers(0, 4, size=(cap, n)).astype(np.int32),
                reward=rng.normal(size=cap).astype(np.float64))


def numpy_assembly(pools, slots):
    """pools: storages in batch order; slots[k]: storage slots of pool k -> the seven arrays of the ragged minibatch"""
    xe, xn, act, rew, col, sizes = [], [], [], [], [], []
    for p, s in zip(pools, slots):
        s = np.asarray(s, np.int64)
        n = p['n']
        xe.append(p['xe'][s].reshape(-1, 16)); xn.append(p['xe_next'][s].reshape(-1, 16))
        act.append(p['action'][s].reshape(-1)); rew.append(p['reward'][s]); col.append(p['col'][s].reshape(-1))
        sizes += [n] * len(s)
    sizes = np.asarray(sizes, np.int64)
    graph_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(np.repeat(sizes - 2, sizes))]).astype(np.int32)
    cat = lambda v, dt: np.concatenate(v).astype(dt)
    return dict(xe=cat(xe, np.float32), xe_next=cat(xn, np.float32), action=cat(act, np.int32), reward=cat(rew, np.float64),
                graph_off=graph_off, row_ptr=row_ptr, col_idx=cat(col, np.int32))


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def _gather(pools, slots):
    """one v2x_replay_gather_mixed call -> the seven output arrays (their written extents), after checking the sentinel behind"""
    import torch
    lib = v2xgnn.load_library()
    want = numpy_assembly(pools, slots)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep, table = [], (vlib.ReplayPool * len(pools))()
    for k, (p, s) in enumerate(zip(pools, slots)):
        table[k].n_nodes, table[k].count = p['n'], len(s)
        if len(s) == 0:
            continue                                   # (an empty pool may leave its pointers null)
        t = {name: dev(p[name]) for name in ("xe", "xe_next", "col", "action", "reward")}
        t['idx'] = dev(np.asarray(s, np.int32))
        keep.append(t)
        for name, v in t.items():
            setattr(table[k], name, v.data_ptr())
    out = {}
    for name, w in want.items():                       # one element (one xe row) more than needed, all sentinel
        shape = (w.shape[0] + 1,) + w.shape[1:]
        out[name] = torch.full(shape, SENTINEL, dtype=getattr(torch, str(w.dtype)), device="cuda")
    desc = vlib.MixedBatch(**{k: v.data_ptr() for k, v in out.items()})
    vlib.check(lib, lib.v2x_replay_gather_mixed(len(pools), table, C.byref(desc), None), None)
    torch.cuda.synchronize()
    got = {}
    for name, w in want.items():
        a = out[name].cpu().numpy()
        assert (a[w.shape[0]:] == SENTINEL).all(), "%s: written past its extent" % name
        got[name] = a[:w.shape[0]]
        _same_bits(got[name], w, name)
    return out, want


def test_gather_mixed_equals_numpy_assembly_bitwise():
    rng = np.random.default_rng(41)
    pools = [_pool(rng, n) for n in (4, 12, 20, 31)]
    slots = [[5, 3, 3, 63, 0, 17, 5], [], [9, 8, 7, 7, 60], [1, 62, 1]]                      # non-monotone, repeated; 12 links empty
    out, want = _gather(pools, slots)
    # the assembled arrays are a valid ragged batch (the layout contract of include/v2xgnn.h)
    B, R, E = len(want['reward']), len(want['action']), len(want['col_idx'])
    eng = v2xgnn.GnnEngine(GnnSpec(n_nodes=1, feat_dim=16, share_weights=True, variable_graphs=True))
    for xe in (out['xe'], out['xe_next']):
        db = DeviceBatch.from_tensors(B, 0, xe[:R], out['row_ptr'][:R + 1], out['col_idx'][:E], 31 * 29, graph_off=out['graph_off'][:B + 1],
                                      max_nodes=31)
        eng.validate(db)
        assert np.isfinite(eng.forward(db).cpu().numpy()).all()
    eng.close()


def test_gather_mixed_one_pool_and_eight_pools():
    rng = np.random.default_rng(42)
    _gather([_pool(rng, 20)], [[63, 0, 31, 31, 2]])
    sizes = (3, 4, 5, 8, 16, 17, 30, 31)
    pools = [_pool(rng, n, cap=16) for n in sizes]
    slots = [list(rng.integers(0, 16, size=c)) for c in (1, 0, 9, 2, 0, 5, 3, 4)]
    _gather(pools, slots)
    _gather(pools, [[], [], [], [], [], [], [], [15]])                                       # only the last pool contributes


def test_gather_mixed_argument_errors():
    import torch
    lib = v2xgnn.load_library()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    desc = vlib.MixedBatch(**{k: buf.data_ptr() for k in ("xe", "xe_next", "action", "reward", "graph_off", "row_ptr", "col_idx")})

    def call(table, n=None, d=desc):
        vlib.check(lib, lib.v2x_replay_gather_mixed(len(table) if n is None else n, table, None if d is None else C.byref(d), None), None)

    def pool(n, count, null=False):
        p = vlib.ReplayPool()
        p.n_nodes, p.count = n, count
        if not null:
            for name in ("xe", "xe_next", "col", "action", "reward", "idx"):
                setattr(p, name, buf.data_ptr())
        return p

    tab = lambda *ps: (vlib.ReplayPool * len(ps))(*ps)
    with pytest.raises(vlib.V2XInvalidArgument, match="counts sum to 0"):
        call(tab(pool(4, 0), pool(8, 0, null=True)))
    for n in (2, 32):
        with pytest.raises(vlib.V2XInvalidArgument, match="n_nodes %d outside 3..31" % n):
            call(tab(pool(4, 1), pool(n, 1)))
    with pytest.raises(vlib.V2XInvalidArgument, match="pool 1 contributes 2 graphs but has a null pointer"):
        call(tab(pool(4, 1), pool(8, 2, null=True)))
    with pytest.raises(vlib.V2XInvalidArgument, match="do not fit int32"):
        call(tab(pool(31, 2 ** 30), pool(31, 2 ** 30)))                                        # (refused before anything is launched)
    with pytest.raises(vlib.V2XInvalidArgument, match="1..8 pools"):
        call(tab(*[pool(4, 1)] * 9))
    with pytest.raises(vlib.V2XInvalidArgument, match="1..8 pools"):
        call(tab(pool(4, 1)), d=None)
    bad = vlib.MixedBatch(**{k: buf.data_ptr() for k in ("xe", "xe_next", "action", "reward", "graph_off", "row_ptr")})
    with pytest.raises(vlib.V2XInvalidArgument, match="null output pointer"):
        call(tab(pool(4, 1)), d=bad)


def _packed_block(rng, n, K, irregular=()):
    """K transitions in the layout BatchedEnviron.observe_packed hands out; `irregular`: transitions whose flag is down (their
    CSR row is zeros, as the simulator leaves it)"""
    adj = oc.random_topology(rng, K, n)
    col = oc.adj_to_csr(adj)[2].reshape(K, n * (n - 2)).astype(np.int32)
    mask = ((adj != 0).astype(np.int64) << np.arange(n, dtype=np.int64)[None, :, None]).sum(axis=1).astype(np.int32)
    regular = np.ones(K, bool)
    regular[list(irregular)] = False
    col[~regular] = 0
    return dict(xe=rng.normal(size=(K, n, 16)).astype(np.float32), xe_next=rng.normal(size=(K, n, 16)).astype(np.float32), col=col,
                mask=mask, regular=regular, action=rng.integers(0, 4, size=(K, n)).astype(np.int32), reward=rng.normal(size=K))


def test_mixed_replay_sample_on_wrapped_rings_and_dropped_irregular():
    from v2xgnn.rl.mixed import MixedReplay
    rng = np.random.default_rng(43)
    cap, sizes = 24, (8, 4, 20)
    mem = MixedReplay(cap, sizes)
    assert mem.sizes == [4, 8, 20]
    fifo = {n: [] for n in sizes}                      # the host's view: every stored transition in arrival order
    for rnd in range(5):                               # 5 x 7 = 35 transitions per size into rings of 24: they wrap
        for n in sizes:
            irregular = (2,) if (rnd == 1 and n == 8) else ()
            b = _packed_block(rng, n, 7, irregular)
            stored = mem.add_many_packed(n, b['xe'], b['xe_next'], b['col'], b['mask'], b['regular'], b['action'], b['reward'])
            assert stored == 7 - len(irregular)
            fifo[n] += [{k: b[k][i] for k in ("xe", "xe_next", "col", "action", "reward")} for i in range(7) if b['regular'][i]]
        if rnd == 2:
            assert len(mem) == 3 * 21 - 1
    assert mem.dropped_irregular == {4: 0, 8: 1, 20: 0}
    assert [mem.stored(n) for n in (4, 8, 20)] == [cap] * 3
    idx = {4: [0, 23, 5, 5], 8: [11], 20: [22, 0, 1, 22, 13]}
    stack = lambda n: dict(n=n, **{k: np.stack([t[k] for t in fifo[n][-cap:]]) for k in ("xe", "xe_next", "col", "action", "reward")})
    want = numpy_assembly([stack(n) for n in (4, 8, 20)], [idx[n] for n in (4, 8, 20)])     # logical index = position among the last `cap`
    for _ in range(2):                                 # the second call reuses the cached output buffers
        sb, sn, action, reward = mem.sample(idx)
        assert sb.graph_off is sn.graph_off and sb.row_ptr is sn.row_ptr and sb.col_idx is sn.col_idx
        assert (sb.n_graphs, sb.n_rows, sb.n_edges, sb.max_nodes, sb.max_edges) == (10, 4 * 4 + 8 + 5 * 20, len(want['col_idx']), 20, 360)
        got = dict(xe=sb.xe, xe_next=sn.xe, action=action, reward=reward, graph_off=sb.graph_off, row_ptr=sb.row_ptr, col_idx=sb.col_idx)
        for name, w in want.items():
            _same_bits(got[name].cpu().numpy(), w, name)
    ptr = sb.xe.data_ptr()
    sb2 = mem.sample({4: [1, 2, 3, 4], 8: [0], 20: [5, 4, 3, 2, 1]})[0]
    assert sb2.xe.data_ptr() == ptr                    # same counts: same buffers (a captured step is replayed)
    sb3 = mem.sample({20: [3]})[0]                     # sizes left out contribute nothing
    assert (sb3.n_graphs, sb3.n_rows, sb3.max_nodes) == (1, 20, 20)
    _same_bits(sb3.xe.cpu().numpy(), fifo[20][-cap:][3]['xe'], "one graph of one pool")
    with pytest.raises(IndexError):
        mem.sample({4: [cap]})
    with pytest.raises(ValueError, match="no pool of 12 links"):
        mem.sample({12: [0]})
    with pytest.raises(ValueError, match="empty minibatch"):
        mem.sample({})
