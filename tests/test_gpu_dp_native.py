"""GPU: the data-parallel step driven by the library (v2x_train_step_dp, v2x_dqn_step_dp; include/v2xgnn.h) against the
Python trainer (v2xgnn.dp.DataParallelTrainer), which issues the same launches and collectives from Python.

* world 1 with the library's RCCL table, against the Python trainer on the nccl backend with the collective forced;
* two ranks on the box's one GPU (gloo, so the collectives go through dp.TorchComm's callbacks), against the Python trainer
  in the same processes, and the DQN replay step against the single-process v2x_dqn_step;
* the error paths of the collective table, with one rank and callbacks of the test's own.
Every process group is created with a timeout, so a rank that fails cannot leave the other one waiting."""
import datetime
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = datetime.timedelta(seconds=120)
FORMS = (("allreduce", {}), ("buckets", dict(overlap=True)), ("sharded", dict(shard_optimizer=True)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _init(backend, rank, world, port):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=TIMEOUT)
    sys.path.insert(0, HERE)


def _case(name):
    """(spec, flat fp32 parameters, PackedBatch, y, n_global) of a named shape"""
    import v2xgnn
    from v2xgnn import GnnSpec, PackedBatch
    from oracle import compact as oc
    from util import f32_params, random_inputs
    rng = np.random.default_rng(31)
    if name in ("ragged", "ragged_dev"):             # one draw; "ragged_dev" is moved to the device by _run_pair
        spec = GnnSpec(n_nodes=1, feat_dim=64, share_weights=True, variable_graphs=True)
        sizes = rng.integers(8, 41, size=48)
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        rp, cols = [0], []
        for n in sizes:
            adj = rng.random((n, n)) < 0.5
            np.fill_diagonal(adj, False)
            for q in range(n):
                src = np.nonzero(adj[:, q])[0]
                cols.append(src)
                rp.append(rp[-1] + len(src))
        R = int(offs[-1])
        x = rng.normal(0.8, 0.4, size=(R, 9)).astype(np.float32)
        e = rng.normal(0.9, 0.1, size=(R, 4)).astype(np.float32)
        pb = PackedBatch(len(sizes), 0, v2xgnn.pack_xe(x, e), np.array(rp, np.int32), np.concatenate(cols).astype(np.int32),
                         graph_off=offs)
        n_global = R
    else:
        B, N, F = {"b512": (512, 20, 64), "b4096": (4096, 20, 64), "wide": (64, 12, 128), "b256": (256, 20, 64)}[name]
        spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=2)
        x, e, adj = random_inputs(rng, B, N)
        pb = PackedBatch.from_dense(x, e, adj)
        n_global = B
    P = oc.params_to_list(f32_params(spec, rng))
    y = rng.normal(2.5, 1.0, size=(pb.n_rows, 4)).astype(np.float32)
    return spec, P, pb, y, n_global


def _host(loss):
    return loss.cpu().numpy() if hasattr(loss, "cpu") else np.asarray(loss)


def _run_pair(spec, P, pb, y, n_global, kw, comm, steps=3, on_device=None):
    """the Python trainer and the native one, each on its own engine with the same weights: -> [(weights, losses, m, v, it)]
    on_device: the batch and its targets are moved to the device first (default: every batch but a ragged one)"""
    import torch
    from v2xgnn import GnnEngine
    from v2xgnn.dp import DataParallelTrainer
    out = []
    for native in (False, True):
        eng = GnnEngine(spec)
        eng.set_weights(P)
        tr = DataParallelTrainer(eng, force=True, native=native, comm=comm if native else None, **kw)
        sb, sy = tr.shard(pb, y)
        if (pb.graph_off is None) if on_device is None else on_device:
            db, yd = eng.to_device(sb), torch.from_numpy(np.ascontiguousarray(sy)).cuda()
        else:
            db, yd = sb, sy          # the ragged batch stays on the host: the trainers' unphased forms
        torch.cuda.synchronize()
        losses = [_host(tr.train_step(db, yd, n_graphs_global=n_global)) for _ in range(steps)]
        torch.cuda.synchronize()
        m, v, it = tr.gather_optimizer_state()
        out.append((eng.get_flat(), np.stack(losses), m, v, it))
        eng.close()
    return out


def _rccl_worker(rank, world, port, ret):
    _init("nccl", rank, world, port)
    import torch
    import torch.distributed as dist
    try:
        from v2xgnn.dp import RcclComm
        comm = RcclComm()
        res = {}
        with torch.cuda.stream(torch.cuda.Stream()):
            for name in ("b512", "b4096", "wide", "ragged", "ragged_dev"):
                spec, P, pb, y, n_global = _case(name)
                for form, kw in FORMS:
                    res[(name, form)] = _run_pair(spec, P, pb, y, n_global, kw, comm, on_device=(name != "ragged"))
        comm.close()
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_world1_rccl_table_equals_python_trainer_bit_for_bit():
    """The library's RCCL table (one rank) against DataParallelTrainer(force=True) on the nccl backend: three steps of each
    form at 512 and 4096 graphs, a wide model (one bucket per layer: L + 2 = 4) and a ragged batch, host-resident
    (the forms without phases) and device-resident (ragged_dev: both trainers run the phased ragged step in the forms
    `buckets` and `sharded` -- the one-launch ragged forward with a layer-wise backward; against the oracle in
    tests/test_gpu_phased_forms.py).  Weights, losses and Adam moments equal bit for bit.  (Models are made and freed one after the
    other in one process: v2x_create's zeroing must not land on the weights a side-stream set_weights writes next.)"""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_rccl_worker, args=(1, _port(), ret), nprocs=1, join=True)
    res = ret[0]
    assert len(res) == 15
    for key, (py, nat) in res.items():
        assert np.all(np.isfinite(py[0])) and py[4] == nat[4] == 3, key
        for i, what in enumerate(("weights", "losses", "m", "v")):
            assert np.array_equal(py[i], nat[i]), (key, what, np.abs(py[i] - nat[i]).max())


def _dqn_inputs(B, N, seed):
    from oracle import compact as oc
    from v2xgnn import GnnSpec
    from util import f32_params, random_inputs
    spec = GnnSpec(n_nodes=N, feat_dim=64, n_mp_layers=2)
    rng = np.random.default_rng(seed)
    P_on, P_tg = oc.params_to_list(f32_params(spec, rng)), oc.params_to_list(f32_params(spec, rng))
    s = random_inputs(rng, B, N)
    s_next = random_inputs(rng, B, N)
    action = rng.integers(0, 4, size=(B, N)).astype(np.int32)
    reward = rng.normal(1.0, 0.5, size=B)
    return spec, P_on, P_tg, s, s_next, action, reward


def _dqn_steps(spec, P_on, P_tg, s, s_next, action, reward, g0, g1, comm=None, n_global=None, profile=False, steps=3):
    """dqn_step (comm None) or dqn_step_dp on graphs [g0, g1) -> (online weights, losses, fused-forward launches per step)"""
    import torch
    from v2xgnn import GnnEngine, PackedBatch
    on, tg = GnnEngine(spec), GnnEngine(spec)
    on.set_weights(P_on)
    tg.set_weights(P_tg)
    sb = on.to_device(PackedBatch.from_dense(*(a[g0:g1] for a in s)))
    sn = on.to_device(PackedBatch.from_dense(*(a[g0:g1] for a in s_next)))
    act = torch.from_numpy(np.ascontiguousarray(action[g0:g1])).cuda()
    rew = torch.from_numpy(np.ascontiguousarray(reward[g0:g1])).cuda()
    torch.cuda.synchronize()
    if profile:
        on.profile(True)
    losses = []
    for _ in range(steps):
        if comm is None:
            losses.append(on.dqn_step(tg, sb, sn, act, rew, 0.5).cpu().numpy())
        else:
            losses.append(on.dqn_step_dp(tg, sb, sn, act, rew, 0.5, comm, n_global).cpu().numpy())
    torch.cuda.synchronize()
    launches = None
    if profile:
        prof = on.profile_read()
        launches = sum(prof.get(k, (0, 0.0))[0] for k in ("k_gnn_fwd_fused", "k_gnn_fwd_split")) / steps
        on.profile(False)
    w = on.get_flat()
    on.close()
    tg.close()
    return w, np.stack(losses), launches


def _two_rank_worker(rank, world, port, ret):
    os.environ["V2X_FUSED_SPLIT"] = "1"          # whole-tile fused kernels at this share: the launches the profiler counts
    _init("gloo", rank, world, port)
    import torch
    import torch.distributed as dist
    try:
        from v2xgnn.dp import TorchComm
        comm = TorchComm()
        res = {}
        with torch.cuda.stream(torch.cuda.Stream()):
            for name in ("b256", "wide"):
                spec, P, pb, y, n_global = _case(name)
                for form, kw in FORMS:
                    res[(name, form)] = _run_pair(spec, P, pb, y, n_global, kw, comm)
            B = 256
            spec, P_on, P_tg, s, s_next, action, reward = _dqn_inputs(B, 20, 8)
            per = B // world
            res["dqn"] = _dqn_steps(spec, P_on, P_tg, s, s_next, action, reward, rank * per, (rank + 1) * per, comm=comm,
                                    n_global=B, profile=(rank == 0))
        assert comm.last_error is None, comm.last_error
        ret[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_native_step_equals_python_trainer_and_dqn_step_runs_the_graph_layers_once():
    """Two ranks on one GPU (gloo, dp.TorchComm): every form of the native step equals the Python trainer in the same
    processes bit for bit (weights, losses, gather_optimizer_state), replicas bit-identical.  v2x_dqn_step_dp on the two
    halves of a minibatch: replicas bit-identical, close to the single-process v2x_dqn_step on the whole minibatch, and ONE
    fused graph-layer forward of the online network per replay step (the four-call path of a Python trainer runs two)."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, _port(), ret), nprocs=2, join=True)
    r0, r1 = ret[0], ret[1]
    for key in r0:
        if key == "dqn":
            continue
        for r in (r0, r1):
            py, nat = r[key]
            assert py[4] == nat[4] == 3, key
            for i, what in enumerate(("weights", "losses", "m", "v")):
                assert np.array_equal(py[i], nat[i]), (key, what, np.abs(py[i] - nat[i]).max())
        assert np.array_equal(r0[key][1][0], r1[key][1][0]), (key, "replicas diverged")
    w0, l0, launches = r0["dqn"]
    w1, l1, _ = r1["dqn"]
    assert launches == 1, launches
    assert np.array_equal(w0, w1) and np.array_equal(l0, l1)
    old = os.environ.get("V2X_FUSED_SPLIT")
    os.environ["V2X_FUSED_SPLIT"] = "1"
    try:
        spec, P_on, P_tg, s, s_next, action, reward = _dqn_inputs(256, 20, 8)
        w, loss, launches1 = _dqn_steps(spec, P_on, P_tg, s, s_next, action, reward, 0, 256, profile=True)
    finally:
        if old is None:
            del os.environ["V2X_FUSED_SPLIT"]
        else:
            os.environ["V2X_FUSED_SPLIT"] = old
    assert launches1 == 1
    assert np.allclose(l0, loss, rtol=2e-4, atol=1e-6)
    assert np.allclose(w0, w, rtol=1e-3, atol=2e-5)


def _loop_worker(rank, world, port, ret):
    import random
    if world > 1:
        _init("gloo", rank, world, port)
    try:
        sys.path.insert(0, HERE)
        from v2xgnn.rl import Agent, RL_Config
        from v2xgnn.rl.train import start_env
        random.seed(9)
        np.random.seed(9)
        cfg = RL_Config()
        cfg.set_train_value(64, 0.5, 64, 1, 0.1)
        env = start_env(20)
        agent = Agent(20, env.n_RB, env.n_Neighbor, 64, env, cfg, seed=2, data_parallel="native" if world > 1 else False)
        assert agent.device_replay is not None
        if world > 1:
            assert agent.brain.model.trainer.native
        loss, reward_step, _, q_mean, _, _, _ = agent.train(1, 3)
        ret[rank] = (np.concatenate([w.ravel() for w in agent.brain.model.get_weights()]), loss, reward_step, q_mean)
        agent.brain.close()                  # (the trainer's collective table goes before the process group)
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()


def test_two_rank_dqn_loop_native():
    """Agent(..., data_parallel="native") on two ranks: rewards identical to the single-process loop, weights close."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_loop_worker, args=(2, _port(), ret), nprocs=2, join=True)
    single = mp.Manager().dict()
    mp.spawn(_loop_worker, args=(1, _port(), single), nprocs=1, join=True)
    w1, loss1, rew1, qm1 = single[0]
    assert np.array_equal(ret[0][0], ret[1][0])
    for r in (0, 1):
        w, loss, rew, qm = ret[r]
        assert np.array_equal(rew, rew1)
        assert np.allclose(loss, loss1, rtol=2e-4, atol=1e-6)
        assert np.allclose(qm, qm1, rtol=1e-3, atol=1e-4)
        assert np.allclose(w, w1, rtol=1e-3, atol=2e-5)


# ---- error paths: one rank, a table of the test's own --------------------------------------------------------------------
class _Table(object):
    """world-1 table whose entries succeed (a sum over one rank is the identity) unless named in `fail`"""

    def __init__(self, world=1, rank=0):
        from v2xgnn import lib
        self.fail, self.calls = set(), []

        def entry(name):
            def call(buf, n, stream, ctx):
                self.calls.append((name, n))
                return -1 if name in self.fail else 0
            return lib.COLLECTIVE(call)
        self._fns = [entry(k) for k in ("all_reduce_sum", "reduce_scatter_sum", "all_gather")]
        self.comm = lib.Comm(world, rank, None, *self._fns)


def test_collective_failure_and_argument_checks():
    import torch
    from v2xgnn import GnnEngine, lib
    spec, P, pb, y, n_global = _case("b256")
    eng = GnnEngine(spec)
    eng.set_weights(P)
    db, yd = eng.to_device(pb), torch.from_numpy(y).cuda()
    w0, (m0, v0, it0) = eng.get_flat(), eng.get_optimizer_state()
    t = _Table()
    for form, coll, where in ((lib.V2X_DP_ALLREDUCE, "all_reduce_sum", "the gradient"),
                              (lib.V2X_DP_BUCKETS, "all_reduce_sum", "bucket 0"),
                              (lib.V2X_DP_SHARDED, "reduce_scatter_sum", "bucket 0")):
        t.fail = {coll}
        with pytest.raises(lib.V2XCommError, match="%s of %s" % (coll, where)):
            eng.train_step_dp(db, yd, t, form, n_global)
        torch.cuda.synchronize()
        assert np.array_equal(eng.get_flat(), w0)
        m, v, it = eng.get_optimizer_state()
        assert it == it0 and np.array_equal(m, m0) and np.array_equal(v, v0)
    t.fail = {"all_reduce_sum"}
    with pytest.raises(lib.V2XCommError, match="all_reduce_sum of the losses"):
        eng.train_step_dp(db, yd, t, lib.V2X_DP_SHARDED, n_global)     # (all-reduced before Adam, like the gradient)
    assert eng.get_optimizer_state()[2] == it0
    t.fail = set()
    for form in (lib.V2X_DP_ALLREDUCE, lib.V2X_DP_BUCKETS, lib.V2X_DP_SHARDED):
        loss = eng.train_step_dp(db, yd, t, form, n_global)
        assert np.all(np.isfinite(loss.cpu().numpy()))
    assert eng.get_optimizer_state()[2] == it0 + 3 and not np.array_equal(eng.get_flat(), w0)
    # argument checks: all V2X_EINVAL
    bad = [(None, lib.V2X_DP_ALLREDUCE, n_global), (t, 3, n_global), (t, -1, n_global), (t, lib.V2X_DP_ALLREDUCE, 0)]
    for world, rank in ((0, 0), (1, 1), (2, -1)):
        bad.append((_Table(world, rank), lib.V2X_DP_ALLREDUCE, n_global))
    no_ar = _Table()
    no_ar.comm.all_reduce_sum = lib.COLLECTIVE()
    bad.append((no_ar, lib.V2X_DP_BUCKETS, n_global))
    for k in ("reduce_scatter_sum", "all_gather"):
        part = _Table()
        setattr(part.comm, k, lib.COLLECTIVE())
        eng.train_step_dp(db, yd, part, lib.V2X_DP_ALLREDUCE, n_global)        # (the other forms do not need it)
        bad.append((part, lib.V2X_DP_SHARDED, n_global))
    it1 = eng.get_optimizer_state()[2]
    for comm, form, n in bad:
        with pytest.raises(lib.V2XInvalidArgument):
            eng.train_step_dp(db, yd, comm, form, n)
    tg = GnnEngine(spec)
    tg.set_weights(P)
    act = torch.zeros((pb.n_graphs, spec.n_nodes), dtype=torch.int32, device="cuda")
    rew = torch.zeros(pb.n_graphs, dtype=torch.float64, device="cuda")
    for comm, n in ((None, n_global), (_Table(1, 1), n_global), (t, 0)):
        with pytest.raises(lib.V2XInvalidArgument):
            eng.dqn_step_dp(tg, db, db, act, rew, 0.5, comm, n)
    w1, (m1, v1, _) = eng.get_flat(), eng.get_optimizer_state()
    t.fail = {"all_reduce_sum"}
    with pytest.raises(lib.V2XCommError, match="all_reduce_sum of the gradient"):
        eng.dqn_step_dp(tg, db, db, act, rew, 0.5, t, n_global)
    torch.cuda.synchronize()
    m, v, it = eng.get_optimizer_state()
    assert it == it1 and np.array_equal(eng.get_flat(), w1) and np.array_equal(m, m1) and np.array_equal(v, v1)
    eng.close()
    tg.close()
