"""Mixed-size DQN (rl/mixed.py) in numbers: pools of 8, 12, 20 and 31 links with equal quotas, minibatches of 4096 graphs
(72,704 node rows), 64 features, 2 message-passing layers.

  (a) assembly   the one-launch assembly of the ragged minibatch (v2x_replay_gather_mixed) against its composition from what the
                 library had before it: v2x_gather_rows_multi per pool (xe, xe', action, reward, CSR sources) into offset views of
                 the same output tensors, graph_off and row_ptr precomputed.  The slot lists are on the device in both.
  (b) step       the one-call replay step (v2x_dqn_step, ragged form) against predict-then-fit composed from two forwards,
                 v2x_dqn_targets_ragged and train_step.
  (c) agent      MixedAgent's wall time per train step at 4 x 10 simulators (8, 12, 20 and 28 links: the simulator places vehicles
                 in groups of four), batch 4096.

(a) and (b): medians over --reps timed steps after --warmup untimed ones, between HIP events step by step and as the wall time of
the whole timed loop (ending in a synchronise) per step.  The forms are taken in turn; the composition is measured five times and
the min-max of its five medians is the spread a difference has to exceed.

    python tools/mixed_replay_timing.py [--out profiles/mixed_replay_timing.json] [--reps 200] [--warmup 20]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES, CAP = (8, 12, 20, 31), 4096


def _timed(fn, reps, warmup, torch):
    """-> (median ms between HIP events per call, wall ms per call of the timed loop)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    t0 = time.perf_counter()
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    return float(np.median([a.elapsed_time(b) for a, b in evs])), wall


def _compare(new, old, reps, warmup, torch):
    """the new form once between five measurements of the composition, taken in turn"""
    comp = [_timed(old, reps, warmup, torch) for _ in range(2)]
    one = _timed(new, reps, warmup, torch)
    comp += [_timed(old, reps, warmup, torch) for _ in range(3)]
    ev, wall = [c[0] for c in comp], [c[1] for c in comp]
    out = {"new_event_ms": one[0], "new_wall_ms": one[1],
           "composition_event_ms": float(np.median(ev)), "composition_event_ms_min_max": [min(ev), max(ev)],
           "composition_wall_ms": float(np.median(wall)), "composition_wall_ms_min_max": [min(wall), max(wall)]}
    out["new_slower_than_spread"] = bool(one[0] - out["composition_event_ms"] > max(ev) - min(ev))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_replay_timing.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--agent-steps", type=int, default=20)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    import v2xgnn
    from v2xgnn import GnnEngine, GnnSpec, lib as vlib
    from v2xgnn.engine import current_stream_ptr
    from v2xgnn.packing import adj_to_csr
    from v2xgnn.rl.mixed import MixedAgent, MixedReplay

    lib = v2xgnn.load_library()
    rng = np.random.default_rng(5)
    per = args.batch // len(SIZES)
    mem = MixedReplay(CAP, SIZES)
    for n in SIZES:
        # the reference's topology: every link q has one receiver dest[q] != q; p -> q unless p == q or p == dest[q]
        dest = rng.integers(0, n - 1, size=(CAP, n))
        dest = dest + (dest >= np.arange(n)[None, :])
        adj = np.ones((CAP, n, n)) - np.eye(n)[None]
        adj[np.repeat(np.arange(CAP), n), dest.reshape(-1), np.tile(np.arange(n), CAP)] = 0.0
        col = adj_to_csr(adj)[1].reshape(CAP, n * (n - 2)).astype(np.int32)
        mask = ((adj != 0).astype(np.int64) << np.arange(n, dtype=np.int64)[None, :, None]).sum(axis=1).astype(np.int32)
        xe = rng.normal(0.8, 0.3, size=(2, CAP, n, 16)).astype(np.float32)
        xe[:, :, :, 13:] = 0.0
        mem.add_many_packed(n, xe[0], xe[1], col, mask, np.ones(CAP, bool), rng.integers(0, 4, size=(CAP, n)), rng.normal(0.0, 1.0, size=CAP))
    idx = {n: rng.integers(0, CAP, size=per) for n in SIZES}
    sb, sn, action, reward = mem.sample(idx)
    torch.cuda.synchronize()
    res = {"sizes": list(SIZES), "batch": per * len(SIZES), "rows": sb.n_rows, "edges": sb.n_edges, "feat_dim": 64, "n_mp_layers": 2,
           "reps": args.reps, "warmup": args.warmup}

    # ------------------------------------------------------------------ (a) the assembly
    stream = lambda: current_stream_ptr(0)
    slots = {n: torch.from_numpy(mem.pools[n].logical_to_slot(idx[n])).cuda() for n in SIZES}
    table = (vlib.ReplayPool * len(SIZES))()
    for k, n in enumerate(SIZES):
        p = mem.pools[n]
        table[k].n_nodes, table[k].count = n, per
        for name in ("xe", "xe_next", "col", "action", "reward"):
            setattr(table[k], name, getattr(p, name).data_ptr())
        table[k].idx = slots[n].data_ptr()
    t = dict(xe=sb.xe, xe_next=sn.xe, action=action, reward=reward, graph_off=sb.graph_off, row_ptr=sb.row_ptr, col_idx=sb.col_idx)
    desc = vlib.MixedBatch(**{k: v.data_ptr() for k, v in t.items()})

    def assemble_new():
        vlib.check(lib, lib.v2x_replay_gather_mixed(len(SIZES), table, C.byref(desc), stream()), None)

    want = {k: v.clone() for k, v in t.items()}
    jobs, g0, r0, e0 = [], 0, 0, 0
    for n in SIZES:                                    # the composition: five gathers per pool into offset views
        p, ne = mem.pools[n], n * (n - 2)
        src = (C.c_void_p * 5)(*[getattr(p, name).data_ptr() for name in ("xe", "xe_next", "action", "reward", "col")])
        dst = (C.c_void_p * 5)(t['xe'][r0:].data_ptr(), t['xe_next'][r0:].data_ptr(), t['action'][r0:].data_ptr(),
                               t['reward'][g0:].data_ptr(), t['col_idx'][e0:].data_ptr())
        rb = (C.c_int64 * 5)(n * 64, n * 64, n * 4, 8, ne * 4)
        jobs.append((src, dst, rb, slots[n]))
        g0, r0, e0 = g0 + per, r0 + per * n, e0 + per * ne

    def assemble_old():
        for src, dst, rb, s in jobs:
            vlib.check(lib, lib.v2x_gather_rows_multi(5, src, dst, rb, s.data_ptr(), per, stream()), None)

    for k in ("xe", "xe_next", "action", "reward", "col_idx"):
        t[k].fill_(-1)
    assemble_old()
    torch.cuda.synchronize()
    for k, v in want.items():                          # faster and different is not faster
        assert torch.equal(v, t[k]), "the composition assembles another %s" % k
    res["assembly"] = _compare(assemble_new, assemble_old, args.reps, args.warmup, torch)
    print("assembly", json.dumps(res["assembly"]), flush=True)

    # ------------------------------------------------------------------ (b) the replay step
    spec = GnnSpec(n_nodes=1, feat_dim=64, n_mp_layers=2, share_weights=True, variable_graphs=True)
    from v2xgnn.bs_brain import _glorot_list
    w_on, w_tg = _glorot_list(spec, np.random.default_rng(1)), _glorot_list(spec, np.random.default_rng(2))
    y = torch.empty((sb.n_rows, 4), dtype=torch.float32, device="cuda")
    steps = {}
    for form in ("one_call", "composed"):
        on, tg = GnnEngine(spec), GnnEngine(spec)
        on.set_weights(w_on)
        tg.set_weights(w_tg)
        if form == "one_call":
            fn = lambda on=on, tg=tg: on.dqn_step(tg, sb, sn, action, reward, 0.5, y_out=y, want_loss=False)
        else:
            q, qn = torch.empty_like(y), torch.empty_like(y)

            def fn(on=on, tg=tg, q=q, qn=qn):
                on.forward(sb, out=q)
                tg.forward(sn, out=qn)
                vlib.check(lib, lib.v2x_dqn_targets_ragged(q.data_ptr(), qn.data_ptr(), action.data_ptr(), reward.data_ptr(), C.c_double(0.5),
                                                           sb.graph_off.data_ptr(), sb.n_graphs, sb.n_rows, 4, y.data_ptr(), stream()), None)
                on.train_step(sb, y, n_global=sb.n_rows, want_loss=False)
        steps[form] = (fn, on, tg)
    res["path_info"] = steps["one_call"][1].path_info(sb)
    res["step"] = _compare(steps["one_call"][0], steps["composed"][0], args.reps, args.warmup, torch)
    print("step", json.dumps(res["step"]), flush=True)
    for _, on, tg in steps.values():
        on.close()
        tg.close()

    # ------------------------------------------------------------------ (c) the agent
    from v2xgnn.rl.sim_config import RL_Config
    from v2xgnn.rl.train import start_env_batched
    np.random.seed(1001)
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, args.batch, 1, 0.1)
    sizes = (8, 12, 20, 28)
    envs = [start_env_batched(n, 10, 1001 + 15485863 * k) for k, n in enumerate(sizes)]
    agent = MixedAgent(envs, cfg, 64, seed=1001)
    agent.train(1, 5)                                  # warm-up: buffers, workspaces, the first replays
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.train(1, args.agent_steps)
    torch.cuda.synchronize()
    res["agent"] = {"sizes": list(sizes), "simulators_per_size": 10, "batch": args.batch, "train_steps": args.agent_steps,
                    "iterations_per_train_step": agent.n_iter, "wall_ms_per_train_step": (time.perf_counter() - t0) * 1e3 / args.agent_steps,
                    "dropped_irregular": {str(n): v for n, v in agent.memory.dropped_irregular.items()}}
    print("agent", json.dumps(res["agent"]), flush=True)
    agent.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
