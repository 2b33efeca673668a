"""Per-state cost of the optimal-allocation search (v2xgnn.rl.OptimalAllocation, csrc/v2xopt.hip) next to the host brute
force of Agent._brute_force: wall time of search() (upload + kernels + download) and the kernels' time between HIP events,
for (N, C) = (4, 4), (8, 4), (12, 4), (16, 4) at one state, 50 states at (8, 4), and the host path at (4, 4) (every joint
action) and at (8, 4) (extrapolated from the first 4096 joint actions).

    python tools/opt_search_timing.py [--out profiles/opt_search_timing.json] [--reps 20]

With --bound: the branch-and-bound search (search_bound, v2x_opt_search_bound) at 12, 16, 20 and 24 links x 4 RBs, ten
seeded states each (min / median / max of the wall and kernel time per state and of the nodes visited), beside the
exhaustive search() at 12 and 16 links on the same states in the same run.

    python tools/opt_search_timing.py --bound [--out profiles/opt_bound_timing.json] [--states 10]

With --local: the multi-start local search (search_local, v2x_opt_search_local) on the same seeded states: wall and kernel
time per state at 20 x 4, 100 x 4, 128 x 4 and 128 x 16 for 128 / 1024 / 8192 restarts and for 50 stacked 20-link states, sweeps per
restart, the share of restarts that end at the winner; hits and worst gap against search_bound at 12 - 24 links; the reward at
100 links against random actions and against 8 x the restarts; search_bound seeded with the local search against unseeded.

    python tools/opt_search_timing.py --local [--out profiles/opt_local_timing.json] [--states 10]

With --landscape: the reward landscape (landscape, v2x_opt_landscape) with 2, 16 and 62 edges at 8, 12 and 16 links x 4 RBs on
the seeded states of --bound, beside search() on the same states, the four taken in turn in the same run: wall and kernel
time per state and the ratio of the landscape's kernel time to the search's.

    python tools/opt_search_timing.py --landscape [--out profiles/opt_landscape_timing.json] [--states 10] [--reps 5]

With --count: the counting branch and bound (count_better, v2x_opt_count_bound) on the seeded states of --bound at 12, 16 and
20 links x 4 RBs, one (state, threshold) per call: the state's optimum (from search_bound), 0.97 x it and the reward of one
seeded random action as thresholds -- better, equal, open, nodes, wall and kernel time --, beside search_bound on the same state
in the same run and, at 12 and 16 links, the landscape (whose counts the exact results must equal).

    python tools/opt_search_timing.py --count [--out profiles/opt_count_bound_timing.json] [--states 10] [--count-max-nodes N]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _state(n, seed=1):
    from v2xgnn.rl.train import start_env
    random.seed(seed)
    np.random.seed(seed)
    return start_env(n)


def _stack(n, E):
    from v2xgnn.rl.train import start_env_batched
    return start_env_batched(n, E, seed=7, lookahead=False)


def device_row(opt, env, reps, label):
    import torch
    w_v2v, w_v2i = 1.0, 0.1
    E = getattr(env, 'E', 1)
    opt.search(env, w_v2v, w_v2i)                                  # warm-up: code objects, workspace
    torch.cuda.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx, rew = opt.search(env, w_v2v, w_v2i)
        walls.append(time.perf_counter() - t0)
    # kernels only: the inputs already on the device (search_device on the same stream), bracketed by events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for _ in range(reps):
        prob, _, _, _ = opt._setup(env, w_v2v, w_v2i, 1 << 36)
        ix = torch.empty(E, dtype=torch.int64, device=opt.device)
        rw = torch.empty(E, dtype=torch.float64, device=opt.device)
        ev[0].record()
        rc = opt._lib.v2x_opt_search(__import__('ctypes').byref(prob), opt._ws.data_ptr(), ix.data_ptr(), rw.data_ptr(),
                                     opt._stream())
        ev[1].record()
        assert rc == 0
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    n, rb = (env.n_Veh if hasattr(env, 'E') else len(env.vehicles)), env.n_RB
    total = rb ** n
    wall, k = float(np.median(walls)), float(np.median(kern))
    return {"case": label, "n": n, "rb": rb, "states": E, "joint_actions_per_state": total,
            "wall_ms_per_state": round(wall * 1e3 / E, 4), "kernel_ms_per_state": round(k * 1e3 / E, 4),
            "wall_ms_call": round(wall * 1e3, 4), "kernel_ms_call": round(k * 1e3, 4),
            "joint_actions_per_s_kernel": float("%.4g" % (total * E / k)),
            "best_index": [int(i) for i in idx[:4]], "best_reward": [float(r) for r in rew[:4]]}


def host_row(n, first):
    from v2xgnn.rl import Agent
    env = _state(n)
    agent = Agent.__new__(Agent)                                   # _brute_force needs the simulator and the weights only
    agent.env, agent.num_D2D, agent.num_CH, agent.v2v_weight, agent.v2i_weight = env, n, env.n_RB, 1.0, 0.1
    import itertools
    joint = np.array(list(itertools.islice(itertools.product(range(env.n_RB), repeat=n), first)), int)
    agent.dump_act = lambda a: env.compute_reward_with_channel_selection(a)
    t0 = time.perf_counter()
    agent._brute_force(joint)
    dt = time.perf_counter() - t0
    total = env.n_RB ** n
    return {"case": "host %d links" % n, "n": n, "rb": env.n_RB, "timed_joint_actions": len(joint),
            "joint_actions_per_state": total, "us_per_joint_action": round(dt / len(joint) * 1e6, 2),
            "ms_per_state" + ("" if len(joint) == total else "_extrapolated"): round(dt / len(joint) * total * 1e3, 2)}


def _mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v))}


def bound_rows(opt, n, states, max_nodes):
    """search_bound on `states` seeded states of n links x 4 RBs, one call per state: wall of the call (upload, launches,
    the per-round counter read-backs, download) and the time between HIP events around v2x_opt_search_bound alone; the
    exhaustive search on the same states at n <= 16 (3 states at 16: 0.8 s each)."""
    import ctypes
    import torch
    from v2xgnn.rl.optimum import BoundBudgetExceeded, MAX_INDEX
    w_v2v, w_v2i = 1.0, 0.1
    wall, kern, nodes, spent, ex_wall, results = [], [], [], [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for seed in range(states):
        env = _state(n, seed)
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx, rew = opt.search_bound(env, w_v2v, w_v2i, max_nodes)
            wall.append((time.perf_counter() - t0) * 1e3)
            spent.append(False)
        except BoundBudgetExceeded as exc:
            wall.append((time.perf_counter() - t0) * 1e3)
            idx, rew = exc.index, exc.reward
            spent.append(True)
        nodes.append(opt.nodes_visited)
        results.append((int(idx[0]), float(rew[0])))
        prob, _, _, _ = opt._setup(env, w_v2v, w_v2i, MAX_INDEX, max_nodes)
        ix = torch.empty(1, dtype=torch.int64, device=opt.device)
        rw = torch.empty(1, dtype=torch.float64, device=opt.device)
        cnt = ctypes.c_int64(0)
        ev[0].record()
        opt._lib.v2x_opt_search_bound(ctypes.byref(prob), opt._ws.data_ptr(), int(max_nodes), ix.data_ptr(), rw.data_ptr(),
                                      ctypes.byref(cnt), opt._stream())
        ev[1].record()
        torch.cuda.synchronize()
        kern.append(ev[0].elapsed_time(ev[1]))
        if n <= 12 or (n <= 16 and seed < 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ei, er = opt.search(env, w_v2v, w_v2i)
            ex_wall.append((time.perf_counter() - t0) * 1e3)
            assert int(ei[0]) == results[-1][0] and float(er[0]) == results[-1][1], (n, seed)
        print(json.dumps({"n": n, "seed": seed, "wall_ms": round(wall[-1], 3), "kernel_ms": round(kern[-1], 3),
                          "nodes": nodes[-1], "budget_spent": spent[-1], "index": results[-1][0],
                          "reward": results[-1][1]}), flush=True)
    row = {"case": "bound %d links" % n, "n": n, "rb": 4, "states": states, "joint_actions_per_state": 4 ** n,
           "max_nodes": int(max_nodes), "wall_ms_per_state": _mmm(wall), "kernel_ms_per_state": _mmm(kern),
           "nodes_visited": _mmm(nodes), "states_that_spent_the_budget": int(np.sum(spent)),
           "nodes_per_s_kernel_median": float("%.4g" % (np.median(np.array(nodes) / (np.array(kern) * 1e-3))))}
    if ex_wall:
        row["exhaustive_wall_ms_per_state"] = _mmm(ex_wall)
        row["exhaustive_states"] = len(ex_wall)
    return row


def main_bound(args):
    import torch
    from v2xgnn.rl import OptimalAllocation
    from v2xgnn.rl.optimum import DEFAULT_MAX_NODES
    opt = OptimalAllocation()
    opt.search_bound(_state(8), 1.0, 0.1)                              # warm-up: code objects, workspace
    rows = []
    for n in args.links:
        rows.append(bound_rows(opt, n, args.states, DEFAULT_MAX_NODES))
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def _state_rb(n, rb, seed):
    env = _state(n, seed)
    if rb != env.n_RB:
        env.n_RB = rb
        env.new_random_game(n)
    return env


RESTARTS = (128, 1024, 8192)


def local_time_rows(opt, n, rb, envs, label):
    """one call per state (or one call of a stacked simulator) and restart count: wall of search_local (upload, four
    launches, download) and the time between HIP events around v2x_opt_search_local alone"""
    import ctypes
    import torch
    from v2xgnn.rl.optimum import MAX_INDEX
    w_v2v, w_v2i = 1.0, 0.1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    for R in RESTARTS:
        wall, kern, share = [], [], []
        for env in envs:
            E = getattr(env, 'E', 1)
            opt.search_local(env, w_v2v, w_v2i, restarts=R)            # workspace of this size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, rew, _, all_r = opt.search_local(env, w_v2v, w_v2i, restarts=R, all_restarts=True)
            wall.append((time.perf_counter() - t0) * 1e3 / E)
            share.append(float(np.mean(all_r == rew[:, None])))
            prob, _, _, _ = opt._setup(env, w_v2v, w_v2i, MAX_INDEX, local=(R, 64))
            act = torch.empty((E, n), dtype=torch.int32, device=opt.device)
            rw = torch.empty(E, dtype=torch.float64, device=opt.device)
            ev[0].record()
            rc = opt._lib.v2x_opt_search_local(ctypes.byref(prob), opt._ws.data_ptr(), R, 0, 64, act.data_ptr(), rw.data_ptr(),
                                               None, None, None, opt._stream())
            ev[1].record()
            assert rc == 0
            torch.cuda.synchronize()
            kern.append(ev[0].elapsed_time(ev[1]) / E)
        rows.append({"case": label, "n": n, "rb": rb, "restarts": R, "calls": len(envs), "states_per_call": getattr(envs[0], 'E', 1),
                     "wall_ms_per_state": _mmm(wall), "kernel_ms_per_state": _mmm(kern),
                     "share_of_restarts_at_the_winner": _mmm(share)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def local_sweeps(opt, n, rb, env, R=128):
    """sweeps a restart runs (the last one makes no move): 1 + the smallest max_sweeps whose result is the final one"""
    final = opt.search_local(env, 1.0, 0.1, restarts=R, all_restarts=True)[2][0]
    need = np.full(R, -1)
    for k in range(1, 25):
        got = opt.search_local(env, 1.0, 0.1, restarts=R, max_sweeps=k, all_restarts=True)[2][0]
        same = np.all(got == final, axis=1)
        need[(need < 0) & same] = k + 1
        if np.all(need > 0):
            break
    return {"case": "sweeps", "n": n, "rb": rb, "restarts": R, "sweeps_per_restart": _mmm(need), "mean": float(need.mean())}


def local_quality_row(opt, n, states):
    """against the exact optimum (unseeded search_bound) and search_bound seeded with 128 restarts, on the seeded states"""
    import torch
    w_v2v, w_v2i = 1.0, 0.1
    hits = {R: 0 for R in RESTARTS}
    gaps = {R: [] for R in RESTARTS}
    wall_plain, wall_seeded, wall_local, nodes_plain, nodes_seeded = [], [], [], [], []
    for seed in range(states):
        env = _state(n, seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, rew = opt.search_bound(env, w_v2v, w_v2i)
        wall_plain.append((time.perf_counter() - t0) * 1e3)
        nodes_plain.append(opt.nodes_visited)
        t0 = time.perf_counter()
        si, sr = opt.search_bound(env, w_v2v, w_v2i, incumbent='local', restarts=128)
        wall_seeded.append((time.perf_counter() - t0) * 1e3)
        nodes_seeded.append(opt.nodes_visited)
        assert int(si[0]) == int(idx[0]) and float(sr[0]) == float(rew[0]), (n, seed)
        for R in RESTARTS:
            t0 = time.perf_counter()
            a, r = opt.search_local(env, w_v2v, w_v2i, restarts=R)
            if R == 128:
                wall_local.append((time.perf_counter() - t0) * 1e3)
            assert r[0] <= rew[0]
            hits[R] += int(r[0] == rew[0] and int(opt.encode(a, 4)[0]) == int(idx[0]))
            gaps[R].append(float((rew[0] - r[0]) / rew[0]))
    return {"case": "quality %d links" % n, "n": n, "rb": 4, "states": states,
            "exact_optimum_found": {str(R): hits[R] for R in RESTARTS},
            "worst_relative_gap": {str(R): max(gaps[R]) for R in RESTARTS},
            "wall_ms_search_local_128": _mmm(wall_local),
            "wall_ms_bound_unseeded": _mmm(wall_plain), "wall_ms_bound_seeded_including_local_128": _mmm(wall_seeded),
            "nodes_unseeded": _mmm(nodes_plain), "nodes_seeded": _mmm(nodes_seeded),
            "per_state": {"wall_unseeded": [round(v, 2) for v in wall_plain], "wall_seeded": [round(v, 2) for v in wall_seeded],
                          "nodes_unseeded": nodes_plain, "nodes_seeded": nodes_seeded}}


def local_wide_row(opt, n, states):
    """100 links: no exact optimum; the reward against 200 random joint actions and against 8 x the restarts"""
    out = []
    for seed in range(states):
        env = _state(n, seed)
        rng = np.random.default_rng(seed)
        rnd = opt.rewards_of(env, 1.0, 0.1, rng.integers(0, env.n_RB, size=(1, 200, n)))[0]
        row = {"seed": seed, "random_mean": float(rnd.mean()), "random_best": float(rnd.max())}
        for R in (1, 16) + RESTARTS:
            row["local_%d" % R] = float(opt.search_local(env, 1.0, 0.1, restarts=R)[1][0])
        out.append(row)
    gain = lambda a, b: _mmm([r["local_%d" % b] / r["local_%d" % a] - 1.0 for r in out])
    return {"case": "reward at %d links" % n, "n": n, "rb": 4, "states": out, "gain_128_over_16": gain(16, 128),
            "gain_1024_over_128": gain(128, 1024), "gain_8192_over_1024": gain(1024, 8192)}


def main_local(args):
    import torch
    from v2xgnn.rl import OptimalAllocation
    opt = OptimalAllocation()
    opt.search_local(_state(8), 1.0, 0.1)                              # warm-up: code objects
    opt.search_bound(_state(8), 1.0, 0.1, incumbent='local')
    rows = []
    for n, rb in ((20, 4), (100, 4), (128, 4), (128, 16)):
        envs = [_state_rb(n, rb, seed) for seed in range(args.states)]
        rows += local_time_rows(opt, n, rb, envs, "local %d x %d" % (n, rb))
        rows.append(local_sweeps(opt, n, rb, envs[0]))
        print(json.dumps(rows[-1]), flush=True)
    rows += local_time_rows(opt, 20, 4, [_stack(20, 50)], "local 20 x 4, 50 stacked states")
    for n in args.links:
        rows.append(local_quality_row(opt, n, args.states))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(local_wide_row(opt, 100, args.states))
    print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


LANDSCAPE_EDGES = (2, 16, 62)


def landscape_rows(opt, n, states, reps):
    """search() and landscape() with 2 / 16 / 62 edges on `states` seeded states of n links x 4 RBs, one state per call, the
    four in turn `reps` times per state: wall of the Python call (upload, launches, download) and the time between HIP
    events around the C entry point alone (inputs on the device); the median over the reps of a state, then min / median /
    max over the states.  The edges are evenly spaced over [0, best reward]."""
    import ctypes
    import torch
    from v2xgnn.rl.optimum import MAX_SEARCH
    w_v2v, w_v2i = 1.0, 0.1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    cases = ("search",) + tuple("landscape_%d" % k for k in LANDSCAPE_EDGES)
    wall = {c: [] for c in cases}
    kern = {c: [] for c in cases}
    ratio = {k: [] for k in LANDSCAPE_EDGES}
    for seed in range(states):
        env = _state(n, seed)
        index, best = opt.search(env, w_v2v, w_v2i)
        edges = {k: np.linspace(0.0, float(best[0]), k + 1)[1:] for k in LANDSCAPE_EDGES}
        for k in LANDSCAPE_EDGES:                                   # warm-up: the workspace of each size
            counts, sums = opt.landscape(env, w_v2v, w_v2i, edges[k])
            assert int(counts.sum()) == 4 ** n and int(counts[0, k]) >= 1 and int(counts[0, k + 1]) == 0
        w = {c: [] for c in cases}
        t = {c: [] for c in cases}
        for _ in range(reps):
            for c in cases:
                k = None if c == "search" else int(c.split("_")[1])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k is None:
                    opt.search(env, w_v2v, w_v2i)
                else:
                    opt.landscape(env, w_v2v, w_v2i, edges[k])
                w[c].append((time.perf_counter() - t0) * 1e3)
                prob, _, _, _ = opt._setup(env, w_v2v, w_v2i, MAX_SEARCH, n_edges=k)
                if k is None:
                    ix = torch.empty(1, dtype=torch.int64, device=opt.device)
                    rw = torch.empty(1, dtype=torch.float64, device=opt.device)
                    ev[0].record()
                    rc = opt._lib.v2x_opt_search(ctypes.byref(prob), opt._ws.data_ptr(), ix.data_ptr(), rw.data_ptr(), opt._stream())
                else:
                    ed = torch.from_numpy(edges[k]).to(opt.device)
                    cn = torch.empty(k + 2, dtype=torch.int64, device=opt.device)
                    sm = torch.empty(1, dtype=torch.float64, device=opt.device)
                    ev[0].record()
                    rc = opt._lib.v2x_opt_landscape(ctypes.byref(prob), opt._ws.data_ptr(), ed.data_ptr(), k, cn.data_ptr(),
                                                    sm.data_ptr(), opt._stream())
                ev[1].record()
                assert rc == 0
                torch.cuda.synchronize()
                t[c].append(ev[0].elapsed_time(ev[1]))
        for c in cases:
            wall[c].append(float(np.median(w[c])))
            kern[c].append(float(np.median(t[c])))
        for k in LANDSCAPE_EDGES:
            ratio[k].append(kern["landscape_%d" % k][-1] / kern["search"][-1])
        print(json.dumps({"n": n, "seed": seed, "kernel_ms": {c: round(kern[c][-1], 4) for c in cases},
                          "wall_ms": {c: round(wall[c][-1], 4) for c in cases}}), flush=True)
    return {"case": "landscape %d links" % n, "n": n, "rb": 4, "states": states, "reps": reps, "joint_actions_per_state": 4 ** n,
            "wall_ms_per_state": {c: _mmm(wall[c]) for c in cases}, "kernel_ms_per_state": {c: _mmm(kern[c]) for c in cases},
            "kernel_ratio_to_search": {str(k): _mmm(ratio[k]) for k in LANDSCAPE_EDGES}}


def main_landscape(args):
    import torch
    from v2xgnn.rl import OptimalAllocation
    opt = OptimalAllocation()
    opt.search(_state(8), 1.0, 0.1)                                    # warm-up: code objects
    opt.landscape(_state(8), 1.0, 0.1, [1.0])
    rows = []
    for n in (8, 12, 16):
        rows.append(landscape_rows(opt, n, args.states if n < 16 else min(args.states, 3), args.reps if n < 16 else min(args.reps, 2)))
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


COUNT_THRESHOLDS = ("optimum", "0.97 x optimum", "random action")


def count_rows(opt, n, states, max_nodes):
    """count_better on `states` seeded states of n links x 4 RBs, one threshold per call (so every threshold has its own nodes
    and times): wall of the Python call (upload, launches, the per-round counter read-backs, download) and the time between HIP
    events around v2x_opt_count_bound alone.  search_bound on the same state first (its optimum is the first threshold); the
    landscape with the three thresholds' edges at n <= 12, and for 3 states at 16 links."""
    import ctypes
    import torch
    from v2xgnn.rl.optimum import MAX_INDEX, rank_edges, rank_from_counts
    w_v2v, w_v2i = 1.0, 0.1
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per_state = []
    for seed in range(states):
        env = _state(n, seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, best = opt.search_bound(env, w_v2v, w_v2i)
        row = {"seed": seed, "search_bound": {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "nodes": opt.nodes_visited,
                                              "reward": float(best[0])}}
        rnd = np.random.default_rng(seed).integers(0, 4, size=(1, n))
        th = np.array([[best[0], 0.97 * best[0], opt.rewards_of(env, w_v2v, w_v2i, rnd)[0]]])
        truth = None
        if n <= 12 or (n <= 16 and seed < 3):
            edges = rank_edges(th)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts, _ = opt.landscape(env, w_v2v, w_v2i, edges)
            row["landscape_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            truth = rank_from_counts(counts, edges, th)
        for k, name in enumerate(COUNT_THRESHOLDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = opt.count_better(env, w_v2v, w_v2i, th[:, k], max_nodes)
            wall = (time.perf_counter() - t0) * 1e3
            prob, _, _, _ = opt._setup(env, w_v2v, w_v2i, MAX_INDEX, max_nodes, n_thr=1)
            dev = torch.from_numpy(np.ascontiguousarray(th[:, k:k + 1])).to(opt.device)
            outs = [torch.empty((1, 1), dtype=torch.int64, device=opt.device) for _ in range(4)]
            cnt = ctypes.c_int64(0)
            ev[0].record()
            opt._lib.v2x_opt_count_bound(ctypes.byref(prob), opt._ws.data_ptr(), dev.data_ptr(), 1, int(max_nodes),
                                         *[o.data_ptr() for o in outs], ctypes.byref(cnt), opt._stream())
            ev[1].record()
            torch.cuda.synchronize()
            better, opened = int(got['better'][0, 0]), int(got['open'][0, 0])
            if truth is not None:
                assert better <= int(truth[0][0, k]) <= better + opened and int(got['equal'][0, 0]) <= int(truth[1][0, k]), (n, seed, name)
                assert not got['exact'][0, 0] or better == int(truth[0][0, k]), (n, seed, name)
            row[name] = {"threshold": float(th[0, k]), "better": better, "equal": int(got['equal'][0, 0]), "open": opened,
                         "exact": bool(got['exact'][0, 0]), "nodes": got['nodes_visited'], "wall_ms": round(wall, 3),
                         "kernel_ms": round(ev[0].elapsed_time(ev[1]), 3),
                         "nodes_per_better": round(got['nodes_visited'] / better, 2) if better else None}
        print(json.dumps({"n": n, **row}), flush=True)
        per_state.append(row)
    out = {"case": "count %d links" % n, "n": n, "rb": 4, "states": states, "joint_actions_per_state": 4 ** n,
           "max_nodes": int(max_nodes), "search_bound_wall_ms": _mmm([r["search_bound"]["wall_ms"] for r in per_state]),
           "search_bound_nodes": _mmm([r["search_bound"]["nodes"] for r in per_state])}
    for name in COUNT_THRESHOLDS:
        rows = [r[name] for r in per_state]
        exact = [r for r in rows if r["exact"]]
        out[name] = {"states_exact": len(exact), "nodes": _mmm([r["nodes"] for r in rows]), "wall_ms": _mmm([r["wall_ms"] for r in rows]),
                     "kernel_ms": _mmm([r["kernel_ms"] for r in rows]),
                     "nodes_per_s_kernel_median": float("%.4g" % np.median([r["nodes"] / (r["kernel_ms"] * 1e-3) for r in rows]))}
        if exact:
            out[name]["better_where_exact"] = _mmm([r["better"] for r in exact])
            ratios = [r["nodes_per_better"] for r in exact if r["nodes_per_better"]]
            if ratios:
                out[name]["nodes_per_better_where_exact"] = _mmm(ratios)
        if len(exact) < len(rows):
            out[name]["open_share_where_bracketed"] = _mmm([r["open"] / 4.0 ** n for r in rows if not r["exact"]])
    out["per_state"] = per_state
    return out


def main_count(args):
    import torch
    from v2xgnn.rl import OptimalAllocation
    opt = OptimalAllocation()
    opt.search_bound(_state(8), 1.0, 0.1)                              # warm-up: code objects, workspace
    opt.count_better(_state(8), 1.0, 0.1, [1.0])
    rows = []
    for n in (12, 16, 20):
        rows.append(count_rows(opt, n, args.states, args.count_max_nodes))
        print(json.dumps({k: v for k, v in rows[-1].items() if k != "per_state"}), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bound", action="store_true", help="measure the branch-and-bound search instead")
    ap.add_argument("--local", action="store_true", help="measure the multi-start local search instead")
    ap.add_argument("--landscape", action="store_true", help="measure the reward landscape beside search() instead")
    ap.add_argument("--count", action="store_true", help="measure the counting branch and bound beside search_bound instead")
    ap.add_argument("--count-max-nodes", type=int, default=1 << 26,
                    help="--count: node budget of one (state, threshold) call (default: DEFAULT_RANK_MAX_NODES of rl/optimum.py)")
    ap.add_argument("--states", type=int, default=10, help="--bound / --local / --landscape / --count: seeded states per size")
    ap.add_argument("--links", type=int, nargs="+", default=[12, 16, 20, 24], help="--bound / --local: sizes against the exact optimum")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("opt_search_timing.py measures the GPU search: no GPU here")
    if args.bound:
        return main_bound(args)
    if args.local:
        return main_local(args)
    if args.landscape:
        return main_landscape(args)
    if args.count:
        return main_count(args)
    from v2xgnn.rl import OptimalAllocation
    opt = OptimalAllocation()
    rows = []
    for n in (4, 8, 12, 16):
        rows.append(device_row(opt, _state(n), args.reps if n < 16 else 3, "device %d links" % n))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(device_row(opt, _stack(8, 50), args.reps, "device 8 links x 50 states"))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(host_row(4, 256))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(host_row(8, 4096))
    print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
