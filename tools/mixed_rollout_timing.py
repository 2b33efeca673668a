"""The mixed-size resident rollout (v2x_rollout_steps_mixed, MixedAgent(rollout='trajectory')) in numbers, at pools of 8 / 12 / 20 /
28 links x 10 simulators (the configuration behind DESIGN.md's 3.2 ms per train step) and 8 / 12 / 20 links x 1 and x 10 simulators;
64 features, 2 message-passing layers, batch 4096, T = ceil(50 / simulators) iterations per rollout.

  (a) call    between HIP events and as wall time: the ONE mixed call (walk, assembly, ragged forward, finish: four launches)
              against what the library had before it -- one v2x_rollout_steps per pool (P walk and P finish launches, nobody
              greedy) plus the same ragged forward of the same batch.  Both through rl/device_sim.py's resident wrappers, so both
              carry their policy uploads and result downloads.  The composition is measured five times around the new form; the
              min-max of its five medians is the spread a difference has to exceed.
  (b) agent   MixedAgent's wall time per train step in three forms that are alive in one process, warmed up and taken in turn:
              rollout='trajectory' (device simulators, device streams), the host rollout on host simulators (the default), the
              host rollout on device simulators.  Medians over --repeats runs of --agent-steps train steps, with their min-max.

  (c) walk    --walk-leg: the serial mixed call against the mixed wide walk (v2x_rollout_steps_mixed_wide), both alive in one
              process and taken in turn, at the pools of (a) and at 8 / 12 / 20 links x 17 simulators (T = 1): the call between
              HIP events, its host enqueue, the wall time of a rollout, MixedAgent's train step with either walk, and the
              kernels' own durations through torch's profiler.  Written under "rollout" into profiles/mixed_wide_timing.json
              (tools/mixed_eval_timing.py --walk-leg writes "eval" beside it); nothing else is measured then.

    python tools/mixed_rollout_timing.py [--out profiles/mixed_rollout_timing.json] [--reps 100] [--warmup 10]
    python tools/mixed_rollout_timing.py --walk-leg [--walk-out profiles/mixed_wide_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = (((8, 12, 20, 28), 10), ((8, 12, 20), 1), ((8, 12, 20), 10))
WALK_CONFIGS = CONFIGS + (((8, 12, 20), 17),)            # ... and 51 simulators: T = 1
SERIAL_KERNELS = ("k_sim_trajectory_mixed",)
WIDE_KERNELS = ("k_traj_words_mixed", "k_traj_walk_mixed", "k_traj_uniforms_mixed", "k_traj_terms_mixed", "k_traj_scan_mixed",
                "k_traj_observe_mixed")
SHARED_KERNELS = ("k_traj_assemble_mixed", "k_rollout_finish_mixed")
FORMS = (("trajectory", "device", "device", "trajectory"), ("host_on_host_simulators", "host", "host", "host"),
         ("host_on_device_simulators", "device", "device", "host"))


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
    out = {"mixed_event_ms": one[0], "mixed_wall_ms": one[1],
           "per_pool_event_ms": float(np.median(ev)), "per_pool_event_ms_min_max": [min(ev), max(ev)],
           "per_pool_wall_ms": float(np.median(wall)), "per_pool_wall_ms_min_max": [min(wall), max(wall)]}
    out["mixed_wins_by_more_than_spread_event"] = bool(out["per_pool_event_ms"] - one[0] > max(ev) - min(ev))
    out["mixed_wins_by_more_than_spread_wall"] = bool(out["per_pool_wall_ms"] - one[1] > max(wall) - min(wall))
    return out


def _envs(sizes, E, backend, streams):
    from v2xgnn.rl.train import start_env_batched
    return [start_env_batched(n, E, 1001 + 15485863 * k, backend=backend, streams=streams) for k, n in enumerate(sizes)]


def time_call(sizes, E, args, torch):
    from v2xgnn import GnnEngine, GnnSpec
    from v2xgnn.bs_brain import _glorot_list
    from v2xgnn.engine import DeviceBatch
    from v2xgnn.rl.device_sim import mixed_rollout_buffers, resident_rollout_steps_mixed
    from v2xgnn.rl.mixed import MixedReplay
    T = -(-50 // (E * len(sizes)))
    envs = _envs(sizes, E, "device", "device")
    spec = GnnSpec(n_nodes=1, feat_dim=64, n_mp_layers=2, share_weights=True, variable_graphs=True)
    eng = GnnEngine(spec)
    eng.set_weights(_glorot_list(spec, np.random.default_rng(1)))
    mem = MixedReplay(4096, sizes)
    rng = np.random.default_rng(3)
    explore = [(rng.random((T, E)) < 0.5).astype(np.uint8) for _ in sizes]
    ones = [np.ones((T, E), np.uint8) for _ in sizes]
    actions = [rng.integers(0, 4, size=(T, E, n)).astype(np.int32) for n in sizes]
    for n in sizes:
        mem.reserve(n, T * E)
    stores, heads, caps = [mem.storage(n) for n in sizes], [0] * len(sizes), [4096] * len(sizes)

    def mixed():
        resident_rollout_steps_mixed(envs, explore, actions, stores, heads, caps, 1.0, 0.1, engine=eng)

    mixed()
    buf = mixed_rollout_buffers([e.device_channels for e in envs], T)
    n_max = max(sizes)
    db = DeviceBatch.from_tensors(buf['sizes'][0], 0, buf['xe'], buf['row_ptr'], buf['col_idx'], n_max * (n_max - 2),
                                  graph_off=buf['graph_off'], max_nodes=n_max)
    q = torch.empty_like(buf['q'])

    def per_pool():
        for k, env in enumerate(envs):
            env.rollout_steps(ones[k], actions[k], stores[k], 0, 4096, 1.0, 0.1)
        eng.forward(db, out=q)

    out = _compare(mixed, per_pool, args.reps, args.warmup, torch)
    out.update(sizes=list(sizes), simulators_per_size=E, T=T, graphs=buf['sizes'][0], rows=buf['sizes'][1], pools=len(sizes))
    eng.close()
    return out


def time_agent(sizes, E, args, torch):
    from v2xgnn.rl.mixed import MixedAgent
    from v2xgnn.rl.sim_config import RL_Config
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, args.batch, 1, 0.1)
    agents = {}
    for name, backend, streams, rollout in FORMS:
        np.random.seed(1001)
        agents[name] = MixedAgent(_envs(sizes, E, backend, streams), cfg, 64, seed=1001, rollout=rollout)
        agents[name].train(1, 5)                       # warm-up: buffers, workspaces, the first replays
    torch.cuda.synchronize()
    ms = {name: [] for name in agents}
    for _ in range(args.repeats):
        for name, agent in agents.items():
            t0 = time.perf_counter()
            agent.train(1, args.agent_steps)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.agent_steps)
    out = {"sizes": list(sizes), "simulators_per_size": E, "batch": args.batch, "train_steps": args.agent_steps,
           "repeats": args.repeats, "iterations_per_train_step": agents["trajectory"].n_iter}
    for name, v in ms.items():
        out[name] = {"wall_ms_per_train_step": float(np.median(v)), "min_max": [min(v), max(v)],
                     "rollouts_by_path": dict(agents[name].rollout_stats)}
    t, h = out["trajectory"], out["host_on_host_simulators"]
    spread = max(t["min_max"][1] - t["min_max"][0], h["min_max"][1] - h["min_max"][0])
    out["trajectory_wins_over_default_by_more_than_spread"] = bool(h["wall_ms_per_train_step"] - t["wall_ms_per_train_step"] > spread)
    for agent in agents.values():
        agent.close()
    return out


def _timed_enqueue(fn, reps, warmup, torch):
    """_timed() with the host's own time inside fn() (the enqueue) -> (event ms, wall ms, enqueue ms), medians per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    host = []
    t0 = time.perf_counter()
    for a, b in evs:
        a.record()
        t1 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t1) * 1e3)
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    return float(np.median([a.elapsed_time(b) for a, b in evs])), wall, float(np.median(host))


def walks_in_turn(calls, reps, warmup, torch, rounds=3):
    """calls: {'serial': fn, 'wide': fn}, measured `rounds` times each, in turn -> per walk the median of the rounds' medians
    and their min-max, and who wins by more than the larger spread"""
    seen = {w: [] for w in calls}
    for _ in range(rounds):
        for w, fn in calls.items():
            seen[w].append(_timed_enqueue(fn, reps, warmup, torch))
    out = {}
    for w, v in seen.items():
        out[w] = {}
        for i, name in enumerate(("event_ms", "wall_ms", "enqueue_ms")):
            col = [r[i] for r in v]
            out[w][name] = float(np.median(col))
            out[w][name + "_min_max"] = [min(col), max(col)]
    for name in ("event_ms", "wall_ms"):
        s, w = out["serial"], out["wide"]
        spread = max(s[name + "_min_max"][1] - s[name + "_min_max"][0], w[name + "_min_max"][1] - w[name + "_min_max"][0])
        diff = s[name] - w[name]
        out["winner_" + name] = "wide" if diff > spread else "serial" if -diff > spread else "level"
        out["serial_over_wide_" + name] = round(s[name] / w[name], 3)
    return out


def walk_call(sizes, E, args, torch):
    from sim_device_timing import kernel_times
    from v2xgnn import GnnEngine, GnnSpec
    from v2xgnn.bs_brain import _glorot_list
    from v2xgnn.rl.device_sim import resident_rollout_steps_mixed
    from v2xgnn.rl.mixed import MixedReplay
    T = -(-50 // (E * len(sizes)))
    envs = _envs(sizes, E, "device", "device")
    spec = GnnSpec(n_nodes=1, feat_dim=64, n_mp_layers=2, share_weights=True, variable_graphs=True)
    eng = GnnEngine(spec)
    eng.set_weights(_glorot_list(spec, np.random.default_rng(1)))
    mem = MixedReplay(4096, sizes)
    rng = np.random.default_rng(3)
    explore = [(rng.random((T, E)) < 0.5).astype(np.uint8) for _ in sizes]
    actions = [rng.integers(0, 4, size=(T, E, n)).astype(np.int32) for n in sizes]
    for n in sizes:
        mem.reserve(n, T * E)
    stores, heads, caps = [mem.storage(n) for n in sizes], [0] * len(sizes), [4096] * len(sizes)
    calls = {w: (lambda w=w: resident_rollout_steps_mixed(envs, explore, actions, stores, heads, caps, 1.0, 0.1, engine=eng, walk=w))
             for w in ("serial", "wide")}
    out = walks_in_turn(calls, args.reps, args.warmup, torch)
    out["kernels_ms"] = {"serial": kernel_times(calls["serial"], SERIAL_KERNELS + SHARED_KERNELS, 20),
                         "wide": kernel_times(calls["wide"], WIDE_KERNELS + SHARED_KERNELS, 20)}
    out.update(sizes=list(sizes), simulators_per_size=E, T=T, pools=len(sizes))
    eng.close()
    return out


def walk_agent(sizes, E, args, torch):
    from v2xgnn.rl.mixed import MixedAgent
    from v2xgnn.rl.sim_config import RL_Config
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, args.batch, 1, 0.1)
    agents = {}
    for walk in ("serial", "wide"):
        np.random.seed(1001)
        agents[walk] = MixedAgent(_envs(sizes, E, "device", "device"), cfg, 64, seed=1001, rollout="trajectory", trajectory_walk=walk)
        agents[walk].train(1, 5)                       # warm-up: buffers, workspaces, the first replays
    torch.cuda.synchronize()
    ms = {walk: [] for walk in agents}
    for _ in range(args.repeats):
        for walk, agent in agents.items():
            t0 = time.perf_counter()
            agent.train(1, args.agent_steps)
            torch.cuda.synchronize()
            ms[walk].append((time.perf_counter() - t0) * 1e3 / args.agent_steps)
    out = {"sizes": list(sizes), "simulators_per_size": E, "batch": args.batch, "train_steps": args.agent_steps,
           "repeats": args.repeats, "iterations_per_train_step": agents["wide"].n_iter}
    for walk, v in ms.items():
        out[walk] = {"wall_ms_per_train_step": float(np.median(v)), "min_max": [min(v), max(v)],
                     "rollouts_by_path": dict(agents[walk].rollout_stats),
                     "walk_calls": [dict(e.device_channels.walk_calls) for e in agents[walk].envs]}
    s, w = out["serial"], out["wide"]
    spread = max(s["min_max"][1] - s["min_max"][0], w["min_max"][1] - w["min_max"][0])
    diff = s["wall_ms_per_train_step"] - w["wall_ms_per_train_step"]
    out["winner"] = "wide" if diff > spread else "serial" if -diff > spread else "level"
    for agent in agents.values():
        agent.close()
    return out


def merge_walk_leg(path, key, value):
    """profiles/mixed_wide_timing.json holds the walk legs of this tool ("rollout") and of tools/mixed_eval_timing.py ("eval")"""
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)
    res[key] = value
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def walk_leg(args, torch):
    res = {"feat_dim": 64, "n_mp_layers": 2, "reps": args.reps, "warmup": args.warmup, "call": [], "agent": [],
           "baseline": "the serial mixed call of the same build, alive in the same process and taken in turn with the wide one "
                       "(its kernels and its host path are the parent commit's, unchanged)"}
    for sizes, E in WALK_CONFIGS:
        res["call"].append(walk_call(sizes, E, args, torch))
        print("walk call", json.dumps(res["call"][-1]), flush=True)
    for sizes, E in WALK_CONFIGS:
        res["agent"].append(walk_agent(sizes, E, args, torch))
        print("walk agent", json.dumps(res["agent"][-1]), flush=True)
    merge_walk_leg(args.walk_out, "rollout", res)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk-leg", action="store_true", help="measure the serial against the wide mixed walk, and nothing else")
    ap.add_argument("--walk-out", default=os.path.join(ROOT, "profiles", "mixed_wide_timing.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_rollout_timing.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--agent-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if args.walk_leg:
        return walk_leg(args, torch)
    res = {"feat_dim": 64, "n_mp_layers": 2, "reps": args.reps, "warmup": args.warmup, "call": [], "agent": []}
    for sizes, E in CONFIGS:
        res["call"].append(time_call(sizes, E, args, torch))
        print("call", json.dumps(res["call"][-1]), flush=True)
    for sizes, E in CONFIGS:
        res["agent"].append(time_agent(sizes, E, args, torch))
        print("agent", json.dumps(res["agent"][-1]), flush=True)
    res["trajectory_wins_everywhere"] = all(a["trajectory_wins_over_default_by_more_than_spread"] for a in res["agent"])
    res["mixed_call_wins_everywhere"] = all(c["mixed_wins_by_more_than_spread_event"] for c in res["call"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
