"""The resident rollout beyond 31 links in numbers: Agent.train on the receiver replay with the rollouts on the host simulator
(--replay receivers, the array path: 50 host simulator steps, two float64 observations and a PackedBatch.from_dense per
predict) against the same memory with every rollout as ONE call on the state resident in HBM (--rollout trajectory:
v2x_rollout_steps_recv), at 32, 64 and 100 links.  One process, the forms taken in turn, one simulator, batch 512, F = 16.

  (a) train step   wall ms per train step of Agent.train (50 simulator steps + 1 replay step), the same seed before every call
                   of either form: median and min-max over --reps calls of --steps train steps, each ending in a synchronise.
  (b) rollout call DeviceChannels.rollout_steps_recv alone (T = 50, E = 1, every second step greedy: a forward in every call)
                   between HIP events, and the wall time per call of the timed loop (ending in a synchronise).
  (c) launches     the duration of each of the call's launches through torch's profiler, in a run of its own (the forward's
                   launches as one sum), and which of them is the longest.
  (d) bytes        what one rollout moves over the bus, up and down (DeviceChannels.traffic), and the workspace's size.

    python tools/rollout_recv_timing.py [--out profiles/rollout_recv_timing.json] [--links 32,64,100]

--stream-phases: the leg of the split stream phase instead (v2x_rollout_steps_recv_split against v2x_rollout_steps_recv), one
process, two resident agents per size built from the same seed, the two forms taken in turn with the same seed before every
call: (a) ms per train step, (b) the rollout call alone between HIP events, (c) the launches of each form (the split form's
k_traj_words_recv / k_traj_walk_recv / k_traj_uniforms separately), (e) the split workspace's size.  Sizes: --links with one
simulator, and --batched N:E pairs (64:10 by default).

    python tools/rollout_recv_timing.py --stream-phases [--out profiles/rollout_recv_split_timing.json] [--links 32,64,100,128]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAUNCHES = ("k_traj_stream", "k_traj_terms", "k_traj_scan", "k_traj_observe", "k_csr_from_recv", "k_rollout_finish")
SPLIT_LAUNCHES = ("k_traj_words", "k_traj_walk", "k_traj_uniforms") + LAUNCHES[1:]


def _stats(ms):
    ms = [float(v) for v in ms]
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _pct(ms):
    ms = sorted(float(v) for v in ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": ms[len(ms) // 10], "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def _agent(n, resident, args, E=1, receiver_streams='chain'):
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env, start_env_batched
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, 0.5, args.batch, 1, 0.1)
    if resident:
        env = start_env_batched(n, E, args.seed, lookahead=False, backend="device", streams="device")
        return Agent(n, env.n_RB, env.n_Neighbor, args.feedback, env, cfg, seed=args.seed, device_replay='receivers',
                     rollout_backend='trajectory', trajectory_walk='wide', receiver_streams=receiver_streams)
    env = start_env(n)
    return Agent(n, env.n_RB, env.n_Neighbor, args.feedback, env, cfg, seed=args.seed, device_replay='receivers')


def train_steps(n, args, torch):
    agents = {"host_rollout": _agent(n, False, args), "resident_rollout": _agent(n, True, args)}
    per_step = {k: [] for k in agents}
    for rep in range(-1, args.reps):                       # rep -1: warm-up (buffers, workspaces, first allocation), untimed
        for name, agent in agents.items():
            random.seed(args.seed + rep)
            np.random.seed(args.seed + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = agent.train(1, args.steps)[0]
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / args.steps
            assert np.all(np.isfinite(loss))
            if rep >= 0:
                per_step[name].append(dt)
    out = {"train_step": {k: _stats(v) for k, v in per_step.items()}}
    out["train_step"]["host_over_resident"] = (out["train_step"]["host_rollout"]["median_ms"]
                                               / out["train_step"]["resident_rollout"]["median_ms"])
    dc = agents["resident_rollout"].env.device_channels
    out["resident_calls"] = dict(dc.walk_calls)
    return out, agents["resident_rollout"]


def _kernel_times(call, reps, torch, LAUNCHES=LAUNCHES):
    """median duration (ms) of every launch of `call` by kernel name, the launches that are none of LAUNCHES summed per call as
    'forward'; through torch's profiler, or the reason why not"""
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        seen, other = {k: [] for k in LAUNCHES}, 0.0
        for ev in prof.events():
            us = getattr(ev, "device_time", None)
            us = float(getattr(ev, "cuda_time", 0.0) if us is None else us)
            hit = [k for k in LAUNCHES if k in ev.name]
            if hit:
                seen[hit[0]].append(us)
            elif "Memcpy" not in ev.name and "Memset" not in ev.name:
                other += us
        if not all(seen.values()):
            return {"error": "no kernel records for %s" % [k for k, v in seen.items() if not v]}
        res = {k: round(float(np.median(v)) * 1e-3, 4) for k, v in seen.items()}
        res["forward"] = round(other * 1e-3 / reps, 4)
        res["longest"] = max(res, key=res.get)
        return res
    except Exception as exc:                                           # written down, not hidden
        return {"error": "%s: %s" % (type(exc).__name__, exc)}


def rollout_call(n, agent, args, torch):
    env, rep, T = agent.env, agent.device_replay, 50
    dc = env.device_channels
    engine = agent.brain.model.engine
    rng = np.random.default_rng(args.seed + n)
    explore = np.ones((T, 1), np.uint8)
    explore[::2] = 0
    rand = rng.integers(0, 4, size=(T, 1, n)).astype(np.int32)
    own = env.own_receivers()

    def call():
        head = rep.reserve(T)                              # (never committed: the same block is rewritten)
        return dc.rollout_steps_recv(explore, rand, rep.storage(), head, rep.capacity, 1.0, 0.1, engine=engine, own=own)

    if not dc._recv_ready:
        dc.observe_recv(env.dest)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    before = dict(dc.traffic)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.call_reps)]
    t0 = time.perf_counter()
    for a, b in evs:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    loop_wall = (time.perf_counter() - t0) * 1e3 / args.call_reps
    ev = sorted(a.elapsed_time(b) for a, b in evs)
    out = {"T": T, "E": 1, "event_median_ms": float(np.median(ev)), "event_p10_ms": ev[len(ev) // 10],
           "event_p90_ms": ev[(9 * len(ev)) // 10], "loop_wall_ms_per_call": loop_wall, "n": args.call_reps,
           "event_ms_per_simulator_step": float(np.median(ev)) / T,
           "bytes_up_per_rollout": (dc.traffic['bytes_up'] - before['bytes_up']) // args.call_reps,
           "bytes_down_per_rollout": (dc.traffic['bytes_down'] - before['bytes_down']) // args.call_reps,
           "workspace_bytes": int(dc.rollout_steps_recv_buffers(T)['workspace'].numel()),
           "uniforms_per_step": int(dc.n_u), "mt19937_words_per_step": 2 * int(dc.n_u)}
    out["launches_ms"] = _kernel_times(call, args.profile_reps, torch)
    env._resident_after(None)                              # (the calls stepped the resident state behind the simulator's back)
    return out


def stream_phases(n, E, args, torch):
    """chain against split at n links and E simulators: two resident agents from the same seed, the forms in turn"""
    from v2xgnn.rl.device_sim import split_workspace_layout
    agents = {p: _agent(n, True, args, E, p) for p in ("chain", "split")}
    per_step = {p: [] for p in agents}
    for rep in range(-1, args.call_reps):                  # rep -1: warm-up (buffers, workspaces, first allocation), untimed
        for phase, agent in agents.items():
            random.seed(args.seed + rep)
            np.random.seed(args.seed + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = agent.train(1, args.steps)[0]
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / args.steps
            assert np.all(np.isfinite(loss))
            if rep >= 0:
                per_step[phase].append(dt)
    out = {"E": E, "train_step": {p: _pct(v) for p, v in per_step.items()}}
    out["stream_phase_calls"] = {p: dict(a.env.device_channels.stream_phase_calls) for p, a in agents.items()}
    T = 50
    rng = np.random.default_rng(args.seed + n)
    explore = np.ones((T, E), np.uint8)
    explore[::2] = 0
    rand = rng.integers(0, 4, size=(T, E, n)).astype(np.int32)
    calls = {}
    for phase, agent in agents.items():
        env, rep = agent.env, agent.device_replay
        dc, engine, own = env.device_channels, agent.brain.model.engine, env.own_receivers()
        if not dc._recv_ready:
            dc.observe_recv(env.dest)

        def call(dc=dc, rep=rep, engine=engine, own=own, phase=phase):
            head = rep.reserve(T * E)                      # (never committed: the same block is rewritten)
            return dc.rollout_steps_recv(explore, rand, rep.storage(), head, rep.capacity, 1.0, 0.1, engine=engine, own=own,
                                         stream_phase=phase)
        calls[phase] = call
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    evs = {p: [] for p in calls}
    for _ in range(args.call_reps):
        for phase, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            evs[phase].append((a, b))
    torch.cuda.synchronize()
    out["rollout_call"] = {"T": T, "E": E}
    for phase in calls:
        st = _pct([a.elapsed_time(b) for a, b in evs[phase]])
        out["rollout_call"][phase] = {"event_median_ms": st["median_ms"], "event_p10_ms": st["p10_ms"], "event_p90_ms": st["p90_ms"],
                                      "n": st["n"]}
    c, s = out["rollout_call"]["chain"], out["rollout_call"]["split"]
    out["rollout_call"]["chain_over_split"] = c["event_median_ms"] / s["event_median_ms"]
    out["rollout_call"]["split_faster_than_chain_spread"] = bool(s["event_p90_ms"] < c["event_p10_ms"])
    t = out["train_step"]
    t["chain_over_split"] = t["chain"]["median_ms"] / t["split"]["median_ms"]
    t["split_faster_than_chain_spread"] = bool(t["split"]["p90_ms"] < t["chain"]["p10_ms"])
    out["launches_ms"] = {"chain": _kernel_times(calls["chain"], args.profile_reps, torch),
                          "split": _kernel_times(calls["split"], args.profile_reps, torch, SPLIT_LAUNCHES)}
    dc = agents["split"].env.device_channels
    io = dc.rollout_steps_recv_buffers(T)
    out["workspace_bytes"] = int(io['workspace'].numel())
    out["split_workspace_bytes"] = int(io['split_workspace'].numel())
    assert out["split_workspace_bytes"] == split_workspace_layout(E, n, dc.rb, T, dc._grid[0].shape[1])[1]
    for agent in agents.values():
        agent.env._resident_after(None)                    # (the calls stepped the resident state behind the simulator's back)
        agent.brain.close()
    return out


def main_stream_phases(args, torch):
    out_path = args.out or os.path.join(ROOT, "profiles", "rollout_recv_split_timing.json")
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "feat_dim": args.feedback, "seed": args.seed,
           "train_steps_per_call": args.steps, "calls_per_form": args.call_reps,
           "how": "one process, two resident agents per size from the same seed, chain and split taken in turn; train_step: wall ms "
                  "per train step of Agent.train(1, steps) ending in a synchronise, the same seed before every call, median and "
                  "p10-p90; rollout_call: HIP events around DeviceChannels.rollout_steps_recv(stream_phase=...) (T = 50, every "
                  "second step greedy), median and p10-p90; launches_ms: torch's profiler in a run of its own per form, median per "
                  "launch, the forward's launches summed; split_faster_than_chain_spread: split's p90 below chain's p10",
           "sizes": {}}
    sizes = [(int(v), 1) for v in args.links.split(",") if v] + [tuple(int(x) for x in v.split(":")) for v in args.batched.split(",") if v]
    for n, E in sizes:
        entry = stream_phases(n, E, args, torch)
        print(n, E, json.dumps(entry), flush=True)
        res["sizes"]["%d links x %d" % (n, E)] = entry
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/rollout_recv_timing.json (rollout_recv_split_timing.json "
                                                "with --stream-phases)")
    ap.add_argument("--links", default=None, help="default: 32,64,100 (32,64,100,128 with --stream-phases)")
    ap.add_argument("--stream-phases", action="store_true", help="the leg of chain against split (see the module text)")
    ap.add_argument("--batched", default="64:10", help="with --stream-phases: further sizes as links:simulators pairs")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4, help="train steps per timed Agent.train call")
    ap.add_argument("--reps", type=int, default=5, help="timed Agent.train calls per form")
    ap.add_argument("--call-reps", type=int, default=20)
    ap.add_argument("--profile-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1001)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_recv_timing: needs a GPU (a timing taken without one says nothing)")
    if args.stream_phases:
        args.links = "32,64,100,128" if args.links is None else args.links
        return main_stream_phases(args, torch)
    args.out = args.out or os.path.join(ROOT, "profiles", "rollout_recv_timing.json")
    args.links = args.links or "32,64,100"
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "feat_dim": args.feedback, "seed": args.seed,
           "train_steps_per_call": args.steps, "calls_per_form": args.reps,
           "how": "one process, the forms taken in turn; train_step: wall ms per train step of Agent.train(1, steps) ending in a "
                  "synchronise, the same seed before every call; rollout_call: HIP events around DeviceChannels.rollout_steps_recv "
                  "(T = 50, one simulator, every second step greedy) and the wall ms per call of that loop; launches_ms: torch's profiler "
                  "in a run of its own, median per launch, the forward's launches summed",
           "links": {}}
    for n in [int(v) for v in args.links.split(",")]:
        entry, agent = train_steps(n, args, torch)
        print(n, "train", json.dumps(entry), flush=True)
        entry["rollout_call"] = rollout_call(n, agent, args, torch)
        print(n, "call", json.dumps(entry["rollout_call"]), flush=True)
        res["links"][str(n)] = entry
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
