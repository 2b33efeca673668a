"""The device evaluation episode beyond 31 links in numbers: Agent.test_run of one 50-step episode on one simulator with the
episode on the host loop (eval_backend='host': 50 act / observe / predict round trips) against the same episode as ONE call
on the state resident in HBM (eval_backend='device': v2x_eval_steps_recv, and with receiver_streams='split'
v2x_eval_steps_recv_split), at 32, 64, 100 and 128 links.  One process, three agents per size built from the same seed on
DeviceBatchedEnviron(streams='device'), the legs taken in turn, F = 16, an untrained seeded network (the time does not depend
on the weights).

  (a) episode   wall ms of Agent.test_run(1, 50, eval_backend=...) ending in a synchronise, the same seed before every call of
                every leg: median and p10-p90 over --reps calls after one untimed warm-up call per leg.  The episode's reset
                (new_random_game) is inside all three.
  (b) call      DeviceChannels.eval_steps_recv alone (T = 50, E = 1, every step greedy as in test_run, with the baseline
                scheme) between HIP events, chain and split taken in turn: median and p10-p90.
  (c) bytes     what one episode's call moves over the bus, up and down (DeviceChannels.traffic), and the workspaces' sizes.

    python tools/eval_recv_timing.py [--out profiles/eval_recv_timing.json] [--links 32,64,100,128]
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

LEGS = (("host", "host", "chain"), ("device_chain", "device", "chain"), ("device_split", "device", "split"))
T = 50


def _pct(ms):
    ms = sorted(float(v) for v in ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": ms[len(ms) // 10], "p90_ms": ms[(9 * len(ms)) // 10], "n": len(ms)}


def _agent(n, args, receiver_streams):
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, 0.5, args.batch, 1, 0.1)
    env = start_env_batched(n, 1, args.seed, lookahead=False, backend="device", streams="device")
    return Agent(n, env.n_RB, env.n_Neighbor, args.feedback, env, cfg, seed=args.seed, device_replay=False,
                 receiver_streams=receiver_streams)


def episodes(n, args, torch):
    agents = {name: _agent(n, args, streams) for name, _, streams in LEGS}
    ms = {name: [] for name in agents}
    rewards = {}
    for rep in range(-1, args.reps):                       # rep -1: warm-up (buffers, workspaces, first allocation), untimed
        for name, backend, _ in LEGS:
            random.seed(args.seed + rep)
            np.random.seed(args.seed + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = agents[name].test_run(1, T, eval_backend=backend)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert np.all(np.isfinite(out[1]))
            if rep >= 0:
                ms[name].append(dt)
            rewards.setdefault(rep, {})[name] = (out[1].tobytes(), out[6].tobytes())
    res = {"episode": {name: _pct(v) for name, v in ms.items()}}
    e = res["episode"]
    for name in ("device_chain", "device_split"):
        e["host_over_" + name] = e["host"]["median_ms"] / e[name]["median_ms"]
        e[name + "_faster_than_host_spread"] = bool(e[name]["p90_ms"] < e["host"]["p10_ms"])
    e["chain_over_split"] = e["device_chain"]["median_ms"] / e["device_split"]["median_ms"]
    # the three legs walked the same episodes: the random scheme's rewards are the host loop's, the two device legs agree in all
    res["same_random_scheme_rewards"] = all(len({v[1] for v in r.values()}) == 1 for r in rewards.values())
    res["chain_and_split_same_policy_rewards"] = all(r["device_chain"][0] == r["device_split"][0] for r in rewards.values())
    res["policy_rewards_same_as_host"] = all(r["device_chain"][0] == r["host"][0] for r in rewards.values())
    res["episodes_by_path"] = {name: dict(a.eval_stats) for name, a in agents.items()}
    return res, agents


def calls(n, agents, args, torch):
    rng = np.random.default_rng(args.seed + n)
    explore = np.zeros((T, 1), np.uint8)
    rand = np.zeros((T, 1, n), np.int32)
    baseline = rng.integers(0, 4, size=(T, 1, n)).astype(np.int32)
    run, before = {}, {}
    for phase in ("chain", "split"):
        agent = agents["device_" + phase]
        env = agent.env
        dc, engine, own = env.device_channels, agent.brain.model.engine, env.own_receivers()
        if not dc._recv_ready:
            dc.observe_recv(env.dest)

        def call(dc=dc, engine=engine, own=own, phase=phase):
            return dc.eval_steps_recv(explore, rand, baseline, 1.0, 0.1, engine=engine, own=own, stream_phase=phase)
        run[phase] = call
        for _ in range(args.warmup):
            call().resolve()
        before[phase] = dict(dc.traffic)
    torch.cuda.synchronize()
    evs = {p: [] for p in run}
    results = []
    for _ in range(args.reps):
        for phase, call in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            results.append(call())
            b.record()
            evs[phase].append((a, b))
    torch.cuda.synchronize()
    for r in results:
        r.resolve()                                        # (the page-locked result copies go back to their pools)
    out = {"T": T, "E": 1}
    for phase in run:
        st = _pct([a.elapsed_time(b) for a, b in evs[phase]])
        dc = agents["device_" + phase].env.device_channels
        out[phase] = {"event_median_ms": st["median_ms"], "event_p10_ms": st["p10_ms"], "event_p90_ms": st["p90_ms"], "n": st["n"],
                      "bytes_up_per_episode": (dc.traffic['bytes_up'] - before[phase]['bytes_up']) // args.reps,
                      "bytes_down_per_episode": (dc.traffic['bytes_down'] - before[phase]['bytes_down']) // args.reps}
    out["chain_over_split"] = out["chain"]["event_median_ms"] / out["split"]["event_median_ms"]
    out["split_faster_than_chain_spread"] = bool(out["split"]["event_p90_ms"] < out["chain"]["event_p10_ms"])
    io = agents["device_split"].env.device_channels.eval_steps_recv_buffers(T)
    out["workspace_bytes"] = int(io['workspace'].numel())
    out["split_workspace_bytes"] = int(io['split_workspace'].numel())
    out["result_block_bytes"] = int(io['eval_result_dev'].numel())
    for name, agent in agents.items():
        if name != "host":
            agent.env._resident_after(None)                # (the calls stepped the resident state behind the simulator's back)
        agent.brain.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_recv_timing.json"))
    ap.add_argument("--links", default="32,64,100,128")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1001)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_recv_timing: needs a GPU (a timing taken without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "feat_dim": args.feedback, "seed": args.seed, "steps_per_episode": T,
           "calls_per_leg": args.reps,
           "how": "one process, three agents per size from the same seed on one resident simulator, the legs host / device_chain / "
                  "device_split taken in turn; episode: wall ms of Agent.test_run(1, 50, eval_backend=...) ending in a synchronise, "
                  "the same seed before every call, median and p10-p90 after one untimed call per leg; call: HIP events around "
                  "DeviceChannels.eval_steps_recv(stream_phase=...) (T = 50, every step greedy, with the baseline scheme), chain and "
                  "split in turn, median and p10-p90; x_faster_than_host_spread: x's p90 below the host leg's p10",
           "links": {}}
    for n in [int(v) for v in args.links.split(",")]:
        entry, agents = episodes(n, args, torch)
        print(n, "episode", json.dumps(entry), flush=True)
        entry["call"] = calls(n, agents, args, torch)
        print(n, "call", json.dumps(entry["call"]), flush=True)
        res["links"][str(n)] = entry
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
