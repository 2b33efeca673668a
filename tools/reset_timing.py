"""The episode reset of a DeviceBatchedEnviron(streams='device') in numbers: reset='host' (the default: one download of the stream
state, the host library's draws, uploads at the next device call) against reset='device' (v2x_sim_reset: three launches on the
resident state and one small download).  Both forms are alive in one process, warmed up and taken in turn; medians of --reps
after --warmup, with their min-max.  "Wins" means by more than the larger of the two spreads; no ratio is promised, the file says
who won.  The baseline is the host reset of the same build, whose code is the parent commit's.

  reset           new_random_game alone at 20 links with 1 / 10 / 50 simulators and at 8 and 28 links with one.  Before every
                  timed reset one untimed act() leaves the state as an episode does: the device holds the newer streams,
                  positions and channels.  The timed span ends when the next device call could start: for the host reset that
                  includes the uploads it leaves pending (device_channels flushes them); the device reset leaves none.
  episode         Agent.test_run(1, 50, eval_backend='device') at 20 links, one simulator: reset, draws, one evaluate_steps call.
  train_step      Agent.train(1, 20) with rollout_backend='trajectory' at 20 links with 10 and 50 simulators: wall / 20.

    python tools/reset_timing.py [--out profiles/reset_device_timing.json] [--reps 20] [--warmup 3]
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

FEAT, RESETS = 64, ("host", "device")


def in_turn(forms, reps, warmup, torch, before=None):
    """forms: name -> callable; -> name -> {median_ms, min_max} of `reps` timed calls each, taken in turn after `warmup`"""
    ms = {name: [] for name in forms}
    for rep in range(warmup + reps):
        for name, fn in forms.items():
            if before is not None:
                before(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": float(np.median(v)), "min_max": [min(v), max(v)]} for name, v in ms.items()}


def verdict(out, a="host", b="device"):
    spread = max(out[a]["min_max"][1] - out[a]["min_max"][0], out[b]["min_max"][1] - out[b]["min_max"][0])
    diff = out[a]["median_ms"] - out[b]["median_ms"]
    out["winner"] = b if diff > spread else a if -diff > spread else "level"
    out["host_over_device"] = round(out[a]["median_ms"] / out[b]["median_ms"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reset_device_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    res = {"feat_dim": FEAT, "reps": args.reps, "warmup": args.warmup, "reset": [],
           "baseline": "reset='host' of the same build, alive in the same process and taken in turn with reset='device' (its code is "
                       "the parent commit's, unchanged)"}

    def save():                                               # after every leg: what is measured so far
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    def env_of(n, E, reset, seed=1001):
        return start_env_batched(n, E, seed, backend="device", streams="device", reset=reset)

    # (1) the reset alone
    for n, E in ((20, 1), (20, 10), (20, 50), (8, 1), (28, 1)):
        envs = {r: env_of(n, E, r) for r in RESETS}
        rng = np.random.default_rng(1)

        def step(name):
            envs[name].act(rng.integers(0, 4, size=(E, n, 1)))

        def reset(name):
            envs[name].new_random_game(n)
            envs[name].device_channels                        # (what the reset left pending for the next device call)

        out = verdict(in_turn({r: (lambda r=r: reset(r)) for r in RESETS}, args.reps, args.warmup, torch, before=step))
        out.update(links=n, simulators=E, resets_by_path=dict(envs["device"].reset_stats), flagged_states=envs["device"].reset_ties)
        res["reset"].append(out)
        print("reset", json.dumps(out), flush=True)
    save()

    # (2) an evaluation episode, (3) a train step
    def agent_of(n, E, reset, batch, **kw):
        random.seed(1001)
        np.random.seed(1001)
        env = env_of(n, E, reset)
        cfg = RL_Config()
        cfg.set_train_value(FEAT, 0.5, batch, 1, 0.1)
        return Agent(n, env.n_RB, env.n_Neighbor, FEAT, env, cfg, seed=1001, **kw)

    agents = {r: agent_of(20, 1, r, 512, device_replay=False) for r in RESETS}
    out = verdict(in_turn({r: (lambda r=r: agents[r].test_run(1, 50, False, eval_backend='device')) for r in RESETS}, args.reps,
                          args.warmup, torch))
    out.update(links=20, simulators=1, steps=50, episodes_by_path={r: dict(agents[r].eval_stats) for r in RESETS},
               resets_by_path=dict(agents["device"].env.reset_stats))
    res["episode"] = out
    print("episode", json.dumps(out), flush=True)
    save()
    for a in agents.values():
        a.brain.close()

    res["train_step"] = []
    for E in (10, 50):
        agents = {r: agent_of(20, E, r, 512, device_replay=True, rollout_backend='trajectory') for r in RESETS}
        out = in_turn({r: (lambda r=r: agents[r].train(1, 20)) for r in RESETS}, max(3, args.reps // 4), 1, torch)
        for r in RESETS:                                      # an episode of 20 train steps -> per train step
            out[r] = {"median_ms": out[r]["median_ms"] / 20, "min_max": [v / 20 for v in out[r]["min_max"]]}
        out = verdict(out)
        out.update(links=20, simulators=E, train_steps_per_episode=20, batch=512, rollout="trajectory",
                   resets_by_path=dict(agents["device"].env.reset_stats))
        res["train_step"].append(out)
        print("train_step", json.dumps(out), flush=True)
        for a in agents.values():
            a.brain.close()

    save()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
