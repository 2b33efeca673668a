"""The jump-ahead words of the receiver-form split stream phase in numbers (v2x_rollout_steps_recv_jump / v2x_eval_steps_recv_jump
against their _split forms: receiver_words='jump' against 'serial', both with receiver_streams='split').  One process, two
resident agents per size built from the same seed, serial and jump taken in turn with the same seed before every call.

  (a) train step    wall ms per train step of Agent.train (50 simulator steps + 1 replay step) ending in a synchronise.
  (b) rollout call  DeviceChannels.rollout_steps_recv(stream_phase='split', stream_words=...) alone (T = 50, every second step
                    greedy: a forward in every call) between HIP events.
  (c) launches      the duration of each of the call's launches through torch's profiler, in a run of its own per form (the
                    forward's launches as one sum): k_traj_words_recv (jump: the prefix), k_traj_jump_seeds, k_traj_jump_chunks.
  (d) episode call  DeviceChannels.eval_steps_recv (T = 50, every step greedy, with the baseline scheme) between HIP events.
  (e) memory, table the polynomial table and the scratch in bytes, the chunks, and the host's wall time for the table
                    (v2x_mt_jump_polys; the first call of a process also finds the characteristic polynomial).
  (f) strides       --strides: the rollout call and the three launches with the chunk stride forced to each of the listed
                    values (DeviceChannels.jump_plan overridden; the table of each built outside the timed calls).

Sizes: --links with one simulator, and --batched N:E pairs (64:10 by default).  Median and p10-p90 of --call-reps calls after
untimed warm-up calls.

    python tools/rollout_recv_jump_timing.py [--out profiles/rollout_recv_jump_timing.json] [--links 32,64,100,128]
                                             [--strides 32688,58112,116224,232448]
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rollout_recv_timing import LAUNCHES, _kernel_times, _pct  # noqa: E402

SERIAL_LAUNCHES = ("k_traj_words", "k_traj_walk", "k_traj_uniforms") + LAUNCHES[1:]
JUMP_LAUNCHES = ("k_traj_jump_seeds", "k_traj_jump_chunks") + SERIAL_LAUNCHES
T = 50


def _agent(n, args, E, words):
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, 0.5, args.batch, 1, 0.1)
    env = start_env_batched(n, E, args.seed, lookahead=False, backend="device", streams="device")
    return Agent(n, env.n_RB, env.n_Neighbor, args.feedback, env, cfg, seed=args.seed, device_replay='receivers',
                 rollout_backend='trajectory', trajectory_walk='wide', receiver_streams='split', receiver_words=words)


def _events(calls, reps, torch):
    """the calls taken in turn, each between HIP events -> {name: median / p10 / p90 ms}"""
    evs = {k: [] for k in calls}
    for _ in range(reps):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            evs[name].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for name in calls:
        st = _pct([a.elapsed_time(b) for a, b in evs[name]])
        out[name] = {"event_median_ms": st["median_ms"], "event_p10_ms": st["p10_ms"], "event_p90_ms": st["p90_ms"], "n": st["n"]}
    return out


def _verdict(d, prefix="event_"):
    """serial over jump, and whether jump's p90 lies below serial's p10"""
    d["serial_over_jump"] = d["serial"][prefix + "median_ms"] / d["jump"][prefix + "median_ms"]
    d["jump_faster_than_serial_spread"] = bool(d["jump"][prefix + "p90_ms"] < d["serial"][prefix + "p10_ms"])


def one_size(n, E, args, torch):
    from v2xgnn.rl.device_sim import MT_WORDS, split_stream_blocks
    agents = {w: _agent(n, args, E, w) for w in ("serial", "jump")}
    per_step = {w: [] for w in agents}
    for rep in range(-1, args.call_reps):                  # rep -1: warm-up (buffers, workspaces, the table), untimed
        for words, agent in agents.items():
            random.seed(args.seed + rep)
            np.random.seed(args.seed + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = agent.train(1, args.steps)[0]
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3 / args.steps
            assert np.all(np.isfinite(loss))
            if rep >= 0:
                per_step[words].append(dt)
    out = {"E": E, "train_step": {w: _pct(v) for w, v in per_step.items()}}
    _verdict(out["train_step"], prefix="")
    out["stream_words_calls"] = {w: dict(a.env.device_channels.stream_words_calls) for w, a in agents.items()}
    rng = np.random.default_rng(args.seed + n)
    explore = np.ones((T, E), np.uint8)
    explore[::2] = 0
    rand = rng.integers(0, 4, size=(T, E, n)).astype(np.int32)
    baseline = rng.integers(0, 4, size=(T, E, n)).astype(np.int32)
    greedy = np.zeros((T, E), np.uint8)
    rollouts, episodes = {}, {}
    for words, agent in agents.items():
        env, rep = agent.env, agent.device_replay
        dc, engine, own = env.device_channels, agent.brain.model.engine, env.own_receivers()
        if not dc._recv_ready:
            dc.observe_recv(env.dest)

        def rollout(dc=dc, rep=rep, engine=engine, own=own, words=words):
            head = rep.reserve(T * E)                      # (never committed: the same block is rewritten)
            return dc.rollout_steps_recv(explore, rand, rep.storage(), head, rep.capacity, 1.0, 0.1, engine=engine, own=own,
                                         stream_phase='split', stream_words=words)

        def episode(dc=dc, engine=engine, own=own, words=words):
            return dc.eval_steps_recv(greedy, rand, baseline, 1.0, 0.1, engine=engine, own=own, stream_phase='split', stream_words=words)

        rollouts[words], episodes[words] = rollout, episode
        for _ in range(args.warmup):
            rollout()
            episode()
    torch.cuda.synchronize()
    out["rollout_call"] = dict(_events(rollouts, args.call_reps, torch), T=T, E=E)
    _verdict(out["rollout_call"])
    out["episode_call"] = dict(_events(episodes, args.call_reps, torch), T=T, E=E)
    _verdict(out["episode_call"])
    out["launches_ms"] = {"serial": _kernel_times(rollouts["serial"], args.profile_reps, torch, SERIAL_LAUNCHES),
                          "jump": _kernel_times(rollouts["jump"], args.profile_reps, torch, JUMP_LAUNCHES)}
    dc = agents["jump"].env.device_channels
    io = dc.rollout_steps_recv_buffers(T)
    jump = dc._recv_jump_table(T)
    nbw = split_stream_blocks(n, dc.rb, T, dc._grid[0].shape[1]) * MT_WORDS
    out["words_per_state"] = int(nbw)
    out["plan"] = {"first": int(jump.first), "stride": int(jump.stride), "chunks": int(jump.count)}
    out["table_bytes"] = 4 * MT_WORDS * int(jump.count)
    out["scratch_bytes"] = int(jump.scratch_bytes)
    out["split_workspace_bytes"] = int(io['split_workspace'].numel())
    host = np.zeros((max(int(jump.count), 1), MT_WORDS), np.uint32)
    t0 = time.perf_counter()
    rc = dc._lib.v2x_mt_jump_polys(int(jump.first), int(jump.stride), max(int(jump.count), 1), host.ctypes.data)
    out["table_host_ms"] = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    if args.strides:
        out["strides"] = {}
        for stride in [int(v) for v in args.strides.split(",")]:
            first = int(jump.first)
            count = -(-(nbw - first) // stride)
            dc.jump_plan = lambda _nbw, plan=(first, stride, count): plan
            io.pop('jump', None)
            for _ in range(args.warmup):
                rollouts["jump"]()
            torch.cuda.synchronize()
            entry = dict(_events({"jump": rollouts["jump"]}, args.call_reps, torch)["jump"], chunks=int(count))
            entry["launches_ms"] = _kernel_times(rollouts["jump"], args.profile_reps, torch, JUMP_LAUNCHES)
            out["strides"][str(stride)] = entry
        del dc.jump_plan
        io.pop('jump', None)
    for agent in agents.values():
        agent.env._resident_after(None)                    # (the calls stepped the resident state behind the simulator's back)
        agent.brain.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_recv_jump_timing.json"))
    ap.add_argument("--links", default="32,64,100,128")
    ap.add_argument("--batched", default="64:10", help="further sizes as links:simulators pairs")
    ap.add_argument("--strides", default="", help="chunk strides to force in turn (multiples of 227), e.g. 32688,58112,116224,232448")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4, help="train steps per timed Agent.train call")
    ap.add_argument("--call-reps", type=int, default=20)
    ap.add_argument("--profile-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1001)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_recv_jump_timing: needs a GPU (a timing taken without one says nothing)")
    t0 = time.perf_counter()
    from v2xgnn.lib import load_library
    one = np.zeros((1, 624), np.uint32)
    assert load_library().v2x_mt_jump_polys(20561, 624, 1, one.ctypes.data) == 0
    first_table_ms = (time.perf_counter() - t0) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "feat_dim": args.feedback, "seed": args.seed,
           "train_steps_per_call": args.steps, "calls_per_form": args.call_reps,
           "first_table_of_the_process_ms": first_table_ms,
           "how": "one process, two resident agents per size from the same seed (receiver_streams='split'), receiver_words 'serial' "
                  "and 'jump' taken in turn; train_step: wall ms per train step of Agent.train(1, steps) ending in a synchronise, the "
                  "same seed before every call, median and p10-p90; rollout_call / episode_call: HIP events around "
                  "DeviceChannels.rollout_steps_recv / eval_steps_recv (T = 50), median and p10-p90 after one untimed call; "
                  "launches_ms: torch's profiler in a run of its own per form, median per launch, the forward's launches summed; "
                  "table_host_ms: wall time of v2x_mt_jump_polys for the size's plan (the characteristic polynomial cached: "
                  "first_table_of_the_process_ms holds the first call, library load included); strides: the jump form's rollout "
                  "call and launches with the stride forced",
           "sizes": {}}
    sizes = [(int(v), 1) for v in args.links.split(",") if v] + [tuple(int(x) for x in v.split(":")) for v in args.batched.split(",") if v]
    for n, E in sizes:
        entry = one_size(n, E, args, torch)
        print(n, E, json.dumps(entry), flush=True)
        res["sizes"]["%d links x %d" % (n, E)] = entry
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
