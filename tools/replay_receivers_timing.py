"""Training beyond 31 links in numbers: the reference's host replay memory (Agent.replay's host path: a float64 state +
dense adjacency per transition, np.stack per minibatch, predict / predict / fit as three calls) against the HBM memory that
stores the receivers (rl/replay.py ReceiverReplay: one v2x_replay_gather_recv launch, one v2x_dqn_step call), at 32, 64 and
100 links.  One process, the two forms taken in turn.

  (a) train step   wall time per train step of Agent.train (50 simulator steps + 1 replay step; one host simulator, batch 512),
                   same seed before every call of either form: median and min-max over --reps calls of --steps train steps;
                   and the replay step alone (Agent.replay, ending in the read-back of its losses), median and min-max.
  (b) sample       the minibatch made ready in HBM, batch 4096 (halved until the host form's arrays fit the free host
                   memory; the batch used is recorded): ReceiverReplay.sample between HIP events (all graphs regular, and
                   with own-receiver graphs in the minibatch) and as wall time per call of the timed loop; the host form --
                   Memory.sample, np.stack of s and s', PackedBatch.from_dense of both, copy to the device, synchronise --
                   as wall time.  Synthetic transitions (random receivers and features): the work depends on shapes only.

    python tools/replay_receivers_timing.py [--out profiles/replay_receivers_timing.json] [--links 32,64,100]
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


def _stats(ms):
    ms = [float(v) for v in ms]
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _agent(n, mode, args):
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, 0.5, args.batch, 1, 0.1)
    env = start_env(n)
    return Agent(n, env.n_RB, env.n_Neighbor, args.feedback, env, cfg, seed=args.seed, device_replay=mode)


def train_steps(n, args, torch):
    agents = {"host": _agent(n, False, args), "receivers": _agent(n, 'receivers', args)}
    assert agents["host"].device_replay is None and agents["receivers"].device_replay is not None
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
    replay = {k: [] for k in agents}
    for rep in range(args.replay_reps):
        for name, agent in agents.items():
            np.random.seed(args.seed + 1000 + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.replay()
            torch.cuda.synchronize()
            replay[name].append((time.perf_counter() - t0) * 1e3)
    out = {"train_step": {k: _stats(v) for k, v in per_step.items()}, "replay_step": {k: _stats(v) for k, v in replay.items()},
           "stored_transitions": {"host": len(agents["host"].memory.samples), "receivers": len(agents["receivers"].device_replay)}}
    for sec in ("train_step", "replay_step"):
        out[sec]["host_over_receivers"] = out[sec]["host"]["median_ms"] / out[sec]["receivers"]["median_ms"]
    return out


def _free_host_bytes():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def _synthetic(rng, K, n):
    """K transitions with random receivers: (x, e, adj, action, reward, x', e') as the rollouts hand them to a memory"""
    from v2xgnn.rl.replay import receivers_to_adjacency
    r = rng.integers(0, n - 1, size=(K, n))
    recv = r + (r >= np.arange(n)[None, :])
    return (rng.normal(size=(K, n, 9)), rng.normal(size=(K, n, 4)), receivers_to_adjacency(recv), rng.integers(0, 4, size=(K, n)),
            rng.normal(size=K), rng.normal(size=(K, n, 9)), rng.normal(size=(K, n, 4)))


def _event_timed(fn, reps, warmup, torch):
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
    ev = sorted(a.elapsed_time(b) for a, b in evs)
    return {"event_median_ms": float(np.median(ev)), "event_p10_ms": ev[len(ev) // 10], "event_p90_ms": ev[(9 * len(ev)) // 10],
            "wall_ms_per_call": wall, "n": reps}


def sample_timing(n, args, torch):
    from v2xgnn import PackedBatch
    from v2xgnn.engine import DeviceBatch
    from v2xgnn.rl.agent import Memory
    from v2xgnn.rl.replay import ReceiverReplay
    B = args.sample_batch
    d = n * 13 + n * n
    free = _free_host_bytes()
    # the host form holds 2 B float64 states in its memory, stacks them again and packs float32 copies: ~5 B d 8 bytes
    while free is not None and B > 64 and 5 * B * d * 8 > 0.5 * free:
        B //= 2
    stored = 2 * B
    rng = np.random.default_rng(args.seed + n)
    rep, mem = ReceiverReplay(stored + 64, n), Memory(stored + 64)
    for first in range(0, stored, 1024):
        K = min(1024, stored - first)
        x, e, adj, a, r, x2, e2 = _synthetic(rng, K, n)
        rep.add_many(x, e, adj, a, r, x2, e2)
        rep.flush()
        if first < B + 1024:                               # (the host form draws from the first B + 1024 only: host memory)
            for k in range(K):
                st = np.concatenate((np.concatenate((x[k], e[k]), axis=1).reshape(1, -1), adj[k].reshape(1, -1)), axis=-1)
                st2 = np.concatenate((np.concatenate((x2[k], e2[k]), axis=1).reshape(1, -1), adj[k].reshape(1, -1)), axis=-1)
                mem.add([st, a[k].reshape(1, -1), float(r[k]), st2])
    out = {"batch": B, "stored_transitions": stored, "transition_bytes": {"receivers": 2 * n * 64 + 2 * n * 4 + 8,
                                                                          "host": 2 * d * 8 + n * 8 + 8}}
    np.random.seed(args.seed)
    draws = [np.random.choice(stored, B, replace=False) for _ in range(8)]
    it = [0]

    def regular():
        it[0] += 1
        rep.sample(draws[it[0] % 8])
    out["receivers_regular"] = _event_timed(regular, args.sample_reps, 20, torch)
    # bytes the launch moves: xe and xe' rows read and written, CSR written, receivers / actions read, actions written
    moved = B * (4 * n * 64 + 4 * (n * (n - 2) + n + 1) + 3 * n * 4 + 16)
    out["receivers_regular"]["bytes_moved"] = moved
    out["receivers_regular"]["GB_per_s_of_event_median"] = moved / out["receivers_regular"]["event_median_ms"] / 1e6
    # own-receiver graphs in the minibatch: 64 more transitions whose link 1 is its own receiver, one of them per draw
    x, e, adj, a, r, x2, e2 = _synthetic(rng, 64, n)
    adj[:, :, 1] = 1
    adj[:, 1, 1] = 0
    rep.add_many(x, e, adj, a, r, x2, e2)
    rep.flush()
    mixed = [np.concatenate((dr[:-1], [stored + k])) for k, dr in enumerate(draws)]

    def with_own():
        it[0] += 1
        rep.sample(mixed[it[0] % 8])
    out["receivers_with_own_receiver_graph"] = _event_timed(with_own, args.sample_reps, 20, torch)
    out["receivers_regular_again"] = _event_timed(regular, args.sample_reps, 20, torch)

    def host():
        batch = mem.sample(B)
        s = np.stack([b[0][0] for b in batch])
        s_ = np.stack([b[3][0] for b in batch])
        act = np.stack([b[1][0] for b in batch]).astype(int)
        rew = np.array([b[2] for b in batch], dtype=np.float64)
        st, adj_ = s[:, :n * 13].reshape(B, n, 13), s[:, n * 13:].reshape(B, n, n)
        st_ = s_[:, :n * 13].reshape(B, n, 13)
        sb = DeviceBatch(PackedBatch.from_dense(st[:, :, :9], st[:, :, 9:], adj_), "cuda:0")
        sn = DeviceBatch(PackedBatch.from_dense(st_[:, :, :9], st_[:, :, 9:], adj_), "cuda:0")
        ta, tr = torch.from_numpy(act.astype(np.int32)).cuda(), torch.from_numpy(rew).cuda()
        torch.cuda.synchronize()
        return sb, sn, ta, tr
    host()
    walls = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["host_assembly_wall"] = _stats(walls)
    out["host_wall_over_receivers_wall"] = out["host_assembly_wall"]["median_ms"] / out["receivers_regular"]["wall_ms_per_call"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_receivers_timing.json"))
    ap.add_argument("--links", default="32,64,100")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4, help="train steps per timed Agent.train call")
    ap.add_argument("--reps", type=int, default=5, help="timed Agent.train calls per form")
    ap.add_argument("--replay-reps", type=int, default=10)
    ap.add_argument("--sample-batch", type=int, default=4096)
    ap.add_argument("--sample-reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1001)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-sample", action="store_true")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("replay_receivers_timing: needs a GPU (a timing taken without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "feat_dim": args.feedback, "seed": args.seed,
           "train_steps_per_call": args.steps, "calls_per_form": args.reps,
           "how": "one process, the forms taken in turn; train_step: wall ms per train step of Agent.train(1, steps) ending in a "
                  "synchronise, the same seed before every call; replay_step: wall ms of Agent.replay(); sample: HIP events "
                  "around ReceiverReplay.sample and wall ms per call of the timed loop, wall ms of the host form's assembly",
           "links": {}}
    for n in [int(v) for v in args.links.split(",")]:
        entry = {}
        if not args.skip_train:
            entry.update(train_steps(n, args, torch))
            print(n, "train", json.dumps(entry), flush=True)
        if not args.skip_sample:
            entry["sample"] = sample_timing(n, args, torch)
            print(n, "sample", json.dumps(entry["sample"]), flush=True)
        res["links"][str(n)] = entry
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
