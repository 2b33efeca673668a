"""The receiver-form checkpoint sweep in numbers: one trial of the evaluation of the training process -- K = 8 checkpoints, one
50-step episode, one simulator -- at 32, 64, 100 and 128 links.  One process; per size one agent per leg built from the same
seed on DeviceBatchedEnviron(streams='device'), the K networks (F = 16, seeded: the time does not depend on the weights) shared
by all legs; the legs taken in turn, the same seed before every call.

  (a) sweep    Agent.evaluate_training_sweep(eval_backend='device'), one trial: the reset, the draws, ONE v2x_eval_sweep_recv
               call (receiver_streams chain | split) and one stacked local search (the first checkpoint's ground truth).
  (b) parent   Agent.evaluate_training_diff_trials(eval_backend='device', load=False), one trial: per checkpoint a reset, the
               draws and one _device_episode (K v2x_eval_steps_recv calls, K walks), one stacked local search.
  (c) host     Agent.evaluate_training_sweep(eval_backend='host'), one trial: the definition.
      Wall ms ending in a synchronise: median and p10-p90 over --reps calls after one untimed call per leg.
  (a') / (b') the same two with opt_flag=True, opt_backend='local' (chain): the parent searches K stacked problems, the sweep one.
  (d) call     DeviceChannels.eval_sweep_recv (K networks, every step greedy, with the baseline scheme) between HIP events,
               beside DeviceChannels.eval_steps_recv with one network, chain and split taken in turn: median and p10-p90.

    python tools/eval_sweep_recv_timing.py [--out profiles/eval_sweep_recv_timing.json] [--links 32,64,100,128]
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

T = 50
TRIAL_LEGS = (("sweep_chain", "chain"), ("sweep_split", "split"), ("parent_chain", "chain"), ("parent_split", "split"),
              ("host", "chain"))


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


def _engines(n, args):
    from v2xgnn import GnnEngine, GnnSpec
    out = []
    for k in range(args.networks):
        eng = GnnEngine(GnnSpec(n_nodes=n, feat_dim=args.feedback, n_mp_layers=2))
        eng.set_flat(np.random.default_rng(args.seed + k).normal(0, 0.3, size=eng.n_params).astype(np.float32))
        out.append(eng)
    return out


def _trial(agent, name, engines, args, opt_flag):
    K = len(engines)
    kw = dict(opt_backend='local', opt_restarts=args.opt_restarts)
    if name.startswith("sweep"):
        return agent.evaluate_training_sweep(5 * K, T, opt_flag, args.epsilon, 1, engines=engines, eval_backend='device', **kw)
    if name.startswith("parent"):
        return agent.evaluate_training_diff_trials(5 * K, T, opt_flag, args.epsilon, 1, load=False, eval_backend='device', **kw)
    return agent.evaluate_training_sweep(5 * K, T, opt_flag, args.epsilon, 1, engines=engines, eval_backend='host', **kw)


def _timed(agents, names, engines, args, torch, opt_flag, reps):
    ms, outs = {name: [] for name in names}, {}
    for rep in range(-1, reps):                            # rep -1: warm-up (buffers, workspaces, first allocation), untimed
        for name in names:
            random.seed(args.seed + rep)
            np.random.seed(args.seed + rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = _trial(agents[name], name, engines, args, opt_flag)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert all(np.all(np.isfinite(a)) for a in out)
            if rep >= 0:
                ms[name].append(dt)
            outs.setdefault(rep, {})[name] = [np.asarray(a).tobytes() for a in out]
    return {name: _pct(v) for name, v in ms.items()}, outs


def trials(n, args, torch):
    agents = {name: _agent(n, args, streams) for name, streams in TRIAL_LEGS}
    engines = _engines(n, args)
    names = [name for name, _ in TRIAL_LEGS]
    e, outs = _timed(agents, names, engines, args, torch, False, args.reps)
    res = {"trial": e}
    for phase in ("chain", "split"):
        s, p = e["sweep_" + phase], e["parent_" + phase]
        e["parent_over_sweep_" + phase] = p["median_ms"] / s["median_ms"]
        e["sweep_%s_faster_than_parent_spread" % phase] = bool(s["p90_ms"] < p["p10_ms"])
    e["host_over_sweep_chain"] = e["host"]["median_ms"] / e["sweep_chain"]["median_ms"]
    # the sweep legs and the host definition walked the same trials: every returned array agrees
    res["sweep_chain_same_as_host"] = all(r["sweep_chain"] == r["host"] for r in outs.values())
    res["sweep_split_same_as_chain"] = all(r["sweep_split"] == r["sweep_chain"] for r in outs.values())
    o, _ = _timed(agents, ["sweep_chain", "parent_chain"], engines, args, torch, True, args.reps)
    o["parent_over_sweep_chain"] = o["parent_chain"]["median_ms"] / o["sweep_chain"]["median_ms"]
    o["sweep_chain_faster_than_parent_spread"] = bool(o["sweep_chain"]["p90_ms"] < o["parent_chain"]["p10_ms"])
    res["trial_with_optimum"] = o
    res["episodes_by_path"] = {name: dict(a.eval_stats) for name, a in agents.items()}
    res["walks"] = {name: dict(a.env.device_channels.walk_calls) for name, a in agents.items()}
    return res, agents, engines


def calls(n, agents, engines, args, torch):
    rng = np.random.default_rng(args.seed + n)
    K = len(engines)
    explore = np.zeros((T, 1), np.uint8)
    rand = np.zeros((T, 1, n), np.int32)
    baseline = rng.integers(0, 4, size=(T, 1, n)).astype(np.int32)
    run = {}
    for phase in ("chain", "split"):
        env = agents["sweep_" + phase].env
        dc, own = env.device_channels, env.own_receivers()
        if not dc._recv_ready:
            dc.observe_recv(env.dest)
        run["sweep_" + phase] = lambda dc=dc, own=own, phase=phase: dc.eval_sweep_recv(
            explore, rand, baseline, 1.0, 0.1, engines=engines, own=own, stream_phase=phase)
        run["single_" + phase] = lambda dc=dc, own=own, phase=phase: dc.eval_steps_recv(
            explore, rand, baseline, 1.0, 0.1, engine=engines[0], own=own, stream_phase=phase)
    for call in run.values():
        for _ in range(args.warmup):
            call().resolve()
    torch.cuda.synchronize()
    evs, results = {p: [] for p in run}, []
    for _ in range(args.reps):
        for name, call in run.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            results.append(call())
            b.record()
            evs[name].append((a, b))
    torch.cuda.synchronize()
    for r in results:
        r.resolve()                                        # (the page-locked result copies go back to their pools)
    out = {"T": T, "E": 1, "K": K}
    for name in run:
        st = _pct([a.elapsed_time(b) for a, b in evs[name]])
        out[name] = {"event_median_ms": st["median_ms"], "event_p10_ms": st["p10_ms"], "event_p90_ms": st["p90_ms"], "n": st["n"]}
    for phase in ("chain", "split"):
        s, o = out["sweep_" + phase]["event_median_ms"], out["single_" + phase]["event_median_ms"]
        out["k_singles_over_sweep_" + phase] = K * o / s
        out["sweep_minus_single_per_further_network_ms_" + phase] = (s - o) / max(1, K - 1)
    dc = agents["sweep_split"].env.device_channels
    io, sw, q = dc._recv_sweep_io(T, K + 1, K)
    out["result_block_bytes"] = int(sw['dev'].numel())
    out["q_bytes"] = int(q.numel() * 4)
    out["workspace_bytes"] = int(io['workspace'].numel())
    for name, agent in agents.items():
        if name != "host":
            agent.env._resident_after(None)                # (the calls stepped the resident state behind the simulator's back)
        agent.brain.close()
    for eng in engines:
        eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_sweep_recv_timing.json"))
    ap.add_argument("--links", default="32,64,100,128")
    ap.add_argument("--networks", type=int, default=8)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--opt-restarts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1001)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("eval_sweep_recv_timing: needs a GPU (a timing taken without one says nothing)")
    res = {"device": torch.cuda.get_device_name(0), "feat_dim": args.feedback, "seed": args.seed, "steps_per_episode": T,
           "networks": args.networks, "epsilon": args.epsilon, "opt_restarts": args.opt_restarts, "calls_per_leg": args.reps,
           "how": "one process, one agent per leg and size from the same seed on one resident simulator, K seeded networks shared by "
                  "all legs, the legs taken in turn; trial: wall ms of ONE trial of Agent.evaluate_training_sweep(eval_backend='device') "
                  "(sweep_*), of Agent.evaluate_training_diff_trials(eval_backend='device', load=False) (parent_*: K device episodes) "
                  "and of Agent.evaluate_training_sweep(eval_backend='host') (host), each ending in a synchronise, the same seed "
                  "before every call, opt_backend='local' (one stacked search per trial without opt_flag), median and p10-p90 after "
                  "one untimed call per leg; trial_with_optimum: the same with opt_flag=True; call: HIP events around "
                  "DeviceChannels.eval_sweep_recv (K networks) and DeviceChannels.eval_steps_recv (one network), T = 50, every step "
                  "greedy, with the baseline scheme, taken in turn; x_faster_than_parent_spread: x's p90 below the parent leg's p10",
           "links": {}}
    for n in [int(v) for v in args.links.split(",")]:
        entry, agents, engines = trials(n, args, torch)
        print(n, "trial", json.dumps(entry), flush=True)
        entry["call"] = calls(n, agents, engines, args, torch)
        print(n, "call", json.dumps(entry["call"]), flush=True)
        res["links"][str(n)] = entry
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                     # (written after every size: a later size that fails loses nothing)
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
