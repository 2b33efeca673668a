"""The checkpoint sweep (v2x_eval_sweep_mixed, MixedAgent.evaluate_training) in numbers: K = 8 networks of 64 features and 2
message-passing layers on ONE episode of 50 steps at 8 / 12 / 20 / 28 links, one simulator each, everybody greedy.  Wall time of
forms that are alive in one process, warmed up and taken in turn; medians with their min-max:

  (a) sweep_call        the reset, the draws and ONE resident_evaluate_sweep_mixed call (one walk, one assembly, K forwards, one
                        finish launch), results resolved;
      single_calls      the same reset and draws and K resident_evaluate_steps_mixed calls on the SAME environments, one per
                        network (K walks, K assemblies, K forwards, K finish launches), results resolved;
  (b) trial_device / trial_host   one trial of MixedAgent.evaluate_training on either backend, without the optimum;
  (c) the same at 20 links alone with the optimum of every state by branch and bound (opt_backend='bound'): one trial on either
      backend.  Few repetitions and no warm-up: a search's time depends on its states, from seconds for the 50 of an episode
      to minutes for a hard one (rl/optimum.py DEFAULT_MAX_NODES), so every form says when it is through.

No ratio is promised; the file says who won and whether by more than the run-to-run spread.

    python tools/mixed_sweep_timing.py [--out profiles/mixed_sweep_timing.json] [--reps 10] [--warmup 2] [--opt-reps 2]
                                        [--legs calls,trial,optimum]
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

SIZES, OPT_SIZES, E, T, FEAT, K = (8, 12, 20, 28), (20,), 1, 50, 64, 8


def _envs(sizes):
    from v2xgnn.rl.train import start_env_batched
    return [start_env_batched(n, E, 1001 + 15485863 * k, backend="device", streams="device") for k, n in enumerate(sizes)]


def in_turn(forms, reps, warmup, torch):
    """-> {name: {"wall_ms": median, "min_max": [min, max]}} of the forms taken in turn, reps times after warmup rounds"""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"wall_ms": float(np.median(v)), "min_max": [min(v), max(v)]} for name, v in ms.items()}


def verdict(res, fast, slow):
    """who won, and whether by more than the larger of the two min-max spreads"""
    a, b = res[fast], res[slow]
    spread = max(a["min_max"][1] - a["min_max"][0], b["min_max"][1] - b["min_max"][0])
    diff = b["wall_ms"] - a["wall_ms"]
    return {"%s_over_%s" % (slow, fast): round(b["wall_ms"] / a["wall_ms"], 3),
            "winner": fast if diff > spread else slow if -diff > spread else "level (within the run-to-run spread)"}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_sweep_timing.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--opt-reps", type=int, default=2)
    ap.add_argument("--legs", default="calls,trial,optimum", help="which of the legs (a) calls, (b) trial, (c) optimum to measure; "
                                                                  "the others keep what --out already holds")
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from v2xgnn import GnnEngine
    from v2xgnn.bs_brain import _glorot_list
    from v2xgnn.rl.device_sim import resident_evaluate_steps_mixed, resident_evaluate_sweep_mixed
    from v2xgnn.rl.mixed import MixedAgent, draw_eval_episode_ahead
    from v2xgnn.rl.sim_config import RL_Config
    cfg = RL_Config()
    cfg.set_train_value(FEAT, 0.5, 4096, 1, 0.1)
    np.random.seed(1001)
    envs = _envs(SIZES)
    agent = MixedAgent(envs, cfg, FEAT, seed=1001)
    nets = []
    for k in range(K):
        nets.append(GnnEngine(agent.spec))
        nets[-1].set_weights(_glorot_list(agent.spec, np.random.default_rng(100 + k)))
    legs = set(args.legs.split(","))
    assert legs and legs <= {"calls", "trial", "optimum"}, args.legs
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update({"sizes": list(SIZES), "simulators_per_size": E, "steps": T, "networks": K, "feat_dim": FEAT, "n_mp_layers": 2,
           "fixed_epsilon": 0.0, "reps": args.reps, "warmup": args.warmup,
           "baseline": "K v2x_eval_steps_mixed calls of the same build on the same environments, alive in the same process and "
                       "taken in turn with the sweep (their kernels and host path are the parent commit's, unchanged)"})

    def save():                                            # (after every leg: a later leg may take minutes)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    def reset_and_draw():
        for env in envs:
            env.new_random_game(env.n_Veh)
        return draw_eval_episode_ahead(envs, 4, 0.0, T)

    def sweep_call():
        baseline, explore, rand = reset_and_draw()
        for r in resident_evaluate_sweep_mixed(envs, explore, rand, baseline, 1.0, 0.1, engines=nets):
            r.resolve()

    def single_calls():
        baseline, explore, rand = reset_and_draw()
        rows = [resident_evaluate_steps_mixed(envs, explore, rand, baseline, 1.0, 0.1, engine=net) for net in nets]
        for per_net in rows:
            for r in per_net:
                r.resolve()

    # (a) the calls
    if "calls" in legs:
        res["calls"] = in_turn({"sweep_call": sweep_call, "single_calls": single_calls}, args.reps, args.warmup, torch)
        res["calls"].update(verdict(res["calls"], "sweep_call", "single_calls"))
        print("calls", json.dumps(res["calls"]), flush=True)
        save()

    # (b) a trial through the agent, without the optimum
    if "trial" in legs:
        trial = lambda backend: agent.evaluate_training(envs, None, T, 1, 0.0, eval_backend=backend, engines=nets)     # noqa: E731
        res["trial"] = in_turn({"trial_device": lambda: trial('device'), "trial_host": lambda: trial('host')},
                               max(2, args.reps // 2), 1, torch)
        res["trial"].update(verdict(res["trial"], "trial_device", "trial_host"))
        res["trial"]["episodes_by_path"] = dict(agent.eval_stats)
        print("trial", json.dumps(res["trial"]), flush=True)
        save()
    agent.close()

    # (c) with the optimum by branch and bound at 20 links
    if "optimum" in legs:
        opt_envs = _envs(OPT_SIZES)
        opt_agent = MixedAgent(opt_envs, cfg, FEAT, seed=1001)
        kw = dict(opt_flag=True, opt_backend='bound')

        def said(name, fn):                                # (a form takes from seconds to a minute: say when one is through)
            def run():
                t0 = time.perf_counter()
                fn()
                print("  %s %.1f s" % (name, time.perf_counter() - t0), flush=True)
            return run

        forms = {"trial_device": lambda: opt_agent.evaluate_training(opt_envs, None, T, 1, 0.0, eval_backend='device', engines=nets, **kw),
                 "trial_host": lambda: opt_agent.evaluate_training(opt_envs, None, T, 1, 0.0, eval_backend='host', engines=nets, **kw)}
        res["trial_with_optimum"] = in_turn({name: said(name, fn) for name, fn in forms.items()}, args.opt_reps, 0, torch)
        res["trial_with_optimum"].update({"sizes": list(OPT_SIZES), "opt_backend": "bound", "reps": args.opt_reps, "warmup": 0})
        res["trial_with_optimum"].update(verdict(res["trial_with_optimum"], "trial_device", "trial_host"))
        print("trial with optimum", json.dumps(res["trial_with_optimum"]), flush=True)
        opt_agent.close()

    save()
    for net in nets:
        net.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
