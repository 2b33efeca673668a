"""The mixed-size evaluation episode (v2x_eval_steps_mixed, MixedAgent.test_run(eval_backend='device')) in numbers: ONE episode of
50 steps at 8 / 12 / 20 / 28 links, one simulator each, everybody greedy, without the optimum; 64 features, 2 message-passing
layers.  Wall time per episode -- the reset of every environment, the draws, the steps, the downloads -- of forms that are alive
in one process, warmed up and taken in turn:

  (a) mixed_call        the draws taken ahead and ONE resident_evaluate_steps_mixed call (walk, assembly, ragged forward, finish:
                        four launches for all link counts), results resolved;
      test_run_device   the same through MixedAgent.test_run(eval_backend='device'), which also fills the books;
  (b) per_size_calls    the same draws and four single-size evaluate_steps calls on the SAME environments (v2x_eval_steps: a walk,
                        a forward and a finish launch per link count), each scored by a fixed-size shared-weight engine of its
                        own link count, results resolved;
  (c) test_run_host     MixedAgent.test_run's host loop (the default) on the same device simulators: per step the baseline's
                        rates, one score() of all observations, one act() per environment;
      test_run_host_on_host_simulators   the host loop on host simulators.

Medians of --reps episodes after --warmup, with their min-max; no ratio is promised, the file says who won.

--walk-leg measures something else and nothing of the above: the serial mixed call against the mixed wide walk
(v2x_eval_steps_mixed_wide) on the same pools, both alive in one process and taken in turn -- the call between HIP events and
its host enqueue (draws and reset outside), the wall time of an episode through mixed_call and through test_run_device with
either walk, and the kernels' own durations through torch's profiler; the call also at T = 1.  Written under "eval" into
profiles/mixed_wide_timing.json (tools/mixed_rollout_timing.py --walk-leg writes "rollout" beside it).

    python tools/mixed_eval_timing.py [--out profiles/mixed_eval_timing.json] [--reps 20] [--warmup 3]
    python tools/mixed_eval_timing.py --walk-leg [--walk-out profiles/mixed_wide_timing.json]
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

SIZES, E, T, FEAT = (8, 12, 20, 28), 1, 50, 64


def _envs(backend, streams):
    from v2xgnn.rl.train import start_env_batched
    return [start_env_batched(n, E, 1001 + 15485863 * k, backend=backend, streams=streams) for k, n in enumerate(SIZES)]


def walk_leg(args, torch):
    from mixed_rollout_timing import SERIAL_KERNELS, WIDE_KERNELS, merge_walk_leg, walks_in_turn
    from sim_device_timing import kernel_times
    from v2xgnn.rl.device_sim import resident_evaluate_steps_mixed
    from v2xgnn.rl.mixed import MixedAgent, draw_eval_episode_ahead
    from v2xgnn.rl.sim_config import RL_Config
    cfg = RL_Config()
    cfg.set_train_value(FEAT, 0.5, 4096, 1, 0.1)
    np.random.seed(1001)
    envs = _envs("device", "device")
    agent = MixedAgent(envs, cfg, FEAT, seed=1001)
    shared = ("k_traj_assemble_mixed", "k_eval_finish_mixed")
    res = {"sizes": list(SIZES), "simulators_per_size": E, "feat_dim": FEAT, "n_mp_layers": 2, "fixed_epsilon": 0.0, "optimum": False,
           "reps": args.reps, "warmup": args.warmup, "call": [],
           "baseline": "the serial mixed call of the same build, alive in the same process and taken in turn with the wide one "
                       "(its kernels and its host path are the parent commit's, unchanged)"}

    def reset_and_draw(steps):
        for env in envs:
            env.new_random_game(env.n_Veh)
        return draw_eval_episode_ahead(envs, 4, 0.0, steps)

    # (1) the call alone, on one set of draws: between HIP events, the host enqueue, the kernels
    for steps in (T, 1):
        baseline, explore, rand = reset_and_draw(steps)
        calls = {w: (lambda w=w: resident_evaluate_steps_mixed(envs, explore, rand, baseline, 1.0, 0.1, engine=agent.online, walk=w))
                 for w in ("serial", "wide")}
        out = walks_in_turn(calls, args.reps, args.warmup, torch)
        out["kernels_ms"] = {"serial": kernel_times(calls["serial"], SERIAL_KERNELS + shared, 10),
                             "wide": kernel_times(calls["wide"], WIDE_KERNELS + shared, 10)}
        out["steps"] = steps
        res["call"].append(out)
        print("walk call", json.dumps(out), flush=True)

    # (2) an episode: reset, draws, the call, the downloads -- and through test_run, which also fills the books
    def mixed_call(walk):
        baseline, explore, rand = reset_and_draw(T)
        for r in resident_evaluate_steps_mixed(envs, explore, rand, baseline, 1.0, 0.1, engine=agent.online, walk=walk):
            r.resolve()

    def test_run(walk):
        agent.trajectory_walk = walk
        agent.test_run(envs, 1, T, eval_backend='device')

    forms = {"mixed_call_serial": lambda: mixed_call("serial"), "mixed_call_wide": lambda: mixed_call("wide"),
             "test_run_device_serial": lambda: test_run("serial"), "test_run_device_wide": lambda: test_run("wide")}
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    res["steps"] = T
    for name, v in ms.items():
        res[name] = {"wall_ms_per_episode": float(np.median(v)), "min_max": [min(v), max(v)]}
    for form in ("mixed_call", "test_run_device"):
        s, w = res[form + "_serial"], res[form + "_wide"]
        spread = max(s["min_max"][1] - s["min_max"][0], w["min_max"][1] - w["min_max"][0])
        diff = s["wall_ms_per_episode"] - w["wall_ms_per_episode"]
        res[form + "_winner"] = "wide" if diff > spread else "serial" if -diff > spread else "level"
        res[form + "_serial_over_wide"] = round(s["wall_ms_per_episode"] / w["wall_ms_per_episode"], 3)
    res["walk_calls"] = [dict(e.device_channels.walk_calls) for e in envs]
    print("walk episode", json.dumps({k: v for k, v in res.items() if k != "call"}), flush=True)
    merge_walk_leg(args.walk_out, "eval", res)
    agent.close()
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk-leg", action="store_true", help="measure the serial against the wide mixed walk, and nothing else")
    ap.add_argument("--walk-out", default=os.path.join(ROOT, "profiles", "mixed_wide_timing.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_eval_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if args.walk_leg:
        return walk_leg(args, torch)
    from v2xgnn import GnnEngine, GnnSpec
    from v2xgnn.bs_brain import _glorot_list
    from v2xgnn.rl.device_sim import resident_evaluate_steps_mixed
    from v2xgnn.rl.mixed import MixedAgent, draw_eval_episode_ahead
    from v2xgnn.rl.sim_config import RL_Config
    cfg = RL_Config()
    cfg.set_train_value(FEAT, 0.5, 4096, 1, 0.1)
    np.random.seed(1001)
    dev_envs, host_envs = _envs("device", "device"), _envs("host", "host")
    agent = MixedAgent(dev_envs, cfg, FEAT, seed=1001)
    host_agent = MixedAgent(host_envs, cfg, FEAT, seed=1001)
    singles = []
    for n in SIZES:
        spec = GnnSpec(n_nodes=n, feat_dim=FEAT, n_mp_layers=2, share_weights=True)
        singles.append(GnnEngine(spec))
        singles[-1].set_weights(_glorot_list(spec, np.random.default_rng(1)))

    def reset_and_draw():
        for env in dev_envs:
            env.new_random_game(env.n_Veh)
        return draw_eval_episode_ahead(dev_envs, 4, 0.0, T)

    def mixed_call():
        baseline, explore, rand = reset_and_draw()
        for r in resident_evaluate_steps_mixed(dev_envs, explore, rand, baseline, 1.0, 0.1, engine=agent.online):
            r.resolve()

    def per_size_calls():
        baseline, explore, rand = reset_and_draw()
        rows = [env.evaluate_steps(explore[k], rand[k], baseline[k], 1.0, 0.1, engine=singles[k]) for k, env in enumerate(dev_envs)]
        for r in rows:
            r.resolve()

    forms = {"mixed_call": mixed_call, "per_size_calls": per_size_calls,
             "test_run_device": lambda: agent.test_run(dev_envs, 1, T, eval_backend='device'),
             "test_run_host": lambda: agent.test_run(dev_envs, 1, T, eval_backend='host'),
             "test_run_host_on_host_simulators": lambda: host_agent.test_run(host_envs, 1, T, eval_backend='host')}
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    agent.eval_stats = {'device_episodes': 0, 'host_episodes': 0}
    ms = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    res = {"sizes": list(SIZES), "simulators_per_size": E, "steps": T, "feat_dim": FEAT, "n_mp_layers": 2, "fixed_epsilon": 0.0,
           "optimum": False, "reps": args.reps, "warmup": args.warmup, "test_run_episodes_by_path": dict(agent.eval_stats)}
    for name, v in ms.items():
        res[name] = {"wall_ms_per_episode": float(np.median(v)), "min_max": [min(v), max(v)]}
    order = sorted(forms, key=lambda k: res[k]["wall_ms_per_episode"])
    res["fastest_to_slowest"] = order
    a, b, c = res["mixed_call"], res["per_size_calls"], res["test_run_host"]
    spread = lambda x, y: max(x["min_max"][1] - x["min_max"][0], y["min_max"][1] - y["min_max"][0])      # noqa: E731
    res["mixed_call_wins_over_per_size_calls_by_more_than_spread"] = bool(
        b["wall_ms_per_episode"] - a["wall_ms_per_episode"] > spread(a, b))
    d = res["test_run_device"]
    res["test_run_device_wins_over_host_loop_by_more_than_spread"] = bool(
        c["wall_ms_per_episode"] - d["wall_ms_per_episode"] > spread(c, d))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    agent.close()
    host_agent.close()
    for eng in singles:
        eng.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
