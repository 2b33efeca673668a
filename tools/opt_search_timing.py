"""Per-state cost of the optimal-allocation search (v2xgnn.rl.OptimalAllocation, csrc/v2xopt.hip) next to the host brute
force of Agent._brute_force: wall time of search() (upload + kernels + download) and the kernels' time between HIP events,
for (N, C) = (4, 4), (8, 4), (12, 4), (16, 4) at one state, 50 states at (8, 4), and the host path at (4, 4) (every joint
action) and at (8, 4) (extrapolated from the first 4096 joint actions).

    python tools/opt_search_timing.py [--out profiles/opt_search_timing.json] [--reps 20]
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("opt_search_timing.py measures the GPU search: no GPU here")
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
