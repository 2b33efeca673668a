"""Cost of a simulator step on the device (v2xgnn.rl.DeviceChannels / DeviceBatchedEnviron, csrc/v2xsimdev.hip) next to the host
library (libv2xsim.so at its default thread count) on the same box, 20 links x 4 resource blocks, E = 1, 50 and 200 simulators:

  device leg  per simulator step of all E states, the wall time of rates + step + observe on DeviceChannels with the uniforms'
              upload and the small downloads (rates, xe / mask / col / regular) included, and the three kernels' time between
              HIP events with every input already on the device;
  host leg    native_sim.advance (mobility + uniforms + channels + interference + observation) from the same state, and
              env.act() of both environments (rates + the whole step, mobility and MT19937 on the host either way);
  loop leg    python -m v2xgnn.rl.train --links 20 --feedback 64 --batch 4096 --train-steps 20 --use-graph --envs 50 with both
              backends, the two taken in turn: ms per train step of the whole run (start-up included), and of the steady
              state as the difference between a 3-episode and a 1-episode run over their 40 extra train steps (the driver's
              clock starts after the environment exists, so the device runs have initialised the GPU before it and the host
              runs after it: only the difference compares like with like); and the same loop with both environments in ONE
              process, warmed up, Agent.train(1, 20) timed in turn.

Medians over --reps timed steps after --warmup untimed ones; the box's usable CPUs are recorded.

    python tools/sim_device_timing.py [--out profiles/sim_device_timing.json] [--reps 200] [--loop-reps 3] [--no-loop]

--mode streams measures the device environment with mobility and the MT19937 streams on the device too (streams='device':
one v2x_sim_advance per step) against the same environment with host streams and against the host simulator, all three alive
in one process: env.act() + observe_packed() wall time, the bytes each device environment moves per step (DeviceChannels.traffic),
the four launches of v2x_sim_advance between HIP events, and the DQN loop of the in-process leg above for the three of them.

    python tools/sim_device_timing.py --mode streams [--out profiles/sim_device_streams_timing.json]

--mode rollout measures the device-resident rollout iteration (Agent(rollout_backend='device'): v2x_rollout_step) with the recipe
of --mode streams: the iteration alone at 1, 50 and 200 simulators (Agent.generate_d2d_transition(E) wall time, epsilon held near
0.5, and the bytes DeviceChannels.traffic counts per iteration) next to the host rollout on the same kind of environment, and the
DQN loop at 50 simulators -- the device rollout, the host rollout on device streams and the host simulator with look-ahead, all
alive in one process, Agent.train(1, 20) timed in turn; and the call alone between HIP events, issued eagerly and replayed from
a graph the tool captures itself (the agent issues it eagerly: head moves with every block).

    python tools/sim_device_timing.py --mode rollout [--out profiles/rollout_device_timing.json]

--mode trajectory measures the whole-rollout call (Agent(rollout_backend='trajectory'): v2x_rollout_steps) with the same recipe at
E = 1, 5, 10, 25 and 50 simulators: a 50-transition rollout (Agent.generate_d2d_transition(50), epsilon held near 0.4) for
'trajectory' in its three forms (the serial walk, the wide walk, the wide walk with the split stream phase), for 'device' (one
v2x_rollout_step per iteration) and, at E = 1, for the host simulator's single-call native rollout; the bytes each moves per
rollout; the one call alone between HIP events and its host enqueue time, the three forms on one agent's state taken in turn,
and their kernels one by one (WALK_KERNELS); and the DQN loop Agent.train(1, 20) per train step for the same backends, all
agents of one E alive in one process and taken in turn.

    python tools/sim_device_timing.py --mode trajectory [--out profiles/rollout_trajectory_timing.json]
    python tools/sim_device_timing.py --mode trajectory --out profiles/trajectory_split_timing.json     (the run with the split form)

--mode evaluate measures an evaluation run, Agent.test_run(--episodes episodes, 50 steps), with eval_backend 'host' and 'device'
(the serial walk, the wide walk, the wide walk with the split stream phase) on the same kind of device-streams environment
(E = 1) and with the host loop on the host BatchedEnviron (E = 1), the agents alive in one process and taken in turn, medians after warm-up: without the optimum at 20 links, with --opt-backend bound at 20
links and with --opt-backend device at 12 links (--loop-reps timed runs each for the two with an optimum); and the bytes each
device environment moves per episode (DeviceChannels.traffic).

    python tools/sim_device_timing.py --mode evaluate [--out profiles/eval_device_timing.json] [--episodes 1]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINKS, RB = 20, 4


def _median_ms(xs):
    return round(float(np.median(xs)) * 1e3, 4)


def step_legs(E, reps, warmup):
    import torch
    from v2xgnn.rl import native_sim
    from v2xgnn.rl.train import start_env_batched
    host = start_env_batched(LINKS, E, 7, lookahead=False)
    dev = start_env_batched(LINKS, E, 7, backend="device")
    dc = dev.device_channels
    rng = np.random.default_rng(3)
    pool = [rng.random((E, dc.n_u)) for _ in range(8)]
    actions = [rng.integers(0, RB, size=(E, LINKS, 1)) for _ in range(8)]
    a32 = [a.reshape(E, LINKS).astype(np.int32) for a in actions]

    def device_step(k):
        dc.rates(a32[k % 8], dest=dev.dest)
        dc.fetch_rates()
        dc.step(pool[k % 8], dev.vel, dev.pos)
        dc.observe(dev.dest)
        dc.fetch_observation()

    for k in range(warmup):
        device_step(k)
    torch.cuda.synchronize()
    wall = []
    for k in range(reps):
        t0 = time.perf_counter()
        device_step(k)                                            # ends in the observation's download: synchronised
        wall.append(time.perf_counter() - t0)

    # the three kernels alone: inputs on the device, HIP events around the launches
    u_t = torch.from_numpy(pool[0]).to(dc.device)
    vel_t, pos_t = dc.tensor('vel'), dc.tensor('pos')
    a_t = torch.from_numpy(a32[0]).to(dc.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for k in range(warmup + reps):
        ev[0].record()
        dc.step(u_t, vel_t, pos_t)
        dc.observe()
        dc.rates(a_t)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= warmup:
            kern.append(ev[0].elapsed_time(ev[1]) * 1e-3)

    # host: the one-call step of the library from the current state (results dropped: the state does not move)
    for k in range(warmup):
        host._start_job(False)
    adv = []
    for k in range(reps):
        t0 = time.perf_counter()
        host._start_job(False)
        adv.append(time.perf_counter() - t0)

    def act_times(env):
        for k in range(warmup):
            env.act(actions[k % 8])
            env.observe_packed(RB)
        out = []
        for k in range(reps):
            t0 = time.perf_counter()
            env.act(actions[k % 8])
            env.observe_packed(RB)
            out.append(time.perf_counter() - t0)
        return out

    act_host, act_dev = act_times(host), act_times(dev)
    return {"simulators": E, "links": LINKS, "rb": RB, "uniforms_uploaded_bytes": int(pool[0].nbytes),
            "device_step_wall_ms": _median_ms(wall), "device_step_wall_us_per_simulator": round(_median_ms(wall) * 1e3 / E, 2),
            "device_kernels_ms": _median_ms(kern), "host_advance_ms": _median_ms(adv),
            "host_advance_us_per_simulator": round(_median_ms(adv) * 1e3 / E, 2), "host_threads": native_sim._load().v2xsim_max_threads(),
            "act_host_env_ms": _median_ms(act_host), "act_device_env_ms": _median_ms(act_dev)}


def loop_leg(loop_reps):
    base = [sys.executable, "-m", "v2xgnn.rl.train", "--links", "20", "--feedback", "64", "--batch", "4096", "--train-steps", "20",
            "--use-graph", "--envs", "50"]
    runs = {b: {1: [], 3: []} for b in ("host", "device")}
    for rep in range(loop_reps):
        for episodes in (1, 3):
            for backend in ("host", "device"):                      # taken in turn: the box's load drifts
                cmd = base + ["--episodes", str(episodes), "--sim-backend", backend]
                done = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
                if done.returncode != 0:
                    raise RuntimeError("%s failed (%d):\n%s" % (" ".join(cmd), done.returncode, done.stdout[-2000:]))
                line = [x for x in done.stdout.splitlines() if x.startswith("{")][-1]
                runs[backend][episodes].append(float(json.loads(line)["wall_s"]))
    out = {"command": " ".join(base[1:]) + " --sim-backend {host,device}", "runs_per_setting": loop_reps}
    for b in ("host", "device"):
        w1, w3 = float(np.median(runs[b][1])), float(np.median(runs[b][3]))
        out[b] = {"wall_s_1_episode": runs[b][1], "wall_s_3_episodes": runs[b][3],
                  "ms_per_train_step_whole_run": round(w1 * 1e3 / 20, 3),
                  "ms_per_train_step_steady": round((w3 - w1) * 1e3 / 40, 3)}
    return out


def loop_in_process(reps):
    """The same loop with both environments alive in ONE process, so that start-up (device context, library load, replay
    allocation, captures) is outside the timed region for both alike: one untimed Agent.train(1, 20) each, then `reps` timed
    ones each, the two backends taken in turn; ms per train step = wall of the call / 20 (one episode reset included)."""
    import random
    import torch
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    agents, walls = {}, {"host": [], "device": []}
    with torch.cuda.stream(torch.cuda.Stream(device=0)):
        for backend in ("host", "device"):
            random.seed(1001)
            np.random.seed(1001)
            cfg = RL_Config()
            cfg.set_train_value(64, 0.5, 4096, 1, 0.1)
            cfg.Num_Episodes, cfg.Num_Train_Steps = 1, 20
            env = start_env_batched(LINKS, 50, 1001, backend=backend)
            agents[backend] = Agent(env.n_Veh, env.n_RB, env.n_Neighbor, 64, env, cfg, device=0, seed=1001, use_graph=True)
            agents[backend].train(1, 20)                              # warm-up, untimed
        torch.cuda.synchronize()
        for rep in range(reps):
            for backend in ("host", "device"):
                t0 = time.perf_counter()
                agents[backend].train(1, 20)
                torch.cuda.synchronize()
                walls[backend].append(time.perf_counter() - t0)
    return {b: {"wall_s_per_call": [round(w, 4) for w in walls[b]], "ms_per_train_step": round(float(np.median(walls[b])) * 1e3 / 20, 3)}
            for b in walls}


SETTINGS = {"host": dict(backend="host"), "device_host_streams": dict(backend="device", streams="host"),
            "device_device_streams": dict(backend="device", streams="device")}


def streams_legs(E, reps, warmup):
    import torch
    from v2xgnn.rl.train import start_env_batched
    envs = {"host": start_env_batched(LINKS, E, 7, lookahead=False)}
    for name in ("device_host_streams", "device_device_streams"):
        envs[name] = start_env_batched(LINKS, E, 7, **SETTINGS[name])
    rng = np.random.default_rng(3)
    actions = [rng.integers(0, RB, size=(E, LINKS, 1)) for _ in range(8)]
    walls = {name: [] for name in envs}
    traffic = {}
    for k in range(warmup):
        for env in envs.values():
            env.act(actions[k % 8])
            env.observe_packed(RB)
    for name in ("device_host_streams", "device_device_streams"):
        traffic[name] = dict(envs[name].device_channels.traffic)
    for k in range(reps):
        for name, env in envs.items():                              # taken in turn: the box's load drifts
            t0 = time.perf_counter()
            env.act(actions[k % 8])
            env.observe_packed(RB)                                  # (what the agent reads next: ends synchronised)
            walls[name].append(time.perf_counter() - t0)
    row = {"simulators": E, "links": LINKS, "rb": RB}
    for name in envs:
        row["act_%s_ms" % name] = _median_ms(walls[name])
    for name, before in traffic.items():
        after = envs[name].device_channels.traffic
        for k in ("bytes_up", "bytes_down"):
            row["%s_%s_per_step" % (name, k)] = (after[k] - before[k]) // reps
    # the four launches of one v2x_sim_advance alone: actions on the device, HIP events around the call
    dc = envs["device_device_streams"].device_channels
    a_t = torch.from_numpy(actions[0].reshape(E, LINKS).astype(np.int32)).to(dc.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kern = []
    for k in range(warmup + reps):
        ev[0].record()
        dc.advance(a_t)
        ev[1].record()
        torch.cuda.synchronize()
        if k >= warmup:
            kern.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    row["advance_kernels_ms"] = _median_ms(kern)
    return row


def loop_in_process_streams(reps):
    """loop_in_process for the host simulator (with look-ahead), the device environment with host streams and the device
    environment with device streams: all three alive and warmed up in ONE process, Agent.train(1, 20) timed in turn"""
    import random
    import torch
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    agents, walls = {}, {name: [] for name in SETTINGS}
    with torch.cuda.stream(torch.cuda.Stream(device=0)):
        for name, kw in SETTINGS.items():
            random.seed(1001)
            np.random.seed(1001)
            cfg = RL_Config()
            cfg.set_train_value(64, 0.5, 4096, 1, 0.1)
            cfg.Num_Episodes, cfg.Num_Train_Steps = 1, 20
            env = start_env_batched(LINKS, 50, 1001, **kw)
            agents[name] = Agent(env.n_Veh, env.n_RB, env.n_Neighbor, 64, env, cfg, device=0, seed=1001, use_graph=True)
            agents[name].train(1, 20)                                 # warm-up, untimed
        torch.cuda.synchronize()
        for rep in range(reps):
            for name in SETTINGS:
                t0 = time.perf_counter()
                agents[name].train(1, 20)
                torch.cuda.synchronize()
                walls[name].append(time.perf_counter() - t0)
    return {b: {"wall_s_per_call": [round(w, 4) for w in walls[b]], "ms_per_train_step": round(float(np.median(walls[b])) * 1e3 / 20, 3)}
            for b in walls}


ROLLOUT_SETTINGS = {"host_lookahead": (dict(backend="host"), "host"),
                    "device_streams_host_rollout": (dict(backend="device", streams="device"), "host"),
                    "device_streams_device_rollout": (dict(backend="device", streams="device"), "device")}


def _rollout_agent(E, kw, rollout, batch=4096, walk="serial", streams="chain"):
    import random
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(1001)
    np.random.seed(1001)
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, batch, 1, 0.1)
    cfg.Num_Episodes, cfg.Num_Train_Steps = 1, 20
    env = start_env_batched(LINKS, E, 1001, **kw)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, 64, env, cfg, device=0, seed=1001, use_graph=True, rollout_backend=rollout,
                 trajectory_walk=walk, trajectory_streams=streams)


def rollout_legs(E, reps, warmup):
    """one rollout iteration of E simulators alone (no replay in between): wall time per iteration with epsilon held near 0.5,
    the host synchronised at the end of every iteration (the result row is read), and the bytes moved per iteration"""
    import torch
    agents = {name: _rollout_agent(E, kw, rollout) for name, (kw, rollout) in ROLLOUT_SETTINGS.items() if name != "host_lookahead"}
    walls = {name: [] for name in agents}
    traffic = {}
    for ag in agents.values():
        ag.num_Train_Step = 20
    for k in range(warmup + reps):
        if k == warmup:
            traffic = {name: dict(ag.env.device_channels.traffic) for name, ag in agents.items()}
        for name, ag in agents.items():                              # taken in turn: the box's load drifts
            ag.num_step = 10 * ag.num_transition                       # epsilon = 1 - 0.99 * 500 / 800: both branches every iteration
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ag.generate_d2d_transition(E)
            if k >= warmup:
                walls[name].append(time.perf_counter() - t0)
    row = {"simulators": E, "links": LINKS, "rb": RB}
    for name, ag in agents.items():
        row["iteration_%s_ms" % name] = _median_ms(walls[name])
        after = ag.env.device_channels.traffic
        for key in ("bytes_up", "bytes_down"):
            row["%s_%s_per_iteration" % (name, key)] = (after[key] - traffic[name][key]) // reps
    # the call alone between HIP events, eagerly and replayed from a captured graph (policy already on the device)
    ag = agents["device_streams_device_rollout"]
    dc, rep = ag.env.device_channels, ag.device_replay
    engine, rp = ag.brain.model.engine, rep.row_ptr(E)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    from v2xgnn.lib import check
    import ctypes
    out = {}
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        head = rep.reserve(E)
        r = dc.rollout_struct(rep.storage(), head, rep.capacity, 1.0, 0.1, engine=engine, row_ptr=rp)
        call = lambda: check(dc._lib, dc._lib.v2x_rollout_step(ctypes.byref(r), torch.cuda.current_stream().cuda_stream))   # noqa: E731
        call()
        torch.cuda.synchronize()
        graph, captured = torch.cuda.CUDAGraph(), None
        try:
            with torch.cuda.graph(graph, stream=side):
                call()
            captured = graph.replay
        except Exception as exc:                                       # written down, not hidden
            out["graph_error"] = "%s: %s" % (type(exc).__name__, exc)
        for tag, fn in (("eager", call), ("graph", captured)):
            if fn is None:
                continue
            gpu, host = [], []
            for k in range(warmup + reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                fn()
                ev[1].record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if k >= warmup:
                    gpu.append(ev[0].elapsed_time(ev[1]) * 1e-3)
                    host.append(t1 - t0)
            out["call_%s_gpu_ms" % tag], out["call_%s_enqueue_ms" % tag] = _median_ms(gpu), _median_ms(host)
    row.update(out)
    return row


def loop_in_process_rollout(reps):
    """loop_in_process_streams for the three settings of ROLLOUT_SETTINGS at 50 simulators, batch 4096"""
    import torch
    agents, walls = {}, {name: [] for name in ROLLOUT_SETTINGS}
    with torch.cuda.stream(torch.cuda.Stream(device=0)):
        for name, (kw, rollout) in ROLLOUT_SETTINGS.items():
            agents[name] = _rollout_agent(50, kw, rollout)
            agents[name].train(1, 20)                                 # warm-up, untimed
        torch.cuda.synchronize()
        for rep in range(reps):
            for name in ROLLOUT_SETTINGS:
                t0 = time.perf_counter()
                agents[name].train(1, 20)
                torch.cuda.synchronize()
                walls[name].append(time.perf_counter() - t0)
    return {b: {"wall_s_per_call": [round(w, 4) for w in walls[b]], "ms_per_train_step": round(float(np.median(walls[b])) * 1e3 / 20, 3)}
            for b in walls}


TRAJECTORY_SETTINGS = {"trajectory": (dict(backend="device", streams="device"), "trajectory"),
                       "trajectory_wide": (dict(backend="device", streams="device"), "trajectory", 4096, "wide"),
                       "trajectory_split": (dict(backend="device", streams="device"), "trajectory", 4096, "wide", "split"),
                       "device": (dict(backend="device", streams="device"), "device"),
                       "host_native_rollout": (dict(backend="host"), "host")}            # (E = 1 only: the single-call v2xsim_rollout)


WALK_KERNELS = {"serial": ("k_sim_trajectory",), "wide": ("k_traj_stream", "k_traj_terms", "k_traj_scan", "k_traj_observe"),
                "split": ("k_traj_words", "k_traj_walk", "k_traj_uniforms", "k_traj_terms", "k_traj_scan", "k_traj_observe")}


def kernel_times(call, names, reps):
    """median duration in ms of every kernel whose name holds one of `names`, over `reps` calls of call() under torch's
    profiler (the device's own kernel timestamps: a launch inside a library call cannot be bracketed by events from outside)
    -> {name: ms}, or {"error": text} when the profiler gives no kernel records"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        seen = {k: [] for k in names}
        for ev in prof.events():
            for k in names:
                if k in ev.name:
                    seen[k].append(float(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)))
        if not all(seen.values()):
            return {"error": "no kernel records for %s" % [k for k, v in seen.items() if not v]}
        return {k: round(float(np.median(v)) * 1e-3, 4) for k, v in seen.items()}
    except Exception as exc:                                           # written down, not hidden
        return {"error": "%s: %s" % (type(exc).__name__, exc)}


def trajectory_legs(E, reps, warmup, loop_reps):
    """a 50-transition rollout of E simulators alone (no replay in between), the one call between HIP events, and the DQN loop"""
    import ctypes
    import torch
    from v2xgnn.lib import check
    names = [k for k in TRAJECTORY_SETTINGS if k != "host_native_rollout" or E == 1]
    row = {"simulators": E, "links": LINKS, "rb": RB, "transitions": 50, "iterations": -(-50 // E)}
    with torch.cuda.stream(torch.cuda.Stream(device=0)):
        agents = {k: _rollout_agent(E, *TRAJECTORY_SETTINGS[k]) for k in names}
        walls, traffic = {k: [] for k in names}, {}
        for ag in agents.values():
            ag.num_Train_Step = 20
        for k in range(warmup + reps):
            if k == warmup:
                traffic = {name: dict(ag.env.device_channels.traffic) for name, ag in agents.items() if name != "host_native_rollout"}
            for name, ag in agents.items():                          # taken in turn: the box's load drifts
                ag.num_step = 10 * 50                                  # epsilon = 1 - 0.99 * 500 / 800: both branches in every rollout
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ag.generate_d2d_transition(50)
                torch.cuda.synchronize()
                if k >= warmup:
                    walls[name].append(time.perf_counter() - t0)
        for name, ag in agents.items():
            row["rollout_%s_ms" % name] = _median_ms(walls[name])
            if name in traffic:
                after = ag.env.device_channels.traffic
                for key in ("bytes_up", "bytes_down"):
                    row["%s_%s_per_rollout" % (name, key)] = (after[key] - traffic[name][key]) // reps
        # the call alone between HIP events (policy already on the device), and what the host spends enqueueing it: the serial
        # form, the wide form and the wide form with the split stream phase on the same agent's state, taken in turn; then the
        # trajectory's own kernels, one by one
        ag = agents["trajectory"]
        dc, rep, T = ag.env.device_channels, ag.device_replay, -(-50 // E)
        engine, rp = ag.brain.model.engine, rep.row_ptr(T * E)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        head = rep.reserve(T * E)
        r = dc.rollout_steps_struct(T, rep.storage(), head, rep.capacity, 1.0, 0.1, engine=engine, row_ptr=rp)
        ws, ss = dc._wide_workspace(T), dc._split_workspace(T)
        stream = lambda: torch.cuda.current_stream().cuda_stream           # noqa: E731
        calls = {"serial": lambda: check(dc._lib, dc._lib.v2x_rollout_steps(ctypes.byref(r), stream())),
                 "wide": lambda: check(dc._lib, dc._lib.v2x_rollout_steps_wide(ctypes.byref(r), ws.data_ptr(), ws.numel(), stream())),
                 "split": lambda: check(dc._lib, dc._lib.v2x_rollout_steps_split(ctypes.byref(r), ws.data_ptr(), ws.numel(), ss.data_ptr(),
                                                                                 ss.numel(), stream()))}
        gpu, host = {w: [] for w in calls}, {w: [] for w in calls}
        for k in range(warmup + reps):
            for w, call in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                call()
                ev[1].record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if k >= warmup:
                    gpu[w].append(ev[0].elapsed_time(ev[1]) * 1e-3)
                    host[w].append(t1 - t0)
        row["call_gpu_ms"], row["call_enqueue_ms"] = _median_ms(gpu["serial"]), _median_ms(host["serial"])
        row["call_wide_gpu_ms"], row["call_wide_enqueue_ms"] = _median_ms(gpu["wide"]), _median_ms(host["wide"])
        row["call_split_gpu_ms"], row["call_split_enqueue_ms"] = _median_ms(gpu["split"]), _median_ms(host["split"])
        for w, call in calls.items():
            row["kernels_%s_ms" % w] = kernel_times(call, WALK_KERNELS[w], min(reps, 20))
        # the loop: Agent.train(1, 20), the agents taken in turn
        loop = {k: [] for k in names}
        for ag in agents.values():
            ag.train(1, 20)                                            # warm-up, untimed
        torch.cuda.synchronize()
        for _ in range(loop_reps):
            for name, ag in agents.items():
                t0 = time.perf_counter()
                ag.train(1, 20)
                torch.cuda.synchronize()
                loop[name].append(time.perf_counter() - t0)
        for name in names:
            row["loop_%s_ms_per_train_step" % name] = round(float(np.median(loop[name])) * 1e3 / 20, 3)
        for ag in agents.values():
            ag.brain.close()
    return row


EVALUATE_CONFIGS = (("no_optimum", 20, False, "host"), ("optimum_bound", 20, True, "bound"), ("optimum_device", 12, True, "device"))
# name -> (simulator backend, streams, eval_backend)
EVALUATE_SETTINGS = {"device_eval": ("device", "device", "device"), "device_eval_wide": ("device", "device", "device", "wide"),
                     "device_eval_split": ("device", "device", "device", "wide", "split"),
                     "host_eval_device_streams": ("device", "device", "host"), "host_eval_host_simulator": ("host", "host", "host")}


def _evaluate_agent(links, backend, streams, walk="serial", stream_phase="chain"):
    import random
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(7)
    np.random.seed(7)
    env = start_env_batched(links, 1, 7, lookahead=False, backend=backend, streams=streams)
    cfg = RL_Config()
    cfg.set_train_value(64, 0.5, 4096, 1, 0.1)
    return Agent(links, env.n_RB, env.n_Neighbor, 64, env, cfg, seed=7, device_replay=False, trajectory_walk=walk,
                 trajectory_streams=stream_phase)


def evaluate_legs(name, links, opt_flag, opt_backend, episodes, reps, warmup):
    """test_run(episodes, 50 steps) of the three agents, taken in turn"""
    import torch
    row = {"config": name, "links": links, "rb": RB, "episodes": episodes, "steps": 50, "opt_backend": opt_backend if opt_flag else None,
           "reps": reps, "warmup": warmup}
    agents = {k: _evaluate_agent(links, v[0], v[1], *v[3:]) for k, v in EVALUATE_SETTINGS.items()}
    walls, traffic = {k: [] for k in agents}, {}
    for k in range(warmup + reps):
        if k == warmup:
            traffic = {n: dict(ag.env.device_channels.traffic) for n, ag in agents.items() if EVALUATE_SETTINGS[n][0] == "device"}
        for n, ag in agents.items():                                 # taken in turn: the box's load drifts
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ag.test_run(episodes, 50, opt_flag, opt_backend=opt_backend, eval_backend=EVALUATE_SETTINGS[n][2])
            torch.cuda.synchronize()
            if k >= warmup:
                walls[n].append(time.perf_counter() - t0)
    for n, ag in agents.items():
        row["%s_ms_per_episode" % n] = round(float(np.median(walls[n])) * 1e3 / episodes, 3)
        if n in traffic:
            after = ag.env.device_channels.traffic
            for key in ("bytes_up", "bytes_down"):
                row["%s_%s_per_episode" % (n, key)] = (after[key] - traffic[n][key]) // (reps * episodes)
        row["%s_stats" % n] = dict(ag.eval_stats)
        if n in traffic:
            row["%s_walk_calls" % n] = dict(ag.env.device_channels.walk_calls)
            row["%s_stream_phase_calls" % n] = dict(ag.env.device_channels.stream_phase_calls)
        ag.brain.close()
    return row


def main_evaluate(args):
    import torch
    from v2xgnn.rl.batched_env import _usable_cpus
    result = {"device": torch.cuda.get_device_name(0), "usable_cpus": _usable_cpus(), "runs": []}
    for name, links, opt_flag, opt_backend in EVALUATE_CONFIGS:
        if args.eval_configs and name not in args.eval_configs:
            continue
        reps, warmup = (max(3, args.loop_reps), 1) if opt_flag else (min(args.reps, 20), min(args.warmup, 3))
        result["runs"].append(evaluate_legs(name, links, opt_flag, opt_backend, args.episodes, reps, warmup))
        print(json.dumps(result["runs"][-1]), flush=True)
    return result


def main_trajectory(args):
    import torch
    from v2xgnn.rl.batched_env import _usable_cpus
    result = {"device": torch.cuda.get_device_name(0), "usable_cpus": _usable_cpus(), "reps": args.reps, "warmup": args.warmup,
              "loop_reps": max(3, args.loop_reps), "rollouts": []}
    for E in args.simulators:
        result["rollouts"].append(trajectory_legs(E, args.reps, args.warmup, max(3, args.loop_reps)))
        print(json.dumps(result["rollouts"][-1]), flush=True)
    return result


def main_rollout(args):
    import torch
    from v2xgnn.rl.batched_env import _usable_cpus
    result = {"device": torch.cuda.get_device_name(0), "usable_cpus": _usable_cpus(), "reps": args.reps, "warmup": args.warmup,
              "iterations": [rollout_legs(E, args.reps, args.warmup) for E in args.simulators]}
    for row in result["iterations"]:
        print(json.dumps(row))
    if not args.no_loop:
        result["loop_in_process"] = loop_in_process_rollout(max(3, args.loop_reps))
        print(json.dumps(result["loop_in_process"]))
    return result


def main_streams(args):
    import torch
    from v2xgnn.rl.batched_env import _usable_cpus
    result = {"device": torch.cuda.get_device_name(0), "usable_cpus": _usable_cpus(), "reps": args.reps, "warmup": args.warmup,
              "steps": [streams_legs(E, args.reps, args.warmup) for E in args.simulators]}
    for row in result["steps"]:
        print(json.dumps(row))
    if not args.no_loop:
        result["loop_in_process"] = loop_in_process_streams(max(3, args.loop_reps))
        print(json.dumps(result["loop_in_process"]))
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["channels", "streams", "rollout", "trajectory", "evaluate"], default="channels")
    ap.add_argument("--episodes", type=int, default=1, help="--mode evaluate: episodes per timed test_run")
    ap.add_argument("--eval-configs", nargs="+", default=None, choices=[c[0] for c in EVALUATE_CONFIGS],
                    help="--mode evaluate: only these configurations (default: all)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--simulators", type=int, nargs="+", default=None)
    args = ap.parse_args()
    if args.simulators is None:
        args.simulators = [1, 5, 10, 25, 50] if args.mode == "trajectory" else [1, 50, 200]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sim_device_timing needs a GPU: nothing is measured without one")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"streams": "sim_device_streams_timing.json", "rollout": "rollout_device_timing.json",
                                                           "trajectory": "rollout_trajectory_timing.json",
                                                           "evaluate": "eval_device_timing.json"}.get(
            args.mode, "sim_device_timing.json"))
    from v2xgnn.rl.batched_env import _usable_cpus
    if args.mode == "streams":
        result = main_streams(args)
    elif args.mode == "rollout":
        result = main_rollout(args)
    elif args.mode == "trajectory":
        result = main_trajectory(args)
    elif args.mode == "evaluate":
        result = main_evaluate(args)
    else:
        result = {"device": torch.cuda.get_device_name(0), "usable_cpus": _usable_cpus(), "reps": args.reps, "warmup": args.warmup,
                  "steps": [step_legs(E, args.reps, args.warmup) for E in args.simulators]}
        for row in result["steps"]:
            print(json.dumps(row))
    if args.mode == "channels" and not args.no_loop:
        result["loop"] = loop_leg(args.loop_reps)
        print(json.dumps(result["loop"]))
        try:
            result["loop_in_process"] = loop_in_process(max(3, args.loop_reps))
        except Exception as exc:                                       # the legs above are still worth writing down
            result["loop_in_process"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        print(json.dumps(result["loop_in_process"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
