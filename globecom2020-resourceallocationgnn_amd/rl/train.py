"""Training driver: the counterpart of the reference's RL_Train_main.py (main :21-75, start_env :78-95,
run_train :98-118) on the engine, for any number of V2V links and -- launched with torch.distributed.run --
data-parallel over the GPUs of one node (BASELINE.json configs[0] and configs[2]).

    python -m v2xgnn.rl.train --links 4 --feedback 16 --batch 512 --episodes 2 --train-steps 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m v2xgnn.rl.train --links 20 --feedback 64 --batch 4096 --episodes 1 --train-steps 20

Data-parallel scheme (--rollouts replicated, the default): every rank runs the SAME seeded simulator and replay sampling (a few hundred microseconds of
numpy per step), so all ranks hold the identical minibatch without any broadcast; each fit step takes the rank's
contiguous shard of it and all-reduces the gradient (v2xgnn.dp).  Weights therefore stay bit-identical on all ranks
and the epsilon-greedy rollouts stay in lock-step.  --rollouts sharded gives every rank its own simulator and replay
memory and 50/G of the transitions of a train step (Agent docstring): the simulator work per rank drops by G.
"""
import argparse
import json
import os
import random
import time

import numpy as np

from .agent import Agent
from .environment import Environ
from .sim_config import RL_Config


def start_env(n_links=None):
    """Lane grid of RL_Train_main.py:82-88; n_links: number of V2V links (default: the simulator's 4)."""
    up_lanes = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
    down_lanes = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
    left_lanes = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
    right_lanes = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
    env = Environ(down_lanes, up_lanes, left_lanes, right_lanes, 750, 1299)
    env.new_random_game(env.n_Veh)
    if n_links is not None and n_links != env.n_Veh:
        env.new_random_game(n_links)
    return env


def start_env_batched(n_links, n_envs, seed, lookahead=None, backend="host", device=0, streams="host", reset="host"):
    """E environments on the same lane grid, environment e seeded with seed + 104729 e (rl/batched_env.py).
    lookahead: compute every next simulator step on the library's worker thread while the agent scores and replays (same
    trajectories, see BatchedEnviron); default on, V2X_SIM_LOOKAHEAD=0 switches it off.
    backend: "host" (the default: BatchedEnviron) or "device" (rl/device_sim.py: channel update, observation and rates on the
    GPU `device`; it has no look-ahead).
    streams: with backend="device", where mobility and the MT19937 streams advance: "host" (libv2xsim.so, the default) or
    "device" (a step is then one enqueue that takes only the actions from the host).
    reset: with streams="device", who runs new_random_game: "host" (the default) or "device" (one call on the resident state)."""
    import os
    if lookahead is None:
        lookahead = os.environ.get("V2X_SIM_LOOKAHEAD", "1") != "0"
    from .batched_env import BatchedEnviron
    up_lanes = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
    down_lanes = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
    left_lanes = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
    right_lanes = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
    if backend not in ("host", "device"):
        raise ValueError("backend must be 'host' or 'device', got %r" % (backend,))
    if streams not in ("host", "device"):
        raise ValueError("streams must be 'host' or 'device', got %r" % (streams,))
    if streams == "device" and backend != "device":
        raise ValueError("streams='device' needs backend='device' (the host simulator's streams live in libv2xsim.so)")
    if reset not in ("host", "device"):
        raise ValueError("reset must be 'host' or 'device', got %r" % (reset,))
    if reset == "device" and streams != "device":
        raise ValueError("reset='device' needs backend='device' and streams='device' (the reset draws from the streams where they live)")
    if backend == "device":
        from .device_sim import DeviceBatchedEnviron
        env = DeviceBatchedEnviron(down_lanes, up_lanes, left_lanes, right_lanes, 750, 1299, n_envs=n_envs,
                                   seeds=[seed + 104729 * e for e in range(n_envs)], device=device, streams=streams,
                                   reset=reset)
        env.new_random_game(n_links)
        return env
    env = BatchedEnviron(down_lanes, up_lanes, left_lanes, right_lanes, 750, 1299, n_envs=n_envs,
                         seeds=[seed + 104729 * e for e in range(n_envs)])
    env.lookahead = bool(lookahead) and env.native
    env.new_random_game(n_links)
    return env


def run_train(env, cfg, brain=None, save_dir=None, verbose=False, **brain_kwargs):
    """RL_Train_main.py:98-118"""
    agent = Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain, **brain_kwargs)
    out = agent.train(cfg.Num_Episodes, cfg.Num_Train_Steps, save_dir=save_dir, verbose=verbose)
    return agent, out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1001)           # RL_Train_main.py:44
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--use-graph", action="store_true")
    ap.add_argument("--envs", type=int, default=0,
                    help="step this many independent simulators as arrays (rl/batched_env.py) instead of one")
    ap.add_argument("--rollouts", choices=["replicated", "sharded"], default="replicated",
                    help="data-parallel runs: every rank steps the same simulator (bit-identical to one process) or every "
                         "rank its own, contributing 50/G transitions per train step (Agent docstring)")
    ap.add_argument("--sim-backend", choices=["host", "device"], default="host",
                    help="with --envs: where the simulators' channel update, observation and rates run -- libv2xsim.so on the "
                         "host (the default, and the definition) or the GPU (rl/device_sim.py)")
    ap.add_argument("--sim-streams", choices=["host", "device"], default="host",
                    help="with --sim-backend device: where mobility and the simulators' MT19937 streams advance -- libv2xsim.so "
                         "(the default) or the GPU, where a step is one enqueue that takes only the actions from the host")
    ap.add_argument("--sim-reset", choices=["host", "device"], default="host",
                    help="with --sim-backend device --sim-streams device: who resets the simulators at the start of an episode -- "
                         "the host library (the default) or the GPU, one call on the state resident in HBM (v2x_sim_reset)")
    ap.add_argument("--rollout", choices=["host", "device", "trajectory"], default="host",
                    help="with --sim-backend device --sim-streams device: 'device' runs a whole rollout iteration (score, pick, "
                         "step, reward, store) as one call on the state resident in HBM, 'trajectory' all iterations of a "
                         "rollout as one call (one kernel walks the simulators, one forward scores every observation, one kernel "
                         "picks, pays and stores); 'host' (the default) scores and stores through the host")
    ap.add_argument("--trajectory-walk", choices=["serial", "wide"], default="serial",
                    help="with --rollout trajectory: how a simulator's steps are walked -- 'serial' (the default: one workgroup "
                         "per simulator, step after step) or 'wide' (the steps spread over the chip in four launches; the same "
                         "bits; DESIGN.md section 6 says at which sizes it wins)")
    ap.add_argument("--trajectory-streams", choices=["chain", "split"], default="chain",
                    help="with --trajectory-walk wide: the stream phase of the wide walk -- 'chain' (the default: one launch draws "
                         "the streams of all steps) or 'split' (raw words, offset walk and conversion in three launches; the same bits)")
    ap.add_argument("--receiver-streams", choices=["chain", "split"], default="chain",
                    help="with --replay receivers --rollout trajectory: the stream phase of the resident rollout of 3..128 links -- "
                         "'chain' (the default: one launch draws the streams of all steps) or 'split' (raw words, the offset walk "
                         "for up to 128 vehicles and the conversion in three launches; the same bits)")
    ap.add_argument("--receiver-words", choices=["serial", "jump"], default="serial",
                    help="with --receiver-streams split: how the raw words are drawn -- 'serial' (the default: one workgroup per "
                         "simulator) or 'jump' (the words beyond a prefix in chunks entered by jump-ahead polynomials of MT19937, "
                         "spread over the chip; the same bits; DESIGN.md section 6 says at which sizes it pays)")
    ap.add_argument("--replay", choices=["auto", "receivers"], default="auto",
                    help="the replay memory: 'auto' (the default: in HBM up to 31 links, the reference's host memory beyond) or "
                         "'receivers' (rl/replay.py ReceiverReplay: in HBM for 3..128 links, the adjacency stored as the links' "
                         "receivers, one gather launch and one replay-step call per train step; one GPU; --rollout host, or --rollout "
                         "trajectory with --sim-backend device --sim-streams device: the whole rollout as one resident call)")
    ap.add_argument("--mixed-links", default=None, metavar="N1,N2,...",
                    help="train ONE shared-weight network on scenarios of these link counts at once (rl/mixed.py: MixedAgent), "
                         "--envs simulators per size; distinct multiples of 4 up to 28, at most 8 of them.  Host simulators, host "
                         "rollouts, one GPU unless the --mixed-* options below say otherwise; --links is ignored")
    ap.add_argument("--mixed-sim-backend", choices=["host", "device"], default="host",
                    help="with --mixed-links: --sim-backend for every link count's simulators (--sim-backend itself holds one link "
                         "count and stays refused)")
    ap.add_argument("--mixed-sim-streams", choices=["host", "device"], default="host",
                    help="with --mixed-links --mixed-sim-backend device: --sim-streams for every link count's simulators")
    ap.add_argument("--mixed-sim-reset", choices=["host", "device"], default="host",
                    help="with --mixed-links --mixed-sim-backend device --mixed-sim-streams device: --sim-reset for every link "
                         "count's simulators")
    ap.add_argument("--mixed-rollout", choices=["host", "trajectory"], default="host",
                    help="with --mixed-links --mixed-sim-backend device --mixed-sim-streams device: 'trajectory' runs all iterations "
                         "of a rollout for ALL link counts as one call on the resident states (one walk launch, one assembly launch, "
                         "one ragged forward, one finish launch); 'host' (the default) scores and stores through the host")
    ap.add_argument("--mixed-trajectory-walk", choices=["serial", "wide"], default="serial",
                    help="with --mixed-links --mixed-rollout trajectory: how that call walks the simulators' steps -- 'serial' (the "
                         "default: one workgroup per simulator, step after step) or 'wide' (the steps of all link counts spread "
                         "over the chip, six launches in the walk's place; the same bits; DESIGN.md section 3.8 says where it wins)")
    ap.add_argument("--save-interval", type=int, default=None, metavar="K",
                    help="with --mixed-links --save-dir: also save the two networks after every K-th episode (the reference saves "
                         "every 5): the checkpoints rl.evaluate --mixed-links scores")
    return ap


def parse_mixed_links(text):
    """'8,12,20' -> [8, 12, 20]; ValueError with the reason for anything MixedAgent or the simulator cannot take"""
    try:
        sizes = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError("--mixed-links takes link counts separated by commas, got %r" % (text,))
    if not 1 <= len(sizes) <= 8:
        raise ValueError("--mixed-links takes 1 to 8 link counts, got %d" % len(sizes))
    if len(set(sizes)) != len(sizes):
        raise ValueError("--mixed-links: the link counts must be distinct, got %s" % sizes)
    for n in sizes:
        # (groups of four vehicles, as for --links; the replay pools hold graphs of up to 31 links)
        if n < 4 or n % 4 or n > 31:
            raise ValueError("--mixed-links: every link count must be a multiple of 4 between 4 and 28 (got %d)" % n)
    return sorted(sizes)


def run_mixed(args):
    """--mixed-links: one MixedAgent over one batched simulator per link count (--mixed-sim-backend / --mixed-sim-streams say
    where they run, --mixed-rollout who makes the rollout, --mixed-trajectory-walk how its steps are walked); with --save-dir the two networks are saved at the end, with
    --save-interval K also after every K-th episode"""
    from .mixed import MixedAgent
    sizes = parse_mixed_links(args.mixed_links)
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)
    envs = [start_env_batched(n, args.envs, args.seed + 15485863 * k, backend=args.mixed_sim_backend, streams=args.mixed_sim_streams,
                              reset=args.mixed_sim_reset)
            for k, n in enumerate(sizes)]
    import contextlib
    ctx = contextlib.nullcontext()
    if args.use_graph:
        import torch
        ctx = torch.cuda.stream(torch.cuda.Stream())
    t0 = time.perf_counter()
    with ctx:
        agent = MixedAgent(envs, cfg, args.feedback, use_graph=args.use_graph, seed=args.seed, rollout=args.mixed_rollout,
                           trajectory_walk=args.mixed_trajectory_walk)
        loss, rewards, q_mean, q_max = agent.train(args.episodes, args.train_steps, verbose=True, save_dir=args.save_dir,
                                                   save_interval=args.save_interval)
    dt = time.perf_counter() - t0
    n_fit = args.episodes * args.train_steps
    print(json.dumps({"mixed_links": sizes, "envs_per_size": args.envs, "feat_dim": args.feedback, "batch": args.batch,
                      "episodes": args.episodes, "train_steps": args.train_steps, "env_steps": int(agent.num_step),
                      "sim_backend": args.mixed_sim_backend, "sim_streams": args.mixed_sim_streams, "sim_reset": args.mixed_sim_reset,
                      "rollout": args.mixed_rollout,
                      "trajectory_walk": args.mixed_trajectory_walk,
                      "rollouts_by_path": dict(agent.rollout_stats),
                      "stored": {str(n): agent.memory.stored(n) for n in sizes},
                      "dropped_irregular": {str(n): v for n, v in agent.memory.dropped_irregular.items()},
                      "wall_s": round(dt, 3), "fit_steps_per_s": round(n_fit / dt, 2),
                      "mean_loss_last_episode": round(float(loss[0, -1].mean()), 6),
                      "reward_last_episode": {str(n): round(float(v[-1].sum()), 4) for n, v in rewards.items()}}))
    agent.close()
    return 0


def parse_args(argv=None):
    """the command line, parsed, with every check that concerns --mixed-links made (a refusal exits with its message)
    -> (parser, arguments)"""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.replay == "receivers":
        if args.mixed_links is not None:
            ap.error("--replay receivers holds one link count: --mixed-links keeps one DeviceReplay per link count (4..28 links)")
        if args.rollout == "device":
            ap.error("--replay receivers needs --rollout host or --rollout trajectory: the one-iteration resident rollout "
                     "(--rollout device) holds 3..31 links and writes the other memory's layout")
        if args.rollout == "trajectory" and (args.sim_backend != "device" or args.sim_streams != "device"):
            ap.error("--replay receivers needs --rollout host, or --rollout trajectory with --sim-backend device --sim-streams "
                     "device (the whole rollout is then one call on the state resident in HBM, 3..128 links)")
        if args.rollout == "trajectory" and args.trajectory_streams != "chain":
            ap.error("--replay receivers --rollout trajectory walks wide with the chain stream phase: --trajectory-streams split "
                     "holds 3..31 links")
    if args.receiver_streams != "chain" and (args.replay != "receivers" or args.rollout != "trajectory"):
        ap.error("--receiver-streams %s needs --replay receivers --rollout trajectory (it is a form of the stream phase of the "
                 "resident rollout of 3..128 links)" % args.receiver_streams)
    if args.receiver_words != "serial" and args.receiver_streams != "split":
        ap.error("--receiver-words %s needs --receiver-streams split (it draws the split stream phase's words in chunks)"
                 % args.receiver_words)
    if args.mixed_links is not None:
        # the single-size options hold one link count and stay refused; the device simulators and the resident rollout of ALL
        # link counts are asked for by --mixed-sim-backend / --mixed-sim-streams / --mixed-rollout
        if args.sim_backend != "host" or args.sim_streams != "host" or args.sim_reset != "host":
            ap.error("--mixed-links steps host simulators: --sim-backend / --sim-streams device hold one link count "
                     "(--mixed-sim-backend / --mixed-sim-streams put every link count's simulators on the device)")
        if args.rollout != "host":
            ap.error("--mixed-links scores through the host: --rollout %s holds one link count (--mixed-rollout trajectory runs "
                     "the rollouts of all link counts in one call)" % args.rollout)
        if args.trajectory_walk != "serial" or args.trajectory_streams != "chain":
            ap.error("--mixed-links walks serially: the wide and split walks (--trajectory-walk / --trajectory-streams) hold one "
                     "link count (--mixed-trajectory-walk wide spreads the steps of all link counts over the chip)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("V2X_FORCE_DP") == "1" or args.rollouts != "replicated":
            ap.error("--mixed-links runs on one GPU: the ragged replay step has no data-parallel form")
        if args.envs < 1:
            ap.error("--mixed-links steps batched simulators: give --envs (simulators per link count)")
        if args.mixed_sim_streams == "device" and args.mixed_sim_backend != "device":
            ap.error("--mixed-sim-streams device needs --mixed-sim-backend device")
        if args.mixed_sim_reset == "device" and args.mixed_sim_streams != "device":
            ap.error("--mixed-sim-reset device needs --mixed-sim-backend device --mixed-sim-streams device")
        if args.mixed_rollout == "trajectory" and args.mixed_sim_streams != "device":
            ap.error("--mixed-rollout trajectory needs --mixed-sim-backend device --mixed-sim-streams device (the simulators "
                     "advance inside the call)")
        if args.mixed_trajectory_walk != "serial" and args.mixed_rollout != "trajectory":
            ap.error("--mixed-trajectory-walk %s needs --mixed-rollout trajectory" % args.mixed_trajectory_walk)
        if args.save_interval is not None and (args.save_interval < 1 or args.save_dir is None):
            ap.error("--save-interval must be at least 1 and needs --save-dir")
        try:
            parse_mixed_links(args.mixed_links)
        except ValueError as exc:
            ap.error(str(exc))
    elif args.save_interval is not None:
        ap.error("--save-interval needs --mixed-links (a single-size run saves every 5 episodes)")
    elif (args.mixed_sim_backend != "host" or args.mixed_sim_streams != "host" or args.mixed_rollout != "host" or
          args.mixed_trajectory_walk != "serial" or args.mixed_sim_reset != "host"):
        ap.error("--mixed-sim-backend / --mixed-sim-streams / --mixed-sim-reset / --mixed-rollout / --mixed-trajectory-walk need "
                 "--mixed-links")
    return ap, args


def main(argv=None):
    ap, args = parse_args(argv)
    if args.mixed_links is not None:
        return run_mixed(args)
    if args.sim_streams == "device" and args.sim_backend != "device":
        ap.error("--sim-streams device needs --sim-backend device")
    if args.sim_reset == "device" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--sim-reset device needs --sim-backend device --sim-streams device")
    if args.rollout != "host" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--rollout %s needs --sim-backend device --sim-streams device" % args.rollout)
    if args.trajectory_walk != "serial" and args.rollout != "trajectory":
        ap.error("--trajectory-walk %s needs --rollout trajectory" % args.trajectory_walk)
    if args.trajectory_streams != "chain" and args.trajectory_walk != "wide":
        ap.error("--trajectory-streams %s needs --trajectory-walk wide" % args.trajectory_streams)
    if args.sim_backend == "device" and args.envs < 1:
        ap.error("--sim-backend device steps batched simulators: give --envs")
    if args.links < 4 or args.links % 4:
        # the simulator drops vehicles in groups of four, one per direction (Environment.py:217-231), and the
        # observation divides by links - 2 (BS_brain.py:405)
        ap.error("--links must be a multiple of 4 and at least 4 (got %d)" % args.links)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    force_dp = os.environ.get("V2X_FORCE_DP") == "1"            # run the RCCL path with a single rank (tests)
    if world > 1 or force_dp:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29544")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))

    sharded = args.rollouts == "sharded" and world > 1
    random.seed(args.seed + (7919 * rank if sharded else 0))      # sharded rollouts: one simulator / exploration stream per rank
    np.random.seed(args.seed + (7919 * rank if sharded else 0))
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)       # RL_Train_main.py:33-35,60
    cfg.Num_Episodes, cfg.Num_Train_Steps = args.episodes, args.train_steps
    if args.sim_backend == "device":
        env = start_env_batched(args.links, args.envs, args.seed + (7919 * rank if sharded else 0), backend="device", device=local,
                                streams=args.sim_streams, reset=args.sim_reset)
    else:
        env = (start_env_batched(args.links, args.envs, args.seed + (7919 * rank if sharded else 0)) if args.envs > 0
               else start_env(args.links))
    t0 = time.perf_counter()
    import contextlib
    ctx = contextlib.nullcontext()
    if args.use_graph:
        # the engine captures hipGraphs only on a non-default stream (capture is not allowed on the legacy stream)
        import torch
        torch.cuda.set_device(local)
        ctx = torch.cuda.stream(torch.cuda.Stream(device=local))
    with ctx:
        agent, (loss, reward_step, reward_ep, q_mean, q_max, _, _) = run_train(
            env, cfg, save_dir=args.save_dir if rank == 0 else None, verbose=rank == 0,
            device=local, seed=args.seed, use_graph=args.use_graph, data_parallel=world > 1 or force_dp,
            rollouts=args.rollouts, rollout_backend=args.rollout, trajectory_walk=args.trajectory_walk,
            trajectory_streams=args.trajectory_streams, receiver_streams=args.receiver_streams, receiver_words=args.receiver_words,
            device_replay=args.replay)
    dt = time.perf_counter() - t0
    if rank == 0:
        n_fit = args.episodes * args.train_steps
        print(json.dumps({"links": args.links, "feat_dim": args.feedback, "batch": args.batch, "n_gpus": world,
                          "episodes": args.episodes, "train_steps": args.train_steps, "env_steps": int(agent.num_step),
                          "wall_s": round(dt, 3), "fit_steps_per_s": round(n_fit / dt, 2),
                          "mean_loss_last_episode": [round(float(v), 6) for v in loss[:, -1].mean(axis=1)],
                          "reward_last_episode": round(float(reward_ep[-1]), 4)}))
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
