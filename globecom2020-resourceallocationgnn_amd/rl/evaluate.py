"""Evaluation-of-training driver: the counterpart of the reference's RL_Evaluated_main_Epsilon_DiffTrails.py (main :17-,
run_test -> Agent.evaluate_training_diff_trials, BS_brain.py:1164-1451): every checkpoint a training run saved (one per 5
episodes) is evaluated under a fixed epsilon-greedy policy over several re-seeded trials, next to the random-action
baseline and the brute-force optimum.

    python -m v2xgnn.rl.train    --links 4 --episodes 10 --train-steps 20 --batch 512 --save-dir runs/a
    python -m v2xgnn.rl.evaluate --links 4 --episodes 10 --batch 512 --save-dir runs/a --test-steps 100 --trials 10

--sweep scores all checkpoints of a trial on ONE walked episode (Agent.evaluate_training_sweep); beyond 31 links on the GPU:

    python -m v2xgnn.rl.evaluate --links 100 --feedback 64 --episodes 40 --save-dir runs/b --test-steps 50 --trials 10 --sweep \
                                 --opt-backend local --sim-backend device --sim-streams device --eval-backend device

The checkpoints of a shared-weight network trained on several link counts at once (rl.train --mixed-links ... --save-interval 5
--save-dir D) are evaluated per link count, on the training sizes or on others -- every trial ONE re-seeded episode on which
all checkpoints are scored (rl/mixed.py MixedAgent.evaluate_training):

    python -m v2xgnn.rl.evaluate --mixed-links 8,12,20 [--eval-links 8,16,28] [--envs 4] --feedback 64 --batch 4096 \
                                 --episodes 20 --train-steps 20 --save-dir D --test-steps 50 --trials 10 [--epsilon 0.05] \
                                 [--opt --opt-backend device | bound | local] \
                                 [--sim-backend device --sim-streams device --eval-backend device [--mixed-trajectory-walk wide]]
"""
import argparse
import json
import os
import random

import numpy as np

from .agent import Agent
from .sim_config import RL_Config
from .run import add_sim_arguments, check_receiver_arguments, evaluation_env


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=0.05)          # RL_Evaluated_main_Epsilon_DiffTrails.py:25
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--episodes", type=int, default=10, help="training episodes of the run (a checkpoint every 5)")
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--test-steps", type=int, default=100)        # :42
    ap.add_argument("--trials", type=int, default=10)             # :39
    ap.add_argument("--epsilon", type=float, default=0.0)         # :37
    ap.add_argument("--opt", action="store_true")
    ap.add_argument("--opt-backend", choices=("host", "device", "bound", "local"), default=None,
                    help="where the optimum is searched: numpy on the host (the default; C^N <= 65536) or the GPU, exhaustively "
                         "(device: C^N <= 2^36; the default with --mixed-links) or by branch and bound (bound: up to 32 links, "
                         "e.g. 20 x 4); local: NOT the optimum but a lower bound on it, the best of --opt-restarts local searches "
                         "on the GPU (up to 128 links, e.g. 100 x 4)")
    ap.add_argument("--opt-restarts", type=int, default=None,
                    help="restarts per state of --opt-backend local (default: rl/optimum.py DEFAULT_LOCAL_RESTARTS)")
    ap.add_argument("--seed", type=int, default=1)                # :22
    ap.add_argument("--sweep", action="store_true",
                    help="with --links: score all checkpoints on ONE walked episode per trial (Agent.evaluate_training_sweep; with "
                         "--eval-backend device beyond 31 links one library call per trial) instead of one episode per "
                         "(trial, checkpoint)")
    ap.add_argument("--mixed-links", default=None, metavar="N1,N2,...",
                    help="evaluate the checkpoints rl.train --mixed-links N1,N2,... --save-interval K saved (rl/mixed.py): the "
                         "training sizes, used only to find the files; --links is ignored")
    ap.add_argument("--eval-links", default=None, metavar="M1,M2,...",
                    help="with --mixed-links: the link counts to evaluate on (distinct multiples of 4 up to 28, at most 8; "
                         "default: the training sizes)")
    ap.add_argument("--envs", type=int, default=1,
                    help="with --mixed-links: simulators per evaluated link count, each a parallel episode (default 1)")
    ap.add_argument("--mixed-trajectory-walk", choices=["serial", "wide"], default="serial",
                    help="with --mixed-links --eval-backend device: how a trial's steps are walked -- 'serial' (the default) or "
                         "'wide' (the steps of all link counts spread over the chip; the same bits)")
    add_sim_arguments(ap)
    return ap


def parse_args(argv=None):
    """the command line, parsed, with every check that concerns --mixed-links made (a refusal exits with its message: those of
    rl/run.py) -> (parser, arguments); arguments.mixed_links / eval_links are then sorted lists of link counts (or None)"""
    from .train import parse_mixed_links
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.mixed_links is None:
        if args.eval_links is not None or args.envs != 1:
            ap.error("--eval-links / --envs need --mixed-links")
        if args.mixed_trajectory_walk != "serial":
            ap.error("--mixed-trajectory-walk %s needs --mixed-links" % args.mixed_trajectory_walk)
        if args.opt_backend is None:
            args.opt_backend = "host"
        check_receiver_arguments(ap, args)
        return ap, args
    # the mixed network is scored as one ragged batch of all link counts: what holds one link count stays refused
    if args.receiver_streams != "chain":
        ap.error("--mixed-links holds 3..31 links: --receiver-streams is the stream phase of one link count beyond 31 "
                 "(rl.evaluate --links)")
    if args.receiver_words != "serial":
        ap.error("--mixed-links holds 3..31 links: --receiver-words draws the words of one link count beyond 31 (rl.evaluate --links)")
    if args.trajectory_walk != "serial" or args.trajectory_streams != "chain":
        ap.error("--mixed-links walks serially: the wide and split walks (--trajectory-walk / --trajectory-streams) hold one "
                 "link count (--mixed-trajectory-walk wide spreads the steps of all link counts over the chip)")
    if args.opt_backend == "host":
        ap.error("--mixed-links searches the optimum on the GPU: --opt-backend host enumerates one link count on the host "
                 "(--opt-backend device, bound or local)")
    if args.opt_backend is None:
        args.opt_backend = "device"
    if args.envs < 1:
        ap.error("--mixed-links steps batched simulators: --envs must be at least 1 (got %d)" % args.envs)
    if args.trials < 1 or args.test_steps < 1:
        ap.error("--mixed-links: --trials and --test-steps must be at least 1")
    if args.sim_streams == "device" and args.sim_backend != "device":
        ap.error("--sim-streams device needs --sim-backend device")
    if args.sim_reset == "device" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--sim-reset device needs --sim-backend device --sim-streams device")
    if args.eval_backend != "host" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--eval-backend %s needs --sim-backend device --sim-streams device" % args.eval_backend)
    if args.mixed_trajectory_walk != "serial" and args.eval_backend != "device":
        ap.error("--mixed-trajectory-walk %s needs --eval-backend device" % args.mixed_trajectory_walk)
    try:
        args.mixed_links = parse_mixed_links(args.mixed_links)
    except ValueError as exc:
        ap.error(str(exc))
    if args.eval_links is None:
        args.eval_links = list(args.mixed_links)
    else:
        try:
            args.eval_links = parse_mixed_links(args.eval_links)
        except ValueError as exc:
            ap.error(str(exc).replace("--mixed-links", "--eval-links"))
    return ap, args


def saved_checkpoints(save_dir, episodes, train_steps, batch):
    """the episode tags 1..episodes under which rl.train --mixed-links --save-interval left a Q-network in save_dir"""
    from .run import weight_file_names
    return [ep for ep in range(1, episodes + 1) if os.path.exists(os.path.join(save_dir, weight_file_names(ep, train_steps, batch)[0]))]


def run_mixed(ap, args):
    """--mixed-links: score every checkpoint found for --episodes on --eval-links, --envs parallel episodes per link count and
    trial (MixedAgent.evaluate_training) -> the JSON summary, per link count the mean reward per checkpoint next to the random
    scheme's and the optimum's"""
    from .mixed import MixedAgent
    from .train import start_env_batched
    tags = saved_checkpoints(args.save_dir, args.episodes, args.train_steps, args.batch)
    if not tags:
        ap.error("no checkpoint of episodes 1..%d with --train-steps %d --batch %d in %s (rl.train --mixed-links ... "
                 "--save-interval K --save-dir D writes them)" % (args.episodes, args.train_steps, args.batch, args.save_dir))
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)
    envs = [start_env_batched(n, args.envs, args.seed + 15485863 * k, backend=args.sim_backend, streams=args.sim_streams,
                              reset=args.sim_reset)
            for k, n in enumerate(args.eval_links)]
    agent = MixedAgent(envs, cfg, args.feedback, seed=args.seed, trajectory_walk=args.mixed_trajectory_walk)
    books = agent.evaluate_training(envs, tags, args.test_steps, args.trials, args.epsilon, opt_flag=args.opt,
                                    opt_backend=args.opt_backend, opt_restarts=args.opt_restarts, eval_backend=args.eval_backend,
                                    save_dir=args.save_dir, num_train_steps=args.train_steps)
    per_links = {}
    for n in args.eval_links:
        gnn = books[n]['gnn'][1]                                          # [trials, K, E, steps]
        per_links[str(n)] = {"mean_reward_per_checkpoint": [round(float(gnn[:, k].mean()), 4) for k in range(len(tags))],
                             "mean_reward_random": round(float(books[n]['random'][1].mean()), 4)}
        if args.opt:
            per_links[str(n)]["mean_reward_optimal"] = round(float(books[n]['optimal'][1].mean()), 4)
    print(json.dumps({"mixed_links": args.mixed_links, "eval_links": args.eval_links, "envs_per_size": args.envs,
                      "checkpoints": tags, "trials": args.trials, "test_steps": args.test_steps, "epsilon": args.epsilon,
                      "eval_backend": args.eval_backend, "trajectory_walk": args.mixed_trajectory_walk,
                      "episodes_by_path": dict(agent.eval_stats), "per_links": per_links}))
    agent.close()
    return 0


def main(argv=None):
    ap, args = parse_args(argv)
    if args.mixed_links is not None:
        if args.sweep:
            ap.error("--sweep is the single-size path's (--links): --mixed-links always scores all checkpoints on one episode")
        return run_mixed(ap, args)
    if args.sweep and args.eval_backend == "device" and args.links <= 31:
        ap.error("--sweep --eval-backend device needs more than 31 links (the receiver form); --mixed-links scores the checkpoints "
                 "of a shared-weight network at 3..31 links on the GPU")
    if args.links < 4 or args.links % 4:
        ap.error("--links must be a multiple of 4 and at least 4 (got %d)" % args.links)
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)
    env = evaluation_env(ap, args)
    agent = Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, seed=args.seed, device_replay=False,
                  trajectory_walk=args.trajectory_walk, trajectory_streams=args.trajectory_streams,
                  receiver_streams=args.receiver_streams, receiver_words=args.receiver_words)
    evaluate = agent.evaluate_training_sweep if args.sweep else agent.evaluate_training_diff_trials
    out = evaluate(args.episodes, args.test_steps, args.opt, args.epsilon, args.trials, model_dir=args.save_dir,
                   num_train_steps=args.train_steps, opt_backend=args.opt_backend, opt_restarts=args.opt_restarts,
                   eval_backend=args.eval_backend)
    ret, ra = (out[0], out[2]) if args.opt else (out[1], out[3])
    summary = {"links": args.links, "checkpoints": int(ret.shape[1]), "trials": args.trials,
               "mean_return_per_checkpoint": [round(float(v), 4) for v in ret.mean(axis=0)],
               "mean_return_random": round(float(ra.mean()), 4)}
    if args.opt:
        summary["mean_return_optimal"] = round(float(out[4].mean()), 4)
    else:
        summary["optimal_return_per_trial"] = [round(float(v), 4) for v in out[0]]
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
