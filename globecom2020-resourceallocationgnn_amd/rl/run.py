"""Evaluation driver: the counterpart of the reference's RL_Run_main.py (load_trained_model :105-148, run_test :151-)
-- load the weights a training run saved, then compare the greedy policy with the random-action baseline and
(optionally) the brute-force optimum.

    python -m v2xgnn.rl.train --links 4 --episodes 5 --train-steps 20 --batch 512 --save-dir runs/a
    python -m v2xgnn.rl.run   --links 4 --episodes 5 --train-steps 20 --batch 512 --save-dir runs/a \\
                              --test-episodes 10 --test-steps 50 --opt [--opt-backend device | bound | local] \\
                              [--opt-rank [--opt-rank-backend bound [--opt-rank-max-nodes N]]] \\
                              [--sim-backend device --sim-streams device --eval-backend device
                               [--trajectory-walk wide [--trajectory-streams split]]]
    python -m v2xgnn.rl.run   --links 100 --save-dir runs/b --opt --opt-backend local \\
                              --sim-backend device --sim-streams device --eval-backend device [--receiver-streams split [--receiver-words jump]]

A shared-weight network trained on several link counts at once (rl.train --mixed-links ... --save-dir D) is evaluated per link
count, on the training sizes or on others, --envs parallel episodes per size (rl/mixed.py MixedAgent.test_run):

    python -m v2xgnn.rl.run   --mixed-links 8,12,20 [--eval-links 8,16,28] [--envs 4] --feedback 64 --batch 4096 --train-steps 20 \\
                              --save-dir D [--opt --opt-backend device | bound | local] \\
                              [--sim-backend device --sim-streams device --eval-backend device [--mixed-trajectory-walk wide]]
"""
import argparse
import json
import os
import random

import numpy as np

from .agent import Agent
from .sim_config import RL_Config
from .train import start_env, start_env_batched


def weight_file_names(num_episodes, num_train_steps, batch_size):
    """The reference's naming scheme (BS_brain.py:859-868, RL_Run_main.py:135-141)."""
    tag = '-Episode-%d-Step-%d-Batch-%d.h5' % (num_episodes, num_train_steps, batch_size)
    return 'Q-Network_model_weights' + tag, 'Target-Network_model_weights' + tag


def load_trained_model(env, cfg, model_dir, brain=None, **brain_kwargs):
    """RL_Run_main.py:105-148"""
    agent = Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain, **brain_kwargs)
    online, target = weight_file_names(cfg.Num_Episodes, cfg.Num_Train_Steps, cfg.Batch_Size)
    agent.brain.model.load_weights(os.path.join(model_dir, online))
    agent.brain.target_model.load_weights(os.path.join(model_dir, target))
    return agent


RECEIVER_FORM_ABOVE = 31                                 # the packed observation's links (rl/device_sim.py OBSERVE_MAX_LINKS)


def add_sim_arguments(ap):
    """--sim-backend / --sim-streams / --sim-reset / --eval-backend / --trajectory-walk / --trajectory-streams /
    --receiver-streams / --receiver-words of the two evaluation drivers"""
    ap.add_argument("--sim-backend", choices=["host", "device"], default="host",
                    help="where the simulator's channel update, observation and rates run: the single host simulator (the "
                         "default) or ONE batched simulator on the GPU (rl/device_sim.py)")
    ap.add_argument("--sim-streams", choices=["host", "device"], default="host",
                    help="with --sim-backend device: where mobility and the simulator's MT19937 stream advance")
    ap.add_argument("--sim-reset", choices=["host", "device"], default="host",
                    help="with --sim-backend device --sim-streams device: who resets the simulator at the start of an episode -- "
                         "the host library (the default) or the GPU, one call on the state resident in HBM (v2x_sim_reset)")
    ap.add_argument("--eval-backend", choices=["host", "device"], default="host",
                    help="with --sim-backend device --sim-streams device: 'device' runs an evaluation episode as one call for "
                         "its steps and both schemes, one stacked optimum search and one rates call (Agent.test_run)")
    ap.add_argument("--trajectory-walk", choices=["serial", "wide"], default="serial",
                    help="with --eval-backend device: how the episode's steps are walked -- 'serial' (the default: one workgroup, "
                         "step after step) or 'wide' (the steps spread over the chip in four launches; the same bits)")
    ap.add_argument("--trajectory-streams", choices=["chain", "split"], default="chain",
                    help="with --trajectory-walk wide: the stream phase of the wide walk -- 'chain' (the default: one launch draws "
                         "the streams of all steps) or 'split' (raw words, offset walk and conversion in three launches; the same bits)")
    ap.add_argument("--receiver-streams", choices=["chain", "split"], default="chain",
                    help="with --eval-backend device beyond %d links (the episode then runs in receiver form and walks wide): its "
                         "stream phase -- 'chain' (the default) or 'split' (three launches on a second workspace; the same bits)"
                         % RECEIVER_FORM_ABOVE)
    ap.add_argument("--receiver-words", choices=["serial", "jump"], default="serial",
                    help="with --receiver-streams split: how the raw words are drawn -- 'serial' (the default: one workgroup per "
                         "simulator) or 'jump' (the words beyond a prefix in chunks entered by jump-ahead polynomials of MT19937, "
                         "spread over the chip; the same bits)")


def check_receiver_arguments(ap, args):
    """the checks of one link count (--links) that concern the receiver form: beyond 31 links --eval-backend device runs the
    episode as v2x_eval_steps_recv, whose stream phase is --receiver-streams; what that form cannot honour is refused with
    the option to use instead"""
    wide = args.links > RECEIVER_FORM_ABOVE
    if args.receiver_streams != "chain" and not (wide and args.eval_backend == "device"):
        ap.error("--receiver-streams %s needs --eval-backend device and more than %d links (the receiver form); at %d links the "
                 "option is --trajectory-walk wide --trajectory-streams %s"
                 % (args.receiver_streams, RECEIVER_FORM_ABOVE, args.links, args.receiver_streams))
    if args.receiver_words != "serial" and args.receiver_streams != "split":
        ap.error("--receiver-words %s needs --receiver-streams split (it draws the split stream phase's words in chunks)"
                 % args.receiver_words)
    if wide and args.eval_backend == "device" and args.trajectory_streams != "chain":
        ap.error("--trajectory-streams %s holds 3..%d links: at %d links the episode runs in receiver form, use "
                 "--receiver-streams %s" % (args.trajectory_streams, RECEIVER_FORM_ABOVE, args.links, args.trajectory_streams))


def evaluation_env(ap, args):
    """the simulator the evaluation drivers step: start_env(links) unless --sim-backend device asks for the batched one (E = 1);
    the argument errors are those of rl/train.py"""
    if args.sim_streams == "device" and args.sim_backend != "device":
        ap.error("--sim-streams device needs --sim-backend device")
    if args.sim_reset == "device" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--sim-reset device needs --sim-backend device --sim-streams device")
    if args.eval_backend != "host" and (args.sim_backend != "device" or args.sim_streams != "device"):
        ap.error("--eval-backend %s needs --sim-backend device --sim-streams device" % args.eval_backend)
    if args.trajectory_walk != "serial" and args.eval_backend != "device":
        ap.error("--trajectory-walk %s needs --eval-backend device" % args.trajectory_walk)
    if args.trajectory_streams != "chain" and args.trajectory_walk != "wide":
        ap.error("--trajectory-streams %s needs --trajectory-walk wide" % args.trajectory_streams)
    if args.sim_backend == "device":
        return start_env_batched(args.links, 1, args.seed, backend="device", streams=args.sim_streams, reset=args.sim_reset)
    return start_env(args.links)


def run_test(cfg, agent, opt_backend='host', opt_restarts=None, opt_rank=False, eval_backend='host', rank_backend='landscape',
             rank_max_nodes=None):
    """RL_Run_main.py:151-: -> dict of the test_run outputs plus the mean rewards per scheme.  opt_backend: where the
    optimum is searched ('host': numpy over every joint action; 'device' / 'bound': the GPU searches of rl/optimum.py;
    'local': its local search with opt_restarts restarts -- a lower bound on the optimum, not the optimum).  opt_rank: also
    rank every step's greedy and random action among all C^N joint actions of its state (agent.rank_book; rank_summary);
    rank_backend / rank_max_nodes: how ('landscape': C^N <= 2^36; 'bound': counting branch and bound, up to 32 links)."""
    out = agent.test_run(cfg.Num_Run_Episodes, cfg.Num_Test_Steps, cfg.Opt_Flag, opt_backend=opt_backend,
                         opt_restarts=opt_restarts, opt_rank=opt_rank, eval_backend=eval_backend, rank_backend=rank_backend,
                         rank_max_nodes=rank_max_nodes)
    names = ['Expect_Return', 'Reward', 'Per_V2V_Rate', 'Per_V2I_Rate', 'Per_V2B_Interference']
    res = {}
    for prefix, chunk in zip(('', 'RA_', 'Opt_'), (out[0:5], out[5:10], out[10:15])):
        for name, arr in zip(names, chunk):
            res[prefix + name] = arr
    return res


def rank_summary(book):
    """The --opt-rank entries of the JSON summary from Agent.rank_book."""
    total = book['total'].astype(np.float64)
    if 'exact' in book:                               # --opt-rank-backend bound: exact where the node budget sufficed, else a bracket
        out = {}
        for name, pre in (('gnn', ''), ('random', 'ra_')):
            exact = book[pre + 'exact']
            share = book[pre + 'better'][exact] / total[exact]
            upper = book[pre + 'better_max'][~exact].astype(np.float64) / total[~exact]
            out["share_states_%s_ranked_exactly" % name] = float(np.mean(exact))
            if name == 'gnn':
                out["share_exact_states_gnn_optimal"] = float(np.mean(book['better'][exact] == 0)) if exact.any() else None
            out["median_share_better_%s_exact_states" % name] = float(np.median(share)) if exact.any() else None
            out["median_upper_share_better_%s_bracketed_states" % name] = float(np.median(upper)) if (~exact).any() else None
        return out
    return {"share_states_gnn_optimal": float(np.mean(book['better'] == 0)),
            "median_share_better_gnn": float(np.median(book['better'] / total)),
            "median_share_better_random": float(np.median(book['ra_better'] / total)),
            "mean_reward_uniform_exact": float(book['uniform_mean_reward'].mean())}


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--feedback", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--episodes", type=int, default=1, help="episode count of the training run whose weights are loaded")
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--save-dir", required=True)
    ap.add_argument("--test-episodes", type=int, default=10)
    ap.add_argument("--test-steps", type=int, default=50)
    ap.add_argument("--opt", action="store_true", help="also run the brute-force optimum (C^N joint actions)")
    ap.add_argument("--opt-backend", choices=("host", "device", "bound", "local"), default=None,
                    help="where --opt searches: numpy on the host (the default; C^N <= 65536) or the GPU, exhaustively (device: "
                         "C^N <= 2^36; the default with --mixed-links) or by branch and bound (bound: up to 32 links, e.g. 20 x 4); "
                         "local: NOT the optimum but a lower bound on it, the best of --opt-restarts local searches on the GPU "
                         "(up to 128 links, e.g. 100 x 4)")
    ap.add_argument("--opt-restarts", type=int, default=None,
                    help="restarts per state of --opt-backend local (default: rl/optimum.py DEFAULT_LOCAL_RESTARTS)")
    ap.add_argument("--opt-rank", action="store_true",
                    help="rank every step's greedy and random action among ALL C^N joint actions of its state on the GPU "
                         "(C^N <= 2^36; with or without --opt, any --opt-backend) and add the shares to the summary")
    ap.add_argument("--opt-rank-backend", choices=("landscape", "bound"), default="landscape",
                    help="how --opt-rank counts: the whole reward landscape (C^N <= 2^36) or counting branch and bound (bound: up "
                         "to 32 links, e.g. 20 x 4; exact for a good allocation, a certified bracket where the budget runs out)")
    ap.add_argument("--opt-rank-max-nodes", type=int, default=None,
                    help="node budget per ranked step of --opt-rank-backend bound (default: rl/optimum.py DEFAULT_RANK_MAX_NODES)")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--mixed-links", default=None, metavar="N1,N2,...",
                    help="evaluate the shared-weight network rl.train --mixed-links N1,N2,... saved (rl/mixed.py): the training "
                         "sizes, used only to find the files; --links is ignored")
    ap.add_argument("--eval-links", default=None, metavar="M1,M2,...",
                    help="with --mixed-links: the link counts to evaluate on (distinct multiples of 4 up to 28, at most 8; "
                         "default: the training sizes)")
    ap.add_argument("--envs", type=int, default=1,
                    help="with --mixed-links: simulators per evaluated link count, each a parallel episode (default 1)")
    ap.add_argument("--mixed-trajectory-walk", choices=["serial", "wide"], default="serial",
                    help="with --mixed-links --eval-backend device: how an episode's steps are walked -- 'serial' (the default: one "
                         "workgroup per simulator, step after step) or 'wide' (the steps of all link counts spread over the chip, "
                         "six launches in the walk's place; the same bits)")
    add_sim_arguments(ap)
    return ap


def parse_args(argv=None):
    """the command line, parsed, with every check that concerns --mixed-links made (a refusal exits with its message)
    -> (parser, arguments); arguments.mixed_links / eval_links are then sorted lists of link counts (or None)"""
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
    if args.opt_rank:
        ap.error("--mixed-links has no ranks: --opt-rank ranks the actions of one link count (rl.run --links)")
    if args.receiver_streams != "chain":
        ap.error("--mixed-links holds 3..31 links: --receiver-streams is the stream phase of one link count beyond 31 (rl.run --links)")
    if args.receiver_words != "serial":
        ap.error("--mixed-links holds 3..31 links: --receiver-words draws the words of one link count beyond 31 (rl.run --links)")
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


def run_mixed(args):
    """--mixed-links: load the two networks rl.train --mixed-links saved and evaluate them on --eval-links, --envs parallel
    episodes per link count (MixedAgent.test_run) -> the JSON summary, per link count the mean rewards per scheme"""
    from .mixed import MixedAgent
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)
    envs = [start_env_batched(n, args.envs, args.seed + 15485863 * k, backend=args.sim_backend, streams=args.sim_streams,
                              reset=args.sim_reset)
            for k, n in enumerate(args.eval_links)]
    agent = MixedAgent(envs, cfg, args.feedback, seed=args.seed, trajectory_walk=args.mixed_trajectory_walk)
    agent.load_weights(args.save_dir, args.episodes, args.train_steps)
    books = agent.test_run(envs, args.test_episodes, args.test_steps, opt_flag=args.opt, opt_backend=args.opt_backend,
                           opt_restarts=args.opt_restarts, eval_backend=args.eval_backend)
    per_links = {}
    for n in args.eval_links:
        per_links[str(n)] = {"mean_reward_gnn": float(books[n]['gnn'][1].mean()),
                             "mean_reward_random": float(books[n]['random'][1].mean())}
        if args.opt:
            per_links[str(n)]["mean_reward_optimal"] = float(books[n]['optimal'][1].mean())
    print(json.dumps({"mixed_links": args.mixed_links, "eval_links": args.eval_links, "envs_per_size": args.envs,
                      "test_episodes": args.test_episodes, "test_steps": args.test_steps, "eval_backend": args.eval_backend,
                      "trajectory_walk": args.mixed_trajectory_walk, "episodes_by_path": dict(agent.eval_stats), "per_links": per_links}))
    agent.close()
    return 0


def main(argv=None):
    ap, args = parse_args(argv)
    if args.mixed_links is not None:
        return run_mixed(args)
    if args.links < 4 or args.links % 4:
        # the simulator drops vehicles in groups of four, one per direction (Environment.py:217-231), and the
        # observation divides by links - 2 (BS_brain.py:405)
        ap.error("--links must be a multiple of 4 and at least 4 (got %d)" % args.links)
    random.seed(args.seed)
    np.random.seed(args.seed)
    cfg = RL_Config()
    cfg.set_train_value(args.feedback, args.gamma, args.batch, 1, 0.1)
    cfg.Num_Episodes, cfg.Num_Train_Steps = args.episodes, args.train_steps
    cfg.set_test_values(args.test_episodes, args.test_steps, args.opt, 1, 0.1)
    env = evaluation_env(ap, args)
    agent = load_trained_model(env, cfg, args.save_dir, seed=args.seed, trajectory_walk=args.trajectory_walk,
                               trajectory_streams=args.trajectory_streams, receiver_streams=args.receiver_streams,
                               receiver_words=args.receiver_words)
    res = run_test(cfg, agent, opt_backend=args.opt_backend, opt_restarts=args.opt_restarts, opt_rank=args.opt_rank,
                   eval_backend=args.eval_backend, rank_backend=args.opt_rank_backend, rank_max_nodes=args.opt_rank_max_nodes)
    summary = {"links": args.links, "test_episodes": args.test_episodes, "test_steps": args.test_steps,
               "mean_reward_gnn": float(res['Reward'].mean()), "mean_reward_random": float(res['RA_Reward'].mean())}
    if args.opt:
        summary["mean_reward_optimal"] = float(res['Opt_Reward'].mean())
    if args.opt_rank:
        summary.update(rank_summary(agent.rank_book))
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
