"""GPU: the counting branch and bound (v2x_opt_count_bound through OptimalAllocation.count_better / rank_of(backend='bound'),
csrc/v2xopt.hip) against the reward landscape (v2x_opt_landscape: every joint action walked, existing code) where that can be
walked -- integer equality, no tolerance --, against itself between stacked and single-state calls and between two runs, and at
20 links x 4 channels against the optimum of search_bound."""
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import rank_edges, rank_from_counts
from v2xgnn.rl.train import start_env
from test_gpu_eval_device import _run
from test_gpu_optimum import W_V2I, W_V2V, Stack, make_state
from test_rl_agent import RecordingBrain
from test_rl_env import make_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    return OptimalAllocation()


def seeded_env(n, seed):
    random.seed(seed)
    np.random.seed(seed)
    return start_env(n)


def five_thresholds(opt, env, n, rb, seed):
    """-> (actions [1, 4, n], thresholds [1, 5]): the best, the median and the worst of 64 local optima and a random action, as
    rewards_of scores them, and 0.97 x the best local optimum"""
    _, _, all_a, all_r = opt.search_local(env, W_V2V, W_V2I, restarts=64, seed=seed, all_restarts=True)
    order = np.argsort(all_r[0], kind='stable')
    rnd = np.random.default_rng(seed).integers(0, rb, size=n)
    actions = np.stack([all_a[0, order[-1]], all_a[0, order[32]], all_a[0, order[0]], rnd])[None]
    r = opt.rewards_of(env, W_V2V, W_V2I, actions)
    return actions, np.concatenate([r, 0.97 * r[:, :1]], axis=1)


def truth(opt, env, th):
    """(better, equal) of thresholds [E, A] from the landscape over the edges { v, nextafter(v) }"""
    edges = rank_edges(th)
    counts, _ = opt.landscape(env, W_V2V, W_V2I, edges)
    return rank_from_counts(counts, edges, th)


@pytest.fixture(scope="module")
def twelve(opt):
    """one 12 x 4 state, its five thresholds, the landscape's counts and ONE count_better call with the default budget"""
    env = seeded_env(12, 1)
    actions, th = five_thresholds(opt, env, 12, 4, 1)
    better, equal = truth(opt, env, th)
    return dict(env=env, actions=actions, th=th, better=better, equal=equal, got=opt.count_better(env, W_V2V, W_V2I, th))


def check_exact(got, better, equal):
    assert got['better'].dtype == np.int64 and got['equal'].dtype == np.int64 and got['exact'].dtype == bool
    assert got['better'].shape == better.shape and got['open'].shape == better.shape
    assert got['exact'].all() and all(o == 0 for o in got['open'].reshape(-1))
    assert np.array_equal(got['better'], better), (got['better'], better)
    assert np.array_equal(got['equal'], equal), (got['equal'], equal)


def test_eight_links_match_the_landscape(opt):
    env = seeded_env(8, 2)
    actions, th = five_thresholds(opt, env, 8, 4, 2)
    better, equal = truth(opt, env, th)
    got = opt.count_better(env, W_V2V, W_V2I, th)
    print("8 x 4: better", got['better'][0].tolist(), "equal", got['equal'][0].tolist(), "nodes", got['nodes_visited'])
    check_exact(got, better, equal)
    assert better[0, 0] <= better[0, 1] <= better[0, 2] and np.all(equal[0, :4] >= 1) and better[0, 4] >= better[0, 0]
    rk = opt.rank_of(env, W_V2V, W_V2I, actions, backend='bound')
    ref = opt.rank_of(env, W_V2V, W_V2I, actions)
    for k in ('better', 'equal'):
        assert rk[k].shape == (1, 4) and np.array_equal(rk[k], ref[k]), k
    assert rk['reward'].tobytes() == ref['reward'].tobytes() and rk['total'] == ref['total'] == 4 ** 8
    assert rk['mean_reward'] is None and rk['exact'].all()
    assert rk['better_max'].tolist() == rk['better'].tolist() and rk['equal_max'].tolist() == rk['equal'].tolist()
    one = opt.rank_of(env, W_V2V, W_V2I, actions[:, 0], backend='bound')                     # [E, n] actions -> [E] results
    assert one['better'].shape == (1,) and one['better'][0] == ref['better'][0, 0] and one['exact'].shape == (1,)


def test_twelve_links_match_the_landscape(opt, twelve):
    got = twelve['got']
    print("12 x 4: better", got['better'][0].tolist(), "equal", got['equal'][0].tolist(), "nodes", got['nodes_visited'])
    check_exact(got, twelve['better'], twelve['equal'])
    assert twelve['better'][0, 3] > 4 ** 12 // 100                     # the random action: the budget test's threshold is no easy one


@pytest.mark.parametrize("n,rb,seed", [(5, 16, 45), (3, 3, 1)])
def test_sixteen_and_three_channels_match_the_landscape(opt, n, rb, seed):
    """5 x 16: every child loop at its widest (nr = n < C: the V2I slots stop below the channels); 3 x 3: 27 leaves, one lane"""
    env = make_state(n, rb, seed)
    _, th = five_thresholds(opt, env, n, rb, seed)
    better, equal = truth(opt, env, th)
    check_exact(opt.count_better(env, W_V2V, W_V2I, th), better, equal)


@pytest.mark.parametrize("A", [1, 31])
def test_a_stacked_call_is_its_single_state_calls(opt, A):
    """6 states of 8 x 4 with a threshold row of their own: E * A root items, (state, slot) totals that must not mix"""
    envs = [seeded_env(8, 60 + e) for e in range(6)]
    stack = Stack(envs)
    rng = np.random.default_rng(A)
    th = opt.rewards_of(stack, W_V2V, W_V2I, rng.integers(0, 4, size=(6, A, 8)))
    assert th.shape == (6, A) and len({row.tobytes() for row in th}) == 6
    got = opt.count_better(stack, W_V2V, W_V2I, th)
    better, equal = truth(opt, stack, th)
    check_exact(got, better, equal)
    for e, env in enumerate(envs):
        one = opt.count_better(env, W_V2V, W_V2I, th[e])
        assert one['better'].shape == (1, A) and one['exact'].all()
        assert np.array_equal(one['better'][0], got['better'][e]) and np.array_equal(one['equal'][0], got['equal'][e]), e


def test_two_runs_count_the_same(opt, twelve):
    again = opt.count_better(twelve['env'], W_V2V, W_V2I, twelve['th'])
    print("nodes", twelve['got']['nodes_visited'], again['nodes_visited'])
    assert np.array_equal(again['better'], twelve['got']['better']) and np.array_equal(again['equal'], twelve['got']['equal'])
    assert again['exact'].all()


def test_ties_and_the_two_ends_of_the_landscape(opt):
    env = seeded_env(8, 3)
    _, best = opt.search(env, W_V2V, W_V2I)
    th = np.array([best[0], np.nextafter(best[0], np.inf), -1.0, np.inf, -np.inf])
    got = opt.count_better(env, W_V2V, W_V2I, th)
    assert got['exact'].all()
    assert got['better'][0, 0] == 0 and got['equal'][0, 0] >= 1                 # the optimum itself: nothing above, itself at
    assert got['better'][0, 1] == 0 and got['equal'][0, 1] == 0                 # one ulp above the optimum: nothing
    for k in (2, 4):                                                            # below every reward: nothing is pruned, 4^8 leaves
        assert got['better'][0, k] == 4 ** 8 and got['equal'][0, k] == 0
    assert got['better'][0, 3] == 0 and got['equal'][0, 3] == 0
    assert got['nodes_visited'] >= 2 * (4 ** 8)
    r = opt.rewards(env, W_V2V, W_V2I)[0]
    assert got['equal'][0, 0] == np.sum(r == best[0])


def test_a_spent_budget_ends_in_a_bracket_that_holds_the_truth(opt, twelve):
    """12 x 4, the random action's threshold, 1000 nodes: V2X_EBUDGET inside, a bracket outside; the same call with the default
    budget (the fixture's) is exact"""
    env, th = twelve['env'], twelve['th'][:, 3:4]
    got = opt.count_better(env, W_V2V, W_V2I, th, max_nodes=1000)
    better, equal, opened = int(got['better'][0, 0]), int(got['equal'][0, 0]), got['open'][0, 0]
    print("budget 1000: nodes", got['nodes_visited'], "better", better, "equal", equal, "open", opened)
    assert not got['exact'][0, 0] and opened > 0 and got['nodes_visited'] >= 1000
    assert better <= twelve['better'][0, 3] <= better + opened
    assert equal <= twelve['equal'][0, 3] <= equal + opened
    assert better + equal + opened <= 4 ** 12
    rk = opt.rank_of(env, W_V2V, W_V2I, twelve['actions'][:, 3], backend='bound', max_nodes=1000)
    assert not rk['exact'][0] and rk['better'][0] <= twelve['better'][0, 3] <= rk['better_max'][0]
    assert rk['equal'][0] <= twelve['equal'][0, 3] <= rk['equal_max'][0]
    # the return code itself, through the C ABI
    import ctypes
    import torch
    from v2xgnn.lib import V2X_EBUDGET
    from v2xgnn.rl.optimum import MAX_INDEX
    prob, E, n, rb = opt._setup(env, W_V2V, W_V2I, MAX_INDEX, 1000, n_thr=1)
    dev = torch.from_numpy(np.ascontiguousarray(th)).to(opt.device)
    outs = [torch.full((1, 1), -1, dtype=torch.int64, device=opt.device) for _ in range(4)]
    nodes = ctypes.c_int64(0)
    rc = opt._lib.v2x_opt_count_bound(ctypes.byref(prob), opt._ws.data_ptr(), dev.data_ptr(), 1, 1000, *[o.data_ptr() for o in outs],
                                      ctypes.byref(nodes), opt._stream())
    assert rc == V2X_EBUDGET and b"node budget spent at 12 links x 4 channels" in opt._lib.v2x_last_error(None)
    assert nodes.value >= 1000 and outs[2].item() == 0 and outs[3].item() > 0
    # a NaN threshold on the device is refused by the library (the host wrapper refuses a host array before)
    dev[0, 0] = float('nan')
    with pytest.raises(ValueError, match="not a number"):
        opt.count_better_device(env, W_V2V, W_V2I, dev)
    # the same call with the default budget
    assert twelve['got']['exact'][0, 3] and twelve['got']['better'][0, 3] == twelve['better'][0, 3]


@pytest.fixture(scope="module")
def twenty(opt):
    env = seeded_env(20, 0)
    index, best = opt.search_bound(env, W_V2V, W_V2I)
    return env, index, best


def test_twenty_links_the_optimum_has_nothing_above_it(opt, twenty):
    env, index, best = twenty
    got = opt.count_better(env, W_V2V, W_V2I, [best[0], np.nextafter(best[0], -np.inf)])
    print("20 x 4: better", got['better'][0].tolist(), "equal", got['equal'][0].tolist(), "nodes", got['nodes_visited'])
    assert got['exact'].all()
    assert got['better'][0, 0] == 0 and got['equal'][0, 0] >= 1
    assert got['better'][0, 1] >= 1 and got['better'][0, 1] == got['equal'][0, 0]          # one ulp below: exactly the optima
    rk = opt.rank_of(env, W_V2V, W_V2I, opt.decode(index, 20, 4), backend='bound')
    assert rk['better'][0] == 0 and rk['equal'][0] == got['equal'][0, 0] and rk['exact'][0] and rk['total'] == 4 ** 20
    assert rk['reward'][0].tobytes() == best[0].tobytes() and rk['mean_reward'] is None


def test_twenty_links_one_node_leaves_everything_open(opt, twenty):
    """threshold 0 prunes nothing; with max_nodes = 1 the call stops after its first round: what was not counted is open"""
    got = opt.count_better(twenty[0], W_V2V, W_V2I, [0.0], max_nodes=1)
    better, equal, opened = int(got['better'][0, 0]), int(got['equal'][0, 0]), got['open'][0, 0]
    print("20 x 4, one node: nodes", got['nodes_visited'], "better", better, "equal", equal, "open", opened)
    assert not got['exact'][0, 0] and better >= 0 and equal == 0
    assert better + equal + opened == 4 ** 20                          # threshold 0 and positive rewards: nothing is pruned


def test_thirty_two_links_count_past_the_64_bit_index(opt):
    """32 x 4 = 2^64 joint actions: no 64-bit index (search_bound refuses), slots above the default 64 KiB of dynamic LDS, and
    an `open` that needs its high word.  Threshold 0 prunes nothing, +inf prunes the root."""
    env = seeded_env(32, 5)
    with pytest.raises(ValueError, match=r"4\^32"):
        opt.search_bound(env, W_V2V, W_V2I)
    got = opt.count_better(env, W_V2V, W_V2I, [0.0, np.inf], max_nodes=1)
    better, opened = int(got['better'][0, 0]), got['open'][0, 0]
    print("32 x 4, one node: nodes", got['nodes_visited'], "better", better, "open", opened)
    assert got['exact'].tolist() == [[False, True]] and opened >= 2 ** 63
    assert better + int(got['equal'][0, 0]) + opened == 4 ** 32
    assert got['better'][0, 1] == 0 and got['equal'][0, 1] == 0 and got['open'][0, 1] == 0
    rk = opt.rank_of(env, W_V2V, W_V2I, np.zeros((1, 32), int), backend='bound', max_nodes=1000)
    assert rk['total'] == 4 ** 32 and rk['better'][0] <= rk['better_max'][0] <= 4 ** 32 and rk['equal_max'][0] >= 1


def _host_agent(links):
    env = make_env()
    env.new_random_game(links)
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def _check_books(land, bound):
    for k in ('better', 'equal', 'ra_better', 'ra_equal'):
        assert bound[k].shape == (1, 3) and bound[k].dtype == np.int64 and np.array_equal(bound[k], land[k]), k
    assert bound['exact'].all() and bound['ra_exact'].all() and np.all(bound['equal'] >= 1)
    assert bound['total'].tolist() == land['total'].tolist() == [[4 ** 8] * 3]
    assert bound['better_max'].tolist() == bound['better'].tolist() and bound['ra_better_max'].tolist() == bound['ra_better'].tolist()
    assert not bound['uniform_mean_reward'].any() and np.all(land['uniform_mean_reward'] > 0)
    assert 'exact' not in land


def test_test_run_ranks_by_counting_what_the_landscape_ranks(opt):
    books, outs = [], []
    for backend in ('landscape', 'bound'):
        random.seed(4243)
        np.random.seed(4243)
        agent = _host_agent(8)
        outs.append(agent.test_run(1, 3, opt_rank=True, rank_backend=backend))
        books.append(agent.rank_book)
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    _check_books(*books)
    from v2xgnn.rl.run import rank_summary
    s = rank_summary(books[1])
    assert s["share_states_gnn_ranked_exactly"] == 1.0 == s["share_states_random_ranked_exactly"]
    assert s["median_share_better_gnn_exact_states"] == float(np.median(books[0]['better'] / 4.0 ** 8))


def test_test_run_on_the_device_ranks_by_counting_in_one_call():
    call = lambda backend: (lambda a: a.test_run(1, 3, False, opt_rank=True, eval_backend='device', rank_backend=backend))  # noqa: E731
    land, bound = _run(8, 32, call('landscape')), _run(8, 32, call('bound'))
    assert land['stats'] == bound['stats'] == {'device_episodes': 1, 'host_episodes': 0}
    for a, b in zip(land['out'], bound['out']):
        assert a.tobytes() == b.tobytes()
    _check_books(land['book'], bound['book'])
