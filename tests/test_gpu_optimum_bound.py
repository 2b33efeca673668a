"""GPU: the branch-and-bound optimal-allocation search (OptimalAllocation.search_bound, v2x_opt_search_bound of
csrc/v2xopt.hip).  The reference of every comparison is the exhaustive search (search / rewards), never the code under
test: bitwise equal (index, reward) wherever the exhaustive search can go, and at 20 links x 4 RBs -- which it refuses --
the optimum's reward against v2x_opt_rewards of its own index, of every joint action one or two links away and of 10^5
seeded random ones."""
import itertools
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, BoundBudgetExceeded, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import decode
from test_gpu_optimum import Stack, make_state
from test_rl_agent import RecordingBrain
from test_rl_env import make_env

pytestmark = pytest.mark.gpu

W_V2V, W_V2I = 1.0, 0.1


def _same(opt, env, w_v2v=W_V2V, w_v2i=W_V2I):
    """search_bound == search, bit for bit, in every state of env"""
    want_i, want_r = opt.search(env, w_v2v, w_v2i)
    got_i, got_r = opt.search_bound(env, w_v2v, w_v2i)
    print("exhaustive", want_i.tolist()[:4], want_r.tolist()[:4], "bound", got_i.tolist()[:4], got_r.tolist()[:4],
          "nodes", opt.nodes_visited)
    assert got_i.dtype == np.int64 and got_r.dtype == np.float64 and got_i.shape == want_i.shape
    assert np.array_equal(got_i, want_i)
    assert got_r.tobytes() == want_r.tobytes()
    assert opt.nodes_visited >= got_i.size
    return got_i, got_r


@pytest.mark.parametrize("n,rb", [(4, 4), (8, 4), (12, 4), (5, 3), (3, 6), (2, 2), (8, 16)])
def test_bound_equals_exhaustive_search_bitwise(n, rb):
    """(5, 3): min(C, N) = C V2I terms; (3, 6): min(C, N) = N; (8, 16): 144 slots per lane, 83 KiB of LDS with
    the table -- above the 64 KiB a launch gets by default; (2, 2): the smallest sizes."""
    opt = OptimalAllocation()
    for seed in range(3 if n < 12 and rb < 16 else 1):
        _same(opt, make_state(n, rb, 300 * n + rb + seed))


def test_bound_equals_exhaustive_search_on_fifty_batched_states():
    opt = OptimalAllocation()
    envs = [make_state(8, 4, 5000 + s) for s in range(50)]
    index, _ = _same(opt, Stack(envs))
    assert index.shape == (50,) and len(set(index.tolist())) > 25


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bound_equals_exhaustive_search_at_sixteen_links(seed):
    _same(OptimalAllocation(), make_state(16, 4, 1600 + seed))


def test_bound_on_the_batched_simulator():
    from v2xgnn.rl.train import start_env_batched
    env = start_env_batched(8, 8, seed=31, lookahead=False)
    _same(OptimalAllocation(), env)


def test_interchangeable_channels_take_the_lowest_index():
    """8 links, w_v2i = 0, RBs 0 and 1 made interchangeable for every link (equal columns of the V2V gains, and the V2I
    transmitters of the two RBs -- vehicles 0 and 1 -- equal as interferers): swapping the labels 0 and 1 in a joint
    action leaves every sum's terms and their order unchanged, so each action has a twin with the same reward bits.  The
    optimum is such a pair; the lower index must win, as in the exhaustive search."""
    n, rb = 8, 4
    env = make_state(n, rb, 77)
    g = env.V2V_channels_with_fastfading
    g[1, :, :] = g[0, :, :]
    g[:, :, 1] = g[:, :, 0]
    opt = OptimalAllocation()
    index, reward = _same(opt, env, 1.0, 0.0)
    a = decode(index, n, rb)[0]
    twin = np.where(a == 0, 1, np.where(a == 1, 0, a))
    twin_index = int(sum(int(d) * rb ** (n - 1 - l) for l, d in enumerate(twin)))
    assert twin_index != int(index[0]), "the optimum uses neither RB 0 nor RB 1: the construction shows nothing"
    twin_reward = opt.rewards(env, 1.0, 0.0, twin_index, 1)[0, 0]
    assert twin_reward.tobytes() == reward[0].tobytes()                        # an exact tie ...
    assert int(index[0]) < twin_index                                          # ... and the lower index won


def test_all_gains_equal_take_the_lowest_index():
    """Every gain equal and w_v2i = 0 (the construction of test_gpu_optimum.test_exact_ties_take_the_lowest_index at
    8 links x 4 RBs): thousands of joint actions share the best reward exactly, and none of them may be pruned."""
    env = make_state(8, 4, 7)
    env.V2V_channels_with_fastfading = np.full_like(env.V2V_channels_with_fastfading, 80.0)
    env.V2I_channels_with_fastfading = np.full_like(env.V2I_channels_with_fastfading, 80.0)
    env.V2I_channels_abs = np.full_like(env.V2I_channels_abs, 80.0)
    opt = OptimalAllocation()
    index, reward = _same(opt, env, 1.0, 0.0)
    vec = opt.rewards(env, 1.0, 0.0)[0]
    assert np.count_nonzero(vec == reward[0]) > 100 and int(np.argmax(vec)) == int(index[0])


def _headline_state(seed):
    random.seed(seed)
    np.random.seed(seed)
    env = make_env()
    env.new_random_game(20)
    return env


def _index(actions, rb):
    n = actions.shape[-1]
    w = rb ** np.arange(n - 1, -1, -1, dtype=np.int64)
    return (actions.astype(np.int64) * w).sum(axis=-1)


_HEADLINE = {}


def _headline(seed):
    """(env, opt, index, reward) of one 20-link state, searched once per session with the default budget"""
    if seed not in _HEADLINE:
        env = _headline_state(seed)
        opt = OptimalAllocation()
        index, reward = opt.search_bound(env, W_V2V, W_V2I)
        print("seed", seed, "index", int(index[0]), "reward", float(reward[0]), "nodes", opt.nodes_visited)
        _HEADLINE[seed] = (env, opt, index, reward)
    return _HEADLINE[seed]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twenty_links_optimum_is_its_own_reward_and_no_neighbour_or_sample_beats_it(seed):
    n, rb = 20, 4
    env, opt, index, reward = _headline(seed)
    assert index.shape == (1,) and 0 <= int(index[0]) < rb ** n and np.isfinite(reward[0]) and reward[0] > 0
    own = opt.rewards(env, W_V2V, W_V2I, int(index[0]), 1)
    assert own[0, 0].tobytes() == reward[0].tobytes()
    best = decode(index, n, rb)[0]
    # every joint action that differs from the optimum in one link (20 * 3) or in two (C(20, 2) * 9)
    near = []
    for l in range(n):
        for c in range(rb):
            if c != best[l]:
                a = best.copy()
                a[l] = c
                near.append(a)
    assert len(near) == 60
    for l, k in itertools.combinations(range(n), 2):
        for c in range(rb):
            for c2 in range(rb):
                if c != best[l] and c2 != best[k]:
                    a = best.copy()
                    a[l], a[k] = c, c2
                    near.append(a)
    assert len(near) == 60 + 1710
    worst_gap = np.inf
    for i in _index(np.array(near), rb):
        r = opt.rewards(env, W_V2V, W_V2I, int(i), 1)[0, 0]
        worst_gap = min(worst_gap, reward[0] - r)
        assert r <= reward[0], (int(i), r, reward[0])
    print("closest neighbour below the optimum by", worst_gap)
    # 10^5 seeded random joint actions: 1000 random range starts x 100 consecutive indices each
    rng = np.random.default_rng(2000 + seed)
    top = -np.inf
    for first in rng.integers(0, rb ** n - 100, size=1000):
        top = max(top, float(opt.rewards(env, W_V2V, W_V2I, int(first), 100).max()))
    print("best of 1e5 random joint actions", top, "optimum", float(reward[0]))
    assert top <= reward[0]


def test_twenty_links_twice_gives_the_same_pair():
    for seed in (0, 1, 2):
        env, opt, index, reward = _headline(seed)
        again_i, again_r = OptimalAllocation().search_bound(_headline_state(seed), W_V2V, W_V2I)
        assert np.array_equal(again_i, index) and again_r.tobytes() == reward.tobytes()


def test_spent_budget_raises_with_the_best_found_and_the_object_stays_usable():
    env, _, index, reward = _headline(0)
    opt = OptimalAllocation()
    with pytest.raises(BoundBudgetExceeded, match=r"20 links x 4 channels.* nodes visited") as info:
        opt.search_bound(env, W_V2V, W_V2I, max_nodes=1000)
    exc = info.value
    print("budget 1000:", exc, exc.index, exc.reward)
    assert exc.nodes_visited >= 1000 and exc.index.shape == (1,) and 0 <= int(exc.index[0]) < 4 ** 20
    assert np.isfinite(exc.reward[0]) and 0 < exc.reward[0] <= reward[0]
    own = opt.rewards(env, W_V2V, W_V2I, int(exc.index[0]), 1)
    assert own[0, 0].tobytes() == exc.reward[0].tobytes()
    again_i, again_r = opt.search_bound(env, W_V2V, W_V2I)
    assert np.array_equal(again_i, index) and again_r.tobytes() == reward.tobytes()


def _agent(env, n):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(n, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(n, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_test_run_bound_backend_equals_device_backend_at_eight_links():
    outs = []
    for backend in ('device', 'bound'):
        random.seed(808)
        np.random.seed(808)
        env = make_env()
        env.new_random_game(8)
        outs.append(_agent(env, 8).test_run(1, 2, True, opt_backend=backend))
    for d, b in zip(*outs):
        assert np.array_equal(d, b)


def test_test_run_at_twenty_links_dominates_both_policies():
    """the evaluation driver at the headline size: the optimum of every step is at least what either policy earned"""
    random.seed(2020)
    np.random.seed(2020)
    env = make_env()
    env.new_random_game(20)
    out = _agent(env, 20).test_run(1, 2, True, opt_backend='bound')
    rl, ra, opt = out[1], out[6], out[11]
    assert np.all(opt > 0)
    assert np.all(opt >= np.maximum(rl, ra) * (1 - 1e-12))
