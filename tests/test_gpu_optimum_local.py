"""GPU: the multi-start local search for a near-optimal channel allocation (OptimalAllocation.search_local, rewards_of,
search_bound(incumbent=), opt_backend='local'; v2x_opt_search_local / v2x_opt_rewards_actions / v2x_opt_search_bound_seeded
of csrc/v2xopt.hip).  The reference of every comparison is the exhaustive search, the unseeded bound search,
v2x_opt_rewards, numpy or the simulator's own reward -- never the code under test."""
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import decode, encode, local_start
from test_gpu_optimum import Stack, landscape, make_state
from test_rl_agent import RecordingBrain
from test_rl_env import make_env

pytestmark = pytest.mark.gpu

W_V2V, W_V2I = 1.0, 0.1
TOL = 1e-12


def _tol(r):
    return TOL * np.maximum(1.0, np.abs(r))


def _game(n, seed):
    random.seed(seed)
    np.random.seed(seed)
    env = make_env()
    env.new_random_game(n)
    return env


def _env_reward(env, action):
    v2v, v2i, _ = env.compute_reward_with_channel_selection(np.asarray(action).reshape(len(env.vehicles), 1))
    return W_V2V * np.sum(v2v) + W_V2I * np.sum(v2i)


# ------------------------------------------------------------------------------------------------------- 3. scoring
@pytest.mark.parametrize("n,rb", [(4, 4), (5, 3), (8, 16), (12, 4), (20, 4)])
def test_rewards_of_equals_the_indexed_rewards_bitwise(n, rb):
    env = make_state(n, rb, 700 * n + rb)
    opt = OptimalAllocation()
    rng = np.random.default_rng(n * 100 + rb)
    actions = rng.integers(0, rb, size=(1, 1000, n))
    actions[0, 0], actions[0, 1] = 0, rb - 1
    got = opt.rewards_of(env, W_V2V, W_V2I, actions)
    assert got.shape == (1, 1000) and got.dtype == np.float64
    idx = encode(actions, rb)[0]
    want = np.array([opt.rewards(env, W_V2V, W_V2I, int(i), 1)[0, 0] for i in idx])
    assert got[0].tobytes() == want.tobytes()
    ref = landscape(env, idx=idx)
    print(n, rb, "max |rewards_of - numpy|", np.abs(got[0] - ref).max())
    assert np.all(np.abs(got[0] - ref) <= _tol(ref))
    one = opt.rewards_of(env, W_V2V, W_V2I, actions[:, 7])                     # [E, n] -> [E]
    assert one.shape == (1,) and one[0].tobytes() == got[0, 7].tobytes()


@pytest.mark.parametrize("n", [100, 128])
def test_rewards_of_matches_the_simulator_beyond_thirty_two_links(n):
    env = _game(n, 40 + n)
    opt = OptimalAllocation()
    rng = np.random.default_rng(n)
    actions = rng.integers(0, 4, size=(1, 32, n))
    got = opt.rewards_of(env, W_V2V, W_V2I, actions)[0]
    want = np.array([_env_reward(env, a) for a in actions[0]])
    print(n, "max |rewards_of - simulator|", np.abs(got - want).max(), "rewards", want.min(), want.max())
    assert np.all(np.abs(got - want) <= _tol(want))


def test_a_device_action_outside_the_channels_scores_nan():
    import torch
    env = make_state(8, 4, 3)
    opt = OptimalAllocation()
    good = np.array([[[0, 1, 2, 3, 0, 1, 2, 3], [1, 1, 1, 1, 2, 2, 2, 2], [3, 3, 3, 3, 3, 3, 3, 3]]])
    want = opt.rewards_of(env, W_V2V, W_V2I, good)
    bad = good.copy()
    bad[0, 1, 5] = 4
    dev = torch.from_numpy(bad.astype(np.int32)).to(opt.device)
    got = opt.rewards_of_device(env, W_V2V, W_V2I, dev).cpu().numpy()
    assert np.isnan(got[0, 1]) and got[0, 0].tobytes() == want[0, 0].tobytes() and got[0, 2].tobytes() == want[0, 2].tobytes()


# ------------------------------------------------------------------------------------------- 4 / 5. what a result is
def _states(n, rb, count):
    if rb == 4 and n % 4 == 0:
        return [_game(n, 900 + 10 * n + s) for s in range(count)]
    return [make_state(n, rb, 900 + 10 * n + s) for s in range(count)]


def _numpy_winner(all_actions, all_rewards):
    """(larger reward, else lexicographically lower action) over one state's restarts"""
    best = np.flatnonzero(all_rewards == all_rewards.max())
    return min(best, key=lambda r: tuple(all_actions[r]))


_RESULTS = {}


def _result(n, rb):
    """one state and five stacked, searched once per session: (envs, opt, single, stacked)"""
    if (n, rb) not in _RESULTS:
        envs = _states(n, rb, 5)
        opt = OptimalAllocation()
        single = opt.search_local(envs[0], W_V2V, W_V2I, all_restarts=True)
        info1 = opt.local_info.copy()
        stacked = opt.search_local(Stack(envs), W_V2V, W_V2I, all_restarts=True)
        info5 = opt.local_info.copy()
        _RESULTS[(n, rb)] = (envs, opt, single + (info1,), stacked + (info5,))
    return _RESULTS[(n, rb)]


SIZES = [(8, 4), (12, 4), (20, 4), (100, 4), (128, 16)]


@pytest.mark.parametrize("n,rb", SIZES)
def test_a_result_is_the_best_restart_scored_from_scratch(n, rb):
    envs, opt, single, stacked = _result(n, rb)
    for env, (actions, reward, all_a, all_r, info) in ((envs[0], single), (Stack(envs), stacked)):
        E = reward.shape[0]
        R = all_r.shape[1]
        assert actions.shape == (E, n) and actions.dtype == np.int64 and reward.dtype == np.float64
        assert all_a.shape == (E, R, n) and all_r.shape == (E, R) and info.shape == (E, 2) and R == 1024
        assert actions.min() >= 0 and actions.max() < rb and all_a.min() >= 0 and all_a.max() < rb
        assert reward.tobytes() == opt.rewards_of(env, W_V2V, W_V2I, actions).tobytes()
        assert all_r.tobytes() == opt.rewards_of(env, W_V2V, W_V2I, all_a).tobytes()
        assert np.all(info[:, 1] == 1), "not converged within the default max_sweeps"
        for e in range(E):
            w = _numpy_winner(all_a[e], all_r[e])
            assert np.array_equal(actions[e], all_a[e, w]) and reward[e].tobytes() == all_r[e, w].tobytes()
            assert np.array_equal(all_a[e, info[e, 0]], actions[e])
        print(n, rb, "E", E, "reward", reward.tolist(), "restarts at the winner",
              [int(np.count_nonzero(all_r[e] == reward[e])) for e in range(E)])
    # a stacked state's result is its single-state result; the simulator agrees with the reward
    assert np.array_equal(stacked[0][0], single[0][0]) and stacked[1][0].tobytes() == single[1][0].tobytes()
    assert stacked[2][0].tobytes() == single[2][0].tobytes() and stacked[3][0].tobytes() == single[3][0].tobytes()
    if rb == 4:
        for e, env in enumerate(envs):
            want = _env_reward(env, stacked[0][e])
            assert abs(want - stacked[1][e]) <= _tol(want)


@pytest.mark.parametrize("n,rb", SIZES)
def test_two_runs_are_identical_and_the_plain_call_equals_all_restarts(n, rb):
    envs, opt, single, stacked = _result(n, rb)
    again = OptimalAllocation()
    actions, reward = again.search_local(Stack(envs), W_V2V, W_V2I)
    assert np.array_equal(actions, stacked[0]) and reward.tobytes() == stacked[1].tobytes()
    assert np.array_equal(again.local_info, stacked[4])
    a1, r1 = again.search_local(envs[0], W_V2V, W_V2I)
    assert np.array_equal(a1, single[0]) and r1.tobytes() == single[1].tobytes()


def test_restarts_start_where_local_start_says():
    """max_sweeps = 1 at w = 0: no candidate is strictly better than the current total (all 0), so nothing moves and every
    restart returns its start."""
    env = make_state(8, 4, 11)
    opt = OptimalAllocation()
    for seed in (0, 7):
        _, _, all_a, all_r = opt.search_local(env, 0.0, 0.0, restarts=40, seed=seed, max_sweeps=1, all_restarts=True)
        for r in range(40):
            assert all_a[0, r].tolist() == local_start(seed, r, 8, 4).tolist(), (seed, r)
        assert np.all(all_r == 0.0) and np.all(opt.local_info[:, 1] == 1)


def test_one_sweep_is_reported_as_not_converged_when_it_moved():
    env = _game(20, 5)
    opt = OptimalAllocation()
    a1, r1 = opt.search_local(env, W_V2V, W_V2I, restarts=1, max_sweeps=1)
    assert opt.local_info[0].tolist() == [0, 0]                                 # the round-robin start is not 1-opt here
    assert r1.tobytes() == opt.rewards_of(env, W_V2V, W_V2I, a1).tobytes()
    a64, r64 = opt.search_local(env, W_V2V, W_V2I, restarts=1)
    assert opt.local_info[0].tolist() == [0, 1] and r64[0] >= r1[0]


@pytest.mark.parametrize("n,rb", SIZES)
def test_no_single_link_change_improves_the_result(n, rb):
    envs, opt, single, stacked = _result(n, rb)
    actions, reward = stacked[0], stacked[1]
    near = np.repeat(actions[:, None, :], n * (rb - 1), axis=1)
    j = 0
    for l in range(n):
        for d in range(1, rb):
            near[:, j, l] = (actions[:, l] + d) % rb
            j += 1
    assert j == n * (rb - 1)
    got = opt.rewards_of(Stack(envs), W_V2V, W_V2I, near)
    gap = reward[:, None] - got
    print(n, rb, "closest single-link change below the result by", gap.min(axis=1).tolist())
    assert np.all(got <= reward[:, None] + _tol(reward)[:, None])


# --------------------------------------------------------------------------------------- 6. against the exact optimum
def _against(opt, env, want_i, want_r, rb):
    actions, reward = opt.search_local(env, W_V2V, W_V2I, restarts=128, seed=0)
    assert reward[0] <= want_r[0]
    hit = int(encode(actions, rb)[0]) == int(want_i[0]) and reward[0].tobytes() == want_r[0].tobytes()
    return hit, float((want_r[0] - reward[0]) / want_r[0])


def test_eight_links_reach_the_exhaustive_optimum():
    opt = OptimalAllocation()
    hits, gaps = 0, []
    for s in range(20):
        env = make_state(8, 4, 9804 + s)
        hit, gap = _against(opt, env, *opt.search(env, W_V2V, W_V2I), rb=4)
        hits += hit
        gaps.append(gap)
    print("8 x 4: exact optimum in", hits, "of 20, worst relative gap", max(gaps))
    assert hits >= 18 and max(gaps) <= 1e-2


@pytest.mark.parametrize("n,need", [(12, 8), (16, 6), (20, 7)])
def test_seeded_games_reach_the_branch_and_bound_optimum(n, need):
    opt = OptimalAllocation()
    hits, gaps = 0, []
    for s in range(10):
        env = _game(n, s)
        hit, gap = _against(opt, env, *opt.search_bound(env, W_V2V, W_V2I), rb=4)
        hits += hit
        gaps.append(gap)
    print(n, "x 4: exact optimum in", hits, "of 10, worst relative gap", max(gaps), "gaps", gaps)
    assert hits >= need and max(gaps) <= 1e-2


# -------------------------------------------------------------------------------------------- 7. seeded bound search
def _seeded_same(opt, env, want, w_v2v=W_V2V, w_v2i=W_V2I, incumbent='local'):
    got_i, got_r = opt.search_bound(env, w_v2v, w_v2i, incumbent=incumbent)
    print("seeded", got_i.tolist()[:4], got_r.tolist()[:4], "nodes", opt.nodes_visited)
    assert got_i.dtype == np.int64 and np.array_equal(got_i, want[0]) and got_r.tobytes() == want[1].tobytes()
    return got_i, got_r


@pytest.mark.parametrize("n,rb", [(4, 4), (8, 4), (12, 4), (5, 3), (3, 6), (2, 2), (8, 16)])
def test_seeded_bound_equals_exhaustive_search_bitwise(n, rb):
    opt = OptimalAllocation()
    for seed in range(3 if n < 12 and rb < 16 else 1):
        env = make_state(n, rb, 300 * n + rb + seed)
        want = opt.search(env, W_V2V, W_V2I)
        _seeded_same(opt, env, want)
        _seeded_same(opt, env, want, incumbent=np.zeros((1, n), np.int64))          # a poor start
        _seeded_same(opt, env, want, incumbent=decode(want[0], n, rb))              # the optimum itself
        _seeded_same(opt, env, want, incumbent=np.full((1, n), rb - 1))


def test_seeded_bound_equals_exhaustive_search_on_fifty_batched_states():
    opt = OptimalAllocation()
    env = Stack([make_state(8, 4, 5000 + s) for s in range(50)])
    want = opt.search(env, W_V2V, W_V2I)
    _seeded_same(opt, env, want)
    _seeded_same(opt, env, want, incumbent=np.zeros((50, 8), int))
    _seeded_same(opt, env, want, incumbent=decode(want[0], 8, 4))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_seeded_bound_equals_the_unseeded_one_at_twenty_links(seed):
    env = _game(20, seed)
    opt = OptimalAllocation()
    want = opt.search_bound(env, W_V2V, W_V2I)
    plain = opt.nodes_visited
    _seeded_same(opt, env, want)
    print("20 x 4 seed", seed, "nodes unseeded", plain, "seeded", opt.nodes_visited)
    _seeded_same(opt, env, want, incumbent=decode(want[0], 20, 4))


def test_seeded_bound_keeps_the_lowest_index_among_interchangeable_channels():
    """the construction of test_gpu_optimum_bound.test_interchangeable_channels_take_the_lowest_index, seeded with the
    HIGHER-index twin of the optimum: an equal reward at a lower index must still be found"""
    n, rb = 8, 4
    env = make_state(n, rb, 77)
    g = env.V2V_channels_with_fastfading
    g[1, :, :] = g[0, :, :]
    g[:, :, 1] = g[:, :, 0]
    opt = OptimalAllocation()
    want = opt.search(env, 1.0, 0.0)
    a = decode(want[0], n, rb)[0]
    twin = np.where(a == 0, 1, np.where(a == 1, 0, a))
    assert int(encode(twin, rb)) > int(want[0][0])
    assert opt.rewards_of(env, 1.0, 0.0, twin[None])[0].tobytes() == want[1][0].tobytes()
    _seeded_same(opt, env, want, 1.0, 0.0, incumbent=twin[None])
    _seeded_same(opt, env, want, 1.0, 0.0)


def test_seeded_bound_keeps_the_lowest_index_when_all_gains_are_equal():
    env = make_state(8, 4, 7)
    env.V2V_channels_with_fastfading = np.full_like(env.V2V_channels_with_fastfading, 80.0)
    env.V2I_channels_with_fastfading = np.full_like(env.V2I_channels_with_fastfading, 80.0)
    env.V2I_channels_abs = np.full_like(env.V2I_channels_abs, 80.0)
    opt = OptimalAllocation()
    want = opt.search(env, 1.0, 0.0)
    vec = opt.rewards(env, 1.0, 0.0)[0]
    ties = np.flatnonzero(vec == want[1][0])
    assert ties.size > 100 and ties[0] == want[0][0]
    _seeded_same(opt, env, want, 1.0, 0.0)
    _seeded_same(opt, env, want, 1.0, 0.0, incumbent=decode(ties[-1:], 8, 4))       # the highest-index maximiser


# ------------------------------------------------------------------------------------------------------- 8. drivers
def _agent(env, n):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(n, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(n, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_test_run_local_backend_beside_device_backend_at_eight_links():
    outs = []
    for backend in ('device', 'local'):
        random.seed(808)
        np.random.seed(808)
        env = make_env()
        env.new_random_game(8)
        outs.append(_agent(env, 8).test_run(1, 2, True, opt_backend=backend))
    dev, loc = outs
    for i in range(10):                                                        # the policy and the random baseline
        assert np.array_equal(dev[i], loc[i])
    print("8 links: optimum", dev[11].tolist(), "local", loc[11].tolist())
    assert np.all(loc[11] <= dev[11]) and np.all(loc[11] >= dev[11] * (1 - 1e-2))
    assert np.all(loc[10] <= dev[10])


def test_test_run_at_one_hundred_links_dominates_both_policies():
    random.seed(100100)
    np.random.seed(100100)
    env = make_env()
    env.new_random_game(100)
    agent = _agent(env, 100)
    seen = []
    inner = agent._local_search_device
    agent._local_search_device = lambda opt, restarts: seen.append(inner(opt, restarts)) or seen[-1]
    out = agent.test_run(1, 2, True, opt_backend='local')
    rl, ra, best = out[1], out[6], out[11]
    print("100 links: policy", rl.tolist(), "random", ra.tolist(), "local search", best.tolist())
    assert best.shape == (1, 2) and np.all(best > 0)
    assert np.all(best >= np.maximum(rl, ra))
    assert len(seen) == 2
    for st, (index, reward, res) in enumerate(seen):
        assert index == -1                                                     # 4^100 has no 64-bit index
        assert best[0, st] == W_V2V * np.sum(res[0]) + W_V2I * np.sum(res[1]) == reward
        assert np.array_equal(out[12][0, st], np.sum(res[0], axis=1))


def test_evaluate_training_diff_trials_accepts_the_local_backend():
    random.seed(3)
    np.random.seed(3)
    env = make_env()
    env.new_random_game(8)
    agent = _agent(env, 8)
    loc = agent.evaluate_training_diff_trials(5, 2, True, 0.0, 1, load=False, opt_backend='local', opt_restarts=64)
    random.seed(3)
    np.random.seed(3)
    env = make_env()
    env.new_random_game(8)
    dev = _agent(env, 8).evaluate_training_diff_trials(5, 2, True, 0.0, 1, load=False, opt_backend='device')
    for i in range(4):
        assert np.array_equal(loc[i], dev[i])
    assert np.all(loc[5] <= dev[5]) and np.all(loc[5] >= dev[5] * (1 - 1e-2))
