"""CPU: the host side of the reward landscape (v2xgnn.rl.optimum: rank_edges, rank_from_counts, the argument checks of
landscape / rank_of, which run before any device work) and the opt_rank switch of Agent.test_run left off."""
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import rank_edges, rank_from_counts
from test_rl_agent import RecordingBrain
from test_rl_env import make_env


def _histogram(edges, r):
    """what v2x_opt_landscape defines: slot = searchsorted(edges, r, 'right'), NaN rewards in the last slot"""
    K = len(edges)
    nan = np.isnan(r)
    c = np.bincount(np.searchsorted(edges, r[~nan], side='right'), minlength=K + 2)
    c[K + 1] = nan.sum()
    return c


def _synthetic(seed, with_nan=False):
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.0, 40.0, size=5000)
    r[100:140] = r[7]                                   # exact duplicates of a queried value
    r[200] = np.nextafter(r[9], np.inf)                 # two queried values that are adjacent floats
    r[300] = r.max() + 1.0                              # the maximum, present once
    r[400:403] = r.min() - 1.0                          # the minimum, three times
    if with_nan:
        r[500:510] = np.nan
    queried = np.array([r[7], r[9], r[200], r[300], r[400], r[11], r[7]])     # r[11]: present once; r[7] asked twice
    return r, queried


@pytest.mark.parametrize("with_nan", [False, True])
def test_ranks_from_a_numpy_histogram(with_nan):
    rows = [_synthetic(s, with_nan) for s in range(3)]
    rewards = np.stack([q for _, q in rows])
    edges = rank_edges(rewards)
    assert edges.shape == (3, 2 * rewards.shape[1]) and edges.dtype == np.float64
    assert np.all(edges[:, 1:] >= edges[:, :-1])
    for e, (r, q) in enumerate(rows):
        finite = edges[e][np.isfinite(edges[e])]
        assert np.array_equal(finite, np.unique(np.concatenate([q, np.nextafter(q, np.inf)])))
        assert np.all(edges[e][finite.size:] == np.inf)
    counts = np.stack([_histogram(edges[e], r) for e, (r, _) in enumerate(rows)])
    assert np.all(counts.sum(axis=1) == 5000)
    better, equal = rank_from_counts(counts, edges, rewards)
    assert better.shape == equal.shape == rewards.shape and better.dtype == equal.dtype == np.int64
    for e, (r, q) in enumerate(rows):
        for a, v in enumerate(q):
            assert better[e, a] == np.sum(r > v), (e, a)
            assert equal[e, a] == np.sum(r == v), (e, a)
        assert better[e, 3] == 0 and equal[e, 3] == 1                   # the maximum
        assert equal[e, 0] == 41 and equal[e, 5] == 1 and equal[e, 4] == 3
        assert better[e, 1] == better[e, 2] + 1                         # adjacent floats, each present once


def test_rank_edges_limits():
    assert rank_edges(np.ones((2, 31))).shape == (2, 62)
    with pytest.raises(ValueError, match="1..31"):
        rank_edges(np.ones((2, 32)))
    # a NaN reward gets no edge and no rank
    r = np.array([[1.0, np.nan, 2.0]])
    ed = rank_edges(r)
    assert np.array_equal(ed[0], [1.0, np.nextafter(1.0, 2.0), 2.0, np.nextafter(2.0, 3.0), np.inf, np.inf])
    better, equal = rank_from_counts(_histogram(ed[0], np.array([1.0, 2.0, 2.0, 3.0]))[None], ed, r)
    assert better.tolist() == [[3, -1, 1]] and equal.tolist() == [[1, -1, 2]]


def _env(links=4):
    random.seed(5)
    np.random.seed(5)
    env = make_env()
    if links != 4:
        env.new_random_game(links)
    return env


def test_landscape_checks_its_edges_before_any_device_work():
    env, opt = _env(), OptimalAllocation()
    with pytest.raises(ValueError, match="1..62 edges, got 0"):
        opt.landscape(env, 1.0, 0.1, np.zeros(0))
    with pytest.raises(ValueError, match="1..62 edges, got 63"):
        opt.landscape(env, 1.0, 0.1, np.arange(63.0))
    with pytest.raises(ValueError, match="ascending"):
        opt.landscape(env, 1.0, 0.1, [3.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="ascending"):
        opt.landscape(env, 1.0, 0.1, [[1.0, 2.0, 1.5]])
    with pytest.raises(ValueError, match=r"edges of shape \[2\] or \[1, 2\]"):
        opt.landscape(env, 1.0, 0.1, np.zeros((3, 2)))
    assert opt.torch is None                                            # no device was touched


def test_landscape_and_rank_refuse_twenty_links_before_any_device_work():
    env, opt = _env(20), OptimalAllocation()
    with pytest.raises(ValueError, match=r"4\^20 .*estimated"):
        opt.landscape(env, 1.0, 0.1, [1.0, 2.0])
    with pytest.raises(ValueError, match=r"4\^20 .*estimated"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int))
    assert opt.torch is None
    with pytest.raises(ValueError, match="1..31 joint actions"):
        OptimalAllocation().rank_of(_env(), 1.0, 0.1, np.zeros((1, 32, 4), int))


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_test_run_refuses_opt_rank_where_the_device_search_would():
    with pytest.raises(ValueError, match=r"4\^20"):
        _agent(_env(20)).test_run(1, 1, False, opt_rank=True)
    env = _env()
    agent = _agent(env)
    agent.num_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        agent.test_run(1, 1, False, opt_rank=True)


@pytest.mark.parametrize("opt_flag", [False, True])
def test_test_run_with_opt_rank_off_is_the_call_without_the_keyword(opt_flag):
    outs = []
    for kw in ({}, {'opt_rank': False}):
        random.seed(77)
        np.random.seed(77)
        agent = _agent(make_env())
        outs.append(agent.test_run(2, 3, opt_flag, **kw))
        assert not hasattr(agent, 'rank_book')
        outs.append((random.random(), np.random.random()))              # the RNG streams end in the same place
    assert len(outs[0]) == (15 if opt_flag else 10) and len(outs[2]) == len(outs[0])
    for a, b in zip(outs[0], outs[2]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert outs[1] == outs[3]


def test_cli_accepts_the_rank_switch():
    from v2xgnn.rl import run
    with pytest.raises(SystemExit):
        run.main(["--save-dir", "x", "--opt-rank", "--links", "6"])
    book = {'better': np.array([[0, 5], [0, 20]]), 'ra_better': np.array([[100, 200], [40, 60]]),
            'total': np.full((2, 2), 256), 'uniform_mean_reward': np.array([[1.0, 2.0], [3.0, 4.0]])}
    s = run.rank_summary(book)
    assert s == {"share_states_gnn_optimal": 0.5, "median_share_better_gnn": 2.5 / 256,
                 "median_share_better_random": 80.0 / 256, "mean_reward_uniform_exact": 2.5}
