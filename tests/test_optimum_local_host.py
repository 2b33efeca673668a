"""CPU: the host side of the multi-start local search for a near-optimal channel allocation (OptimalAllocation.search_local /
rewards_of, opt_backend='local'; v2x_opt_search_local of csrc/v2xopt.hip): the start rule, encode, and the argument checks,
all of which run before any device work -- a call that passes them fails on a machine without a GPU with RuntimeError
("needs a GPU"), never ValueError."""
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl import optimum
from v2xgnn.rl.agent import OPT_BACKENDS, _check_opt_backend
from v2xgnn.rl.optimum import decode, encode, local_start, splitmix64
from test_rl_agent import RecordingBrain
from test_rl_env import make_env


def _env(links=4):
    random.seed(5)
    np.random.seed(5)
    env = make_env()
    if links != 4:
        env.new_random_game(links)
    return env


def test_splitmix64_and_the_starts_match_the_pinned_values():
    assert splitmix64(0) == 0xe220a8397b1dcdaf
    assert splitmix64(1) == 0x910a2dec89025cc1
    assert local_start(0, 1, 8, 4).tolist() == [3, 0, 0, 0, 3, 2, 1, 1]
    assert local_start(0, 2, 8, 4).tolist() == [2, 1, 2, 2, 0, 3, 2, 0]
    assert local_start(7, 5, 12, 3).tolist() == [2, 2, 1, 1, 1, 2, 2, 2, 2, 1, 1, 2]
    assert local_start(1, 1000, 6, 16).tolist() == [12, 15, 5, 5, 14, 11]
    # restart 0 is the round-robin start, whatever the seed
    assert local_start(0, 0, 10, 4).tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    assert local_start(99, 0, 5, 3).tolist() == [0, 1, 2, 0, 1]
    assert local_start(3, 7, 128, 16).dtype == np.int64 and set(local_start(3, 7, 128, 16).tolist()) <= set(range(16))


def test_encode_is_the_inverse_of_decode():
    rng = np.random.default_rng(1)
    for n, rb in ((4, 4), (5, 3), (8, 16), (20, 4), (31, 4), (15, 16)):
        idx = rng.integers(0, rb ** n, size=50)
        idx[:2] = (0, rb ** n - 1)
        assert np.array_equal(encode(decode(idx, n, rb), rb), idx)
    a = np.array([[[0, 1, 2], [2, 1, 0]]])
    assert encode(a, 3).tolist() == [[5, 21]] and encode(a, 3).dtype == np.int64
    assert OptimalAllocation.encode(a, 3).tolist() == [[5, 21]]
    encode(np.zeros(31, int), 4)                                   # 4^31 = 2^62: the last size with an index
    with pytest.raises(ValueError, match=r"4\^32 .*2\^62"):
        encode(np.zeros(32, int), 4)
    with pytest.raises(ValueError, match="channel outside"):
        encode(np.array([0, 4]), 4)


def test_check_local_limits():
    ok = OptimalAllocation.check_local
    ok(1, 2, 1, 1)
    ok(128, 16, 65536, 64)
    ok(100, 4)
    for n, rb in ((0, 4), (129, 4)):
        with pytest.raises(ValueError, match="1..128 links and 2..16 channels"):
            ok(n, rb)
    for n, rb in ((20, 1), (20, 17)):
        with pytest.raises(ValueError, match="1..128 links and 2..16 channels"):
            ok(n, rb)
    for restarts in (0, 65537, 2.5):
        with pytest.raises(ValueError, match="restarts"):
            ok(20, 4, restarts)
    for sweeps in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_sweeps"):
            ok(20, 4, 128, sweeps)
    # the index-based searches keep their 32 links
    with pytest.raises(ValueError, match="1..32 links"):
        OptimalAllocation.check_bound(100, 4)


def test_search_local_and_rewards_of_refuse_before_any_device_work():
    opt = OptimalAllocation()
    env = _env(8)
    for kw in (dict(restarts=0), dict(restarts=65537), dict(max_sweeps=0), dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError):
            opt.search_local(env, 1.0, 0.1, **kw)
    wide = _env(8)
    wide.n_RB = 17
    with pytest.raises(ValueError, match="2..16 channels"):
        opt.rewards_of(wide, 1.0, 0.1, np.zeros((1, 8), int))
    narrow = _env(8)
    narrow.n_RB = 1
    with pytest.raises(ValueError, match="2..16 channels"):
        opt.rewards_of(narrow, 1.0, 0.1, np.zeros((1, 8), int))
    two = _env(8)
    two.n_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        opt.search_local(two, 1.0, 0.1)
    idle = _env(8)
    idle.activate_links[3, 0] = False
    with pytest.raises(ValueError, match="every link active"):
        opt.search_local(idle, 1.0, 0.1)
    # joint actions: a channel outside [0, rb), a wrong shape, a wrong type
    for bad in (np.full((1, 8), 4), np.full((1, 8), -1), np.array([[0, 1, 2, 3, 0, 1, 2, 4]])):
        with pytest.raises(ValueError, match=r"channel outside \[0, 4\)"):
            opt.rewards_of(env, 1.0, 0.1, bad)
    for bad in (np.zeros((1, 7), int), np.zeros((2, 8), int), np.zeros(8, int), np.zeros((1, 2, 3, 8), int),
                np.zeros((1, 0, 8), int)):
        with pytest.raises(ValueError, match="joint actions of shape"):
            opt.rewards_of(env, 1.0, 0.1, bad)
    with pytest.raises(ValueError, match="integers"):
        opt.rewards_of(env, 1.0, 0.1, np.zeros((1, 8)))
    # search_bound's incumbent
    with pytest.raises(ValueError, match="incumbent"):
        opt.search_bound(env, 1.0, 0.1, incumbent='nonsense')
    with pytest.raises(ValueError, match="incumbent"):
        opt.search_bound(env, 1.0, 0.1, incumbent=np.zeros((1, 2, 8), int))
    with pytest.raises(ValueError, match="channel outside"):
        opt.search_bound(env, 1.0, 0.1, incumbent=np.full((1, 8), 9))
    with pytest.raises(ValueError, match="restarts"):
        opt.search_bound(env, 1.0, 0.1, incumbent='local', restarts=0)
    assert opt.torch is None                                       # nothing above reached the device


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_drivers_know_the_local_backend():
    assert 'local' in OPT_BACKENDS and OPT_BACKENDS[:3] == ('host', 'device', 'bound')
    _check_opt_backend('local')
    with pytest.raises(ValueError, match="opt_backend"):
        _check_opt_backend('nonsense')
    agent = _agent(_env(100))
    assert callable(agent._optimum_search('local'))                # 100 links: accepted, nothing touched the device yet
    assert callable(agent._optimum_search('local', 16))
    with pytest.raises(ValueError, match="1..32 links"):
        agent._optimum_search('bound')                             # ... where the exact backends keep refusing
    with pytest.raises(ValueError, match="restarts"):
        agent._optimum_search('local', 0)
    with pytest.raises(ValueError, match="restarts"):
        agent.test_run(1, 1, True, opt_backend='local', opt_restarts=70000)
    big = _agent(_env())
    big.num_D2D = 129
    with pytest.raises(ValueError, match="1..128 links"):
        big._optimum_search('local')
    two = _agent(_env())
    two.num_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        two._optimum_search('local')
    assert optimum.DEFAULT_LOCAL_RESTARTS >= 128 and optimum.DEFAULT_MAX_SWEEPS == 64


def test_cli_drivers_accept_the_local_backend():
    import contextlib
    import io
    from v2xgnn.rl import run, evaluate
    for mod in (run, evaluate):
        err = io.StringIO()
        with contextlib.redirect_stderr(err), pytest.raises(SystemExit):
            mod.main(["--save-dir", "x", "--opt-backend", "local", "--opt-restarts", "64", "--no-such-option"])
        assert "no-such-option" in err.getvalue() and "invalid choice" not in err.getvalue()
        out = io.StringIO()
        with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
            mod.main(["--help"])
        assert "lower bound" in " ".join(out.getvalue().split())
