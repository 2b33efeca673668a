"""CPU: the argument checks and index order of the GPU optimal-allocation search (v2xgnn.rl.optimum, csrc/v2xopt.hip).
Every check here runs before any device work, so no GPU is needed."""
import itertools
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import decode
from test_rl_agent import RecordingBrain
from test_rl_env import make_env


def test_decode_is_itertools_product_order():
    for n, rb in ((1, 2), (3, 2), (4, 4), (5, 3), (3, 6)):
        want = np.array(list(itertools.product(range(rb), repeat=n)), np.int64)
        got = decode(np.arange(rb ** n), n, rb)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, rb)
    assert np.array_equal(OptimalAllocation.decode(27, 4, 4), [[0, 1, 2, 3]])
    # high index of the 2^36 limit: 64-bit digits
    assert np.array_equal(decode(4 ** 18 - 1, 18, 4), np.full((1, 18), 3))


def test_decode_matches_reference_digit_extraction_4x4():
    """BS_brain.py:1071-1078: the reference's four nested digit extractions for 4 links x 4 channels."""
    for idx in range(256):
        a0 = idx // 64
        a1 = (idx - a0 * 64) // 16
        a2 = (idx - a0 * 64 - a1 * 16) // 4
        a3 = idx - a0 * 64 - a1 * 16 - a2 * 4
        assert decode(idx, 4, 4).tolist() == [[a0, a1, a2, a3]]


def _env(links=4):
    random.seed(5)
    np.random.seed(5)
    env = make_env()
    if links != 4:
        env.new_random_game(links)
    return env


def test_search_rejects_two_receivers_per_link():
    env = _env()
    env.n_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        OptimalAllocation().search(env, 1.0, 0.1)
    with pytest.raises(ValueError, match="one receiver"):
        OptimalAllocation().rewards(env, 1.0, 0.1, 0, 4)


def test_search_rejects_an_inactive_link():
    env = _env()
    env.activate_links[2, 0] = False
    with pytest.raises(ValueError, match="every link active"):
        OptimalAllocation().search(env, 1.0, 0.1)


def test_search_rejects_joint_actions_beyond_the_limit_with_an_estimate():
    with pytest.raises(ValueError, match=r"4\^19 .*estimated .* per state on the GPU"):
        OptimalAllocation.check_size(19, 4)
    OptimalAllocation.check_size(18, 4)                        # 2^36: the largest search
    with pytest.raises(ValueError, match=r"4\^20 .*estimated"):
        OptimalAllocation().search(_env(20), 1.0, 0.1)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels"):
        OptimalAllocation.check_size(4, 17)


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_drivers_reject_an_unknown_backend():
    agent = _agent(_env())
    with pytest.raises(ValueError, match="opt_backend"):
        agent.test_run(1, 1, True, opt_backend='bogus')
    with pytest.raises(ValueError, match="opt_backend"):
        agent.test_run(1, 1, False, opt_backend='bogus')
    with pytest.raises(ValueError, match="opt_backend"):
        agent.evaluate_training_diff_trials(5, 1, True, 0.0, 1, load=False, opt_backend='bogus')


def test_device_backend_checks_size_before_any_device_work():
    """20 links x 4 channels: the host path's cap refuses it, and so does the device search (4^20 > 2^36)."""
    agent = _agent(_env(20))
    with pytest.raises(ValueError, match="not feasible"):
        agent.test_run(1, 1, True)
    with pytest.raises(ValueError, match=r"4\^20"):
        agent.test_run(1, 1, True, opt_backend='device')


def test_cli_drivers_accept_the_backend_switch():
    from v2xgnn.rl import run, evaluate
    for mod in (run, evaluate):
        with pytest.raises(SystemExit):
            mod.main(["--save-dir", "x", "--opt-backend", "bogus"])
