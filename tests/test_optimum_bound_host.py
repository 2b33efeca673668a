"""CPU: the argument checks of the branch-and-bound optimal-allocation search (OptimalAllocation.search_bound,
opt_backend='bound', v2x_opt_search_bound of csrc/v2xopt.hip).  Every check here runs before any device work, so no GPU is
needed: a call that passes them fails on a machine without one with RuntimeError ("needs a GPU"), never ValueError."""
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, BoundBudgetExceeded, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import DEFAULT_MAX_NODES
from test_rl_agent import RecordingBrain
from test_rl_env import make_env


def _env(links=4):
    random.seed(5)
    np.random.seed(5)
    env = make_env()
    if links != 4:
        env.new_random_game(links)
    return env


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_search_bound_rejects_two_receivers_per_link():
    env = _env()
    env.n_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        OptimalAllocation().search_bound(env, 1.0, 0.1)


def test_search_bound_rejects_an_inactive_link():
    env = _env()
    env.activate_links[2, 0] = False
    with pytest.raises(ValueError, match="every link active"):
        OptimalAllocation().search_bound(env, 1.0, 0.1)


def test_search_bound_rejects_a_negative_weight():
    for w in ((-1.0, 0.1), (1.0, -0.1), (float('nan'), 0.1)):
        with pytest.raises(ValueError, match="weights >= 0"):
            OptimalAllocation().search_bound(_env(), *w)
        with pytest.raises(ValueError, match="weights >= 0"):
            OptimalAllocation.check_bound(20, 4, *w)


def test_search_bound_rejects_sizes_outside_the_supported_range():
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels"):
        OptimalAllocation.check_bound(33, 4)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels"):
        OptimalAllocation.check_bound(4, 17)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels"):
        OptimalAllocation.check_bound(4, 1)
    with pytest.raises(ValueError, match=r"16\^16 .*exceeds the limit of 2\^62"):
        OptimalAllocation.check_bound(16, 16)                  # the joint-action index has to fit in 64 bits
    OptimalAllocation.check_bound(32, 3)
    OptimalAllocation.check_bound(15, 16)


def test_search_bound_rejects_a_budget_below_one_node():
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError, match="max_nodes"):
            OptimalAllocation().search_bound(_env(), 1.0, 0.1, max_nodes=bad)
    OptimalAllocation.check_bound(20, 4, 1.0, 0.1, max_nodes=1)
    assert DEFAULT_MAX_NODES >= 1000 * 1.9e6                   # three orders of magnitude over the worst 20-link state measured


def test_twenty_links_pass_the_bound_check_and_still_fail_the_exhaustive_one():
    OptimalAllocation.check_bound(20, 4, 1.0, 0.1)
    OptimalAllocation.check_bound(24, 4, 1.0, 0.1)
    with pytest.raises(ValueError, match=r"4\^20"):
        OptimalAllocation.check_size(20, 4)
    with pytest.raises(ValueError, match=r"4\^20"):
        OptimalAllocation().search(_env(20), 1.0, 0.1)


def _passes_the_checks(call):
    """`call` gets past every argument check: it succeeds (a GPU is present) or stops where the device is first needed."""
    try:
        call()
    except ValueError:
        raise
    except RuntimeError as exc:                                # no GPU / library not built for one: past the checks
        assert not isinstance(exc, BoundBudgetExceeded), exc


def test_drivers_accept_the_bound_backend_and_check_before_device_work():
    agent = _agent(_env(20))
    search = agent._optimum_search('bound')                    # 20 x 4 is accepted; nothing touched the device yet
    assert callable(search)
    with pytest.raises(ValueError, match=r"4\^20"):
        agent._optimum_search('device')                        # ... while the exhaustive backend keeps refusing it
    # the drivers themselves: every argument check passes (the run goes on to the device, where there is one)
    small = _agent(_env())
    _passes_the_checks(lambda: small.test_run(1, 1, True, opt_backend='bound'))
    _passes_the_checks(lambda: small.evaluate_training_diff_trials(5, 1, True, 0.0, 1, load=False, opt_backend='bound'))
    # rejected arguments, as ValueError before any device work
    two = _agent(_env())
    two.num_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        two._optimum_search('bound')
    neg = _agent(_env())
    neg.v2i_weight = -0.1
    with pytest.raises(ValueError, match="weights >= 0"):
        neg.test_run(1, 1, True, opt_backend='bound')
    with pytest.raises(ValueError, match="weights >= 0"):
        neg.evaluate_training_diff_trials(5, 1, True, 0.0, 1, load=False, opt_backend='bound')
    big = _agent(_env())
    big.num_D2D = 33
    with pytest.raises(ValueError, match="1..32 links"):
        big._optimum_search('bound')
    wide = _agent(_env())
    wide.num_CH = 17
    with pytest.raises(ValueError, match="2..16 channels"):
        wide._optimum_search('bound')


def test_cli_drivers_accept_the_bound_backend():
    """argparse stops at the unknown option, not at `--opt-backend bound`; a bogus backend's error names 'bound'."""
    import contextlib
    import io
    from v2xgnn.rl import run, evaluate
    for mod in (run, evaluate):
        err = io.StringIO()
        with contextlib.redirect_stderr(err), pytest.raises(SystemExit):
            mod.main(["--save-dir", "x", "--opt-backend", "bound", "--no-such-option"])
        assert "no-such-option" in err.getvalue() and "invalid choice" not in err.getvalue()
        err = io.StringIO()
        with contextlib.redirect_stderr(err), pytest.raises(SystemExit):
            mod.main(["--save-dir", "x", "--opt-backend", "bogus"])
        assert "invalid choice" in err.getvalue() and "'bound'" in err.getvalue()
