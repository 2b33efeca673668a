"""No GPU needed: the C ABI of the wide trajectory walk (v2x_traj_wide_workspace_bytes, v2x_rollout_steps_wide,
v2x_eval_steps_wide) is declared, exported and bound alike; the workspace size is the formula the header documents; a null
struct, a null workspace and a workspace one byte short come back as V2X_EINVAL before anything is launched (the pointers
handed over are never dereferenced by the host: a check that let one through would reach a launch, which fails without a
device); the Python layers refuse an unknown walk, and 'wide' where no trajectory call can ever run, before any device work;
and the draws of a rollout taken ahead do not depend on the walk."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_eval_device_host import _eval
from test_rollout_trajectory_host import P, _brain, _host_env, _traj
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL
from v2xgnn.rl import Agent, DeviceChannels, RL_Config
from v2xgnn.rl import evaluate, run, train
from v2xgnn.rl.device_sim import wide_workspace_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTIONS = ('u_all', 'xy_all', 'pl', 'gs', 'ob_state', 'ob_interf')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_traj_wide_workspace_bytes", "int64_t", C.c_int64, 4),
                                                    ("v2x_rollout_steps_wide", "int", C.c_int, 4),
                                                    ("v2x_eval_steps_wide", "int", C.c_int, 4)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


# ------------------------------------------------------------------------------------------------------- the workspace size
def _raw(E, n, rb, T):
    n_u, n_el = n + n * n + 2 * n * rb + 2 * n * n * rb, n + n * n
    return [8 * T * E * n_u, 16 * T * E * n, 8 * T * E * n_el, 8 * T * E * n_el, 8 * (T - 1) * E * n * (3 * rb + 1),
            8 * (T - 1) * E * n * rb]


def documented_bytes(E, n, rb, T):
    """the formula of include/v2xgnn.h (the wide walk), restated"""
    return sum(-(-x // 256) * 256 for x in _raw(E, n, rb, T))


@pytest.mark.parametrize("E,n,rb,T", [(1, 3, 1, 1), (3, 4, 4, 3), (1, 20, 4, 50), (2, 31, 5, 2)])
def test_workspace_bytes_is_the_documented_formula(E, n, rb, T):
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T)
    assert lib.v2x_traj_wide_workspace_bytes(E, n, rb, T) == want > 0
    offs, size = wide_workspace_layout(E, n, rb, T)                      # what DeviceChannels sizes the allocation by
    assert size == want and tuple(offs) == SECTIONS
    o = [offs[k] for k in SECTIONS] + [size]
    raw = _raw(E, n, rb, T)
    assert o[0] == 0 and all(x % 256 == 0 for x in o)
    assert all(0 <= o[i + 1] - o[i] - raw[i] < 256 for i in range(6))    # back to back: every array fits, nothing overlaps
    text = open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()
    assert "A(8 T E n_u) + A(16 T E n) + A(8 T E n_el) + A(8 T E n_el) + A(8 (T-1) E n (3 rb + 1)) + A(8 (T-1) E n rb)" in text


@pytest.mark.parametrize("E,n,rb,T", [(1, 2, 1, 1), (1, 32, 4, 1), (1, 4, 5, 1), (1, 4, 4, 0), (0, 4, 4, 1), (1, 8, 6, 1), (65536, 4, 4, 1),
                                      (1, 4, 0, 1), (1, 4, 4, -1)])
def test_workspace_bytes_is_negative_on_sizes_outside_the_limits(E, n, rb, T):
    lib = vlib.load_library()
    assert lib.v2x_traj_wide_workspace_bytes(E, n, rb, T) == V2X_EINVAL < 0
    assert lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T) == V2X_EINVAL      # the limits are the trajectory's


# ------------------------------------------------------------------------------------------------------- the argument checks
def _err(lib):
    return lib.v2x_last_error(None).decode()


def _calls(lib):
    """(entry point, a good struct of E = 2, n = 4, rb = 4, T = 3, the bytes its workspace needs)"""
    need = lib.v2x_traj_wide_workspace_bytes(2, 4, 4, 3)
    assert need == documented_bytes(2, 4, 4, 3)
    return [(lib.v2x_rollout_steps_wide, _traj(), need), (lib.v2x_eval_steps_wide, _eval(), need)]


def test_a_null_struct_is_refused():
    lib = vlib.load_library()
    for call in (lib.v2x_rollout_steps_wide, lib.v2x_eval_steps_wide):
        assert call(None, P, 1 << 30, None) == V2X_EINVAL and "null" in _err(lib)


def test_a_null_workspace_is_refused_before_any_launch():
    lib = vlib.load_library()
    for call, r, need in _calls(lib):
        assert call(C.byref(r), None, need, None) == V2X_EINVAL
        assert "null wide-walk workspace" in _err(lib)


def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    lib = vlib.load_library()
    for call, r, need in _calls(lib):
        assert call(C.byref(r), P, need - 1, None) == V2X_EINVAL
        assert "needs %d bytes, got %d" % (need, need - 1) in _err(lib)
        assert call(C.byref(r), P, 0, None) == V2X_EINVAL and "needs" in _err(lib)


def test_the_serial_checks_run_first():
    lib = vlib.load_library()
    assert lib.v2x_rollout_steps_wide(C.byref(_traj(T=5)), None, 0, None) == V2X_EINVAL and "T E <= capacity" in _err(lib)
    assert lib.v2x_rollout_steps_wide(C.byref(_traj(traj_xe=None)), None, 0, None) == V2X_EINVAL and "trajectory workspace" in _err(lib)
    assert lib.v2x_eval_steps_wide(C.byref(_eval(T=0)), None, 0, None) == V2X_EINVAL and "T = 0" in _err(lib)


# ------------------------------------------------------------------------------------------------------- the Python layers
def _mk(env, **kw):
    return Agent(4, 4, 1, 16, env, RL_Config(), brain=_brain(), device_replay=False, **kw)


def test_agent_refuses_an_unknown_walk_and_wide_where_no_trajectory_call_can_run():
    assert _mk(_host_env()).trajectory_walk == 'serial'                  # the default stays
    assert _mk(_host_env(), trajectory_walk='serial').trajectory_walk == 'serial'
    for bad in ('sideways', None, 'auto'):
        with pytest.raises(ValueError, match="trajectory_walk must be one of"):
            _mk(_host_env(), trajectory_walk=bad)
    with pytest.raises(ValueError, match="trajectory_walk='wide' needs rollout_backend='trajectory'") as exc:
        _mk(_host_env(), rollout_backend='host', trajectory_walk='wide')
    assert "DeviceBatchedEnviron" in str(exc.value)                      # ... and why no evaluation on the device can run either


def test_channels_refuse_an_unknown_walk_before_any_device_work():
    dc = DeviceChannels(2, 4, 4)
    dc.set_grid([[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]], 750, 1299, 0.01)
    ex, ra = np.ones((3, 2), np.uint8), np.zeros((3, 2, 4), np.int32)
    with pytest.raises(ValueError, match="walk must be one of 'serial', 'wide'"):
        dc.rollout_steps(ex, ra, {}, 0, 8, 1.0, 0.1, walk='sideways')
    with pytest.raises(ValueError, match="walk must be one of 'serial', 'wide'"):
        dc.eval_steps(ex, ra, None, 1.0, 0.1, walk='sideways')
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0} and dc.walk_calls == {'serial': 0, 'wide': 0}


@pytest.mark.parametrize("main,argv", [(train.main, ["--envs", "2"]), (run.main, ["--save-dir", "x"]), (evaluate.main, ["--save-dir", "x"])])
def test_the_command_line_flag_refuses_an_unknown_value(main, argv, capsys):
    with pytest.raises(SystemExit) as exc:
        main(argv + ["--trajectory-walk", "sideways"])
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "invalid choice" in err and "--trajectory-walk" in err


def test_wide_on_the_command_line_needs_the_backend_that_uses_it(capsys):
    with pytest.raises(SystemExit) as exc:
        train.main(["--envs", "2", "--trajectory-walk", "wide"])
    assert exc.value.code == 2 and "--trajectory-walk wide needs --rollout trajectory" in capsys.readouterr().err
    for main in (run.main, evaluate.main):
        with pytest.raises(SystemExit) as exc:
            main(["--save-dir", "x", "--trajectory-walk", "wide"])
        assert exc.value.code == 2 and "--trajectory-walk wide needs --eval-backend device" in capsys.readouterr().err
    assert train.build_parser().parse_args([]).trajectory_walk == 'serial'


# ------------------------------------------------------------------------------------------------------- the draws, taken ahead
def test_draws_taken_ahead_are_identical_for_both_walks():
    """the walk is not an input of the draws: an agent of either walk takes the same numpy values and leaves the same stream
    (the agents differ in trajectory_walk alone; 'wide' cannot be constructed on a host environment, so it is set after)"""
    runs = {}
    for walk in ('serial', 'wide'):
        agent = _mk(_host_env(3))
        agent.trajectory_walk = walk
        agent.num_Episodes, agent.num_Train_Step, agent.num_transition = 1, 2, 50
        np.random.seed(99)
        agent.num_step = 60                                              # the block crosses the end of the epsilon schedule (80)
        drawn = agent._draw_rollout_ahead(10)
        runs[walk] = (drawn, agent.epsilon, agent.num_step, np.random.get_state())
    (d1, e1, n1, s1), (d2, e2, n2, s2) = runs['serial'], runs['wide']
    assert len(d1) == len(d2) == 10 and e1 == e2 and n1 == n2 == 60
    assert s1[0] == s2[0] and np.array_equal(s1[1], s2[1]) and s1[2:] == s2[2:]
    for (a1, g1), (a2, g2) in zip(d1, d2):
        assert a1.tobytes() == a2.tobytes() and list(g1) == list(g2)
    assert any(len(g) for _, g in d1)
