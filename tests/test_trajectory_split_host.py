"""No GPU needed: the C ABI of the split stream phase of the wide walk (v2x_traj_split_workspace_bytes,
v2x_rollout_steps_split, v2x_eval_steps_split) is declared, exported and bound alike; the workspace size is the formula the
header documents; a null struct, null and too-small workspaces and every check of the serial call come back as V2X_EINVAL
before anything is launched (the pointers handed over are never dereferenced by the host: a check that let one through would
reach a launch, which fails without a device); the Python layers refuse an unknown stream phase, and 'split' without the wide
walk, before any device work; and the streaming form of the MT19937 recurrence the generation kernel rests on -- word i + 624
from words i, i + 1 and i + 397 of one long stream -- gives the blocks the host library's reloads give."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_eval_device_host import ERRORS as EVAL_ERRORS, _eval
from test_rollout_trajectory_host import INHERITED_ERRORS, OWN_ERRORS, P, _brain, _host_env, _traj
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL
from v2xgnn.rl import Agent, DeviceChannels, RL_Config
from v2xgnn.rl import evaluate, native_sim, run, train
from v2xgnn.rl.device_sim import (STREAM_PHASES, check_stream_phase, split_workspace_layout, uniforms_per_step,
                                  wide_workspace_layout)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES2 = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]      # the grid of _traj() / _eval(): n_lanes = 2


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_traj_split_workspace_bytes", "int64_t", C.c_int64, 5),
                                                    ("v2x_rollout_steps_split", "int", C.c_int, 6),
                                                    ("v2x_eval_steps_split", "int", C.c_int, 6)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


# ------------------------------------------------------------------------------------------------------- the workspace size
def _blocks(n, rb, T, n_lanes):
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    return 1 + -(-(T * (2 * n_u + 4 * n * n_lanes)) // 624)


def documented_bytes(E, n, rb, T, n_lanes):
    """the formula of include/v2xgnn.h (the split stream phase), restated"""
    return sum(-(-x // 256) * 256 for x in (4 * E * _blocks(n, rb, T, n_lanes) * 624, 8 * (T + 1) * E))


@pytest.mark.parametrize("E,n,rb,T,n_lanes", [(1, 3, 1, 1, 1), (3, 4, 4, 3, 6), (1, 20, 4, 50, 6), (5, 20, 4, 10, 6), (2, 31, 5, 2, 64)])
def test_workspace_bytes_is_the_documented_formula(E, n, rb, T, n_lanes):
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T, n_lanes)
    assert lib.v2x_traj_split_workspace_bytes(E, n, rb, T, n_lanes) == want > 0
    offs, size = split_workspace_layout(E, n, rb, T, n_lanes)            # what DeviceChannels sizes the allocation by
    assert size == want and tuple(offs) == ('words', 'off') and offs['words'] == 0 and offs['off'] % 256 == 0
    words = 4 * E * _blocks(n, rb, T, n_lanes) * 624
    assert 0 <= offs['off'] - words < 256 and 0 <= size - offs['off'] - 8 * (T + 1) * E < 256
    text = open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()
    assert "NB = 1 + ceil(T (2 n_u + 4 n n_lanes) / 624)" in text and "A(4 E NB 624) + A(8 (T + 1) E)" in text


def test_the_block_bound_at_the_reference_shape():
    """20 links x 4 RBs, 6 lanes per table, T = 50: 50 (7560 + 480) = 402000 words are 644.2 blocks -> NB = 646, 1.61 MB"""
    assert uniforms_per_step(20, 4) == 3780 and _blocks(20, 4, 50, 6) == 646
    assert split_workspace_layout(1, 20, 4, 50, 6)[0]['off'] == -(-4 * 646 * 624 // 256) * 256


@pytest.mark.parametrize("E,n,rb,T,n_lanes", [(1, 2, 1, 1, 6), (1, 32, 4, 1, 6), (1, 4, 5, 1, 6), (1, 4, 4, 0, 6), (0, 4, 4, 1, 6), (1, 8, 6, 1, 6),
                                              (65536, 4, 4, 1, 6), (1, 4, 0, 1, 6), (1, 4, 4, -1, 6), (1, 4, 4, 1, 0), (1, 4, 4, 1, 65),
                                              (1, 4, 4, 1, -3)])
def test_workspace_bytes_is_negative_on_sizes_outside_the_limits(E, n, rb, T, n_lanes):
    lib = vlib.load_library()
    assert lib.v2x_traj_split_workspace_bytes(E, n, rb, T, n_lanes) == V2X_EINVAL < 0
    if 1 <= n_lanes <= 64:
        assert lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T) == V2X_EINVAL  # the limits are the trajectory's
    else:
        assert lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T) > 0 and "n_lanes" in lib.v2x_last_error(None).decode()


# ------------------------------------------------------------------------------------------------------- the argument checks
def _err(lib):
    return lib.v2x_last_error(None).decode()


def _calls(lib):
    """(entry point, a good struct of E = 2, n = 4, rb = 4, T = 3, the bytes its two workspaces need)"""
    r, ev = _traj(), _eval()
    assert r.r.step.n_lanes == ev.step.n_lanes == 2
    wide, need = lib.v2x_traj_wide_workspace_bytes(2, 4, 4, 3), lib.v2x_traj_split_workspace_bytes(2, 4, 4, 3, 2)
    assert wide == wide_workspace_layout(2, 4, 4, 3)[1] and need == documented_bytes(2, 4, 4, 3, 2)
    return [(lib.v2x_rollout_steps_split, r, wide, need), (lib.v2x_eval_steps_split, ev, wide, need)]


def test_a_null_struct_is_refused():
    lib = vlib.load_library()
    for call in (lib.v2x_rollout_steps_split, lib.v2x_eval_steps_split):
        assert call(None, P, 1 << 30, P, 1 << 30, None) == V2X_EINVAL and "null" in _err(lib)


def test_null_workspaces_are_refused_before_any_launch_the_wide_one_first():
    lib = vlib.load_library()
    for call, r, wide, need in _calls(lib):
        assert call(C.byref(r), P, wide, None, need, None) == V2X_EINVAL
        assert "null split-stream workspace" in _err(lib)
        assert call(C.byref(r), None, wide, None, need, None) == V2X_EINVAL
        assert "null wide-walk workspace" in _err(lib)
        assert call(C.byref(r), None, wide, P, need, None) == V2X_EINVAL
        assert "null wide-walk workspace" in _err(lib)


def test_workspaces_one_byte_short_are_refused_before_any_launch():
    lib = vlib.load_library()
    for call, r, wide, need in _calls(lib):
        assert call(C.byref(r), P, wide, P, need - 1, None) == V2X_EINVAL
        assert "split-stream workspace" in _err(lib) and "needs %d bytes, got %d" % (need, need - 1) in _err(lib)
        assert call(C.byref(r), P, wide, P, 0, None) == V2X_EINVAL and "needs %d bytes" % need in _err(lib)
        assert call(C.byref(r), P, wide - 1, P, need, None) == V2X_EINVAL        # the wide form's check comes first
        assert "wide-walk workspace" in _err(lib) and "needs %d bytes, got %d" % (wide, wide - 1) in _err(lib)


def test_the_need_follows_the_steps_own_number_of_lanes():
    lib = vlib.load_library()
    r = _traj()
    r.r.step.n_lanes = 64
    wide, small, big = (lib.v2x_traj_wide_workspace_bytes(2, 4, 4, 3), lib.v2x_traj_split_workspace_bytes(2, 4, 4, 3, 2),
                        lib.v2x_traj_split_workspace_bytes(2, 4, 4, 3, 64))
    assert big > small
    assert lib.v2x_rollout_steps_split(C.byref(r), P, wide, P, small, None) == V2X_EINVAL
    assert "n_lanes = 64 needs %d bytes, got %d" % (big, small) in _err(lib)


def test_the_serial_checks_run_first():
    lib = vlib.load_library()
    call = lib.v2x_rollout_steps_split
    assert call(C.byref(_traj(T=5)), None, 0, None, 0, None) == V2X_EINVAL and "T E <= capacity" in _err(lib)
    assert call(C.byref(_traj(traj_xe=None)), None, 0, None, 0, None) == V2X_EINVAL and "trajectory workspace" in _err(lib)
    assert call(C.byref(_traj(step_null=('lanes',))), P, 1 << 30, P, 1 << 30, None) == V2X_EINVAL and "null pointer" in _err(lib)
    assert lib.v2x_eval_steps_split(C.byref(_eval(T=0)), None, 0, None, 0, None) == V2X_EINVAL and "T = 0" in _err(lib)
    assert "rollout_steps_split" in (call(C.byref(_traj(T=5)), None, 0, None, 0, None), _err(lib))[1]      # the text names the entry point


def test_every_check_of_the_serial_calls_refuses_the_split_calls_too_with_good_workspaces():
    lib = vlib.load_library()
    big = 1 << 40
    for change, word in OWN_ERRORS + INHERITED_ERRORS:
        assert lib.v2x_rollout_steps_split(C.byref(_traj(**change)), P, big, P, big, None) == V2X_EINVAL, change
        assert word in _err(lib), (change, _err(lib))
    for change, word in EVAL_ERRORS:
        assert lib.v2x_eval_steps_split(C.byref(_eval(**change)), P, big, P, big, None) == V2X_EINVAL, change
        assert word in _err(lib), (change, _err(lib))


# ------------------------------------------------------------------------------------------------------- the Python layers
def test_check_stream_phase():
    assert STREAM_PHASES == ('chain', 'split')
    assert check_stream_phase("who", 'chain') == 'chain' and check_stream_phase("who", 'split') == 'split'
    assert check_stream_phase("who", 'chain', 'serial') == 'chain' and check_stream_phase("who", 'split', 'wide') == 'split'
    for bad in ('sideways', None, 'auto', 'wide'):
        with pytest.raises(ValueError, match="who: stream_phase must be one of 'chain', 'split'"):
            check_stream_phase("who", bad)
    with pytest.raises(ValueError, match="who: stream_phase='split' needs walk='wide'"):
        check_stream_phase("who", 'split', 'serial')


def test_channels_refuse_a_bad_stream_phase_before_any_device_work():
    dc = DeviceChannels(2, 4, 4)
    dc.set_grid(LANES2, 750, 1299, 0.01)
    ex, ra = np.ones((3, 2), np.uint8), np.zeros((3, 2, 4), np.int32)
    for walk in ('serial', 'wide'):
        with pytest.raises(ValueError, match="rollout_steps: stream_phase must be one of 'chain', 'split'"):
            dc.rollout_steps(ex, ra, {}, 0, 8, 1.0, 0.1, walk=walk, stream_phase='sideways')
        with pytest.raises(ValueError, match="eval_steps: stream_phase must be one of 'chain', 'split'"):
            dc.eval_steps(ex, ra, None, 1.0, 0.1, walk=walk, stream_phase='sideways')
    with pytest.raises(ValueError, match="rollout_steps: stream_phase='split' needs walk='wide'"):
        dc.rollout_steps(ex, ra, {}, 0, 8, 1.0, 0.1, stream_phase='split')
    with pytest.raises(ValueError, match="eval_steps: stream_phase='split' needs walk='wide'"):
        dc.eval_steps(ex, ra, None, 1.0, 0.1, walk='serial', stream_phase='split')
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}
    assert dc.walk_calls == {'serial': 0, 'wide': 0} and dc.stream_phase_calls == {'chain': 0, 'split': 0}


def _mk(env, **kw):
    return Agent(4, 4, 1, 16, env, RL_Config(), brain=_brain(), device_replay=False, **kw)


def test_agent_refuses_an_unknown_stream_phase_and_split_without_the_wide_walk():
    assert _mk(_host_env()).trajectory_streams == 'chain'                # the default stays
    assert _mk(_host_env(), trajectory_streams='chain').trajectory_streams == 'chain'
    for bad in ('sideways', None, 'auto'):
        with pytest.raises(ValueError, match="trajectory_streams must be one of"):
            _mk(_host_env(), trajectory_streams=bad)
    with pytest.raises(ValueError, match="trajectory_streams='split' needs trajectory_walk='wide'"):
        _mk(_host_env(), trajectory_streams='split')
    with pytest.raises(ValueError, match="trajectory_streams='split' needs trajectory_walk='wide'"):
        _mk(_host_env(), trajectory_walk='serial', trajectory_streams='split')
    with pytest.raises(ValueError, match="trajectory_walk='wide' needs rollout_backend='trajectory'"):
        _mk(_host_env(), trajectory_walk='wide', trajectory_streams='split')      # the walk is checked first, as before


@pytest.mark.parametrize("main,argv", [(train.main, ["--envs", "2"]), (run.main, ["--save-dir", "x"]), (evaluate.main, ["--save-dir", "x"])])
def test_the_command_line_flag_refuses_an_unknown_value(main, argv, capsys):
    with pytest.raises(SystemExit) as exc:
        main(argv + ["--trajectory-streams", "sideways"])
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "invalid choice" in err and "--trajectory-streams" in err


def test_split_on_the_command_line_needs_the_wide_walk(capsys):
    for main, argv in ((train.main, ["--envs", "2"]), (run.main, ["--save-dir", "x"]), (evaluate.main, ["--save-dir", "x"])):
        with pytest.raises(SystemExit) as exc:
            main(argv + ["--trajectory-streams", "split"])
        assert exc.value.code == 2 and "--trajectory-streams split needs --trajectory-walk wide" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:                               # ... and the walk's own condition still comes first
        train.main(["--envs", "2", "--trajectory-walk", "wide", "--trajectory-streams", "split"])
    assert exc.value.code == 2 and "--trajectory-walk wide needs --rollout trajectory" in capsys.readouterr().err
    assert train.build_parser().parse_args([]).trajectory_streams == 'chain'


# ------------------------------------------------------------------------------------------------------- the recurrence
def _twist(cur, nxt, far):
    y = (cur & np.uint32(0x80000000)) | (nxt & np.uint32(0x7fffffff))
    return far ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908b0df), np.uint32(0))


def test_the_streaming_recurrence_over_three_blocks_equals_three_reloads_of_the_host_library():
    """k_traj_words restated in numpy: the stream w with w[0:624] the key array and w[i + 624] = twist(w[i], w[i + 1],
    w[i + 397]), made 227 words at a time (every operand of a round is older than the round).  The host library's reload,
    forced by drawing 312 doubles from a used-up block, gives the same three blocks; so do numpy's own generators."""
    E = 3
    keys = np.ascontiguousarray(np.stack([np.random.RandomState(41 + e).get_state()[1] for e in range(E)]).astype(np.uint32))
    w = np.zeros((E, 4 * 624), np.uint32)
    w[:, :624] = keys
    rounds = 0
    for s0 in range(624, 4 * 624, 227):
        j = np.arange(s0, min(s0 + 227, 4 * 624))
        assert j.max() - 227 < s0 and (j - 624 + 1).max() < s0           # all three operands are older than the round
        w[:, j] = _twist(w[:, j - 624], w[:, j - 623], w[:, j - 227])
        rounds += 1
    assert rounds == -(-3 * 624 // 227) == 9                             # 2.75 rounds per block
    k, pos = keys.copy(), np.full(E, 624, np.int32)
    for b in (1, 2, 3):
        u = native_sim.mt_uniforms(k, pos, 312)                          # 624 words: the whole of the next block
        assert np.all(pos == 624) and k.tobytes() == np.ascontiguousarray(w[:, 624 * b:624 * (b + 1)]).tobytes(), b
        t = w[:, 624 * b:624 * (b + 1)].copy()                           # ... and the doubles are its tempered words
        t ^= t >> np.uint32(11)
        t ^= (t << np.uint32(7)) & np.uint32(0x9d2c5680)
        t ^= (t << np.uint32(15)) & np.uint32(0xefc60000)
        t ^= t >> np.uint32(18)
        d = ((t[:, 0::2] >> np.uint32(5)).astype(np.float64) * 67108864.0 + (t[:, 1::2] >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0
        assert d.tobytes() == u.tobytes(), b
    rs = np.random.RandomState(41)
    rs.random_sample(312 * 3)
    assert rs.get_state()[1].astype(np.uint32).tobytes() == w[0, 3 * 624:].tobytes() and rs.get_state()[2] == 624
