"""No GPU needed: the C ABI of the device stream step (v2x_sim_stream, v2x_sim_advance) is declared, exported and bound alike,
and the Python layers refuse bad arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.rl import DeviceBatchedEnviron, DeviceChannels
from v2xgnn.rl.train import main, start_env_batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]


def declared_arguments(name):
    hdr = open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m, "%s is not declared in include/v2xgnn.h" % name
    return [a for a in m.group(1).split(',') if a.strip()]


@pytest.mark.parametrize("name,count", [("v2x_sim_stream", 15), ("v2x_sim_advance", 2)])
def test_stream_entry_points_are_declared_exported_and_bound_alike(name, count):
    assert len(declared_arguments(name)) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == count


def test_sim_step_binding_has_the_fields_of_the_declared_struct():
    hdr = open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()
    body = re.search(r'typedef struct v2x_sim_step \{(.*?)\} v2x_sim_step;', hdr, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part).split(' ')[-1] for part in re.split(r',', decl.split(None, 1)[1] if ' ' in decl else decl)]
    names = [re.sub(r'^(const)?(double|float|u?int\d+_t|v2x_opt_problem)', '', n) for n in names]
    assert names == [f[0] for f in vlib.SimStep._fields_], (names, [f[0] for f in vlib.SimStep._fields_])
    # pointers and doubles are 8 bytes, the two int32 share a slot: no padding anywhere
    assert C.sizeof(vlib.SimStep) == C.sizeof(vlib.OptProblem) + 8 * (len(vlib.SimStep._fields_) - 3) + 8


def test_streams_option_is_checked_without_a_gpu():
    with pytest.raises(ValueError, match="streams"):
        DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], streams='bogus')
    with pytest.raises(ValueError, match="streams"):
        start_env_batched(4, 2, 1, backend="host", streams="device")
    with pytest.raises(ValueError, match="streams"):
        start_env_batched(4, 2, 1, backend="device", streams="gpu")
    with pytest.raises(ValueError, match="lookahead"):
        DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], streams='device',
                             lookahead=True)
    env = DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], streams='device')
    assert env.stream_backend == 'device' and env._mt_keys.shape == (2, 624) and env._mt_keys.dtype == np.uint32
    rs = np.random.RandomState(0)                                      # the attached stream state is a valid MT19937 state
    rs.set_state(('MT19937', env._mt_keys[0], int(env._mt_pos[0])))
    assert DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2]).stream_backend == 'host'


def test_device_channels_stream_and_advance_refuse_bad_arguments_before_any_device_work():
    dc = DeviceChannels(2, 4, 4)
    ok = np.zeros((2, 4), np.int64)
    with pytest.raises(ValueError, match="set_grid"):
        dc.stream()
    with pytest.raises(ValueError, match="set_grid"):
        dc.advance(ok)
    for lanes in (np.zeros((3, 6)), np.zeros((4, 0)), np.zeros((4, 65)), np.zeros(6), [[1.0, 2.0], [1.0]], np.full((4, 6), np.nan)):
        with pytest.raises(ValueError, match="set_grid"):
            dc.set_grid(lanes, 750, 1299, 0.01)
    with pytest.raises(ValueError, match="finite"):
        dc.set_grid(np.zeros((4, 6)), np.inf, 1299, 0.01)
    dc.set_grid(LANES, 750, 1299, 0.01)
    with pytest.raises(ValueError, match="mobility"):
        dc.stream(mobility=1)
    with pytest.raises(ValueError, match="shape"):
        dc.advance(np.zeros((2, 5), np.int64))
    with pytest.raises(ValueError, match="integers"):
        dc.advance(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="32-bit"):
        dc.upload('keys', np.zeros((2, 624), np.uint64))
    with pytest.raises(ValueError, match="shape"):
        dc.upload('keys', np.zeros((2, 625), np.uint32))
    with pytest.raises(ValueError, match="integers"):
        dc.upload('dirs', np.zeros((2, 4)))
    with pytest.raises(ValueError, match="shape"):
        dc.upload('mtpos', np.zeros((3,), np.int32))
    with pytest.raises(ValueError, match="links"):
        DeviceChannels(2, 32, 4).advance(np.zeros((2, 32), np.int64))   # the observation's limit comes before the grid's
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}


def test_sim_streams_device_needs_the_device_backend_on_the_command_line(capsys):
    with pytest.raises(SystemExit) as exc:
        main(["--envs", "2", "--sim-streams", "device"])
    assert exc.value.code == 2 and "--sim-backend device" in capsys.readouterr().err
