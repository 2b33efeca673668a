"""No GPU needed: the C ABI of the device episode reset (v2x_sim_reset, v2x_sim_reset_draw) is declared, exported and bound
alike, reset_tie_flags flags the resets whose receivers depend on a sort's order among equal keys, and the Python layers and
the command lines refuse reset='device' where it cannot run."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.rl import DeviceBatchedEnviron, DeviceChannels
from v2xgnn.rl import evaluate, run, train
from v2xgnn.rl.device_sim import check_reset_grid, reset_tie_flags
from v2xgnn.rl.train import start_env_batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]      # up, down, left, right


def _header():
    return open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read()


@pytest.mark.parametrize("name", ["v2x_sim_reset", "v2x_sim_reset_draw"])
def test_reset_entry_points_are_declared_exported_and_bound_alike(name):
    hdr = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert [a.strip() for a in m.group(1).split(',')] == ["const v2x_sim_reset_args* r", "void* stream"]
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert bound[name] == (C.c_int, [C.POINTER(vlib.SimReset), C.c_void_p])


def test_reset_binding_has_the_fields_of_the_declared_struct():
    body = re.search(r'typedef struct v2x_sim_reset_args \{(.*?)\} v2x_sim_reset_args;', _header(), flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [re.sub(r'[\s*]', '', d.split()[-1]) for d in body.split(';') if d.strip()]
    assert names == [f[0] for f in vlib.SimReset._fields_] == ['step', 'vel', 'dest', 'status']
    assert vlib.SimReset._fields_[0][1] is vlib.SimStep and C.sizeof(vlib.SimReset) == C.sizeof(vlib.SimStep) + 24


def test_reset_tie_flags_on_hand_made_positions():
    # state 0: vehicles 1 and 2 stand on one spot, and link 0's receiver is one of them (a coincident pair);
    # state 1: vehicles 1 and 2 are both 5 away from vehicle 0, whose receiver is vehicle 2 (an equidistant pair);
    # state 2: the same positions, but every receiver has its distance to itself alone; state 3: all distances distinct
    pos = np.array([[[0, 0], [7, 1], [7, 1], [100, 50]],
                    [[0, 0], [3, 4], [4, -3], [100, 50]],
                    [[0, 0], [3, 4], [4, -3], [100, 50]],
                    [[0, 0], [1, 0], [3, 0], [7, 0]]], np.float64)
    dest = np.array([[1, 0, 0, 0],
                     [2, 0, 0, 0],
                     [3, 0, 0, 0],
                     [1, 2, 3, 2]], np.int64)
    flags = reset_tie_flags(pos, dest)
    assert flags.dtype == np.uint8 and flags.tolist() == [1, 1, 0, 0]
    # a link whose receiver stands on the link's own spot: "the link itself included"
    assert reset_tie_flags(pos[:1], np.array([[3, 2, 0, 0]])).tolist() == [1]
    assert reset_tie_flags(pos[:1], np.array([[3, 0, 0, 0]])).tolist() == [0]


def test_reset_option_is_checked_at_construction_without_a_gpu():
    make = lambda **kw: DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], **kw)   # noqa: E731
    assert make().reset_backend == 'host' and make(streams='device').reset_backend == 'host'
    env = make(streams='device', reset='device')
    assert env.reset_backend == 'device' and env.reset_ties == 0 and not any(env.reset_stats.values())
    with pytest.raises(ValueError, match="reset must be 'host' or 'device'"):
        make(streams='device', reset='gpu')
    with pytest.raises(ValueError, match="reset='device' needs streams='device'"):
        make(reset='device')
    with pytest.raises(ValueError, match="reset='device' needs streams='device'"):
        make(streams='host', reset='device')
    # a lane off the grid of 2^-10, a lane beyond 2^15, a map too large for exact squared distances
    for lanes, width in (([1.75, 5.0 + 2.0 ** -11], 750), ([1.75, 40000.0], 750), ([1.75, -1.0], 750), ([1.75, 5.25], 32768),
                         ([1.75, 5.25], 750.5)):
        with pytest.raises(ValueError, match=r"2\^15"):
            DeviceBatchedEnviron(LANES[1], lanes, LANES[2], LANES[3], width, 1299, n_envs=2, seeds=[1, 2], streams='device',
                                 reset='device')
        DeviceBatchedEnviron(LANES[1], lanes, LANES[2], LANES[3], width, 1299, n_envs=2, seeds=[1, 2], streams='device')   # 'host' takes it
    check_reset_grid("t", LANES, 750, 1299)
    with pytest.raises(ValueError, match="reset"):
        start_env_batched(4, 2, 1, backend="device", streams="host", reset="device")
    with pytest.raises(ValueError, match="reset"):
        start_env_batched(4, 2, 1, backend="host", reset="device")
    with pytest.raises(ValueError, match="reset"):
        start_env_batched(4, 2, 1, backend="device", streams="device", reset="gpu")


def test_device_channels_reset_refuses_bad_arguments_before_any_device_work():
    dc = DeviceChannels(2, 8, 4)
    with pytest.raises(ValueError, match="set_grid"):
        dc.reset()
    with pytest.raises(ValueError, match="set_grid"):
        dc.reset_draw()
    dc.set_grid(LANES, 750.5, 1299, 0.01)
    with pytest.raises(ValueError, match="width"):
        dc.reset()
    for n in (6, 3, 30, 32):
        other = DeviceChannels(2, n, 3)
        other.set_grid(LANES, 750, 1299, 0.01)
        with pytest.raises(ValueError, match="multiple of 4 in 4..28"):
            other.reset_draw()
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}


def _exit_message(fn, argv, capsys):
    with pytest.raises(SystemExit) as exc:
        fn(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--envs", "2", "--sim-reset", "device"],
                                  ["--envs", "2", "--sim-backend", "device", "--sim-reset", "device"]])
def test_sim_reset_device_needs_device_streams_on_the_training_command_line(argv, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    assert "--sim-reset device needs --sim-backend device --sim-streams device" in _exit_message(train.main, argv, capsys)


def test_mixed_sim_reset_on_the_training_command_line(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    mixed = ["--mixed-links", "8,12", "--envs", "2"]
    assert "--mixed-sim-reset device needs --mixed-sim-backend device --mixed-sim-streams device" in _exit_message(
        train.main, mixed + ["--mixed-sim-backend", "device", "--mixed-sim-reset", "device"], capsys)
    assert "need --mixed-links" in _exit_message(train.main, ["--links", "8", "--envs", "2", "--mixed-sim-reset", "device"], capsys)
    assert "--mixed-links steps host simulators" in _exit_message(train.main, mixed + ["--sim-reset", "device"], capsys)
    _, args = train.parse_args(mixed + ["--mixed-sim-backend", "device", "--mixed-sim-streams", "device", "--mixed-sim-reset", "device"])
    assert args.mixed_sim_reset == "device" and args.sim_reset == "host"
    _, args = train.parse_args(mixed)
    assert args.mixed_sim_reset == "host"
    _, args = train.parse_args(["--envs", "2", "--sim-backend", "device", "--sim-streams", "device", "--sim-reset", "device"])
    assert args.sim_reset == "device"
    assert train.parse_args(["--envs", "2"])[1].sim_reset == "host"


@pytest.mark.parametrize("driver", [run, evaluate])
def test_sim_reset_device_needs_device_streams_on_the_evaluation_command_lines(driver, capsys):
    base = ["--save-dir", "nowhere"]
    for extra in (["--sim-reset", "device"], ["--sim-backend", "device", "--sim-reset", "device"]):
        assert "--sim-reset device needs --sim-backend device --sim-streams device" in _exit_message(driver.main, base + extra, capsys)


def test_sim_reset_on_the_mixed_evaluation_command_line(capsys):
    mixed = ["--save-dir", "nowhere", "--mixed-links", "8,12"]
    assert "--sim-reset device needs --sim-backend device --sim-streams device" in _exit_message(
        run.main, mixed + ["--sim-backend", "device", "--sim-reset", "device"], capsys)
    _, args = run.parse_args(mixed + ["--sim-backend", "device", "--sim-streams", "device", "--sim-reset", "device"])
    assert args.sim_reset == "device"
    assert run.parse_args(mixed)[1].sim_reset == "host"
