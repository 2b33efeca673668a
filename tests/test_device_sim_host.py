"""Host-side checks of the device simulator step (rl/device_sim.py, csrc/v2xsimdev.hip): the C ABI is declared and
exported, the argument checks raise ValueError before any device work (this file runs without a GPU: a check that came after
the device initialisation would raise RuntimeError instead), the training driver's switch, and the constants header."""
import ctypes
import os
import re

import numpy as np
import pytest

from v2xgnn.lib import library_path
from v2xgnn.rl import BatchedEnviron, DeviceBatchedEnviron, DeviceChannels, Environ, native_sim
from v2xgnn.rl import train as train_mod
from v2xgnn.rl.device_sim import uniforms_per_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_CALLS = ("v2x_sim_channels", "v2x_sim_observe", "v2x_sim_rates")


def _lanes():
    up = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
    down = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
    left = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
    right = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
    return down, up, left, right


def test_header_declares_and_library_exports_the_sim_calls():
    with open(os.path.join(ROOT, "include", "v2xgnn.h")) as f:
        header = f.read()
    for name in SIM_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert os.path.exists(library_path()), "libv2xgnn.so is not built"
    lib = ctypes.CDLL(library_path())
    for name in SIM_CALLS:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("n", [2, 32])
def test_observe_refuses_two_and_thirty_two_links(n):
    dc = DeviceChannels(2, n, 2)
    with pytest.raises(ValueError, match="links"):
        dc.observe(np.zeros((2, n), np.int64))
    assert dc.torch is None                                   # nothing touched the device


def test_observe_refuses_more_blocks_than_links_and_rows_wider_than_sixteen():
    with pytest.raises(ValueError, match="n_RB <= links"):
        DeviceChannels(1, 3, 4).observe(np.zeros((1, 3), np.int64))
    with pytest.raises(ValueError, match="packed width"):
        DeviceChannels(1, 8, 6).observe(np.zeros((1, 8), np.int64))


def test_constructor_limits():
    for E, n, rb in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 129, 4), (1, 4, 0), (1, 4, 17)):
        with pytest.raises(ValueError):
            DeviceChannels(E, n, rb)
    with pytest.raises(ValueError, match="unknown constants"):
        DeviceChannels(1, 4, 4, constants={"p_v2x": 1.0})


def test_step_refuses_a_wrong_number_of_uniforms_and_wrong_shapes():
    dc = DeviceChannels(2, 4, 4)
    n_u = uniforms_per_step(4, 4)
    assert n_u == 4 + 16 + 32 + 128 and dc.n_u == n_u
    vel, pos = np.full((2, 4), 12.0), np.zeros((2, 4, 2))
    for bad in (n_u - 2, n_u + 2, n_u + 1):
        with pytest.raises(ValueError, match="u: an array of shape"):
            dc.step(np.zeros((2, bad)), vel, pos)
    with pytest.raises(ValueError, match="vel"):
        dc.step(np.zeros((2, n_u)), np.zeros((2, 5)), pos)
    with pytest.raises(ValueError, match="pos"):
        dc.step(np.zeros((2, n_u)), vel, np.zeros((2, 4)))
    assert dc.torch is None


def test_rates_refuse_non_integer_actions():
    dc = DeviceChannels(2, 4, 4)
    with pytest.raises(ValueError, match="integers"):
        dc.rates(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="shape"):
        dc.rates(np.zeros((2, 5), np.int64))
    with pytest.raises(ValueError, match="integers"):
        dc.observe(np.zeros((2, 4)))                          # receivers, too
    assert dc.torch is None


def test_device_environment_refuses_lookahead_and_bad_sizes():
    if not native_sim.available():
        pytest.fail("libv2xsim.so is not built")
    lanes = _lanes()
    with pytest.raises(ValueError, match="look-ahead"):
        DeviceBatchedEnviron(*lanes, 750, 1299, n_envs=2, seeds=[1, 2], lookahead=True)
    with pytest.raises(ValueError, match="seed"):
        DeviceBatchedEnviron(*lanes, 750, 1299, n_envs=1)
    env = DeviceBatchedEnviron(*lanes, 750, 1299, n_envs=2, seeds=[1, 2])
    assert isinstance(env, BatchedEnviron) and not env._one_call_step() and env.lookahead is False
    with pytest.raises(ValueError, match="look-ahead"):
        env.lookahead = True
    with pytest.raises(ValueError, match="links"):
        env.new_random_game(32)
    env.n_RB = 6
    with pytest.raises(ValueError, match="packed width"):
        env.new_random_game(8)
    env.n_RB = 4
    env.n_Veh = 4
    with pytest.raises(ValueError, match="integers"):
        env.compute_reward_with_channel_selection(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="n_channels == n_RB"):
        env.observe_packed(3)


def test_train_driver_switch_defaults_to_the_host_simulator():
    ap = train_mod.build_parser()
    assert ap.parse_args([]).sim_backend == "host"
    assert ap.parse_args(["--sim-backend", "device"]).sim_backend == "device"
    with pytest.raises(SystemExit):
        ap.parse_args(["--sim-backend", "elsewhere"])
    env = train_mod.start_env_batched(4, 2, 5, lookahead=False)
    assert type(env) is BatchedEnviron
    with pytest.raises(ValueError, match="backend"):
        train_mod.start_env_batched(4, 2, 5, backend="elsewhere")


def test_constants_header_agrees_with_the_python_simulator():
    with open(os.path.join(ROOT, "include", "v2xsim_const.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    values = {}
    for decl in re.findall(r"static const double ([^;]+);", text):
        for name, expr in re.findall(r"(\w+)\s*=\s*([^,]+)", decl):
            assert re.fullmatch(r"[0-9.\s/*+-]+", expr), expr
            values[name] = float(eval(expr))
    twopi = re.search(r"#define TWOPI\s+([0-9.]+)", text)
    assert twopi and float(twopi.group(1)) == 2.0 * np.pi
    want = dict(V2V_H=Environ.V2V_H, FC=Environ.FC, V2V_DECORR=Environ.V2V_DECORR, V2V_SHADOW_STD=Environ.V2V_SHADOW_STD,
                V2I_H_BS=Environ.V2I_H_BS, V2I_H_MS=Environ.V2I_H_MS, V2I_DECORR=Environ.V2I_DECORR,
                V2I_SHADOW_STD=Environ.V2I_SHADOW_STD, BS_X=Environ.BS_POSITION[0], BS_Y=Environ.BS_POSITION[1])
    assert values == {k: float(v) for k, v in want.items()}
    for src in ("v2xsim.c", "v2xsimdev.hip"):                 # one definition: both translation units include the header
        with open(os.path.join(ROOT, "globecom2020-resourceallocationgnn_amd", "csrc", src)) as f:
            body = f.read()
        assert '#include "../../include/v2xsim_const.h"' in body, src
        assert not re.search(r"static const double\s+V2V_H", body), src
