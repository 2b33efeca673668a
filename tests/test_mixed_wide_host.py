"""Host side of the mixed wide walk (v2x_rollout_steps_mixed_wide / v2x_eval_steps_mixed_wide: the binding of v2x_traj_ws, the
walk argument of rl/device_sim.py's mixed calls and of MixedAgent, --mixed-trajectory-walk of rl/train.py and rl/run.py): no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from v2xgnn import lib as vlib
from v2xgnn.rl import run, train
from v2xgnn.rl.device_sim import (WALKS, eval_steps_mixed, resident_evaluate_steps_mixed, resident_rollout_steps_mixed,
                                  rollout_steps_mixed)
from v2xgnn.rl.mixed import MixedAgent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("v2x_rollout_steps_mixed_wide", "RolloutMixed"), ("v2x_eval_steps_mixed_wide", "EvalMixed"))


# ------------------------------------------------------------------------------------------------------- the binding
def test_the_entry_points_are_declared_exported_and_bound_alike():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    lib = C.CDLL(vlib.library_path())
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    for name, struct in ENTRY_POINTS:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        args = [a.strip() for a in m.group(1).split(',')]
        assert len(args) == 3 and args[1].startswith("const v2x_traj_ws*") and args[2].startswith("void*"), (name, args)
        assert hasattr(lib, name), name
        assert bound[name] == (C.c_int, [C.POINTER(getattr(vlib, struct)), C.POINTER(vlib.TrajWs), C.c_void_p]), name


FIELDS = ("wide_ws", "wide_ws_bytes", "split_ws", "split_ws_bytes")


def test_the_workspace_struct_has_the_size_and_the_offsets_of_the_header(tmp_path):
    """the header compiled as C by gcc, the host compiler csrc/Makefile builds libv2xsim.so with; CC names another one"""
    assert tuple(f[0] for f in vlib.TrajWs._fields_) == FIELDS
    assert C.sizeof(vlib.TrajWs) == 32 and [getattr(vlib.TrajWs, f).offset for f in FIELDS] == [0, 8, 16, 24]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "v2xgnn.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(v2x_traj_ws));\n'
                   + ''.join('  printf(" %%zu", offsetof(v2x_traj_ws, %s));\n' % f for f in FIELDS) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 0, 8, 16, 24]


# ------------------------------------------------------------------------------------------------------- the walk argument
class _Untouchable(object):
    """stands where a DeviceChannels or an environment would: any look at it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the walk is checked before the pools are looked at (read %r)" % name)


def test_an_unknown_walk_is_refused_before_any_device_work():
    assert WALKS == ('serial', 'wide')
    pools = [_Untouchable()]
    for walk in ('auto', 'split', None):
        text = "walk must be one of 'serial', 'wide', got %r" % (walk,)
        with pytest.raises(ValueError, match="rollout_steps_mixed: " + text):
            rollout_steps_mixed(pools, [None], [None], [None], [0], [1], 1.0, 0.1, walk=walk)
        with pytest.raises(ValueError, match="rollout_steps_mixed: " + text):
            resident_rollout_steps_mixed(pools, [None], [None], [None], [0], [1], 1.0, 0.1, walk=walk)
        with pytest.raises(ValueError, match="eval_steps_mixed: " + text):
            eval_steps_mixed(pools, [None], [None], [None], 1.0, 0.1, walk=walk)
        with pytest.raises(ValueError, match="eval_steps_mixed: " + text):
            resident_evaluate_steps_mixed(pools, [None], [None], [None], 1.0, 0.1, walk=walk)


class _FakeEnv(object):
    def __init__(self, n):
        self.n_Veh, self.n_RB, self.E = n, 4, 2
        self.observe_packed = lambda c: None
        self.packed_ok = lambda c: c == 4


def test_mixed_agent_refuses_a_walk_it_does_not_know_at_construction():
    for rollout in ('host', 'trajectory'):
        with pytest.raises(ValueError, match="MixedAgent: trajectory_walk: walk must be one of 'serial', 'wide', got 'auto'"):
            MixedAgent([_FakeEnv(8), _FakeEnv(12)], None, 16, rollout=rollout, trajectory_walk='auto')
    # a known walk passes that check: the next refusal is the constructor's own of host simulators
    with pytest.raises(ValueError, match="rollout='trajectory' steps every environment on the device"):
        MixedAgent([_FakeEnv(8), _FakeEnv(12)], None, 16, rollout='trajectory', trajectory_walk='wide')


# ------------------------------------------------------------------------------------------------------- the command lines
DEVICE = ["--mixed-sim-backend", "device", "--mixed-sim-streams", "device"]
MIXED = ["--mixed-links", "8,12", "--envs", "2"]


@pytest.mark.parametrize("argv,want", [
    (MIXED, ("host", "serial")),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory"], ("trajectory", "serial")),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--mixed-trajectory-walk", "serial"], ("trajectory", "serial")),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--mixed-trajectory-walk", "wide"], ("trajectory", "wide")),
])
def test_train_accepts_the_wide_walk_with_the_trajectory_rollout(argv, want, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    _, args = train.parse_args(argv)
    assert (args.mixed_rollout, args.mixed_trajectory_walk) == want


@pytest.mark.parametrize("argv,text", [
    (MIXED + ["--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --mixed-rollout trajectory"),
    (MIXED + DEVICE + ["--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --mixed-rollout trajectory"),
    (["--links", "8", "--envs", "2", "--mixed-trajectory-walk", "wide"], "need --mixed-links"),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--mixed-trajectory-walk", "auto"], "invalid choice: 'auto'"),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--trajectory-walk", "wide"], "--mixed-links walks serially"),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--mixed-trajectory-walk", "wide", "--trajectory-walk", "wide"],
     "--mixed-links walks serially"),
    (MIXED + DEVICE + ["--mixed-rollout", "trajectory", "--trajectory-walk", "wide", "--trajectory-streams", "split"],
     "--mixed-links walks serially"),
])
def test_train_refuses_the_wide_walk_elsewhere_with_a_message(argv, text, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    with pytest.raises(SystemExit) as exc:
        train.parse_args(argv)
    assert exc.value.code == 2
    assert text in capsys.readouterr().err


RUN = ["--save-dir", "w"]
RUN_DEVICE = ["--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device"]


@pytest.mark.parametrize("argv,want", [
    (RUN + ["--mixed-links", "8,12"], ("host", "serial")),
    (RUN + ["--mixed-links", "8,12"] + RUN_DEVICE, ("device", "serial")),
    (RUN + ["--mixed-links", "8,12", "--eval-links", "8,16,28", "--envs", "4"] + RUN_DEVICE + ["--mixed-trajectory-walk", "wide"],
     ("device", "wide")),
])
def test_run_accepts_the_wide_walk_with_the_device_evaluation(argv, want):
    _, args = run.parse_args(argv)
    assert (args.eval_backend, args.mixed_trajectory_walk) == want


@pytest.mark.parametrize("argv,text", [
    (RUN + ["--mixed-links", "8,12", "--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --eval-backend device"),
    (RUN + ["--mixed-links", "8,12", "--sim-backend", "device", "--sim-streams", "device", "--mixed-trajectory-walk", "wide"],
     "--mixed-trajectory-walk wide needs --eval-backend device"),
    (RUN + ["--links", "8"] + RUN_DEVICE + ["--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --mixed-links"),
    (RUN + ["--mixed-links", "8,12"] + RUN_DEVICE + ["--trajectory-walk", "wide"], "--mixed-links walks serially"),
    (RUN + ["--mixed-links", "8,12"] + RUN_DEVICE + ["--mixed-trajectory-walk", "wide", "--trajectory-walk", "wide"],
     "--mixed-links walks serially"),
])
def test_run_refuses_the_wide_walk_elsewhere_with_a_message(argv, text, capsys):
    with pytest.raises(SystemExit) as exc:
        run.parse_args(argv)
    assert exc.value.code == 2
    assert text in capsys.readouterr().err
