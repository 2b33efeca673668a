"""No GPU needed: the C ABI of the receiver-form rollout with the split stream phase (v2x_rollout_recv_split_workspace_bytes,
v2x_rollout_steps_recv_split) is declared, exported and bound alike; the split workspace's size is the formula the header
documents, for 3..128 links; every refusal of the call comes back as V2X_EINVAL before anything is launched (the pointers
handed over are never dereferenced by the host: a check that let one through would reach a launch, which fails without a
device); and the Python layers take receiver_streams / --receiver-streams / stream_phase where the call serves them and
refuse them elsewhere, before any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, OptProblem, SimStep
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config
from v2xgnn.rl.train import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]
P = 0x10000                                              # a non-null, 256-byte aligned "device pointer": never dereferenced
SECTIONS = ('traj_xe', 'traj_recv', 'traj_flags', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs', 'row_ptr', 'col_idx')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_rollout_recv_split_workspace_bytes", "int64_t", C.c_int64, 5),
                                                    ("v2x_rollout_steps_recv_split", "int", C.c_int, 6)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


# ------------------------------------------------------------------------------------------------------- the workspace size
def documented_bytes(E, n, rb, T, n_lanes):
    """the formula of include/v2xgnn.h (v2x_rollout_steps_recv_split), restated"""
    A = lambda x: -(-x // 256) * 256                                                         # noqa: E731
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    NB = 1 + -(-T * (2 * n_u + 4 * n * n_lanes) // 624)
    return A(4 * E * NB * 624) + A(8 * (T + 1) * E)


@pytest.mark.parametrize("E,n,rb,T,n_lanes", [(1, 3, 1, 1, 1), (3, 65, 4, 4, 4), (1, 128, 4, 50, 4)])
def test_split_workspace_bytes_is_the_documented_formula(E, n, rb, T, n_lanes):
    from v2xgnn.rl.device_sim import split_workspace_layout
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T, n_lanes)
    assert lib.v2x_rollout_recv_split_workspace_bytes(E, n, rb, T, n_lanes) == want > 0
    offs, size = split_workspace_layout(E, n, rb, T, n_lanes)            # what DeviceChannels sizes the allocation by
    assert size == want and offs['words'] == 0 and offs['off'] % 256 == 0


def test_split_workspace_of_one_simulator_is_what_the_design_notes_say():
    lib = vlib.load_library()
    assert lib.v2x_rollout_recv_split_workspace_bytes(1, 100, 4, 50, 2) == documented_bytes(1, 100, 4, 50, 2)
    assert 36e6 < lib.v2x_rollout_recv_split_workspace_bytes(1, 100, 4, 50, 2) < 37e6      # "about 36 MB"
    assert 59e6 < lib.v2x_rollout_recv_split_workspace_bytes(1, 128, 4, 50, 2) < 60e6      # "59 MB"
    one, ten = (lib.v2x_rollout_recv_split_workspace_bytes(E, 64, 4, 50, 2) for E in (1, 10))
    assert abs(ten - 10 * one) <= 10 * 512                                                   # linear in E (up to the rounding)


@pytest.mark.parametrize("args,word", [((1, 2, 1, 1, 2), "n = 2"), ((1, 129, 4, 1, 2), "n = 129"), ((1, 40, 6, 1, 2), "rb = 6"),
                                       ((0, 40, 4, 1, 2), "E = 0"), ((1, 40, 4, 0, 2), "T = 0"), ((1000, 128, 4, 200, 2), "32-bit"),
                                       ((1, 40, 4, 1, 0), "n_lanes = 0"), ((1, 40, 4, 1, 65), "n_lanes = 65")])
def test_split_workspace_bytes_is_negative_on_sizes_outside_the_limits(args, word):
    lib = vlib.load_library()
    assert lib.v2x_rollout_recv_split_workspace_bytes(*args) == V2X_EINVAL < 0
    text = lib.v2x_last_error(None).decode()
    assert word in text and text.startswith(("rollout_steps_recv", "rollout_recv_split_workspace_bytes")), text


# ------------------------------------------------------------------------------------------------------- the argument checks
def _call(E=2, n=40, rb=4, T=3, ws=P, ws_bytes=None, split_ws=P + (1 << 30), split_bytes=None, n_lanes=2, **over):
    """v2x_rollout_steps_recv_split on made-up pointers -> (return code, error text)"""
    from v2xgnn.rl.device_sim import recv_workspace_layout, split_workspace_layout
    lib = vlib.load_library()
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    prob = dict(E=E, n=n, rb=rb, pad_=0, v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300, dest=P, p_v2v=10.0, p_v2i=23.0,
                veh_gain=3.0, bs_gain=8.0, bs_nf=5.0, veh_nf=9.0, sig2=1e-11, w_v2v=0.0, w_v2i=0.0)
    names = [f[0] for f in SimStep._fields_ if f[1] is C.c_void_p and f[0] not in ('actions', 'mask', 'col', 'regular')]
    ptr = {k: P for k in names}
    ptr.update(v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300)
    s = SimStep(problem=OptProblem(**prob), n_lanes=n_lanes, n_u=n_u, timestep=0.01, width=750.0, height=1299.0, power=10.0,
                actions=None, **ptr)
    ok = 3 <= n <= 128 and 1 <= rb <= n and 3 * rb + 1 <= 16 and T >= 1 and E >= 1
    offs, size = recv_workspace_layout(E, n, rb, T) if ok else ({k: 256 * i for i, k in enumerate(SECTIONS)}, 1 << 20)
    need = split_workspace_layout(E, n, rb, T, n_lanes)[1] if ok and n_lanes >= 1 else 1 << 20
    r = dict(model=None, q=None, explore=P, random_actions=P, actions=P, recv=P, flags=P, w_v2v=1.0, w_v2i=0.1, T=T, pad_=0,
             edge_base=None, rep_xe=P, rep_xe_next=P, rep_recv=P, rep_action=P, rep_reward=P, head=0, capacity=8, result_reward=P,
             result_flags=P)
    r.update({k: (ws or P) + offs[k] for k in SECTIONS})
    r.update(over)
    rc = lib.v2x_rollout_steps_recv_split(C.byref(vlib.RolloutRecv(step=s, **r)), ws, size if ws_bytes is None else ws_bytes,
                                          split_ws, need if split_bytes is None else split_bytes, None)
    return rc, lib.v2x_last_error(None).decode()


REFUSALS = [
    # the split workspace's own three ...
    (dict(split_ws=None), "split-stream workspace is null"), (dict(split_ws=P + 64), "256-byte aligned"),
    (dict(split_bytes=1024), "split-stream workspace of E = 2, n = 40"), (dict(n=128, E=1, T=50, capacity=64, split_bytes=59 * 10 ** 6), "needs 59"),
    # ... after every check of v2x_rollout_steps_recv (a sample of each kind: sizes, ring, workspace, pointers, the step)
    (dict(n=129), "n = 129"), (dict(T=0), "T = 0"), (dict(T=5), "T E <= capacity"), (dict(head=8), "head"),
    (dict(ws_bytes=1024), "needs"), (dict(ws=None), "workspace"), (dict(ws=P + 64), "256-byte aligned"),
    (dict(rep_recv=None), "rep_recv"), (dict(result_flags=None), "null result"), (dict(recv=None), "null"),
    (dict(n_lanes=0), "n_lanes"), (dict(n_lanes=65), "n_lanes"), (dict(col_idx=P), "first eight sections"),
]


@pytest.mark.parametrize("over,word", REFUSALS)
def test_a_bad_call_is_refused_before_anything_is_launched(over, word):
    rc, text = _call(**over)
    assert rc == V2X_EINVAL and word in text and text.startswith(("rollout_steps_recv_split", "rollout_steps_recv", "sim_")), (rc, text)


def test_the_chain_checks_come_first_and_a_null_rollout_is_refused():
    lib = vlib.load_library()
    assert lib.v2x_rollout_steps_recv_split(None, P, 1 << 20, P, 1 << 20, None) == V2X_EINVAL
    assert "rollout_steps_recv_split: null rollout" in lib.v2x_last_error(None).decode()
    rc, text = _call(ws=None, split_ws=None)                             # both wrong: the chain form's check speaks
    assert rc == V2X_EINVAL and "split" not in text.split(":", 1)[1] and "workspace is null" in text, text


# ------------------------------------------------------------------------------------------------------- the Python layers
def _dev_env(streams, E=2):
    return DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=E, seeds=list(range(1, E + 1)), streams=streams)


def _gpu_brain():
    b = types.SimpleNamespace(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16)
    b.model = types.SimpleNamespace(engine=types.SimpleNamespace(_h=1, device='cpu'), trainer=None)      # looks like the gfx950 engine
    return b


def _mk(env, n=40, **kw):
    return Agent(n, 4, 1, 16, env, RL_Config(), brain=_gpu_brain(), **kw)


def test_agent_takes_receiver_streams_with_receivers_and_trajectory_only():
    agent = _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory', receiver_streams='split')
    assert agent.receiver_streams == 'split' and agent.trajectory_streams == 'chain' and agent.rollout_backend == 'trajectory'
    assert _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory').receiver_streams == 'chain'
    assert _mk(_dev_env('device'), n=20).receiver_streams == 'chain'     # 'chain' is valid everywhere: nothing existing changes
    needs = "receiver_streams='split' needs device_replay='receivers' and rollout_backend='trajectory'"
    for kw in (dict(device_replay='receivers'), dict(device_replay='receivers', rollout_backend='host'),
               dict(n=20, device_replay=True, rollout_backend='trajectory'),
               dict(n=20, device_replay=True, rollout_backend='trajectory', trajectory_walk='wide', trajectory_streams='split'),
               dict(n=20, device_replay='auto'), dict(n=40, device_replay=False)):
        with pytest.raises(ValueError, match=needs):
            _mk(_dev_env('device'), receiver_streams='split', **kw)
    with pytest.raises(ValueError, match="receiver_streams must be one of"):
        _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory', receiver_streams='wide')
    with pytest.raises(ValueError, match="chain stream phase"):          # the other option's refusal stands next to the new one
        _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory', trajectory_walk='wide',
            trajectory_streams='split', receiver_streams='split')


def test_command_line_takes_receiver_streams_with_receivers_and_trajectory_only(capsys):
    dev = ["--sim-backend", "device", "--sim-streams", "device", "--envs", "1"]
    _, args = parse_args(["--links", "100", "--replay", "receivers", "--rollout", "trajectory", "--receiver-streams", "split"] + dev)
    assert (args.replay, args.rollout, args.receiver_streams, args.trajectory_streams) == ("receivers", "trajectory", "split", "chain")
    _, args = parse_args(["--links", "100", "--replay", "receivers", "--rollout", "trajectory"] + dev)
    assert args.receiver_streams == "chain"
    needs = "--receiver-streams split needs --replay receivers --rollout trajectory"
    for argv, word in ((["--receiver-streams", "split"], needs),
                       (["--replay", "receivers", "--receiver-streams", "split"], needs),
                       (["--rollout", "trajectory", "--receiver-streams", "split"] + dev, needs),
                       (["--rollout", "trajectory", "--trajectory-walk", "wide", "--trajectory-streams", "split",
                         "--receiver-streams", "split"] + dev, needs),
                       (["--mixed-links", "8,12", "--envs", "2", "--receiver-streams", "split"], needs),
                       (["--replay", "receivers", "--rollout", "trajectory", "--receiver-streams", "wide"] + dev, "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert word in capsys.readouterr().err, argv


def test_channels_and_environment_check_the_stream_phase_before_any_device_work():
    dc = DeviceChannels(2, 40, 4)
    dc.set_grid(LANES, 750.0, 1299.0, 0.01)
    tensor = lambda *shape: types.SimpleNamespace(shape=(8,) + shape, is_contiguous=lambda: True)        # noqa: E731
    st = {'xe': tensor(40, 16), 'xe_next': tensor(40, 16), 'recv': tensor(40), 'action': tensor(40), 'reward': tensor()}
    ex, ra, own = np.ones((3, 2), np.uint8), np.zeros((3, 2, 40), np.int32), [0, 0]
    for phase in ('chain', 'split'):
        T, e, r, o = dc.check_rollout_steps_recv(ex, ra, st, 5, 8, own, stream_phase=phase)
        assert T == 3 and e.dtype == np.uint8 and r.dtype == np.int32 and o.tolist() == [0, 0]
    for phase in ('wide', 'serial', None, 1):
        with pytest.raises(ValueError, match="stream_phase must be one of 'chain', 'split'"):
            dc.check_rollout_steps_recv(ex, ra, st, 5, 8, own, stream_phase=phase)
        with pytest.raises(ValueError, match="stream_phase must be one of 'chain', 'split'"):
            dc.rollout_steps_recv(ex, ra, st, 5, 8, 1.0, 0.1, own=own, stream_phase=phase)
    assert dc.stream_phase_calls == {'chain': 0, 'split': 0}
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').rollout_steps_recv(np.ones((1, 2), np.uint8), np.zeros((1, 2, 4), np.int32), {}, 0, 8, 1.0, 0.1,
                                            stream_phase='split')
