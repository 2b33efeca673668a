"""No GPU needed: the C ABI of the resident rollout at 3..128 links on the receiver replay (v2x_sim_observe_recv,
v2x_csr_from_recv, v2x_rollout_recv_workspace_bytes, v2x_rollout_steps_recv) is declared, exported and bound alike; the
workspace size is the formula the header documents; every refusal of the call comes back as V2X_EINVAL before anything is
launched (the pointers handed over are never dereferenced by the host: a check that let one through would reach a launch,
which fails without a device); ReceiverReplay.reserve / commit keep head, size and the own-receiver table; and the Python
layers refuse what the call does not serve before any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, OptProblem, SimStep
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config
from v2xgnn.rl.batched_env import BatchedEnviron
from v2xgnn.rl.replay import ReceiverReplay
from v2xgnn.rl.train import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]
P = 0x10000                                              # a non-null, 256-byte aligned "device pointer": never dereferenced
SECTIONS = ('traj_xe', 'traj_recv', 'traj_flags', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs', 'row_ptr', 'col_idx')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_sim_observe_recv", "int", C.c_int, 17),
                                                    ("v2x_csr_from_recv", "int", C.c_int, 8),
                                                    ("v2x_rollout_recv_workspace_bytes", "int64_t", C.c_int64, 4),
                                                    ("v2x_rollout_steps_recv", "int", C.c_int, 4)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


def test_binding_has_the_fields_of_the_declared_struct_in_order():
    body = re.search(r'typedef struct v2x_rollout_recv \{(.*?)\} v2x_rollout_recv;', _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part) for part in decl.split(None, 1)[1].split(',')]
    names = [n.replace('uint8_t', '').replace('int32_t', '') for n in names]      # ("const T* name": the qualifier is split off first)
    R = vlib.RolloutRecv
    fields = [f[0] for f in R._fields_]
    assert names == fields, (names, fields)
    at = fields.index('traj_xe')
    assert tuple(fields[at:at + 8]) == SECTIONS and fields[at + 8] == 'edge_base'
    kinds = dict(R._fields_)
    assert kinds['batch'] is vlib.Batch and kinds['step'] is SimStep and kinds['T'] is C.c_int32 and kinds['head'] is C.c_int64
    pointers = sum(1 for _, k in R._fields_ if k is C.c_void_p)
    # no padding anywhere: pointers, the batch, the step, two weights, T + pad_, head + capacity
    assert C.sizeof(R) == 8 * pointers + C.sizeof(vlib.Batch) + C.sizeof(SimStep) + 16 + 8 + 16


# ------------------------------------------------------------------------------------------------------- the workspace size
def documented_bytes(E, n, rb, T):
    """the formula of include/v2xgnn.h (v2x_rollout_steps_recv), restated"""
    A = lambda x: -(-x // 256) * 256                                                         # noqa: E731
    n_u, n_el = n + n * n + 2 * n * rb + 2 * n * n * rb, n + n * n
    return (A(4 * (T + 1) * E * n * 16) + A(4 * (T + 1) * E * n) + A((T + 1) * E) + A(8 * T * E * n * n * rb) + A(8 * T * E * n * rb)
            + A(8 * T * E * n) + A(4 * (T * E * n + 1)) + A(4 * T * E * n * (n - 1)) + A(8 * T * E * n_u) + A(16 * T * E * n)
            + A(8 * T * E * n_el) + A(8 * T * E * n_el) + A(8 * (T - 1) * E * n * (3 * rb + 1)) + A(8 * (T - 1) * E * n * rb))


@pytest.mark.parametrize("E,n,rb,T", [(1, 3, 1, 1), (3, 5, 4, 3), (2, 31, 5, 2), (2, 32, 4, 3), (2, 65, 4, 3), (1, 128, 5, 1), (1, 100, 4, 50)])
def test_workspace_bytes_is_the_documented_formula(E, n, rb, T):
    from v2xgnn.rl.device_sim import recv_workspace_layout, wide_workspace_layout
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T)
    assert lib.v2x_rollout_recv_workspace_bytes(E, n, rb, T) == want
    offs, size = recv_workspace_layout(E, n, rb, T)                      # what DeviceChannels carves the allocation by
    assert size == want and tuple(offs) == SECTIONS + ('wide',)
    o = [offs[k] for k in SECTIONS + ('wide',)]
    assert o[0] == 0 and all(x % 256 == 0 for x in o)
    raw = [4 * (T + 1) * E * n * 16, 4 * (T + 1) * E * n, (T + 1) * E, 8 * T * E * n * n * rb, 8 * T * E * n * rb, 8 * T * E * n,
           4 * (T * E * n + 1), 4 * T * E * n * (n - 1)]
    assert all(0 <= o[i + 1] - o[i] - raw[i] < 256 for i in range(8))    # back to back: every array fits, nothing overlaps
    assert size - offs['wide'] == wide_workspace_layout(E, n, rb, T)[1]  # the wide walk's own six, in its own layout


def test_workspace_of_one_simulator_at_100_links_is_what_the_design_notes_say():
    lib = vlib.load_library()
    assert lib.v2x_rollout_recv_workspace_bytes(1, 100, 4, 50) == 63735040
    assert 8 * 50 * (100 + 100 * 100 + 2 * 100 * 4 + 2 * 100 * 100 * 4) == 36360000        # of which the uniforms


@pytest.mark.parametrize("E,n,rb,T", [(1, 2, 1, 1), (1, 129, 4, 1), (1, 4, 5, 1), (1, 4, 4, 0), (0, 4, 4, 1), (1, 8, 6, 1), (65536, 4, 4, 1),
                                      (1, 4, 0, 1), (1, 4, 4, -1), (1000, 128, 4, 200)])
def test_workspace_bytes_is_negative_on_sizes_outside_the_limits(E, n, rb, T):
    lib = vlib.load_library()
    assert lib.v2x_rollout_recv_workspace_bytes(E, n, rb, T) == V2X_EINVAL < 0
    assert "rollout_steps_recv" in lib.v2x_last_error(None).decode()


# ------------------------------------------------------------------------------------------------------- the argument checks
def _err(lib):
    return lib.v2x_last_error(None).decode()


def _call(E=2, n=40, rb=4, T=3, ws=P, ws_bytes=None, step_null=(), **over):
    """v2x_rollout_steps_recv on made-up pointers -> (return code, error text)"""
    from v2xgnn.rl.device_sim import recv_workspace_layout
    lib = vlib.load_library()
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    prob = dict(E=E, n=n, rb=rb, pad_=0, v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300, dest=P, p_v2v=10.0, p_v2i=23.0,
                veh_gain=3.0, bs_gain=8.0, bs_nf=5.0, veh_nf=9.0, sig2=1e-11, w_v2v=0.0, w_v2i=0.0)
    names = [f[0] for f in SimStep._fields_ if f[1] is C.c_void_p and f[0] not in ('actions', 'mask', 'col', 'regular')]
    ptr = {k: P for k in names}
    ptr.update(v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300)
    for k in step_null:
        ptr[k] = None
    step = dict(n_lanes=over.pop('n_lanes', 2), n_u=over.pop('n_u', n_u), timestep=0.01, width=750.0, height=1299.0, power=10.0,
                actions=over.pop('step_actions', None))
    s = SimStep(problem=OptProblem(**prob), **step, **ptr)
    ok = 3 <= n <= 128 and 1 <= rb <= n and 3 * rb + 1 <= 16 and T >= 1 and E >= 1
    offs, size = recv_workspace_layout(E, n, rb, T) if ok else ({k: 256 * i for i, k in enumerate(SECTIONS)}, 1 << 20)
    r = dict(model=None, q=None, explore=P, random_actions=P, actions=P, recv=P, flags=P, w_v2v=1.0, w_v2i=0.1, T=T, pad_=0,
             edge_base=None, rep_xe=P, rep_xe_next=P, rep_recv=P, rep_action=P, rep_reward=P, head=0, capacity=8, result_reward=P,
             result_flags=P)
    r.update({k: (ws or P) + offs[k] for k in SECTIONS})
    r.update(over)
    rc = lib.v2x_rollout_steps_recv(C.byref(vlib.RolloutRecv(step=s, **r)), ws, size if ws_bytes is None else ws_bytes, None)
    return rc, _err(lib)


REFUSALS = [
    (dict(n=129), "n = 129"), (dict(n=2), "n = 2"), (dict(rb=6), "rb = 6"), (dict(E=0), "E = 0"),
    (dict(T=0), "T = 0"), (dict(T=-2), "T = -2"), (dict(T=5), "T E <= capacity"), (dict(E=3, T=3), "T E <= capacity"),
    (dict(capacity=0), "capacity"), (dict(head=8), "head"), (dict(head=-3), "head"),
    (dict(ws_bytes=1024), "needs"), (dict(ws=None), "workspace"), (dict(ws=P + 64), "256-byte aligned"),
    (dict(rep_recv=None), "rep_recv"), (dict(rep_xe=None), "null replay"), (dict(rep_xe_next=None), "null replay"),
    (dict(rep_action=None), "null replay"), (dict(rep_reward=None), "null replay"), (dict(rep_xe=P + 4), "16-byte aligned"),
    (dict(result_reward=None), "null result"), (dict(result_flags=None), "null result"),
    (dict(recv=None), "null"), (dict(flags=None), "null"), (dict(actions=None), "actions"), (dict(random_actions=None), "random_actions"),
    (dict(step_actions=P + 8), "actions"), (dict(n_u=11), "n_u"), (dict(n_lanes=0), "n_lanes"),
    (dict(traj_recv=P + 8), "first eight sections"), (dict(col_idx=P), "first eight sections"),
    (dict(step_null=('xy',)), "xy"), (dict(step_null=('keys',)), "null"), (dict(step_null=('xe',)), "null"),
    (dict(step_null=('v2v_rate',)), "null"),
]


@pytest.mark.parametrize("over,word", REFUSALS)
def test_a_bad_call_is_refused_before_anything_is_launched(over, word):
    rc, text = _call(**over)
    assert rc == V2X_EINVAL and word in text and text.startswith(("rollout_steps_recv", "sim_")), (rc, text)


def test_a_null_rollout_and_the_single_launches_refuse_too():
    lib = vlib.load_library()
    assert lib.v2x_rollout_steps_recv(None, P, 1 << 20, None) == V2X_EINVAL and "null rollout" in _err(lib)
    obs = lambda E, n, Cc, recv=P: lib.v2x_sim_observe_recv(E, n, Cc, P, P, P, 23.0, 3.0, 9.0, 1e-11, 10.0, P, P, P, recv, P, None)   # noqa: E731
    for args, word in (((1, 2, 1), "n = 2"), ((1, 129, 4), "n = 129"), ((1, 40, 6), "C = 6"), ((0, 40, 4), "E = 0"),
                       ((1, 40, 4, None), "null")):
        assert obs(*args) == V2X_EINVAL and word in _err(lib) and "sim_observe_recv" in _err(lib)
    csr = lambda G, E, n, recv=P, rp=P, col=P: lib.v2x_csr_from_recv(G, E, n, recv, None, rp, col, None)                          # noqa: E731
    for args, word in (((1, 1, 2), "outside 3..128"), ((1, 1, 129), "outside 3..128"), ((0, 1, 8), "G = 0"), ((1, 0, 8), "E = 0"),
                       ((1, 1, 8, None), "null"), ((1, 1, 8, P, None), "null"), ((1, 1, 8, P, P, None), "null"),
                       ((200000, 1, 128), "do not fit int32")):
        assert csr(*args) == V2X_EINVAL and word in _err(lib) and "csr_from_recv" in _err(lib)


# ------------------------------------------------------------------------------------------------------- the replay's bookkeeping
def test_receiver_replay_reserve_and_commit_keep_head_size_and_the_own_receiver_table():
    closed = ReceiverReplay(10, 4, device='cpu')                          # the default: add / add_many only, as before
    for call in (closed.storage, lambda: closed.reserve(4), lambda: closed.commit(4, [0] * 4)):
        with pytest.raises(NotImplementedError, match="device_writes=True"):
            call()
    rep = ReceiverReplay(10, 4, device='cpu', device_writes=True)
    with pytest.raises(ValueError, match="1..10 transitions"):
        rep.reserve(11)
    assert rep.reserve(4) == 0 and (rep.size, rep.head) == (0, 0)        # nothing is stored until commit()
    st = rep.storage()
    assert sorted(st) == ['action', 'recv', 'reward', 'xe', 'xe_next']
    assert tuple(st['xe'].shape) == (10, 4, 16) and tuple(st['recv'].shape) == (10, 4) and tuple(st['reward'].shape) == (10,)
    with pytest.raises(ValueError, match="4 own-receiver counts"):
        rep.commit(4, [0, 0, 0])
    rep.commit(4, [0, 2, 0, 0])
    assert (rep.size, rep.head, len(rep)) == (4, 4, 4) and rep._own[:4].tolist() == [0, 2, 0, 0]
    assert rep.regular_flags()[:4].tolist() == [True, False, True, True]
    assert rep.reserve(4) == 4 and rep.storage()['xe'] is st['xe']       # (a small ring is allocated whole at the first block)
    rep.commit(4, np.zeros(4, np.int32))
    assert (rep.size, rep.head) == (8, 8) and rep._own[:8].tolist() == [0, 2, 0, 0, 0, 0, 0, 0]
    assert rep.reserve(4) == 8                                           # the block wraps: slots 8, 9, 0, 1
    rep.commit(4, [1, 0, 3, 0])
    assert (rep.size, rep.head, len(rep)) == (10, 2, 10)
    assert rep._own.tolist() == [3, 0, 0, 0, 0, 0, 0, 0, 1, 0]           # slot 1 (own 2) was overwritten by a regular graph
    # FIFO position -> slot: the oldest transition now sits at the head
    assert rep.logical_to_slot(np.array([0, 7, 8, 9])).tolist() == [2, 9, 0, 1]
    for call in (lambda: rep.stage_early(None, None, None), lambda: rep.add_many_packed(*[None] * 7), lambda: rep.prefetch_indices([0], 1)):
        with pytest.raises(NotImplementedError, match="3..31 links"):
            call()


# ------------------------------------------------------------------------------------------------------- the Python layers
def _dev_env(streams, E=2):
    return DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=E, seeds=list(range(1, E + 1)), streams=streams)


def _gpu_brain():
    b = types.SimpleNamespace(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16)
    b.model = types.SimpleNamespace(engine=types.SimpleNamespace(_h=1, device='cpu'), trainer=None)      # looks like the gfx950 engine
    return b


def _mk(env, n=40, **kw):
    return Agent(n, 4, 1, 16, env, RL_Config(), brain=_gpu_brain(), **kw)


def test_agent_takes_receivers_with_trajectory_on_the_resident_simulator_only():
    agent = _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory', trajectory_walk='wide')
    assert type(agent.device_replay) is ReceiverReplay and agent.rollout_backend == 'trajectory' and not agent._packed_rollouts()
    assert agent.device_replay.device_writes and not _mk(_dev_env('device'), device_replay='receivers').device_replay.device_writes
    assert _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory').trajectory_walk == 'serial'
    with pytest.raises(ValueError, match="'trajectory'") as exc:         # the one-iteration call stays refused, and says what is served
        _mk(_dev_env('device'), device_replay='receivers', rollout_backend='device')
    assert "3..31 links" in str(exc.value)
    for env in (_dev_env('host'), BatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2])):
        with pytest.raises(ValueError, match="streams='device'"):
            _mk(env, device_replay='receivers', rollout_backend='trajectory')
    with pytest.raises(ValueError, match="chain stream phase"):
        _mk(_dev_env('device'), device_replay='receivers', rollout_backend='trajectory', trajectory_walk='wide', trajectory_streams='split')
    with pytest.raises(ValueError, match="3..128 links"):
        _mk(_dev_env('device'), n=132, device_replay='receivers', rollout_backend='trajectory')


def test_environment_and_channels_refuse_before_any_device_work():
    with pytest.raises(ValueError, match="streams='device' only"):
        _dev_env('host').new_random_game(40)
    with pytest.raises(ValueError, match="3..128 links"):
        _dev_env('device').new_random_game(132)
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').rollout_steps_recv(np.ones((1, 2), np.uint8), np.zeros((1, 2, 4), np.int32), {}, 0, 8, 1.0, 0.1)
    env = _dev_env('device')
    env.n_Veh = 40
    assert env._wide() and not env.packed_ok(4)
    env.n_Veh = 28
    assert not env._wide() and env.packed_ok(4)
    env.dest = np.array([[1, 1, 3, 2], [0, 0, 2, 3]])
    assert env.own_receivers().tolist() == [1, 3]
    env.dest = np.array([[1, 0, 3, 4], [1, 0, 3, 2]])
    with pytest.raises(ValueError, match=r"environment\(s\) \[0\]"):
        env.own_receivers()
    dc = DeviceChannels(2, 40, 4)
    dc.set_grid(LANES, 750.0, 1299.0, 0.01)
    tensor = lambda *shape: types.SimpleNamespace(shape=(8,) + shape, is_contiguous=lambda: True)        # noqa: E731
    st = {'xe': tensor(40, 16), 'xe_next': tensor(40, 16), 'recv': tensor(40), 'action': tensor(40), 'reward': tensor()}
    ex, ra, own = np.ones((3, 2), np.uint8), np.zeros((3, 2, 40), np.int32), [0, 0]
    T, e, r, o = dc.check_rollout_steps_recv(ex, ra, st, 5, 8, own)
    assert T == 3 and e.dtype == np.uint8 and r.dtype == np.int32 and o.tolist() == [0, 0]
    for args, word in (((ex[0], ra, st, 0, 8, own), "explore"), ((ex, ra[:, :, :39], st, 0, 8, own), "random_actions"),
                       ((ex, ra, st, 8, 8, own), "head"), ((ex, ra, st, 0, 5, own), "T E <= capacity"),
                       ((ex, ra, dict(st, recv=tensor(39)), 0, 8, own), "'recv'"), ((ex, ra, st, 0, 8, [0, 41]), "own"),
                       ((ex, ra, st, 0, 8, None), "own-receiver counts")):
        with pytest.raises(ValueError, match=word):
            dc.check_rollout_steps_recv(*args)
    with pytest.raises(ValueError, match="3..128 links"):
        DeviceChannels.check_observe_recv(2, 1)
    with pytest.raises(ValueError, match="n_RB <= links|n_channels"):
        DeviceChannels.check_observe_recv(40, 5, 4)
    DeviceChannels.check_observe_recv(128, 4, 4)


def test_command_line_takes_receivers_with_the_resident_rollout(capsys):
    dev = ["--sim-backend", "device", "--sim-streams", "device", "--envs", "1"]
    _, args = parse_args(["--links", "100", "--replay", "receivers", "--rollout", "trajectory"] + dev)
    assert (args.replay, args.rollout, args.links) == ("receivers", "trajectory", 100)
    for argv, word in ((["--replay", "receivers", "--rollout", "device"] + dev, "--rollout trajectory"),
                       (["--replay", "receivers", "--rollout", "trajectory"], "--sim-backend device --sim-streams device"),
                       (["--replay", "receivers", "--rollout", "trajectory", "--trajectory-walk", "wide", "--trajectory-streams", "split"] + dev,
                        "chain stream phase"),
                       (["--replay", "receivers", "--mixed-links", "8,12", "--envs", "2"], "--mixed-links")):
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert word in capsys.readouterr().err, argv
