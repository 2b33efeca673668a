"""No GPU needed: the C ABI of the whole-rollout call (v2x_rollout_steps, v2x_rollout_steps_workspace_bytes) is declared,
exported and bound alike; the workspace size is the formula the header documents; every argument error comes back as
V2X_EINVAL before anything is launched (the pointers handed over are never dereferenced by the host: a check that let one
through would reach a launch, which fails without a device); the Python layers refuse for 'trajectory' what they refuse for
'device'; and taking the policy draws of a whole rollout ahead consumes numpy's stream exactly like taking them iteration by
iteration."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, OptProblem, Rollout, SimStep
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config
from v2xgnn.rl.agent import MIN_EPSILON
from v2xgnn.rl.batched_env import BatchedEnviron
from v2xgnn.rl.train import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]
P = 0x10000                                              # a non-null "device pointer": checked for null-ness only
WORKSPACES = ('traj_xe', 'traj_col', 'traj_mask', 'traj_regular', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_rollout_steps", "int", C.c_int, 2),
                                                    ("v2x_rollout_steps_workspace_bytes", "int64_t", C.c_int64, 4)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


def test_binding_has_the_fields_of_the_declared_struct_in_order():
    body = re.search(r'typedef struct v2x_rollout_traj \{(.*?)\} v2x_rollout_traj;', _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part) for part in decl.split(None, 1)[1].split(',')]
    RolloutTraj = vlib.RolloutTraj
    assert names == [f[0] for f in RolloutTraj._fields_], (names, [f[0] for f in RolloutTraj._fields_])
    assert names[:3] == ['r', 'T', 'pad_'] and tuple(names[3:]) == WORKSPACES
    assert RolloutTraj._fields_[0][1] is Rollout and RolloutTraj._fields_[1][1] is C.c_int32
    assert C.sizeof(RolloutTraj) == C.sizeof(Rollout) + 8 + 8 * len(WORKSPACES)           # no padding anywhere


# ------------------------------------------------------------------------------------------------------- the workspace size
def documented_bytes(E, n, rb, T):
    """the formula of include/v2xgnn.h (v2x_rollout_steps), restated"""
    A = lambda x: -(-x // 256) * 256                                                         # noqa: E731
    return (A(4 * (T + 1) * E * n * 16) + A(4 * (T + 1) * E * n * (n - 2)) + A(4 * (T + 1) * E * n) + A((T + 1) * E)
            + A(8 * T * E * n * n * rb) + A(8 * T * E * n * rb) + A(8 * T * E * n))


@pytest.mark.parametrize("E,n,rb,T", [(1, 3, 1, 1), (3, 4, 4, 3), (2, 31, 5, 2), (1, 20, 4, 50)])
def test_workspace_bytes_is_the_documented_formula(E, n, rb, T):
    from v2xgnn.rl.device_sim import trajectory_workspace_layout
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T)
    assert lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T) == want
    offs, size = trajectory_workspace_layout(E, n, rb, T)                # what DeviceChannels carves the allocation by
    assert size == want and tuple(offs) == WORKSPACES
    o = [offs[k] for k in WORKSPACES] + [size]
    assert o[0] == 0 and all(x % 256 == 0 for x in o)
    raw = [4 * (T + 1) * E * n * 16, 4 * (T + 1) * E * n * (n - 2), 4 * (T + 1) * E * n, (T + 1) * E, 8 * T * E * n * n * rb,
           8 * T * E * n * rb, 8 * T * E * n]
    assert all(0 <= o[i + 1] - o[i] - raw[i] < 256 for i in range(7))    # back to back: every array fits, nothing overlaps


@pytest.mark.parametrize("E,n,rb,T", [(1, 2, 1, 1), (1, 32, 4, 1), (1, 4, 5, 1), (1, 4, 4, 0), (0, 4, 4, 1), (1, 8, 6, 1), (65536, 4, 4, 1),
                                      (1, 4, 0, 1), (1, 4, 4, -1)])
def test_workspace_bytes_is_negative_on_sizes_outside_the_limits(E, n, rb, T):
    lib = vlib.load_library()
    assert lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T) == V2X_EINVAL < 0
    assert "rollout_steps" in lib.v2x_last_error(None).decode()


# ------------------------------------------------------------------------------------------------------- the argument checks
def _err(lib):
    return lib.v2x_last_error(None).decode()


def _traj(E=2, n=4, rb=4, T=3, step_null=(), problem=None, **over):
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    prob = dict(E=E, n=n, rb=rb, pad_=0, v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300, dest=P, p_v2v=10.0, p_v2i=23.0,
                veh_gain=3.0, bs_gain=8.0, bs_nf=5.0, veh_nf=9.0, sig2=1e-11, w_v2v=0.0, w_v2i=0.0)
    prob.update(problem or {})
    names = [f[0] for f in SimStep._fields_ if f[1] is C.c_void_p and f[0] != 'actions']
    ptr = {k: P for k in names}
    ptr.update(v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300)
    for k in step_null:
        ptr[k] = None
    step = dict(n_lanes=2, n_u=n_u, timestep=0.01, width=750.0, height=1299.0, power=10.0, actions=None)
    step.update({k: over.pop(k) for k in list(over) if k in ('n_lanes', 'n_u', 'step_actions')})
    step['actions'] = step.pop('step_actions', None)
    s = SimStep(problem=OptProblem(**prob), **step, **ptr)
    ws = {k: over.pop(k, P + 0x1000 * (i + 1)) for i, k in enumerate(WORKSPACES)}
    r = dict(model=None, q=None, explore=P, random_actions=P, actions=P, w_v2v=1.0, w_v2i=0.1, rep_xe=P, rep_xe_next=P, rep_col=P,
             rep_mask=P, rep_action=P, rep_reward=P, head=0, capacity=8, result_reward=P, result_regular=P)
    r.update(over)
    return vlib.RolloutTraj(r=Rollout(step=s, **r), T=T, pad_=0, **ws)


OWN_ERRORS = [
    (dict(T=0), "T = 0"), (dict(T=-2), "T = -2"), (dict(T=5), "T E <= capacity"), (dict(T=4, capacity=7), "T E <= capacity"),
    (dict(E=3, T=3), "T E <= capacity"),
] + [({k: None}, "workspace") for k in WORKSPACES]

INHERITED_ERRORS = [
    (dict(E=0), "E = 0"), (dict(n=2), "n = 2"), (dict(n=32), "n = 32"), (dict(rb=5), "C = 5"), (dict(capacity=1), "capacity"),
    (dict(head=8), "head"), (dict(head=-3), "head"), (dict(n_u=11), "n_u"), (dict(n_lanes=0), "n_lanes"), (dict(n_lanes=65), "n_lanes"),
    (dict(actions=None), "actions"), (dict(step_actions=P + 8), "actions"), (dict(random_actions=None), "null"),
    (dict(rep_xe=None), "null"), (dict(rep_xe_next=None), "null"), (dict(rep_col=None), "null"), (dict(rep_mask=None), "null"),
    (dict(rep_action=None), "null"), (dict(rep_reward=None), "null"), (dict(result_reward=None), "null"),
    (dict(result_regular=None), "null"),
] + [(dict(step_null=(k,)), "null") for k in ('keys', 'mtpos', 'xy', 'dirs', 'vel', 'lanes', 'u', 'v2i_shadow', 'v2v_shadow', 'v2v_abs',
                                              'interf_db', 'state', 'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate')] + [
    (dict(problem=dict(dest=None)), "null"), (dict(problem=dict(v2v_ff=P + 0x108)), "own channel arrays"),
]


@pytest.mark.parametrize("change,word", OWN_ERRORS + INHERITED_ERRORS)
def test_argument_errors_are_einval_before_any_launch(change, word):
    lib = vlib.load_library()
    r = _traj(**change)
    assert lib.v2x_rollout_steps(C.byref(r), None) == V2X_EINVAL, change
    assert word in _err(lib), (change, _err(lib))


def test_a_null_struct_is_refused():
    lib = vlib.load_library()
    assert lib.v2x_rollout_steps(None, None) == V2X_EINVAL and "null" in _err(lib)


# ------------------------------------------------------------------------------------------------------- the Python layers
def _brain():
    return types.SimpleNamespace(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16)


def _dev_env(streams):
    return DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], streams=streams)


def _host_env(E=2):
    return BatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=E, seeds=list(range(1, E + 1)))


def _mk(env, **kw):
    return Agent(4, 4, kw.pop('nn', 1), 16, env, RL_Config(), brain=_brain(), device_replay=False, **kw)


def test_agent_refuses_for_trajectory_what_it_refuses_for_device():
    assert _mk(_host_env()).rollout_backend == 'host'                    # the default stays
    for bad in ('gpu', 'trajectories', None):
        with pytest.raises(ValueError, match="rollout_backend must be"):
            _mk(_host_env(), rollout_backend=bad)
    cases = [(lambda: _host_env(), {}, "DeviceBatchedEnviron"), (lambda: _dev_env('host'), {}, "streams='device'"),
             (lambda: _dev_env('device'), dict(nn=2), "one receiver per link"), (lambda: _dev_env('device'), {}, "gfx950 engine")]
    for make_env, kw, word in cases:
        texts = {}
        for backend in ('device', 'trajectory'):
            with pytest.raises(ValueError, match=word) as exc:
                _mk(make_env(), rollout_backend=backend, **kw)
            texts[backend] = str(exc.value)
        assert "'trajectory'" in texts['trajectory'] and texts['trajectory'].replace("'trajectory'", "'device'") == texts['device']


def test_environment_and_channels_refuse_bad_block_arguments_before_any_device_work():
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').rollout_steps(np.zeros((3, 2), bool), np.zeros((3, 2, 4), int), {}, 0, 8, 1.0, 0.1)
    dc = DeviceChannels(2, 4, 4)
    ex, ok = np.zeros((3, 2), bool), np.zeros((3, 2, 4), np.int64)
    with pytest.raises(ValueError, match="set_grid"):
        dc.check_rollout_steps(ex, ok, {}, 0, 8)
    dc.set_grid(LANES, 750, 1299, 0.01)
    for bad in (np.zeros(2, bool), np.zeros((3, 3), bool), np.zeros((0, 2), bool), np.zeros((3, 2))):
        with pytest.raises(ValueError, match="explore"):
            dc.check_rollout_steps(bad, ok, {}, 0, 8)
    with pytest.raises(ValueError, match="integers"):
        dc.check_rollout_steps(ex, np.zeros((3, 2, 4)), {}, 0, 8)
    for shape in ((3, 2, 5), (2, 2, 4), (3, 2)):
        with pytest.raises(ValueError, match="shape"):
            dc.check_rollout_steps(ex, np.zeros(shape, int), {}, 0, 8)
    for head, capacity in ((0, 5), (8, 8), (-1, 8)):                     # T E = 6 > 5; head outside the ring
        with pytest.raises(ValueError, match="capacity"):
            dc.check_rollout_steps(ex, ok, {}, head, capacity)
    with pytest.raises(ValueError, match="storage"):
        dc.check_rollout_steps(ex, ok, {}, 0, 8)
    with pytest.raises(ValueError, match="links"):
        DeviceChannels(2, 32, 4).check_rollout_steps(ex, np.zeros((3, 2, 32), int), {}, 0, 8)
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}
    assert dc.rollout_steps_policy_bytes(3) == 4 * 3 * 2 * 4 + 3 * 2 + 2 and dc.rollout_steps_result_bytes(3) == 64
    assert dc.rollout_steps_policy_bytes(1) == dc.rollout_policy_bytes and dc.rollout_steps_result_bytes(1) == dc.rollout_result_bytes


# ------------------------------------------------------------------------------------------------------- one host path
def _cpu_storage(slots, n=4, **other):
    """replay storage on the host: the checks look at shapes and contiguity only"""
    import torch
    st = {'xe': torch.zeros(slots, n, 16), 'xe_next': torch.zeros(slots, n, 16), 'col': torch.zeros(slots, n * (n - 2), dtype=torch.int32),
          'mask': torch.zeros(slots, n, dtype=torch.int32), 'action': torch.zeros(slots, n, dtype=torch.int32),
          'reward': torch.zeros(slots, dtype=torch.float64)}
    st.update(other)
    return st


def test_the_one_step_check_is_the_block_check_with_T_equal_1():
    """check_rollout(ex, ra, ...) and check_rollout_steps(ex[None], ra[None], ...) accept and refuse the same arguments (the bad
    ones of this file and of test_rollout_device_host.py, at one iteration), and what they return differs by the leading axis"""
    import torch
    E, n = 2, 4
    rng = np.random.default_rng(3)
    ex, ra, full = rng.integers(0, 2, E).astype(bool), rng.integers(0, 4, (E, n)), _cpu_storage(8)
    dc = DeviceChannels(E, n, 4)
    for check, a, b in ((dc.check_rollout, ex, ra), (dc.check_rollout_steps, ex[None], ra[None])):
        with pytest.raises(ValueError, match="set_grid"):
            check(a, b, full, 0, 8)
    dc.set_grid(LANES, 750, 1299, 0.01)
    good = [(ex, ra, full, 0, 8), (ex.astype(np.uint8), ra.astype(np.int32), full, 7, 8), (ex.astype(int), ra[:, :, None], full, 6, 8),
            (ex, ra, _cpu_storage(5), 3, 100), (ex, ra, _cpu_storage(2), 0, 2)]
    for e, r, st, head, capacity in good:
        e1, r1 = dc.check_rollout(e, r, st, head, capacity)
        T, eT, rT = dc.check_rollout_steps(np.asarray(e)[None], np.asarray(r)[None], st, head, capacity)
        assert T == 1 and eT.shape == (1, E) and rT.shape == (1, E, n)
        assert e1.dtype == eT.dtype == np.uint8 and r1.dtype == rT.dtype == np.int32 and r1.flags.c_contiguous and rT.flags.c_contiguous
        assert np.array_equal(e1, eT[0]) and np.array_equal(r1, rT[0])
        assert np.array_equal(e1, np.asarray(e).astype(np.uint8)) and np.array_equal(r1, np.asarray(r).reshape(E, n))
    bad = [(np.zeros(3, bool), ra, full, 0, 8, "explore"), (np.zeros(2), ra, full, 0, 8, "explore"),
           (ex, np.zeros((2, 4)), full, 0, 8, "integers"), (ex, np.zeros((2, 5), int), full, 0, 8, "shape"),
           (ex, np.zeros(2, int), full, 0, 8, "shape"), (ex, np.zeros((3, 4), int), full, 0, 8, "shape"),
           (ex, ra, full, 0, 1, "capacity"), (ex, ra, full, 8, 8, "capacity"), (ex, ra, full, -1, 8, "capacity"),
           (ex, ra, {}, 0, 8, "storage"), (ex, ra, _cpu_storage(8, mask=torch.zeros(8, 5, dtype=torch.int32)), 0, 8, "storage"),
           (ex, ra, _cpu_storage(8, xe=torch.zeros(8, 4, 32)[:, :, ::2]), 0, 8, "storage"),
           (ex, ra, _cpu_storage(4), 3, 8, "slots"), (ex, ra, _cpu_storage(7), 7, 8, "slots")]
    for e, r, st, head, capacity, word in bad:
        with pytest.raises(ValueError, match=word) as one:
            dc.check_rollout(e, r, st, head, capacity)
        with pytest.raises(ValueError, match=word) as block:
            dc.check_rollout_steps(e[None], r[None], st, head, capacity)
        assert "rollout_steps" not in str(one.value) and "rollout_step:" not in str(block.value)
    wide = DeviceChannels(2, 32, 4)
    wide.set_grid(LANES, 750, 1299, 0.01)
    for check, a, b in ((wide.check_rollout, ex, np.zeros((2, 32), int)), (wide.check_rollout_steps, ex[None], np.zeros((1, 2, 32), int))):
        with pytest.raises(ValueError, match="links"):
            check(a, b, _cpu_storage(8, n=32), 0, 8)
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}


class _Event(object):
    def __init__(self):
        self.waits = 0

    def synchronize(self):
        self.waits += 1


@pytest.mark.parametrize("T", [None, 2])
def test_rollout_result_on_host_storage(T):
    """RolloutResult on a host buffer in the downloaded layout (reward float64 | regular bytes) and a stub event: shapes and
    values per entry point, the two flat views, and resolve() waits once and returns the buffer once"""
    import torch
    from v2xgnn.rl.device_sim import RolloutResult
    E = 3
    lead = () if T is None else (T,)
    K = (T or 1) * E
    rng = np.random.default_rng(17)
    reward = rng.normal(size=lead + (E,))
    regular = rng.integers(0, 2, size=lead + (2, E)).astype(np.uint8)
    blocks = regular.reshape(-1, 2, E)
    blocks[0, 0], blocks[-1, 1] = (1, 0, 1), (0, 1, 1)                   # (stored and resident flags that differ from each other)
    pin = torch.zeros(-(-10 * K // 8) * 8, dtype=torch.uint8)
    pin.numpy()[:8 * K] = np.frombuffer(reward.tobytes(), np.uint8)
    pin.numpy()[8 * K:10 * K] = regular.reshape(-1)
    free, ev = [], _Event()
    res = RolloutResult(free, ev, pin, E, T)
    assert res.reward is None and res.regular is None and free == [] and ev.waits == 0
    assert res.resolve() is res and ev.waits == 1 and len(free) == 1 and free[0] is pin
    assert res.reward.shape == lead + (E,) and res.reward.dtype == np.float64 and res.reward.tobytes() == reward.tobytes()
    assert res.regular.shape == lead + (2, E) and res.regular.dtype == bool and np.array_equal(res.regular, regular != 0)
    pin.zero_()                                                          # the buffer is somebody else's now: plain copies were kept
    assert res.resolve() is res and ev.waits == 1 and len(free) == 1
    assert res.reward.tobytes() == reward.tobytes() and np.array_equal(res.regular, regular != 0)
    stored, resident = res.stored_regular, res.resident_regular
    assert stored.shape == (K,) and resident.shape == (E,) and ev.waits == 1 and len(free) == 1
    if T is None:
        assert np.array_equal(stored, regular[0] != 0) and np.array_equal(resident, regular[1] != 0)
    else:
        assert np.array_equal(stored, res.regular[:, 0, :].reshape(-1)) and np.array_equal(resident, res.regular[-1, 1])
        assert np.array_equal(stored.reshape(T, E), regular[:, 0] != 0)  # (t major, e minor)
    assert stored[:E].tolist() == [True, False, True] and resident.tolist() == [False, True, True]


def test_the_views_resolve_a_result_that_nobody_resolved():
    import torch
    from v2xgnn.rl.device_sim import RolloutResult
    free, ev = [], _Event()
    pin = torch.zeros(24, dtype=torch.uint8)
    pin[16:20] = torch.tensor([1, 0, 0, 1], dtype=torch.uint8)
    res = RolloutResult(free, ev, pin, 2)
    assert res.resident_regular.tolist() == [False, True] and res.stored_regular.tolist() == [True, False]
    assert ev.waits == 1 and len(free) == 1 and free[0] is pin


@pytest.mark.parametrize("argv", [["--envs", "2", "--rollout", "trajectory"],
                                  ["--envs", "2", "--sim-backend", "device", "--rollout", "trajectory"]])
def test_rollout_trajectory_needs_the_device_simulator_and_streams_on_the_command_line(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        main(argv)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and "--rollout trajectory needs --sim-backend device --sim-streams device" in err


def test_an_unknown_rollout_is_still_refused_on_the_command_line(capsys):
    with pytest.raises(SystemExit) as exc:
        main(["--envs", "2", "--rollout", "gpu"])
    assert exc.value.code == 2 and "invalid choice" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- the draws, taken ahead
def _same_rng(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("n_iter", [1, 4, 50])
def test_draws_taken_ahead_are_the_draws_taken_iteration_by_iteration(E, n_iter):
    agent = _mk(_host_env(E))
    agent.num_Episodes, agent.num_Train_Step, agent.num_transition = 1, 2, 50            # epsilon reaches MIN_EPSILON at step 80
    crossed = False
    for start in (0, 60, 80 - E * n_iter + (E * n_iter) // 2, 79, 80, 500):              # before, across and after the schedule's end
        start = max(start, 0)
        runs = {}
        for how in ('one by one', 'ahead'):
            np.random.seed(1234 + start)
            agent.num_step, agent.epsilon = start, -1.0
            if how == 'ahead':
                drawn = agent._draw_rollout_ahead(n_iter)
                assert agent.num_step == start                           # (the iterations advance it, not the draws)
            else:
                drawn = []
                for _ in range(n_iter):
                    drawn.append(agent._policy_draws())
                    agent.num_step += E
                assert agent.num_step == start + E * n_iter
            runs[how] = (drawn, agent.epsilon, np.random.get_state())
        (d1, eps1, s1), (d2, eps2, s2) = runs['one by one'], runs['ahead']
        assert len(d1) == len(d2) == n_iter and eps1 == eps2 and _same_rng(s1, s2)
        for (a1, g1), (a2, g2) in zip(d1, d2):
            assert a1.shape == a2.shape == (E, 4, 1) and a1.dtype == a2.dtype and a1.tobytes() == a2.tobytes()
            assert list(g1) == list(g2)
        last = start + E * n_iter - 1
        if start < 80 <= last:
            crossed = True
            assert eps1 == MIN_EPSILON
        if last < 80:
            assert eps1 == 1 - (1 - MIN_EPSILON) / 80 * last
        if start >= 80:                                                  # almost everybody is greedy once the schedule has ended
            assert sum(len(g) for _, g in d1) >= 0.8 * E * n_iter - 2
    assert crossed or E * n_iter == 1                                     # (one draw cannot straddle the end of the schedule)
