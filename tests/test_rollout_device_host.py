"""No GPU needed: the C ABI of the device-resident rollout iteration (v2x_rollout_pick, v2x_rollout_store, v2x_rollout_step) is
declared, exported and bound alike; every argument error comes back as V2X_EINVAL before anything is launched (the pointers
handed over are never dereferenced by the host: a check that let one through would reach a launch, which fails without a
device); the Python layers refuse what the device rollout does not support; and the summation order the store kernel
restates is numpy's."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, Batch, OptProblem, Rollout, SimStep
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config
from v2xgnn.rl.batched_env import BatchedEnviron
from v2xgnn.rl.train import main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]
P = 0x10000                                              # a non-null "device pointer": checked for null-ness only


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,count", [("v2x_rollout_pick", 18), ("v2x_rollout_store", 18), ("v2x_rollout_step", 2)])
def test_rollout_entry_points_are_declared_exported_and_bound_alike(name, count):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == count


def test_rollout_binding_has_the_fields_of_the_declared_struct():
    body = re.search(r'typedef struct v2x_rollout \{(.*?)\} v2x_rollout;', _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part) for part in decl.split(None, 1)[1].split(',')]
    names = [re.sub(r'^(const)?(double|float|u?int\d+_t|v2x_\w+?(?=model|batch|step))', '', n) for n in names]
    assert names == [f[0] for f in Rollout._fields_], (names, [f[0] for f in Rollout._fields_])
    # pointers, doubles and int64 are 8 bytes: no padding anywhere
    assert C.sizeof(Rollout) == C.sizeof(Batch) + C.sizeof(SimStep) + 8 * (len(Rollout._fields_) - 2)


def _err(lib):
    return lib.v2x_last_error(None).decode()


PICK = dict(E=2, n=4, C=4, q=P, explore=P, random_actions=P, actions=P, xe=P, col=P, mask=P, regular=P, rep_xe=P, rep_col=P,
            rep_mask=P, head=0, capacity=8, regular_out=P)
STORE = dict(E=2, n=4, rb=4, v2v_rate=P, v2i_rate=P, w_v2v=1.0, w_v2i=0.1, xe=P, actions=P, regular=P, rep_xe_next=P, rep_action=P,
             rep_reward=P, head=0, capacity=8, reward_out=P, regular_out=P)
SHAPE_ERRORS = [(dict(E=0), "E = 0"), (dict(E=65536, capacity=1 << 20), "states"), (dict(n=2), "n = 2"), (dict(n=32), "n = 32"),
                (dict(capacity=1), "capacity"), (dict(head=-1), "head"), (dict(head=8), "head"), (dict(capacity=0), "capacity")]


@pytest.mark.parametrize("change,word", SHAPE_ERRORS + [(dict(C=0), "C = 0"), (dict(C=5, n=4), "C = 5"), (dict(C=6, n=8), "C = 6")]
                         + [({k: None}, "null") for k in PICK if PICK[k] == P and k != 'q'])
def test_pick_argument_errors_are_einval_before_any_launch(change, word):
    lib = vlib.load_library()
    a = dict(PICK, **change)
    assert lib.v2x_rollout_pick(*[a[k] for k in PICK], None) == V2X_EINVAL, change
    assert "rollout_pick" in _err(lib) and word in _err(lib), (change, _err(lib))


def test_pick_takes_null_q_only_as_nobody_is_greedy():
    lib = vlib.load_library()
    a = dict(PICK, q=P, explore=None)                                    # Q-values without the flags that say whose count
    assert lib.v2x_rollout_pick(*[a[k] for k in PICK], None) == V2X_EINVAL and "explore" in _err(lib)


@pytest.mark.parametrize("change,word", SHAPE_ERRORS + [(dict(rb=0), "C = 0"), (dict(rb=5, n=4), "C = 5"), (dict(rb=6, n=8), "C = 6")]
                         + [({k: None}, "null") for k in STORE if STORE[k] == P])
def test_store_argument_errors_are_einval_before_any_launch(change, word):
    lib = vlib.load_library()
    a = dict(STORE, **change)
    assert lib.v2x_rollout_store(*[a[k] for k in STORE], None) == V2X_EINVAL, change
    assert "rollout_store" in _err(lib) and word in _err(lib), (change, _err(lib))


def _rollout(E=2, n=4, rb=4, step_null=(), problem=None, **over):
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
    r = dict(model=None, q=None, explore=P, random_actions=P, actions=P, w_v2v=1.0, w_v2i=0.1, rep_xe=P, rep_xe_next=P, rep_col=P,
             rep_mask=P, rep_action=P, rep_reward=P, head=0, capacity=8, result_reward=P, result_regular=P)
    r.update(over)
    return Rollout(step=s, **r)


STEP_ERRORS = [
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


@pytest.mark.parametrize("change,word", STEP_ERRORS)
def test_step_argument_errors_are_einval_before_any_launch(change, word):
    lib = vlib.load_library()
    r = _rollout(**change)
    assert lib.v2x_rollout_step(C.byref(r), None) == V2X_EINVAL, change
    assert word in _err(lib), (change, _err(lib))


def test_step_refuses_a_null_rollout():
    lib = vlib.load_library()
    assert lib.v2x_rollout_step(None, None) == V2X_EINVAL and "null" in _err(lib)


# ------------------------------------------------------------------------------------------------------- the Python layers
def _brain():
    return types.SimpleNamespace(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16)


def _dev_env(streams):
    return DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2], streams=streams)


def test_agent_refuses_a_device_rollout_it_cannot_run():
    host_env = BatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=2, seeds=[1, 2])
    mk = lambda env, **kw: Agent(4, 4, kw.pop('nn', 1), 16, env, RL_Config(), brain=_brain(), device_replay=False, **kw)   # noqa: E731
    assert mk(host_env).rollout_backend == 'host' and mk(_dev_env('device')).rollout_backend == 'host'     # the default
    with pytest.raises(ValueError, match="rollout_backend must be"):
        mk(host_env, rollout_backend='gpu')
    with pytest.raises(ValueError, match="DeviceBatchedEnviron"):
        mk(host_env, rollout_backend='device')
    with pytest.raises(ValueError, match="streams='device'"):
        mk(_dev_env('host'), rollout_backend='device')
    with pytest.raises(ValueError, match="one receiver per link"):
        mk(_dev_env('device'), rollout_backend='device', nn=2)
    with pytest.raises(ValueError, match="gfx950 engine"):             # (a brain without the engine; with it: the HBM replay, one GPU)
        mk(_dev_env('device'), rollout_backend='device')


def test_environment_and_channels_refuse_bad_rollout_arguments_before_any_device_work():
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').rollout_step(np.zeros(2), np.zeros((2, 4), int), {}, 0, 8, 1.0, 0.1)
    dc = DeviceChannels(2, 4, 4)
    ok = np.zeros((2, 4), np.int64)
    with pytest.raises(ValueError, match="set_grid"):
        dc.check_rollout(np.zeros(2, bool), ok, {}, 0, 8)
    dc.set_grid(LANES, 750, 1299, 0.01)
    with pytest.raises(ValueError, match="explore"):
        dc.check_rollout(np.zeros(3, bool), ok, {}, 0, 8)
    with pytest.raises(ValueError, match="explore"):
        dc.check_rollout(np.zeros(2), ok, {}, 0, 8)
    with pytest.raises(ValueError, match="integers"):
        dc.check_rollout(np.zeros(2, bool), np.zeros((2, 4)), {}, 0, 8)
    with pytest.raises(ValueError, match="shape"):
        dc.check_rollout(np.zeros(2, bool), np.zeros((2, 5), int), {}, 0, 8)
    for head, capacity in ((0, 1), (8, 8), (-1, 8)):
        with pytest.raises(ValueError, match="capacity"):
            dc.check_rollout(np.zeros(2, bool), ok, {}, head, capacity)
    with pytest.raises(ValueError, match="storage"):
        dc.check_rollout(np.zeros(2, bool), ok, {}, 0, 8)
    with pytest.raises(ValueError, match="links"):
        DeviceChannels(2, 32, 4).check_rollout(np.zeros(2, bool), np.zeros((2, 32), int), {}, 0, 8)
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}
    assert dc.rollout_policy_bytes == 4 * 2 * 4 + 4 and dc.rollout_result_bytes == 24


@pytest.mark.parametrize("argv", [["--envs", "2", "--rollout", "device"],
                                  ["--envs", "2", "--sim-backend", "device", "--rollout", "device"]])
def test_rollout_device_needs_the_device_simulator_and_streams_on_the_command_line(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        main(argv)
    assert exc.value.code == 2 and "--sim-backend device --sim-streams device" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- the summation order
def numpy_row_sum(a):
    """S of include/v2xgnn.h (v2x_rollout_store) in Python floats"""
    m = len(a)
    if m < 8:
        r = 0.0
        for x in a:
            r = r + x
        return r
    r = [a[j] for j in range(8)]
    i = 8
    while i + 8 <= m:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < m:
        res = res + a[i]
        i += 1
    return res


@pytest.mark.parametrize("m", range(1, 32))
def test_restated_summation_order_is_ndarray_sum_bit_for_bit(m):
    rng = np.random.default_rng(100 + m)
    for E in (1, 3, 50):
        a = rng.random((E, m, 1)) * rng.choice([1e-6, 1e-3, 1.0, 1e3], size=(E, m, 1))        # rates of very different sizes
        as_v2v, as_v2i = a.sum(axis=(1, 2)), np.ascontiguousarray(a[:, :, 0]).sum(axis=1)
        for e in range(E):
            want = np.float64(numpy_row_sum([float(x) for x in a[e, :, 0]]))
            assert want.tobytes() == as_v2v[e].tobytes() == as_v2i[e].tobytes(), (m, E, e)
    if m >= 9:                                                           # ... and a plain sequential sum is not
        a = rng.random((200, m))
        seq = np.zeros(200)
        for j in range(m):
            seq = seq + a[:, j]
        assert np.any(seq != a.sum(axis=1))
