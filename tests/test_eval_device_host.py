"""No GPU needed: the C ABI of the evaluation call (v2x_eval_steps, v2x_eval_steps_result_bytes) is declared, exported and bound
alike and the ctypes struct has the header's fields and size; every argument error that needs no model comes back as V2X_EINVAL
before anything is launched (the pointers handed over are never dereferenced by the host: a check that let one through would
reach a launch, which fails without a device); eval_backend is refused by both evaluation drivers before any draw; and the
draws of an episode taken ahead leave numpy's and Python's streams where the host loop's statements leave them.
(The refusals that need a model -- wrong link or channel count, a batch that is not the trajectory's -- need a device to create
one: tests/test_gpu_eval_device.py.)"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from test_rollout_trajectory_host import LANES, P, WORKSPACES, _brain, _dev_env, _host_env, _same_rng
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, Batch, Eval, OptProblem, SimStep
from v2xgnn.rl import Agent, DeviceChannels, RL_Config
from v2xgnn.rl.agent import _random_channels
from v2xgnn.rl.device_sim import eval_result_layout
from v2xgnn.rl.train import start_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = ('result_actions', 'result_v2v_rate', 'result_v2i_rate', 'result_interference', 'result_reward', 'result_regular')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_eval_steps", "int", C.c_int, 2),
                                                    ("v2x_eval_steps_result_bytes", "int64_t", C.c_int64, 5)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


def test_binding_has_the_fields_and_the_size_of_the_declared_struct():
    body = re.search(r'typedef struct v2x_eval \{(.*?)\} v2x_eval;', _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part) for part in decl.split(None, 1)[1].split(',')]
    names = [re.sub(r'^(const)?(double|float|u?int\d+_t|v2x_\w+?(?=model|batch|step))', '', n) for n in names]
    assert names == [f[0] for f in Eval._fields_], (names, [f[0] for f in Eval._fields_])
    assert not any(k.startswith('rep_') or k in ('head', 'capacity') for k in names)      # no replay memory in an evaluation
    i = names.index('T')
    assert tuple(names[i + 2:i + 9]) == WORKSPACES and tuple(names[i + 9:]) == RESULTS
    # 8-byte members throughout (T and pad_ share one slot): the header's struct has no padding, so its size is this sum
    assert C.sizeof(Eval) == 8 + C.sizeof(Batch) + 5 * 8 + C.sizeof(SimStep) + 2 * 8 + 8 + 8 * (len(WORKSPACES) + len(RESULTS))


@pytest.mark.parametrize("E,n,rb,T,S", [(1, 3, 1, 1, 1), (3, 4, 4, 3, 2), (2, 31, 5, 2, 2), (1, 20, 4, 50, 2), (1, 20, 4, 50, 1)])
def test_result_bytes_is_the_documented_layout(E, n, rb, T, S):
    lib = vlib.load_library()
    m = min(rb, n)
    want = -(-(8 * S * T * E * (n + m + rb + 1) + 4 * S * T * E * n + (T + 1) * E) // 8) * 8
    assert lib.v2x_eval_steps_result_bytes(E, n, rb, T, S) == want
    offs, size = eval_result_layout(E, n, rb, T, S)
    assert size == want and tuple(offs) == ('v2v_rate', 'v2i_rate', 'interference', 'reward', 'actions', 'regular')
    K = S * T * E
    assert [offs[k] for k in offs] == [0, 8 * K * n, 8 * K * (n + m), 8 * K * (n + m + rb), 8 * K * (n + m + rb + 1),
                                       8 * K * (n + m + rb + 1) + 4 * K * n]
    assert DeviceChannels(E, n, rb).eval_steps_result_bytes(T, S) == want


@pytest.mark.parametrize("E,n,rb,T,S", [(1, 4, 4, 0, 2), (1, 4, 4, 3, 0), (1, 4, 4, 3, 3), (2, 4, 4, 32768, 2), (1, 2, 1, 1, 1), (1, 4, 5, 1, 1)])
def test_result_bytes_is_negative_outside_the_limits(E, n, rb, T, S):
    assert vlib.load_library().v2x_eval_steps_result_bytes(E, n, rb, T, S) == V2X_EINVAL < 0


# ------------------------------------------------------------------------------------------------------- the argument checks
def _err(lib):
    return lib.v2x_last_error(None).decode()


def _eval(E=2, n=4, rb=4, T=3, step_null=(), problem=None, **over):
    n_u = n + n * n + 2 * n * rb + 2 * n * n * rb
    prob = dict(E=E, n=n, rb=rb, pad_=0, v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300, dest=P, p_v2v=10.0, p_v2i=23.0,
                veh_gain=3.0, bs_gain=8.0, bs_nf=5.0, veh_nf=9.0, sig2=1e-11, w_v2v=0.0, w_v2i=0.0)
    prob.update(problem or {})
    ptr = {f[0]: P for f in SimStep._fields_ if f[1] is C.c_void_p and f[0] != 'actions'}
    ptr.update(v2v_ff=P + 0x100, v2i_ff=P + 0x200, v2i_abs=P + 0x300)
    for k in step_null:
        ptr[k] = None
    step = dict(n_lanes=over.pop('n_lanes', 2), n_u=over.pop('n_u', n_u), timestep=0.01, width=750.0, height=1299.0, power=10.0,
                actions=over.pop('step_actions', None))
    s = SimStep(problem=OptProblem(**prob), **step, **ptr)
    r = dict(model=None, q=None, explore=P, random_actions=P, baseline_actions=P, actions=P, w_v2v=1.0, w_v2i=0.1, T=T, pad_=0)
    r.update({k: P + 0x1000 * (i + 1) for i, k in enumerate(WORKSPACES)})
    r.update({k: P + 0x100000 * (i + 1) for i, k in enumerate(RESULTS)})
    r.update(over)
    return Eval(step=s, **r)


ERRORS = [
    (dict(T=0), "T = 0"), (dict(T=-2), "T = -2"), (dict(E=2, T=32768), "T E <= 65535"), (dict(E=65535, T=2), "T E <= 65535"),
    (dict(actions=None), "actions"), (dict(step_actions=P + 8), "step.actions must be NULL or `actions`"),
    (dict(random_actions=None), "random_actions"), (dict(E=0), "E = 0"), (dict(n=2), "n = 2"), (dict(n=32), "n = 32"),
    (dict(rb=5), "C = 5"), (dict(n_u=11), "n_u"), (dict(n_lanes=0), "n_lanes"), (dict(problem=dict(dest=None)), "null"),
    (dict(problem=dict(v2v_ff=P + 0x108)), "own channel arrays"),
] + [({k: None}, "workspace") for k in WORKSPACES] + [({k: None}, "null result") for k in RESULTS] + [
    (dict(step_null=(k,)), "null") for k in ('keys', 'mtpos', 'xy', 'dirs', 'vel', 'lanes', 'u', 'v2i_shadow', 'v2v_shadow', 'v2v_abs',
                                             'interf_db', 'state', 'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate')]


@pytest.mark.parametrize("change,word", ERRORS)
def test_argument_errors_are_einval_before_any_launch(change, word):
    lib = vlib.load_library()
    r = _eval(**change)
    assert lib.v2x_eval_steps(C.byref(r), None) == V2X_EINVAL, change
    assert word in _err(lib), (change, _err(lib))


def test_a_null_struct_is_refused():
    lib = vlib.load_library()
    assert lib.v2x_eval_steps(None, None) == V2X_EINVAL and "null" in _err(lib)


def test_channels_refuse_bad_episode_arguments_before_any_device_work():
    dc = DeviceChannels(2, 4, 4)
    ex, ok = np.zeros((3, 2), bool), np.zeros((3, 2, 4), np.int64)
    with pytest.raises(ValueError, match="set_grid"):
        dc.check_eval_steps(ex, ok, ok)
    dc.set_grid(LANES, 750, 1299, 0.01)
    for bad in (np.zeros(2, bool), np.zeros((3, 3), bool), np.zeros((0, 2), bool), np.zeros((3, 2))):
        with pytest.raises(ValueError, match="explore"):
            dc.check_eval_steps(bad, ok, ok)
    with pytest.raises(ValueError, match="policy_random must be integers"):
        dc.check_eval_steps(ex, np.zeros((3, 2, 4)), ok)
    with pytest.raises(ValueError, match="baseline_actions must be integers"):
        dc.check_eval_steps(ex, ok, np.zeros((3, 2, 4)))
    for shape in ((3, 2, 5), (2, 2, 4), (3, 2)):
        with pytest.raises(ValueError, match="policy_random: an array of shape"):
            dc.check_eval_steps(ex, np.zeros(shape, int), ok)
        with pytest.raises(ValueError, match="baseline_actions: an array of shape"):
            dc.check_eval_steps(ex, ok, np.zeros(shape, int))
    with pytest.raises(ValueError, match="T E <= 65535"):
        dc.check_eval_steps(np.zeros((32768, 2), bool), np.zeros((32768, 2, 4), np.int8), None)
    T, e, r, b = dc.check_eval_steps(ex, ok[..., None], None)
    assert T == 3 and e.dtype == np.uint8 and r.dtype == np.int32 and r.shape == (3, 2, 4) and b is None
    with pytest.raises(ValueError, match="T E <="):
        dc.trajectory_states(40000)
    with pytest.raises(RuntimeError, match="no trajectory call"):
        dc.trajectory_states(3)
    assert dc.torch is None and dc.traffic == {'bytes_up': 0, 'bytes_down': 0}
    assert dc.eval_steps_policy_bytes(3) == 4 * 24 + 8 + 4 * 24 and dc.eval_steps_policy_bytes(3, baseline=False) == 4 * 24 + 8
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').evaluate_steps(ex, ok, ok, 1.0, 0.1)


# ------------------------------------------------------------------------------------------------------- the agent and the drivers
def _mk(env, nn=1):
    return Agent(4, 4, nn, 16, env, RL_Config(), brain=_brain(), device_replay=False)


def _drivers(agent, backend):
    return (lambda: agent.test_run(1, 2, eval_backend=backend),
            lambda: agent.evaluate_training_diff_trials(5, 2, False, 0.5, 1, load=False, eval_backend=backend))


@pytest.mark.parametrize("make_env,word", [(lambda: start_env(4), "DeviceBatchedEnviron"), (lambda: _host_env(1), "DeviceBatchedEnviron"),
                                           (lambda: _dev_env('host'), "streams='device'"), (lambda: _dev_env('device'), "E = 1")])
def test_both_drivers_refuse_the_device_backend_before_any_draw(make_env, word):
    env = make_env()
    agent = _mk(env)
    assert agent.eval_stats == {'device_episodes': 0, 'host_episodes': 0}
    random.seed(5)
    np.random.seed(5)
    before, before_py = np.random.get_state(), random.getstate()
    for backend, text in (('bogus', "eval_backend must be"), (None, "eval_backend must be"), ('device', word)):
        for call in _drivers(agent, backend):
            with pytest.raises(ValueError, match=text) as exc:
                call()
            if backend == 'device':
                assert "eval_backend='device' needs" in str(exc.value)
    assert _same_rng(np.random.get_state(), before) and random.getstate() == before_py
    assert agent.num_step == 0 and agent.eval_stats == {'device_episodes': 0, 'host_episodes': 0}


@pytest.mark.parametrize("T", [1, 7, 50])
def test_test_runs_draws_taken_ahead_are_the_loops(T):
    agent = _mk(_host_env(1))
    runs = {}
    for how in ('loop', 'ahead'):
        np.random.seed(77)
        random.seed(77)
        if how == 'loop':
            acts = np.stack([np.asarray(agent.select_action_random(None)).reshape(4) for _ in range(T)])
        else:
            acts = agent._draw_test_run_ahead(T)
        runs[how] = (acts, np.random.get_state(), random.getstate())
    (a1, s1, p1), (a2, s2, p2) = runs['loop'], runs['ahead']
    assert a2.shape == (T, 4) and a1.tobytes() == a2.tobytes() and _same_rng(s1, s2) and p1 == p2
    assert a1.min() >= 0 and a1.max() < 4 and (T == 1 or len(set(map(bytes, a1))) > 1)


@pytest.mark.parametrize("fixed_epsilon", [0, 0.5, 1])
@pytest.mark.parametrize("T", [1, 50])
def test_the_trials_draws_taken_ahead_are_the_loops(fixed_epsilon, T):
    agent = _mk(_host_env(1))
    n, nn, C = 4, 1, 4
    runs = {}
    for how in ('loop', 'ahead'):
        np.random.seed(9)
        random.seed(9)
        if how == 'loop':                                                # the statements of evaluate_training_diff_trials, in its order
            base, flags, rand = [], [], []
            for _ in range(T):
                base.append(np.asarray(agent.select_action_random(None)).reshape(n))
                if np.random.random() < fixed_epsilon:
                    flags.append(1)
                    rand.append(_random_channels(n, nn, C).reshape(n))
                else:
                    flags.append(0)
                    rand.append(np.zeros(n, int))
            out = (np.stack(base), np.array(flags, np.uint8), np.stack(rand))
        else:
            out = agent._draw_trial_ahead(T, fixed_epsilon)
        runs[how] = (out, np.random.get_state(), random.getstate())
    (o1, s1, p1), (o2, s2, p2) = runs['loop'], runs['ahead']
    for a, b in zip(o1, o2):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert _same_rng(s1, s2) and p1 == p2
    flags = o2[1]
    assert flags.dtype == np.uint8 and {0: not flags.any(), 1: flags.all()}.get(fixed_epsilon, T == 1 or (flags.any() and not flags.all()))


@pytest.mark.parametrize("module", ["run", "evaluate"])
@pytest.mark.parametrize("argv,word", [(["--eval-backend", "device"], "--eval-backend device needs --sim-backend device --sim-streams device"),
                                       (["--sim-backend", "device", "--eval-backend", "device"], "--eval-backend device needs"),
                                       (["--sim-streams", "device"], "--sim-streams device needs --sim-backend device"),
                                       (["--eval-backend", "gpu"], "invalid choice")])
def test_the_drivers_refuse_bad_backend_combinations_on_the_command_line(module, argv, word, capsys):
    import importlib
    main = importlib.import_module("v2xgnn.rl." + module).main
    with pytest.raises(SystemExit) as exc:
        main(["--save-dir", "nowhere"] + argv)
    assert exc.value.code == 2 and word in capsys.readouterr().err
