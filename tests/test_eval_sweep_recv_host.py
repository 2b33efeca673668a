"""No GPU needed: the C ABI of the receiver-form checkpoint sweep (v2x_eval_sweep_recv_result_bytes, v2x_eval_sweep_recv,
v2x_eval_sweep_recv_split) is declared, exported and bound alike and the ctypes struct has the header's fields, offsets and
size; the result block's size is v2x_eval_recv_result_bytes' formula for 1..65 schemes; every refusal that needs no model comes
back as V2X_EINVAL with its text before anything is launched (the pointers handed over are never dereferenced by the host: a
check that let one through would reach a launch, which fails without a device); the Python layers refuse before any draw; and
Agent.evaluate_training_sweep(eval_backend='host'), the definition, is evaluate_training_diff_trials for one checkpoint and
scores K checkpoints on one episode.
(The refusals that need a model -- a mismatching one, a null q -- need a device to create one: tests/test_gpu_eval_sweep_recv.py.)"""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from test_eval_recv_host import LANES, P, REFUSALS, RESULTS, SECTIONS, _dev_env, _mk as _mk_gpu_brain
from test_rollout_trajectory_host import _host_env, _same_rng
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, EvalRecv, EvalSweepRecv, OptProblem, SimStep
from v2xgnn.rl import Agent, RL_Config
from v2xgnn.rl.device_sim import eval_result_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_eval_sweep_recv_result_bytes", "int64_t", C.c_int64, 5),
                                                    ("v2x_eval_sweep_recv", "int", C.c_int, 4),
                                                    ("v2x_eval_sweep_recv_split", "int", C.c_int, 6)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count
    if restype is C.c_int:
        assert bound[name][1][0]._type_ is EvalSweepRecv


def test_the_struct_is_bound_field_for_field_at_the_headers_offsets():
    m = re.search(r'struct v2x_eval_sweep_recv \{(.*?)\};', _header(), flags=re.S)
    assert m, "struct v2x_eval_sweep_recv is not declared in include/v2xgnn.h"
    declared = []
    for line in m.group(1).split(';'):
        names = re.sub(r'^\s*(const\s+)?\w+\s*(const)?\s*\**\s*(const)?\s*\**', '', line.strip())
        declared += [x.strip(' *') for x in names.split(',') if x.strip(' *')]
    assert declared == [f[0] for f in EvalSweepRecv._fields_] == ['base', 'K', 'pad_', 'models', 'q']
    # v2x_eval_recv base; int32_t K, pad_; two pointers: 8-byte members throughout, so the header's struct has no padding
    base = C.sizeof(EvalRecv)
    assert base % 8 == 0 and EvalSweepRecv._fields_[0][1] is EvalRecv
    assert [getattr(EvalSweepRecv, k).offset for k in declared] == [0, base, base + 4, base + 8, base + 16]
    assert C.sizeof(EvalSweepRecv) == base + 24


# ------------------------------------------------------------------------------------------------------- the result block's size
@pytest.mark.parametrize("n", [3, 33, 128])
@pytest.mark.parametrize("S", [1, 2, 3, 65])
def test_result_bytes_is_the_layout_of_s_schemes(n, S):
    lib = vlib.load_library()
    for E, rb, T in ((1, min(4, n), 3), (2, 1, 1)):
        want = eval_result_layout(E, n, rb, T, S)[1]
        assert want == -(-(8 * S * T * E * (n + min(rb, n) + rb + 1) + 4 * S * T * E * n + (T + 1) * E) // 8) * 8
        assert lib.v2x_eval_sweep_recv_result_bytes(E, n, rb, T, S) == want > 0
        if S <= 2:
            assert lib.v2x_eval_recv_result_bytes(E, n, rb, T, S) == want


@pytest.mark.parametrize("args,word", [((1, 40, 4, 1, 0), "got 0"), ((1, 40, 4, 1, 66), "got 66"), ((1, 2, 1, 1, 2), "n = 2"),
                                       ((1, 129, 4, 1, 2), "n = 129"), ((1, 40, 4, 65536, 2), "T E <= 65535"),
                                       ((256, 40, 4, 256, 1), "T E <= 65535")])
def test_result_bytes_is_negative_with_text_outside_the_limits(args, word):
    lib = vlib.load_library()
    assert lib.v2x_eval_sweep_recv_result_bytes(*args) == V2X_EINVAL < 0
    text = lib.v2x_last_error(None).decode()
    assert word in text and text.startswith(("rollout_steps_recv", "eval_sweep_recv")), text


# ------------------------------------------------------------------------------------------------------- the argument checks
def _call(split=False, E=2, n=40, rb=4, T=3, ws=P, ws_bytes=None, split_ws=P + (1 << 30), split_bytes=None, n_lanes=2, K=3,
          models=None, q=None, **over):
    """v2x_eval_sweep_recv (split: _split) on made-up pointers -> (return code, error text); the base struct is the one
    test_eval_recv_host._call makes"""
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
    r = dict(model=None, q=None, explore=P, random_actions=P, baseline_actions=P, actions=P, recv=P, flags=P, w_v2v=1.0, w_v2i=0.1,
             T=T, pad_=0, edge_base=None, **{k: P for k in RESULTS})
    r.update({k: (ws or P) + offs[k] for k in SECTIONS})
    r.update(over)
    sw = EvalSweepRecv(base=EvalRecv(step=s, **r), K=K, pad_=0, models=models, q=q)
    if split:
        rc = lib.v2x_eval_sweep_recv_split(C.byref(sw), ws, size if ws_bytes is None else ws_bytes, split_ws,
                                           need if split_bytes is None else split_bytes, None)
    else:
        rc = lib.v2x_eval_sweep_recv(C.byref(sw), ws, size if ws_bytes is None else ws_bytes, None)
    return rc, lib.v2x_last_error(None).decode()


# (base.model and base.q are ignored by the sweep: the single call's two refusals about them do not apply)
BASE_REFUSALS = [(over, word) for over, word in REFUSALS if 'model' not in over]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("over,word", BASE_REFUSALS)
def test_what_the_single_call_refuses_of_base_and_ws_the_sweep_refuses(over, word, split):
    assert len(BASE_REFUSALS) == len(REFUSALS) - 2
    rc, text = _call(split, **over)
    assert rc == V2X_EINVAL and word in text, (rc, text)
    assert text.startswith(("eval_sweep_recv_split" if split else "eval_sweep_recv:", "rollout_steps_recv", "sim_")), text


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("over,word", [(dict(K=0), "1..64 networks supported, got K = 0"),
                                       (dict(K=65), "1..64 networks supported, got K = 65"),
                                       (dict(K=-1), "got K = -1"),
                                       (dict(K=2, models=(C.c_void_p * 2)(None, None), q=P), "models[0] is NULL"),
                                       (dict(K=1, models=(C.c_void_p * 1)(None), q=None), "models[0] is NULL")])
def test_the_sweeps_own_refusals(over, word, split):
    rc, text = _call(split, **over)
    who = "eval_sweep_recv_split: " if split else "eval_sweep_recv: "
    assert rc == V2X_EINVAL and word in text and text.startswith(who), (rc, text)


def test_base_model_and_q_are_ignored():
    """a model pointer in base would be dereferenced by the single call's checks; the sweep never looks at it: with no models of
    its own the call passes every model check and is refused for the next thing wrong"""
    rc, text = _call(model=P, q=None, result_reward=None)
    assert rc == V2X_EINVAL and "null result" in text, text


@pytest.mark.parametrize("over,word", [(dict(split_ws=None), "split-stream workspace is null"),
                                       (dict(split_ws=P + 64), "256-byte aligned"),
                                       (dict(split_bytes=1024), "split-stream workspace of E = 2, n = 40")])
def test_the_split_call_checks_its_second_workspace(over, word):
    rc, text = _call(True, **over)
    assert rc == V2X_EINVAL and word in text and text.startswith("eval_sweep_recv_split"), (rc, text)


def test_a_null_struct_is_refused_and_the_chain_checks_come_first():
    lib = vlib.load_library()
    assert lib.v2x_eval_sweep_recv(None, P, 1 << 20, None) == V2X_EINVAL
    assert "eval_sweep_recv: null sweep" in lib.v2x_last_error(None).decode()
    assert lib.v2x_eval_sweep_recv_split(None, P, 1 << 20, P, 1 << 20, None) == V2X_EINVAL
    assert "eval_sweep_recv_split: null sweep" in lib.v2x_last_error(None).decode()
    for both in (dict(ws=None, split_ws=None), dict(K=65, split_ws=P + 64), dict(n=129, split_bytes=8)):
        rc, text = _call(True, **both)
        assert rc == V2X_EINVAL and "split-stream" not in text, text


# ------------------------------------------------------------------------------------------------------- the Python layers
def test_channels_check_the_sweep_before_any_device_work():
    from types import SimpleNamespace as NS
    from v2xgnn import GnnSpec
    from v2xgnn.rl import DeviceChannels
    E, n, T = 2, 40, 3
    dc = DeviceChannels(E, n, 4)
    dc.set_grid(LANES, 750.0, 1299.0, 0.01)
    ex, ra, ba, own = np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int64), np.ones((T, E, n), np.int32), [0, 1]
    spec = GnnSpec(n_nodes=n, feat_dim=16)
    good = [NS(spec=spec, _h=1), NS(spec=GnnSpec(n_nodes=n, feat_dim=16), _h=2)]
    assert dc.check_eval_sweep_recv(ex, ra, ba, good, None, own)[-1] == 2
    assert dc.check_eval_sweep_recv(ex, ra, None, None, 5, own, 'split')[-1] == 5
    assert dc.check_eval_sweep_recv(ex, ra, None, None, None, own)[-1] == 1
    bad = [
        (dict(engines=good, K=3), "K = 3, but 2 engines"), (dict(engines=[]), "1..64 networks, got 0"),
        (dict(engines=good * 33), "1..64 networks, got 66"), (dict(K=65), "1..64 networks, got 65"),
        (dict(engines=[good[0], None]), "fixed-size engines of 40 links and 4 channels .engine 1."),
        (dict(engines=[NS(spec=GnnSpec(n_nodes=36, feat_dim=16))]), "fixed-size engines of 40 links"),
        (dict(engines=[NS(spec=GnnSpec(n_nodes=1, feat_dim=16, share_weights=True, variable_graphs=True))]), "fixed-size engines"),
        (dict(engines=[good[0], NS(spec=GnnSpec(n_nodes=n, feat_dim=64))]), "engine 1 has another spec than engine 0"),
        (dict(explore=np.ones((T, E + 1), np.uint8)), "explore"), (dict(own=[0, n + 1]), "eval_sweep_recv: own"),
        (dict(stream_phase='wide'), "stream_phase must be one of 'chain', 'split'"),
    ]
    for over, word in bad:
        kw = dict(explore=ex, policy_random=ra, baseline_actions=ba, engines=None, K=None, own=own, stream_phase='chain')
        kw.update(over)
        with pytest.raises(ValueError, match=word):
            dc.check_eval_sweep_recv(**kw)
        with pytest.raises(ValueError, match=word):
            dc.eval_sweep_recv(kw['explore'], kw['policy_random'], kw['baseline_actions'], 1.0, 0.1, engines=kw['engines'], K=kw['K'],
                               own=kw['own'], stream_phase=kw['stream_phase'])
    assert dc.torch is None and dc.walk_calls == {'serial': 0, 'wide': 0} and dc.stream_phase_calls == {'chain': 0, 'split': 0}


def test_the_environment_serves_the_receiver_form_only():
    env = _dev_env('device')
    env.n_Veh = 20
    ex, ra = np.ones((1, 1), np.uint8), np.zeros((1, 1, 20), np.int32)
    with pytest.raises(ValueError, match="MixedAgent.evaluate_training") as exc:
        env.evaluate_sweep(ex, ra, None, 1.0, 0.1, None, 2, 'chain')
    assert "more than 31 links, got 20" in str(exc.value)


@pytest.mark.parametrize("make_env,n,word", [(lambda: _host_env(1), 40, "DeviceBatchedEnviron"),
                                             (lambda: _dev_env('host'), 40, "streams='device'"),
                                             (lambda: _dev_env('device', E=2), 40, "ONE simulator"),
                                             (lambda: _dev_env('device'), 31, "more than 31 links, got 31"),
                                             (lambda: _dev_env('device'), 4, "more than 31 links, got 4")])
def test_the_agent_refuses_the_device_sweep_before_any_draw(make_env, n, word):
    agent = _mk_gpu_brain(make_env(), n=n)
    random.seed(5)
    np.random.seed(5)
    before, before_py = np.random.get_state(), random.getstate()
    with pytest.raises(ValueError, match=word) as exc:
        agent.evaluate_training_sweep(10, 2, False, 0.5, 1, engines=[object(), object()], opt_backend='local', eval_backend='device')
    assert "eval_backend='device' needs" in str(exc.value)
    if n <= 31:
        assert "MixedAgent.evaluate_training" in str(exc.value)
    for backend in ('bogus', None):
        with pytest.raises(ValueError, match="eval_backend must be"):
            agent.evaluate_training_sweep(10, 2, False, 0.5, 1, engines=[object()], eval_backend=backend)
    assert _same_rng(np.random.get_state(), before) and random.getstate() == before_py
    assert agent.num_step == 0 and agent.eval_stats == {'device_episodes': 0, 'host_episodes': 0}


# ------------------------------------------------------------------------------------------------------- the host definition
class _Engine(object):
    """a deterministic stand-in for a loaded GnnEngine: Q = tanh(xe W), its own W; counts its forwards"""

    def __init__(self, seed, n=4, C=4):
        self.w = np.random.default_rng(seed).normal(size=(16, C))
        self.n, self.calls, self.closed = n, 0, False

    def forward(self, pb):
        self.calls += 1
        xe = np.asarray(pb.xe, np.float64).reshape(-1, 16)
        assert xe.shape[0] == self.n                                      # ONE observation per forward
        return np.tanh(xe @ self.w).astype(np.float32)

    def close(self):
        self.closed = True


class _Model(object):
    """what Agent._predict asks of brain.model, on an _Engine"""

    def __init__(self, engine):
        self.engine = engine

    def predict_arrays(self, x, e, adj):
        from v2xgnn import PackedBatch
        return self.engine.forward(PackedBatch.from_dense(x, e, adj)).reshape(1, self.engine.n, 4)


def _agent(seed=3):
    from types import SimpleNamespace as NS
    brain = NS(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16, model=_Model(_Engine(seed)))
    return Agent(4, 4, 1, 16, _host_env(1), RL_Config(), brain=brain, device_replay=False)


def _state(agent):
    env = agent.env
    return [np.array(getattr(env, k)) for k in ('V2V_channels_with_fastfading', 'V2I_channels_with_fastfading', 'dest')]


@pytest.mark.parametrize("opt_flag", [False, True])
@pytest.mark.parametrize("epsilon", [0.0, 0.5, 1.0])
def test_one_checkpoint_is_evaluate_training_diff_trials(opt_flag, epsilon):
    runs = []
    for how in ('loop', 'sweep'):
        agent = _agent()
        random.seed(11)
        np.random.seed(11)
        if how == 'loop':
            out = agent.evaluate_training_diff_trials(5, 3, opt_flag, epsilon, 2, load=False)
        else:
            out = agent.evaluate_training_sweep(5, 3, opt_flag, epsilon, 2, engines=[agent.brain.model.engine])
        runs.append((out, np.random.get_state(), random.getstate(), agent.num_step, dict(agent.eval_stats), _state(agent)))
    (o1, s1, p1, n1, e1, st1), (o2, s2, p2, n2, e2, st2) = runs
    assert len(o1) == len(o2) == (9 if opt_flag else 5)
    for a, b in zip(o1, o2):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert o2[1 if not opt_flag else 0].shape == (2, 1) and np.all(o2[2 if not opt_flag else 1] != 0)
    assert _same_rng(s1, s2) and p1 == p2 and n1 == n2 == 6 and e1 == e2 == {'device_episodes': 0, 'host_episodes': 2}
    for a, b in zip(st1, st2):
        assert a.tobytes() == b.tobytes()


def test_identical_checkpoints_score_alike_and_the_shared_schemes_do_not_depend_on_k():
    outs = {}
    for K in (1, 3):
        agent = _agent()
        engines = [_Engine(3) for _ in range(K)]
        random.seed(11)
        np.random.seed(11)
        outs[K] = agent.evaluate_training_sweep(5 * K, 4, True, 0.3, 2, engines=engines) + \
            agent.evaluate_training_sweep(5 * K, 4, False, 0.3, 2, engines=engines)[:1]
        assert not any(e.closed for e in engines)                          # the caller's engines stay open
        assert len({e.calls for e in engines}) == 1 and engines[0].calls > 0
        assert agent.num_step == 2 * 2 * 4                                 # one act() per step, whatever K
    one, three = outs[1], outs[3]
    for a in three[:9]:
        assert a.shape[:2] == (2, 3)
        for k in (1, 2):
            assert a[:, k].tobytes() == a[:, 0].tobytes()
    for a, b in zip(one, three):                                           # K = 1's rows are every row of K = 3; the optimum per trial
        assert (a.tobytes() == b.tobytes()) if a.ndim == 1 else (a[:, 0].tobytes() == b[:, 0].tobytes())
    assert np.all(three[4] > 0) and np.all(three[2] != 0)


def test_different_checkpoints_are_scored_on_one_episode_under_the_last_ones_actions():
    """K = 2 different networks: the random scheme and the optimum are those of the run with network 1 alone (the episode is
    walked under network K - 1's actions), and so is network 1's row; network 0's differs"""
    def run(seeds):
        agent = _agent()
        random.seed(4)
        np.random.seed(4)
        out = agent.evaluate_training_sweep(5 * len(seeds), 5, True, 0.0, 1, engines=[_Engine(s) for s in seeds])
        return out, _state(agent)
    (both, st_both), (last, st_last) = run([8, 9]), run([9])
    for a, b in zip(both, last):
        assert a[:, 1].tobytes() == b[:, 0].tobytes()
    assert both[1][:, 0].tobytes() != both[1][:, 1].tobytes()
    for a, b in zip(st_both, st_last):
        assert a.tobytes() == b.tobytes()


def test_the_draw_order_is_draw_trial_aheads():
    """once per trial, after the reset and before the first step; what it returns and where it leaves both generators is what
    the statements of evaluate_training_diff_trials' loop, spelled out on a twin, draw from the trial's seed"""
    from v2xgnn.rl.agent import _random_channels
    agent = _agent()
    seen = []
    real = agent._draw_trial_ahead

    def spy(T, eps):
        out = real(T, eps)
        seen.append((T, eps, agent.num_step, out, np.random.get_state(), random.getstate()))
        return out
    agent._draw_trial_ahead = spy
    agent.evaluate_training_sweep(10, 3, False, 0.5, 2, engines=[_Engine(1), _Engine(2)])
    assert [c[:3] for c in seen] == [(3, 0.5, 0), (3, 0.5, 3)]
    twin = _agent()
    for trial, (_, _, _, (base, flags, rand), rng, py) in enumerate(seen):
        random.seed(trial + 1)
        np.random.seed(trial + 1)
        twin.env.new_random_game(4)
        for st in range(3):                                               # the loop's statements, in its order
            assert np.array_equal(base[st], np.asarray(twin.select_action_random(None)).reshape(4)), (trial, st)
            if np.random.random() < 0.5:
                assert flags[st] == 1 and np.array_equal(rand[st], _random_channels(4, 1, 4).reshape(4)), (trial, st)
            else:
                assert flags[st] == 0 and not rand[st].any(), (trial, st)
        assert _same_rng(rng, np.random.get_state()) and py == random.getstate(), trial
    assert any(c[3][1].any() for c in seen) and not all(c[3][1].all() for c in seen)      # both kinds of step were drawn


def test_checkpoint_files_are_loaded_once_and_closed(tmp_path):
    from v2xgnn.bs_brain import keras_layer_table, save_weight_file
    from v2xgnn import GnnSpec
    spec = GnnSpec(n_nodes=4, feat_dim=16)
    made = []

    class _Loaded(_Engine):
        def __init__(self, spec_):
            _Engine.__init__(self, 0)
            made.append(self)

        def set_weights(self, weights):
            self.w = np.random.default_rng(int(abs(weights[0].ravel()[0]) * 1e6) % 1000).normal(size=(16, 4))

    agent = _agent()
    agent.brain._engine_factory = _Loaded
    agent.brain.model.spec = spec
    agent.batch_size = 64
    with pytest.raises(ValueError, match="no checkpoint .*Episode-5-Step-7-Batch-64"):
        agent.evaluate_training_sweep(10, 2, False, 0.0, 1, model_dir=str(tmp_path), num_train_steps=7)
    assert not made
    from oracle import compact as oc
    from oracle.spec import GnnSpec as OSpec
    table = keras_layer_table(spec)
    for k, ep in enumerate((5, 10)):
        weights = oc.params_to_list(oc.init_params(OSpec(n_nodes=4, feat_dim=16), np.random.default_rng(k), np.float32))
        save_weight_file(str(tmp_path / ('Q-Network_model_weights-Episode-%d-Step-7-Batch-64.h5' % ep)), weights, table)
    out = agent.evaluate_training_sweep(10, 2, False, 0.0, 1, model_dir=str(tmp_path), num_train_steps=7)
    assert len(made) == 2 and all(e.closed for e in made) and out[1].shape == (1, 2)


# ------------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("argv,word", [
    (["--mixed-links", "8,12", "--sweep"], "--sweep is the single-size path's"),
    (["--links", "20", "--sweep", "--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device"],
     "--sweep --eval-backend device needs more than 31 links"),
    (["--links", "40", "--sweep", "--eval-backend", "device"], "--eval-backend device needs --sim-backend device --sim-streams device"),
    (["--links", "40", "--sweep", "--receiver-streams", "split"], "needs --eval-backend device"),
])
def test_the_driver_refuses_what_the_sweep_cannot_serve(argv, word, capsys):
    from v2xgnn.rl.evaluate import main
    with pytest.raises(SystemExit) as exc:
        main(["--save-dir", "nowhere"] + argv)
    assert exc.value.code == 2 and word in capsys.readouterr().err


@pytest.mark.parametrize("sweep", [False, True])
def test_the_driver_calls_the_sweep_only_when_asked(sweep, monkeypatch, capsys):
    import json
    from v2xgnn.rl import evaluate
    calls = []

    class _Agent(object):
        def __init__(self, *a, **kw):
            self.made = kw

        def _out(self, name, *a, **kw):
            calls.append((name, a, kw))
            return np.ones(3), np.ones((3, 2)), np.ones((3, 2, 5)), np.ones((3, 2)), np.ones((3, 2, 5))

        def evaluate_training_sweep(self, *a, **kw):
            return self._out('sweep', *a, **kw)

        def evaluate_training_diff_trials(self, *a, **kw):
            return self._out('loop', *a, **kw)

    monkeypatch.setattr(evaluate, 'Agent', _Agent)
    argv = ["--save-dir", "D", "--links", "4", "--episodes", "10", "--test-steps", "5", "--trials", "3", "--epsilon", "0.25",
            "--train-steps", "7"] + (["--sweep"] if sweep else [])
    assert evaluate.main(argv) == 0
    (name, a, kw), = calls
    assert name == ('sweep' if sweep else 'loop') and a == (10, 5, False, 0.25, 3)
    assert kw == dict(model_dir="D", num_train_steps=7, opt_backend='host', opt_restarts=None, eval_backend='host')
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["checkpoints"] == 2 and summary["trials"] == 3 and len(summary["mean_return_per_checkpoint"]) == 2
