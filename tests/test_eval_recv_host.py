"""No GPU needed: the C ABI of the receiver-form evaluation episode (v2x_eval_recv_result_bytes, v2x_eval_steps_recv,
v2x_eval_steps_recv_split) is declared, exported and bound alike; the result block's size is the formula the header documents
and the layout DeviceChannels carves; every refusal of the two calls comes back as V2X_EINVAL before anything is launched (the
pointers handed over are never dereferenced by the host: a check that let one through would reach a launch, which fails
without a device); and the Python layers take the receiver form beyond 31 links -- Agent, rl.run's command line,
DeviceChannels.check_eval_steps_recv -- with their refusals made before any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, OptProblem, SimStep
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = [[1.75, 5.25], [244.75, 248.25], [1.75, 5.25], [427.75, 431.25]]
P = 0x10000                                              # a non-null, 256-byte aligned "device pointer": never dereferenced
SECTIONS = ('traj_xe', 'traj_recv', 'traj_flags', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs', 'row_ptr', 'col_idx')
RESULTS = ('result_actions', 'result_v2v_rate', 'result_v2i_rate', 'result_interference', 'result_reward', 'result_flags')


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_eval_recv_result_bytes", "int64_t", C.c_int64, 5),
                                                    ("v2x_eval_steps_recv", "int", C.c_int, 4),
                                                    ("v2x_eval_steps_recv_split", "int", C.c_int, 6)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


def test_the_struct_is_bound_field_for_field():
    m = re.search(r'typedef struct v2x_eval_recv \{(.*?)\} v2x_eval_recv;', _header(), flags=re.S)
    assert m, "v2x_eval_recv is not declared in include/v2xgnn.h"
    declared = []
    for line in m.group(1).split(';'):
        names = re.sub(r'^\s*(const\s+)?\w+\s*\**', '', line.strip())
        declared += [x.strip(' *') for x in names.split(',') if x.strip(' *')]
    assert declared == [f[0] for f in vlib.EvalRecv._fields_]
    assert not any(k.startswith('rep_') or k in ('head', 'capacity') for k in declared)
    assert set(RESULTS + ('baseline_actions',)) <= set(declared)


# ------------------------------------------------------------------------------------------------------- the result block's size
def documented_bytes(E, n, rb, T, S):
    """the formula of include/v2xgnn.h (v2x_eval_steps_recv), restated"""
    return -(-(8 * S * T * E * (n + min(rb, n) + rb + 1) + 4 * S * T * E * n + (T + 1) * E) // 8) * 8


@pytest.mark.parametrize("E,n,rb,T,S", [(1, 3, 1, 1, 1), (2, 33, 4, 3, 2), (1, 100, 4, 50, 2), (1, 128, 4, 50, 2)])
def test_result_bytes_is_the_documented_formula_and_the_python_layout(E, n, rb, T, S):
    from v2xgnn.rl.device_sim import eval_result_layout
    lib = vlib.load_library()
    want = documented_bytes(E, n, rb, T, S)
    assert lib.v2x_eval_recv_result_bytes(E, n, rb, T, S) == want > 0
    offs, size = eval_result_layout(E, n, rb, T, S)
    assert size == want
    K, m = S * T * E, min(rb, n)                         # the section order: v2v_rate, v2i_rate, interference, reward, actions, flags
    assert [offs[k] for k in ('v2v_rate', 'v2i_rate', 'interference', 'reward', 'actions', 'regular')] == \
        [0, 8 * K * n, 8 * K * (n + m), 8 * K * (n + m + rb), 8 * K * (n + m + rb + 1), 8 * K * (n + m + rb + 1) + 4 * K * n]
    if n <= 31:                                          # where both forms exist, one block serves either
        assert lib.v2x_eval_steps_result_bytes(E, n, rb, T, S) == want


@pytest.mark.parametrize("args,word", [((1, 2, 4, 1, 2), "n = 2"), ((1, 129, 4, 1, 2), "n = 129"), ((1, 40, 4, 1, 0), "got 0"),
                                       ((1, 40, 4, 1, 3), "got 3"), ((1, 40, 4, 65536, 2), "T E <= 65535"),
                                       ((256, 40, 4, 256, 1), "T E <= 65535")])
def test_result_bytes_is_negative_with_text_outside_the_limits(args, word):
    lib = vlib.load_library()
    assert lib.v2x_eval_recv_result_bytes(*args) == V2X_EINVAL < 0
    text = lib.v2x_last_error(None).decode()
    assert word in text and text.startswith(("rollout_steps_recv", "eval_steps_recv")), text


# ------------------------------------------------------------------------------------------------------- the argument checks
def _call(split=False, E=2, n=40, rb=4, T=3, ws=P, ws_bytes=None, split_ws=P + (1 << 30), split_bytes=None, n_lanes=2, **over):
    """v2x_eval_steps_recv (split: v2x_eval_steps_recv_split) on made-up pointers -> (return code, error text)"""
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
    st = vlib.EvalRecv(step=s, **r)
    if split:
        rc = lib.v2x_eval_steps_recv_split(C.byref(st), ws, size if ws_bytes is None else ws_bytes, split_ws,
                                           need if split_bytes is None else split_bytes, None)
    else:
        rc = lib.v2x_eval_steps_recv(C.byref(st), ws, size if ws_bytes is None else ws_bytes, None)
    return rc, lib.v2x_last_error(None).decode()


REFUSALS = [
    (dict(n=129), "n = 129"), (dict(n=2), "n = 2"), (dict(T=0), "T = 0"), (dict(E=256, T=256), "T E <= 65535"),
    (dict(ws_bytes=1024), "needs"), (dict(ws=None), "workspace is null"), (dict(ws=P + 64), "256-byte aligned"),
    (dict(col_idx=P), "first eight sections"), (dict(traj_flags=P + 8), "first eight sections"),
    (dict(result_reward=None), "null result"), (dict(result_flags=None), "null result"), (dict(result_actions=None), "null result"),
    (dict(model=P, q=None), "a model needs the Q workspace"), (dict(model=P, q=P, explore=None), "explore"),
    (dict(recv=None), "null"), (dict(random_actions=None), "random_actions"), (dict(actions=None), "actions"),
    (dict(n_lanes=0), "n_lanes"),
]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("over,word", REFUSALS)
def test_a_bad_call_is_refused_before_anything_is_launched(over, word, split):
    rc, text = _call(split, **over)
    assert rc == V2X_EINVAL and word in text, (rc, text)
    assert text.startswith(("eval_steps_recv_split" if split else "eval_steps_recv:", "rollout_steps_recv", "sim_")), text


@pytest.mark.parametrize("over,word", [(dict(split_ws=None), "split-stream workspace is null"),
                                       (dict(split_ws=P + 64), "256-byte aligned"),
                                       (dict(split_bytes=1024), "split-stream workspace of E = 2, n = 40")])
def test_the_split_call_checks_its_second_workspace(over, word):
    rc, text = _call(True, **over)
    assert rc == V2X_EINVAL and word in text and text.startswith("eval_steps_recv_split"), (rc, text)


def test_a_null_struct_is_refused_and_the_chain_checks_come_first():
    lib = vlib.load_library()
    assert lib.v2x_eval_steps_recv(None, P, 1 << 20, None) == V2X_EINVAL
    assert "eval_steps_recv: null evaluation" in lib.v2x_last_error(None).decode()
    assert lib.v2x_eval_steps_recv_split(None, P, 1 << 20, P, 1 << 20, None) == V2X_EINVAL
    assert "eval_steps_recv_split: null evaluation" in lib.v2x_last_error(None).decode()
    for both in (dict(ws=None, split_ws=None), dict(result_reward=None, split_ws=P + 64), dict(n=129, split_bytes=8)):
        rc, text = _call(True, **both)                                   # both wrong: the chain form's check speaks
        assert rc == V2X_EINVAL and "split-stream" not in text, text


# ------------------------------------------------------------------------------------------------------- the Python layers
def _dev_env(streams, E=1):
    return DeviceBatchedEnviron(LANES[1], LANES[0], LANES[2], LANES[3], 750, 1299, n_envs=E, seeds=list(range(1, E + 1)), streams=streams)


def _gpu_brain():
    b = types.SimpleNamespace(num_D2D_Input=0, num_One_D2D_Input=13, num_One_Node_Input=9, num_Feedback=16)
    b.model = types.SimpleNamespace(engine=types.SimpleNamespace(_h=1, device='cpu'), trainer=None)      # looks like the gfx950 engine
    return b


def _mk(env, n=40, **kw):
    return Agent(n, 4, 1, 16, env, RL_Config(), brain=_gpu_brain(), device_replay=False, **kw)


@pytest.mark.parametrize("n", [4, 31, 32, 40, 100, 128])
def test_agent_eval_backend_device_names_no_link_limit(n):
    agent = _mk(_dev_env('device'), n=n)
    agent._check_eval_backend('device')                                  # 32..128 links are accepted like 3..31
    for env, word in ((_dev_env('host'), "streams='device'"), (_dev_env('device', E=2), "ONE simulator")):
        with pytest.raises(ValueError, match=word) as exc:
            _mk(env, n=n)._check_eval_backend('device')
        assert "links" not in str(exc.value).replace("one receiver per link", "")


def test_agent_takes_receiver_streams_for_evaluation_only_agents_beyond_31_links():
    agent = _mk(_dev_env('device'), n=40, receiver_streams='split')      # no receiver replay, no trajectory rollouts: evaluation
    assert (agent.receiver_streams, agent.trajectory_walk, agent.trajectory_streams) == ('split', 'serial', 'chain')
    assert agent._receiver_form() and not _mk(_dev_env('device'), n=20)._receiver_form()
    needs = "receiver_streams='split' needs device_replay='receivers' and rollout_backend='trajectory'"
    with pytest.raises(ValueError, match=needs + ".*more than 31 links"):
        _mk(_dev_env('device'), n=20, receiver_streams='split')
    with pytest.raises(ValueError, match=needs + ".*ONE simulator"):
        _mk(_dev_env('device', E=2), n=40, receiver_streams='split')
    with pytest.raises(ValueError, match=needs + ".*streams='device'"):
        _mk(_dev_env('host'), n=40, receiver_streams='split')


def test_run_command_line_takes_the_receiver_form_beyond_31_links(capsys):
    from v2xgnn.rl.run import parse_args
    from v2xgnn.rl.evaluate import parse_args as parse_eval
    dev = ["--save-dir", "runs/none", "--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device"]
    for parse in (parse_args, parse_eval):
        _, args = parse(["--links", "100", "--opt", "--opt-backend", "local"] + dev)
        assert (args.links, args.eval_backend, args.receiver_streams, args.trajectory_streams) == (100, "device", "chain", "chain")
        _, args = parse(["--links", "40", "--receiver-streams", "split"] + dev)
        assert args.receiver_streams == "split"
        _, args = parse(["--links", "40", "--trajectory-walk", "wide"] + dev)                # what the form honours is taken
        assert args.trajectory_walk == "wide"
        _, args = parse(["--links", "20", "--trajectory-walk", "wide", "--trajectory-streams", "split"] + dev)
        assert args.trajectory_streams == "split"                                            # 3..31 links: as before
        for argv, word in ((["--links", "40", "--trajectory-streams", "split"] + dev, "use --receiver-streams split"),
                           (["--links", "40", "--trajectory-walk", "wide", "--trajectory-streams", "split"] + dev,
                            "use --receiver-streams split"),
                           (["--links", "20", "--receiver-streams", "split"] + dev, "--trajectory-walk wide --trajectory-streams split"),
                           (["--save-dir", "runs/none", "--links", "40", "--receiver-streams", "split"], "needs --eval-backend device"),
                           (["--mixed-links", "8,12", "--receiver-streams", "split"] + dev, "--mixed-links holds 3..31 links"),
                           (["--links", "40", "--receiver-streams", "wide"] + dev, "invalid choice")):
            with pytest.raises(SystemExit):
                parse(argv)
            assert word in capsys.readouterr().err, argv


def test_channels_check_the_receiver_form_evaluation_before_any_device_work():
    E, n, T = 2, 40, 3
    dc = DeviceChannels(E, n, 4)
    dc.set_grid(LANES, 750.0, 1299.0, 0.01)
    ex, ra, ba, own = np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int64), np.ones((T, E, n, 1), np.int32), [0, 1]
    for phase in ('chain', 'split'):
        t, e, r, b, o = dc.check_eval_steps_recv(ex, ra, ba, own, stream_phase=phase)
        assert t == T and e.dtype == np.uint8 and r.dtype == np.int32 and b.shape == (T, E, n) and o.tolist() == [0, 1]
    assert dc.check_eval_steps_recv(ex, ra, None, own)[3] is None
    bad = [
        (dict(explore=np.ones((T, E + 1), np.uint8)), "explore"), (dict(explore=np.ones(T, np.uint8)), "explore"),
        (dict(explore=np.ones((T, E))), "explore"), (dict(explore=np.ones((0, E), np.uint8)), "explore"),
        (dict(policy_random=np.zeros((T, E, n + 1), np.int32)), "policy_random"),
        (dict(policy_random=np.zeros((T, E, n))), "policy_random must be integers"),
        (dict(baseline_actions=np.zeros((T + 1, E, n), np.int32)), "baseline_actions"),
        (dict(baseline_actions=np.zeros((T, E, n), np.float32)), "baseline_actions must be integers"),
        (dict(own=[0, n + 1]), "own"), (dict(own=[-1, 0]), "own"), (dict(own=[0]), "own"), (dict(own=[0.5, 0.0]), "own"),
        (dict(own=None), "pass own"),
        (dict(stream_phase='wide'), "stream_phase must be one of 'chain', 'split'"),
    ]
    for over, word in bad:
        kw = dict(explore=ex, policy_random=ra, baseline_actions=ba, own=own, stream_phase='chain')
        kw.update(over)
        with pytest.raises(ValueError, match=word):
            dc.check_eval_steps_recv(**kw)
        with pytest.raises(ValueError, match=word):
            dc.eval_steps_recv(kw['explore'], kw['policy_random'], kw['baseline_actions'], 1.0, 0.1, own=kw['own'],
                               stream_phase=kw['stream_phase'])
    big = DeviceChannels(256, 4, 4)
    big.set_grid(LANES, 750.0, 1299.0, 0.01)
    with pytest.raises(ValueError, match="T E <= 65535"):
        big.check_eval_steps_recv(np.ones((256, 256), np.uint8), np.zeros((256, 256, 4), np.int32), None, np.zeros(256, np.int32))
    assert dc.torch is None and dc.walk_calls == {'serial': 0, 'wide': 0} and dc.stream_phase_calls == {'chain': 0, 'split': 0}


def test_environment_takes_the_receiver_form_wide_only():
    ex, ra = np.ones((1, 1), np.uint8), np.zeros((1, 1, 4), np.int32)
    env = _dev_env('device')
    for walk in ('serial', 'split'):
        with pytest.raises(ValueError, match="pass walk='wide'"):
            env.evaluate_steps(ex, ra, None, 1.0, 0.1, walk=walk, receiver_form=True)
    with pytest.raises(ValueError, match="row_ptr must be None"):
        env.evaluate_steps(ex, ra, None, 1.0, 0.1, walk='wide', row_ptr=object(), receiver_form=True)
    with pytest.raises(ValueError, match="streams='device'"):
        _dev_env('host').evaluate_steps(ex, ra, None, 1.0, 0.1, walk='wide', receiver_form=True)
