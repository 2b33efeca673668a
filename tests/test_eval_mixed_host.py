"""No GPU needed: the C ABI of the mixed-size evaluation call (v2x_eval_steps_mixed) is declared, exported and bound alike, the
ctypes struct has the header's layout, the first argument checks come back as V2X_EINVAL before anything is launched; taking
the draws of an evaluation episode ahead consumes numpy's stream exactly like the host loop's step-by-step draws; and the
evaluation driver refuses with --mixed-links what holds one link count."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL
from v2xgnn.rl import mixed
from v2xgnn.rl import run as rl_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


def test_the_entry_point_is_declared_exported_and_bound_alike():
    m = re.search(r'\bint\s+v2x_eval_steps_mixed\s*\(([^)]*)\)\s*;', _header())
    assert m, "v2x_eval_steps_mixed is not declared in include/v2xgnn.h"
    assert [a.strip() for a in m.group(1).split(',')] == ['const v2x_eval_mixed* m', 'void* stream']
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), 'v2x_eval_steps_mixed'), "libv2xgnn.so does not export v2x_eval_steps_mixed"
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert bound['v2x_eval_steps_mixed'][0] is C.c_int and len(bound['v2x_eval_steps_mixed'][1]) == 2
    assert bound['v2x_eval_steps_mixed'][1][0]._type_ is vlib.EvalMixed


def _declared_fields(struct):
    """[(name, is a pointer, C type)] of `typedef struct <struct> {...}` in the header, in order"""
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(',')
        ctype = re.match(r'(?:const\s+)?(\w+)', first).group(1)
        for part in [first] + rest:
            out.append((re.findall(r'\w+', part)[-1], '*' in part, ctype))
    return out


def test_the_binding_has_the_layout_of_the_declared_struct():
    EvalMixed, RolloutMixed = vlib.EvalMixed, vlib.RolloutMixed
    fields = _declared_fields('v2x_eval_mixed')
    assert [f[0] for f in fields] == [f[0] for f in EvalMixed._fields_]
    assert [f[0] for f in fields] == ['n_pools', 'T', 'pools', 'model', 'xe', 'graph_off', 'row_ptr', 'col_idx', 'q']
    size = 0
    for (name, pointer, ctype), (_, bound) in zip(fields, EvalMixed._fields_):
        width = 8 if pointer else {'int32_t': 4}[ctype]
        assert C.sizeof(bound) == width and getattr(EvalMixed, name).offset == size, name         # no padding anywhere
        size += width
    assert C.sizeof(EvalMixed) == size == 64
    assert fields[2] == ('pools', True, 'v2x_eval') and EvalMixed._fields_[2][1]._type_ is vlib.Eval
    # the sibling of v2x_rollout_mixed: the same fields around another pool type
    assert [f[0] for f in _declared_fields('v2x_rollout_mixed')] == [f[0] for f in fields] and C.sizeof(RolloutMixed) == size


def test_the_first_checks_refuse_before_anything_is_launched():
    lib = vlib.load_library()

    def refused(m, *words):
        assert lib.v2x_eval_steps_mixed(C.byref(m) if m is not None else None, None) == V2X_EINVAL
        err = lib.v2x_last_error(None).decode()
        assert err.startswith("eval_steps_mixed: ") and all(w in err for w in words), err

    table = (vlib.Eval * 9)()
    refused(None, "null evaluation")
    refused(vlib.EvalMixed(n_pools=0, T=1, pools=table), "1..8 pools", "n_pools = 0")
    refused(vlib.EvalMixed(n_pools=9, T=1, pools=table), "1..8 pools", "n_pools = 9")
    refused(vlib.EvalMixed(n_pools=2, T=1), "non-null pool table")
    refused(vlib.EvalMixed(n_pools=2, T=3, pools=table), "pool 0", "walks T = 0 steps, the call T = 3")
    table[0].T = table[1].T = 3
    table[1].model = 0x10000
    refused(vlib.EvalMixed(n_pools=2, T=3, pools=table), "pool 0 (0 links): eval_steps: null pointer (actions is required)")
    table[0].model = 0x10000
    refused(vlib.EvalMixed(n_pools=2, T=3, pools=table), "pool 0", "has a model of its own")


# ------------------------------------------------------------------------------------------------------- the draws of an episode
def _stub_envs(shapes):
    return [types.SimpleNamespace(E=E, n_Veh=n) for E, n in shapes]


@pytest.mark.parametrize("eps", [0.0, 0.4, 1.0])
def test_the_draws_taken_ahead_consume_the_stream_like_the_host_loop(eps):
    shapes, T, C_ = [(2, 4), (1, 8), (3, 12)], 5, 4
    envs = _stub_envs(shapes)
    np.random.seed(77)
    steps = [mixed.draw_eval_step(envs, C_, eps) for _ in range(T)]
    state_loop = np.random.get_state()
    np.random.seed(77)
    baseline, explore, rand = mixed.draw_eval_episode_ahead(envs, C_, eps, T)
    state_ahead = np.random.get_state()
    assert state_loop[2] == state_ahead[2] and np.array_equal(state_loop[1], state_ahead[1])
    # ... and both are the order the host loop is documented with, restated: per step, per environment in ascending size, per
    # simulator the random scheme's action, the uniform draw, and the policy's random action when that draw is below epsilon
    np.random.seed(77)
    for t in range(T):
        for k, (E, n) in enumerate(shapes):
            for e in range(E):
                b = np.random.randint(0, C_, size=(n, 1)).reshape(n)
                x = np.random.random() < eps
                r = np.random.randint(0, C_, size=(n, 1)).reshape(n) if x else np.zeros(n, int)
                for got in ((baseline[k][t, e], explore[k][t, e], rand[k][t, e]), (steps[t][0][k][e], steps[t][1][k][e], steps[t][2][k][e])):
                    assert np.array_equal(got[0], b) and bool(got[1]) == x and np.array_equal(got[2], r), (t, k, e)
    restated = np.random.get_state()
    assert restated[2] == state_ahead[2] and np.array_equal(restated[1], state_ahead[1])
    for k, (E, n) in enumerate(shapes):
        assert baseline[k].shape == rand[k].shape == (T, E, n) and explore[k].shape == (T, E) and explore[k].dtype == np.uint8
    flags = np.concatenate([x.reshape(-1) for x in explore])
    assert flags.all() if eps == 1.0 else not flags.any() if eps == 0.0 else (flags.any() and not flags.all())


# ------------------------------------------------------------------------------------------------------- the driver
BASE = ["--save-dir", "D", "--mixed-links", "8,12"]


@pytest.mark.parametrize("extra,message", [
    (["--opt-rank"], "--mixed-links has no ranks"),
    (["--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device", "--trajectory-walk", "wide"],
     "--mixed-links walks serially"),
    (["--opt", "--opt-backend", "host"], "--mixed-links searches the optimum on the GPU"),
    (["--envs", "0"], "--envs must be at least 1"),
    (["--eval-backend", "device"], "--eval-backend device needs --sim-backend device --sim-streams device"),
    (["--sim-streams", "device"], "--sim-streams device needs --sim-backend device"),
    (["--eval-links", "8,10"], "--eval-links: every link count must be a multiple of 4"),
    (["--eval-links", "8,8"], "--eval-links: the link counts must be distinct"),
])
def test_the_driver_refuses_with_a_message_of_its_own(extra, message, capsys):
    with pytest.raises(SystemExit) as exit_:
        rl_run.parse_args(BASE + extra)
    assert exit_.value.code == 2
    assert message in capsys.readouterr().err


def test_the_mixed_options_need_mixed_links(capsys):
    for extra in (["--eval-links", "8"], ["--envs", "2"]):
        with pytest.raises(SystemExit):
            rl_run.parse_args(["--save-dir", "D"] + extra)
        assert "--eval-links / --envs need --mixed-links" in capsys.readouterr().err


def test_eval_links_default_to_the_training_sizes_and_the_search_to_the_gpu():
    _, args = rl_run.parse_args(["--save-dir", "D", "--mixed-links", "20,8,12"])
    assert args.mixed_links == [8, 12, 20] and args.eval_links == [8, 12, 20] and args.envs == 1
    assert args.opt_backend == "device" and args.eval_backend == "host"
    _, args = rl_run.parse_args(["--save-dir", "D", "--mixed-links", "8,12,20", "--eval-links", "28,8,16", "--envs", "3", "--opt",
                                 "--opt-backend", "bound"])
    assert args.mixed_links == [8, 12, 20] and args.eval_links == [8, 16, 28] and args.envs == 3 and args.opt_backend == "bound"
    _, args = rl_run.parse_args(["--save-dir", "D"])                     # without --mixed-links nothing changes
    assert args.mixed_links is None and args.opt_backend == "host"


def test_test_run_refuses_before_any_draw_or_reset():
    """the checks of MixedAgent.test_run need no engine: an object with the agent's few attributes suffices"""
    resets = []
    env = types.SimpleNamespace(E=2, n_Veh=8, n_RB=4, observe_packed=None, packed_ok=lambda c: True,
                                new_random_game=lambda n: resets.append(n))
    agent = types.SimpleNamespace(num_CH=4)
    check = lambda *a: mixed.MixedAgent._check_test_run(agent, *a)       # noqa: E731
    np.random.seed(3)
    before = np.random.get_state()
    with pytest.raises(ValueError, match="opt_backend must be one of"):
        check([env], 'host', 'host', 5)
    with pytest.raises(ValueError, match="eval_backend must be one of"):
        check([env], 'device', 'trajectory', 5)
    with pytest.raises(ValueError, match="must be a DeviceBatchedEnviron with streams='device', got SimpleNamespace"):
        check([env], 'device', 'device', 5)
    with pytest.raises(ValueError, match="the link counts must be distinct"):
        check([env, env], 'device', 'host', 5)
    with pytest.raises(ValueError, match="1..8 link counts"):
        check([], 'device', 'host', 5)
    assert check([env], 'bound', 'host', 5) == [env]
    assert not resets and np.array_equal(np.random.get_state()[1], before[1]) and np.random.get_state()[2] == before[2]
