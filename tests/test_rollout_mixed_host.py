"""Host side of the mixed-size resident rollout (v2x_rollout_steps_mixed: rl/device_sim.py mixed_rollout_bases, rl/mixed.py
MixedAgent(rollout=...), rl/train.py --mixed-rollout, the binding of the new struct): no GPU."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.rl import train
from v2xgnn.rl.agent import MAX_EPSILON, MIN_EPSILON
from v2xgnn.rl.device_sim import DeviceBatchedEnviron, mixed_rollout_bases
from v2xgnn.rl.mixed import MixedAgent, MixedReplay, ROLLOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the bases
@pytest.mark.parametrize("pools,T", [([(1, 4), (3, 5), (2, 31)], 3), ([(2, 4)], 1), ([(2, 4)], 4), ([(1, n) for n in range(4, 12)], 1),
                                     ([(1, 8), (5, 20)], 2), ([(10, 8), (10, 12), (10, 20), (10, 28)], 2)])
def test_bases_are_a_brute_force_count_of_what_lies_before_a_pool(pools, T):
    graph_pool, row_pool, edge_pool = [], [], []                         # the pool of every graph / row / edge, in batch order
    for k, (E, n) in enumerate(pools):
        for _t in range(T):
            for _e in range(E):
                graph_pool.append(k)
                row_pool += [k] * n
                edge_pool += [k] * (n * (n - 2))
    gbase, rbase, ebase, (B, R, Ed) = mixed_rollout_bases(pools, T)
    assert (B, R, Ed) == (len(graph_pool), len(row_pool), len(edge_pool))
    for k, (E, n) in enumerate(pools):
        assert gbase[k] == graph_pool.index(k) and rbase[k] == row_pool.index(k) and ebase[k] == edge_pool.index(k)
        # transition (k, t, e) reads rows rbase_k + (t E_k + e) n_k + i: the last one is the pool's last row
        assert rbase[k] + ((T - 1) * E + E - 1) * n + n - 1 == len(row_pool) - 1 - row_pool[::-1].index(k)


# ------------------------------------------------------------------------------------------------------- the draws
def _bare_agent(sizes_and_E, num_step, train_steps):
    """a MixedAgent without engines or simulators: what the drawing rule reads"""
    agent = MixedAgent.__new__(MixedAgent)
    agent.envs = [types.SimpleNamespace(E=E, n_Veh=n) for n, E in sizes_and_E]
    agent.num_CH = 4
    agent.n_sims = sum(E for _, E in sizes_and_E)
    agent.n_iter = -(-50 // agent.n_sims)
    agent.num_transition = agent.n_iter * agent.n_sims
    agent.num_Episodes, agent.num_Train_Step = 1, train_steps
    agent.num_step, agent.epsilon = num_step, MAX_EPSILON
    return agent


def _iterations_drawing_loop(agent, n_iter):
    """the drawing loop of MixedAgent._iteration as it stood before the draws could be taken ahead, n_iter iterations of it"""
    num_step, epsilon, out = agent.num_step, None, []
    for _ in range(n_iter):
        steps = agent.num_Episodes * 0.8 * agent.num_Train_Step * agent.num_transition
        per_step = (MAX_EPSILON - MIN_EPSILON) / steps
        actions, greedy, step_no = [], [], num_step
        for env in agent.envs:
            E, n = env.E, env.n_Veh
            a, g = np.zeros((E, n, 1), int), []
            for e in range(E):
                epsilon = MAX_EPSILON - per_step * step_no if step_no < steps else MIN_EPSILON
                step_no += 1
                if np.random.random() < epsilon:
                    a[e] = np.random.randint(0, 4, size=(n, 1))
                else:
                    g.append(e)
            actions.append(a)
            greedy.append(g)
        out.append((actions, greedy))
        num_step += agent.n_sims
    return out, epsilon


@pytest.mark.parametrize("pools,num_step,train_steps", [([(4, 2), (8, 3)], 0, 20), ([(4, 2), (8, 3)], 300, 10),
                                                        ([(4, 17), (8, 17), (12, 17)], 400, 20), ([(8, 1)], 400, 20)])
def test_draws_taken_ahead_are_the_iterations_draws_and_leave_the_same_generator_state(pools, num_step, train_steps):
    agent = _bare_agent(pools, num_step, train_steps)
    np.random.seed(77)
    want, want_eps = _iterations_drawing_loop(agent, agent.n_iter)
    want_state = np.random.get_state()
    np.random.seed(77)
    got = agent._draw_rollout_ahead(agent.n_iter)
    got_state = np.random.get_state()
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1]) and got_state[2:] == want_state[2:]
    assert agent.epsilon == want_eps and agent.num_step == num_step     # (the rollout advances num_step, not the draws)
    assert len(got) == agent.n_iter
    for (ga, gg), (wa, wg) in zip(got, want):
        assert gg == wg and all(np.array_equal(x, y) for x, y in zip(ga, wa))
    if num_step:
        assert any(g for _, gg in got for g in gg) and any(len(g) < env.E for _, gg in got for g, env in zip(gg, agent.envs))


# ------------------------------------------------------------------------------------------------------- the constructor
class _FakeEnv(object):
    def __init__(self, n):
        self.n_Veh, self.n_RB, self.E = n, 4, 2
        self.observe_packed = lambda c: None
        self.packed_ok = lambda c: c == 4


def _device_env(n, streams):
    """a DeviceBatchedEnviron as far as the constructor's checks look at it (no simulator behind it)"""
    env = DeviceBatchedEnviron.__new__(DeviceBatchedEnviron)
    env.n_Veh, env.n_RB, env.E, env.stream_backend = n, 4, 2, streams
    return env


def test_mixed_agent_refuses_a_rollout_it_does_not_know_and_trajectory_without_device_streams():
    assert ROLLOUTS == ('host', 'trajectory')
    with pytest.raises(ValueError, match=r"MixedAgent: rollout must be one of \['host', 'trajectory'\], got 'device'"):
        MixedAgent([_FakeEnv(8), _FakeEnv(12)], None, 16, rollout='device')
    with pytest.raises(ValueError, match="rollout='trajectory' steps every environment on the device: the environment of 8 links "
                                         "must be a DeviceBatchedEnviron with streams='device', got _FakeEnv"):
        MixedAgent([_FakeEnv(8), _FakeEnv(12)], None, 16, rollout='trajectory')
    with pytest.raises(ValueError, match="environment of 12 links must be a DeviceBatchedEnviron with streams='device', got "
                                         "DeviceBatchedEnviron with streams='host'"):
        MixedAgent([_device_env(8, 'device'), _device_env(12, 'host')], None, 16, rollout='trajectory')


def test_mixed_replay_forwards_to_a_pool_it_has():
    rep = MixedReplay.__new__(MixedReplay)
    rep.sizes, rep.pools = [4, 8], {}
    calls = []
    for n in rep.sizes:
        rep.pools[n] = types.SimpleNamespace(reserve=lambda K, n=n: calls.append(('reserve', n, K)) or 5 * n,
                                             commit=lambda K, row, n=n: calls.append(('commit', n, K, row)),
                                             storage=lambda n=n: {'pool': n})
    assert rep.reserve(8, 6) == 40 and rep.storage(4) == {'pool': 4}
    rep.commit(8, 6, 'row')
    assert calls == [('reserve', 8, 6), ('commit', 8, 6, 'row')]
    for call in (lambda: rep.reserve(5, 1), lambda: rep.commit(5, 1, None), lambda: rep.storage(5)):
        with pytest.raises(ValueError, match=r"no pool of 5 links \(pools: \[4, 8\]\)"):
            call()


# ------------------------------------------------------------------------------------------------------- the command line
DEVICE = ["--mixed-sim-backend", "device", "--mixed-sim-streams", "device"]


@pytest.mark.parametrize("argv,want", [
    (["--mixed-links", "8,12", "--envs", "2"], ("host", "host", "host")),
    (["--mixed-links", "8,12", "--envs", "2", "--mixed-sim-backend", "device"], ("device", "host", "host")),
    (["--mixed-links", "8,12", "--envs", "2"] + DEVICE, ("device", "device", "host")),
    (["--mixed-links", "8,12,20,28", "--envs", "10"] + DEVICE + ["--mixed-rollout", "trajectory"], ("device", "device", "trajectory")),
])
def test_mixed_links_is_accepted_with_device_simulators_and_the_trajectory_rollout(argv, want, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    _, args = train.parse_args(argv)
    assert (args.mixed_sim_backend, args.mixed_sim_streams, args.mixed_rollout) == want
    assert train.parse_mixed_links(args.mixed_links)[0] == 8


@pytest.mark.parametrize("argv,text", [
    (["--mixed-links", "8,12", "--envs", "2", "--mixed-rollout", "trajectory"],
     "--mixed-rollout trajectory needs --mixed-sim-backend device"),
    (["--mixed-links", "8,12", "--envs", "2", "--mixed-sim-backend", "device", "--mixed-rollout", "trajectory"],
     "--mixed-rollout trajectory needs --mixed-sim-backend device --mixed-sim-streams device"),
    (["--mixed-links", "8,12", "--envs", "2", "--mixed-sim-streams", "device"],
     "--mixed-sim-streams device needs --mixed-sim-backend device"),
    (["--mixed-links", "8,12", "--envs", "2"] + DEVICE + ["--rollout", "device"], "--rollout device holds one link count"),
    (["--mixed-links", "8,12", "--envs", "2"] + DEVICE + ["--mixed-rollout", "trajectory", "--trajectory-walk", "wide"],
     "--mixed-links walks serially"),
    (["--mixed-links", "8,12", "--envs", "2"] + DEVICE + ["--mixed-rollout", "trajectory", "--rollouts", "sharded"],
     "--mixed-links runs on one GPU"),
    (["--links", "8", "--envs", "2", "--mixed-rollout", "trajectory"], "need --mixed-links"),
])
def test_mixed_rollout_options_are_refused_with_a_message(argv, text, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    with pytest.raises(SystemExit) as exc:
        train.parse_args(argv)
    assert exc.value.code == 2
    assert text in capsys.readouterr().err


def test_mixed_trajectory_rollout_is_refused_under_data_parallelism(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        train.parse_args(["--mixed-links", "8,12", "--envs", "2"] + DEVICE + ["--mixed-rollout", "trajectory"])
    assert "--mixed-links runs on one GPU" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- the binding
FIELDS = ("n_pools", "T", "pools", "model", "xe", "graph_off", "row_ptr", "col_idx", "q")


def test_the_ctypes_struct_has_the_size_and_the_offsets_of_the_headers(tmp_path):
    """the header compiled as C by gcc, the host compiler csrc/Makefile builds libv2xsim.so with (so a machine that built the
    libraries has it); CC names another one"""
    assert tuple(f[0] for f in vlib.RolloutMixed._fields_) == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "v2xgnn.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(v2x_rollout_mixed), sizeof(v2x_rollout_traj));\n'
                   + ''.join('  printf(" %%zu", offsetof(v2x_rollout_mixed, %s));\n' % f for f in FIELDS) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(vlib.RolloutMixed) and got[1] == C.sizeof(vlib.RolloutTraj)
    assert got[2:] == [getattr(vlib.RolloutMixed, f).offset for f in FIELDS]


def test_the_entry_point_is_declared_exported_and_bound_alike():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+v2x_rollout_steps_mixed\s*\(([^)]*)\)\s*;', hdr)
    assert m and len(m.group(1).split(',')) == 2
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), "v2x_rollout_steps_mixed")
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert bound["v2x_rollout_steps_mixed"] == (C.c_int, [C.POINTER(vlib.RolloutMixed), C.c_void_p])
    assert vlib.MIXED_MAX_POOLS == 8
