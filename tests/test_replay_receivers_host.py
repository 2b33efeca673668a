"""No GPU needed: the replay memory that stores a transition's adjacency as its receivers (rl/replay.py ReceiverReplay) and
its one-launch gather (v2x_replay_gather_recv) -- the entry point is declared, exported and bound alike; every argument
error comes back as V2X_EINVAL before anything is launched (the pointers handed over are never dereferenced by the host);
receivers derived from an adjacency give that adjacency back and malformed matrices are refused; the table of first
edges is the host packer's cumulative edge count; the closed-form CSR row the kernel implements is packing.adj_to_csr's;
and Agent / rl.train take the new options and refuse what they do not serve."""
import ctypes as C
import os
import random
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL
from v2xgnn.packing import adj_to_csr
from v2xgnn.rl import Agent, RL_Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000                                              # a non-null, 16-byte aligned "device pointer": checked, never read


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


def _err(lib):
    return lib.v2x_last_error(None).decode()


# ---------------------------------------------------------------------------- symbols
def test_entry_point_is_declared_exported_and_bound_alike():
    m = re.search(r'\bint\s+v2x_replay_gather_recv\s*\(([^)]*)\)\s*;', _header())
    assert m, "v2x_replay_gather_recv is not declared in include/v2xgnn.h"
    assert len([a for a in m.group(1).split(',') if a.strip()]) == 3
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), "v2x_replay_gather_recv")
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert bound["v2x_replay_gather_recv"][0] is C.c_int
    assert bound["v2x_replay_gather_recv"][1] == [C.POINTER(vlib.ReplayRecv), C.POINTER(vlib.MixedBatch), C.c_void_p]


def test_binding_has_the_fields_of_the_declared_struct():
    body = re.search(r'typedef struct v2x_replay_recv \{(.*?)\} v2x_replay_recv;', _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part) for part in decl.split(None, 1)[1].split(',')]
    names = [re.sub(r'^(const)?(double|float|u?int\d+_t)', '', n) for n in names]
    assert names == [f[0] for f in vlib.ReplayRecv._fields_], (names, [f[0] for f in vlib.ReplayRecv._fields_])
    assert C.sizeof(vlib.ReplayRecv) == 2 * 4 + 7 * 8                    # two int32, seven pointers: no padding


# ---------------------------------------------------------------------------- refusals
SRC = dict(n_nodes=32, count=4, xe=P, xe_next=P, recv=P, action=P, reward=P, idx=P, edge_base=None)
OUT = dict(xe=P, xe_next=P, action=P, reward=P, graph_off=None, row_ptr=P, col_idx=P)


def _call(lib, src=None, out=None):
    s = vlib.ReplayRecv(**dict(SRC, **(src or {})))
    o = vlib.MixedBatch(**dict(OUT, **(out or {})))
    return lib.v2x_replay_gather_recv(C.byref(s), C.byref(o), None)


@pytest.mark.parametrize("src,out,word", [
    (dict(n_nodes=2), None, "n_nodes 2"), (dict(n_nodes=129), None, "n_nodes 129"), (dict(n_nodes=0), None, "n_nodes 0"),
    (dict(count=0), None, "count 0"), (dict(count=-3), None, "count -3"),
    (dict(xe=P + 4), None, "16-byte"), (dict(xe_next=P + 8), None, "16-byte"),
    (None, dict(xe=P + 4), "16-byte"), (None, dict(xe_next=P + 12), "16-byte"),
    # K n (n - 1) beyond int32 (K n still fits), K n beyond int32
    (dict(n_nodes=128, count=132105), None, "int32"), (dict(n_nodes=100, count=216931), None, "int32"),
    (dict(n_nodes=3, count=(1 << 31) // 3 + 1), None, "int32")]
    + [({k: None}, None, "null source") for k in ("xe", "xe_next", "recv", "action", "reward", "idx")]
    + [(None, {k: None}, "null output") for k in ("xe", "xe_next", "action", "reward", "row_ptr", "col_idx")])
def test_argument_errors_are_einval_before_any_launch(src, out, word):
    lib = vlib.load_library()
    assert _call(lib, src, out) == V2X_EINVAL, (src, out)
    assert "replay_gather_recv" in _err(lib) and word in _err(lib), (src, out, _err(lib))


def test_null_structs_are_einval():
    lib = vlib.load_library()
    assert lib.v2x_replay_gather_recv(None, C.byref(vlib.MixedBatch(**OUT)), None) == V2X_EINVAL and "null" in _err(lib)
    assert lib.v2x_replay_gather_recv(C.byref(vlib.ReplayRecv(**SRC)), None, None) == V2X_EINVAL and "null" in _err(lib)


# ---------------------------------------------------------------------------- receivers <-> adjacency
def _random_receivers(rng, K, n, own_rate=0.1):
    """recv [K, n]: a random p != q per link, and q itself (own receiver) for about own_rate of the links"""
    r = rng.integers(0, n - 1, size=(K, n))
    r = r + (r >= np.arange(n)[None, :])
    own = rng.random((K, n)) < own_rate
    return np.where(own, np.arange(n)[None, :], r).astype(np.int32)


def _agent_style_adjacency(recv):
    """Agent.adjacency (BS_brain.py:441-445) for given receivers: ones, except the diagonal and Adj[receiver of q, q]"""
    K, n = recv.shape
    adj = np.zeros((K, n, n))
    for k in range(K):
        for p in range(n):
            for q in range(n):
                if p != q and p != recv[k, q]:
                    adj[k, p, q] = 1
    return adj


@pytest.mark.parametrize("n", [3, 20, 32, 33, 100, 128])
def test_receivers_round_trip_through_the_adjacency(n):
    from v2xgnn.rl.replay import receivers_from_adjacency, receivers_to_adjacency
    rng = np.random.default_rng(n)
    K = 6
    recv = _random_receivers(rng, K, n, own_rate=0.15)
    recv[0] = _random_receivers(rng, 1, n, own_rate=0.0)[0]              # one regular graph
    recv[1, n - 1] = n - 1                                               # own receivers at the first and the last link
    recv[1, 0] = 0
    adj = _agent_style_adjacency(recv)
    keep = adj.copy()
    got, own = receivers_from_adjacency(adj)
    assert got.dtype == np.int32 and np.array_equal(got, recv) and np.array_equal(adj, keep)
    assert np.array_equal(own, (recv == np.arange(n)[None, :]).sum(axis=1)) and own[0] == 0 and own[1] >= 2
    assert np.array_equal(receivers_to_adjacency(got), adj)


def test_malformed_adjacencies_are_value_errors_that_name_the_link():
    from v2xgnn.rl.replay import ReceiverReplay, receivers_from_adjacency
    n = 6
    good = _agent_style_adjacency(np.array([[1, 2, 3, 4, 5, 0]]))
    bad = good.copy()
    bad[0, 4, 4] = 1                                                     # a nonzero diagonal entry
    with pytest.raises(ValueError, match="link 4 .*diagonal"):
        receivers_from_adjacency(bad)
    bad = good.copy()
    bad[0, 0, 2] = 0                                                     # two zero off-diagonal entries in column 2 (with [3, 2])
    with pytest.raises(ValueError, match="link 2 has 2"):
        receivers_from_adjacency(bad)
    bad = np.concatenate([good, good, good])
    bad[2, :, 5] = 0                                                     # nobody sends to link 5 of the third transition
    with pytest.raises(ValueError, match="transition 2: link 5 has 5"):
        receivers_from_adjacency(bad)
    with pytest.raises(ValueError):
        receivers_from_adjacency(good[0])                                # [n, n]: not a block of transitions
    rep = ReceiverReplay(16, n)                                          # the memory refuses them when they are added
    z = np.zeros((1, n, 9)), np.zeros((1, n, 4))
    with pytest.raises(ValueError, match="link 5"):
        rep.add_many(z[0], z[1], bad[2:], np.zeros((1, n), int), [0.0], z[0], z[1])
    with pytest.raises(ValueError, match="holds 6 links"):
        rep.add_many(z[0], z[1], np.ones((1, 5, 5)) - np.eye(5), np.zeros((1, n), int), [0.0], z[0], z[1])
    assert len(rep) == 0
    for n_bad in (2, 129):
        with pytest.raises(ValueError, match="3..128"):
            ReceiverReplay(16, n_bad)


def test_edge_base_is_the_cumulative_edge_count_of_the_host_packer():
    from v2xgnn.rl.replay import edge_base_of, receivers_from_adjacency
    rng = np.random.default_rng(9)
    for n in (3, 5, 33):
        recv = _random_receivers(rng, 12, n, own_rate=0.2)
        recv[4] = _random_receivers(rng, 1, n, own_rate=0.0)[0]
        adj = _agent_style_adjacency(recv)
        idx = rng.integers(0, 12, size=17)                               # a minibatch with repeats
        _, own = receivers_from_adjacency(adj)
        eb = edge_base_of(n, own[idx])
        row_ptr, col, _ = adj_to_csr(adj[idx])
        assert eb.dtype == np.int32 and np.array_equal(eb, row_ptr[::n]) and eb[-1] == len(col)
    with pytest.raises(ValueError, match="int32"):
        edge_base_of(128, np.zeros(140000, np.int32))


# ---------------------------------------------------------------------------- the closed-form row
def closed_form_row(n, q, r):
    """sources of row q for receiver r (r == q: own receiver), as csrc/kernels.hpp k_replay_gather_recv computes them:
    entry o is p = o, then p += (p >= min(q, r)), then, if r != q, p += (p >= max(q, r))"""
    o = np.arange(n - 2 + (1 if r == q else 0))
    p = o + (o >= min(q, r))
    if r != q:
        p = p + (p >= max(q, r))
    return p.astype(np.int32)


@pytest.mark.parametrize("n", [3, 4, 33])
def test_closed_form_row_is_the_host_packers_for_every_link_and_receiver(n):
    for q in range(n):
        for r in range(n):
            recv = (np.arange(n, dtype=np.int32)[None, :] + 1) % n       # link q' listens to q' + 1 ...
            recv[0, q] = r                                               # ... except the row under test
            row_ptr, col, _ = adj_to_csr(_agent_style_adjacency(recv))
            assert np.array_equal(closed_form_row(n, q, r), col[row_ptr[q]:row_ptr[q + 1]]), (n, q, r)
            # the row starts where the rule says: q (n - 2) + the own-receiver rows before it
            assert row_ptr[q] == q * (n - 2) + int((recv[0, :q] == np.arange(q)).sum())


# ---------------------------------------------------------------------------- Agent and command line
def _fake_gpu_agent(n, **kw):
    from test_rl_agent import RecordingBrain
    from test_rl_env import make_env
    random.seed(3)
    np.random.seed(3)
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 8, 1, 0.1)
    env = make_env()
    env.new_random_game(n)
    brain = RecordingBrain(n, 3, 1, 16, 1, 4)
    brain.model = types.SimpleNamespace(engine=types.SimpleNamespace(_h=1, device=0))      # looks like the gfx950 engine
    return Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain, **kw), env, cfg, brain


def test_agent_builds_the_receiver_memory_at_32_links_and_keeps_the_other_options():
    from v2xgnn.rl.replay import DeviceReplay, ReceiverReplay
    agent, env, cfg, brain = _fake_gpu_agent(32, device_replay='receivers')
    assert type(agent.device_replay) is ReceiverReplay and agent.device_replay.n == 32
    assert agent._packed_rollouts() is False
    with pytest.raises(ValueError, match="resident rollouts hold 3..31 links"):
        Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain, device_replay='receivers', rollout_backend='device')
    with pytest.raises(ValueError, match="resident rollouts hold 3..31 links"):
        Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain, device_replay='receivers', rollout_backend='trajectory')
    # 'auto' and True as before: the host memory at 32 links, a refusal that says why
    assert Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain).device_replay is None
    with pytest.raises(ValueError, match="at most 31 links"):
        Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain, device_replay=True)
    # without the engine: the refusal of device_replay=True
    host_brain = type(brain)(32, 3, 1, 16, 1, 4)
    with pytest.raises(ValueError, match="gfx950 engine"):
        Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=host_brain, device_replay='receivers')
    # the methods a device call would write through are refused
    rep = agent.device_replay
    for call in (rep.storage, lambda: rep.reserve(4), lambda: rep.commit(4, None), lambda: rep.stage_early(None, None, None),
                 lambda: rep.add_many_packed(*[None] * 7), lambda: rep.prefetch_indices([0], 1)):
        with pytest.raises(NotImplementedError, match="3..31 links"):
            call()


def test_agent_receiver_memory_below_32_links_is_opt_in_too():
    from v2xgnn.rl.replay import DeviceReplay, ReceiverReplay
    agent, env, cfg, brain = _fake_gpu_agent(8, device_replay='receivers')
    assert type(agent.device_replay) is ReceiverReplay
    assert type(Agent(8, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain).device_replay) is DeviceReplay


@pytest.mark.parametrize("envs", [0, 3])
def test_rollouts_stage_their_transitions_in_the_receiver_memory(envs):
    """generate_d2d_transition at 32 links, one simulator (add) and three batched ones (add_many through the array path):
    the transitions are staged for the HBM memory with the simulator's receivers, the host list keeps placeholders only"""
    from v2xgnn.rl.replay import receivers_to_adjacency
    agent, env, cfg, brain = _fake_gpu_agent(32, device_replay='receivers')
    if envs:
        from v2xgnn.rl.train import start_env_batched
        env = start_env_batched(32, envs, 11)
        agent = Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=brain, device_replay='receivers')
        assert agent._batched() and not agent._packed_rollouts()
    agent.num_Episodes, agent.num_Train_Step = 1, 1
    _, adj = agent.observe() if not envs else (None, env.observe(env.n_RB)[1][0])
    agent.generate_d2d_transition(6)
    rep = agent.device_replay
    assert len(rep) == 6 and rep._n_staged == 6 and rep.size == 0
    assert len(agent.memory.samples) == 6 and all(s is None for s in agent.memory.samples)
    recv = np.concatenate([s[2] for s in rep._stage])
    assert recv.shape == (6, 32) and recv.dtype == np.int32
    assert np.array_equal(receivers_to_adjacency(recv[:1])[0], adj)      # (the receivers hold for the whole episode)


def test_command_line_takes_replay_receivers_and_refuses_what_it_does_not_serve(capsys):
    from v2xgnn.rl.train import parse_args
    _, args = parse_args(["--links", "100", "--replay", "receivers"])
    assert args.replay == "receivers" and args.links == 100
    assert parse_args([])[1].replay == "auto"
    for argv, word in ((["--replay", "receivers", "--mixed-links", "8,12", "--envs", "2"], "--mixed-links"),
                       (["--replay", "receivers", "--rollout", "device", "--sim-backend", "device", "--sim-streams", "device",
                         "--envs", "2"], "--rollout host"),
                       (["--replay", "receivers", "--rollout", "trajectory"], "--rollout host"),
                       (["--replay", "hbm"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert word in capsys.readouterr().err, argv
