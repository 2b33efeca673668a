"""GPU: resident DQN rollouts at 3..128 links on the receiver replay -- the observation in receiver form
(v2x_sim_observe_recv), the closed-form CSR of resident graphs (v2x_csr_from_recv), the one-call rollout
(v2x_rollout_steps_recv: the wide walk, k_traj_observe_recv, the CSR, one forward, k_rollout_finish_recv;
DeviceChannels.rollout_steps_recv) and Agent(device_replay='receivers', rollout_backend='trajectory').
Every comparison is byte for byte.  Up to 31 links the references are the existing kernels (v2x_sim_observe,
v2x_rollout_steps_wide into a DeviceReplay); beyond them the single-step device calls that already serve 128 links
(v2x_sim_stream, v2x_sim_channels, v2x_sim_rates), the host library's observation (v2xsim_observe), the host packer
(packing.adj_to_csr, PackedBatch.from_dense) and the engine's forward.  The engine scores 4 channels: rb = 4 throughout."""
import ctypes

import numpy as np
import pytest

from test_gpu_rollout_trajectory import HEIGHT, LANES, WIDTH, _engine, start_channels, start_state
from v2xgnn import PackedBatch
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.packing import adj_to_csr
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config, native_sim
from v2xgnn.rl.device_sim import FLAG_BAD, FLAG_OWN
from v2xgnn.rl.replay import DeviceReplay, ReceiverReplay, receivers_from_adjacency
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

RB = 4
MARK = 7
# every resident tensor a step writes that both forms of the observation share (mask / col / regular and recv / flags apart)
SHARED = ('keys', 'mtpos', 'pos', 'dirs', 'u', 'v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff', 'interf_db', 'state',
          'xe', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf', 'actions')
WALKED = ('keys', 'mtpos', 'pos', 'dirs', 'u', 'v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff')


def _dev():
    import torch
    return torch.device('cuda', 0)


def _bytes(dc, *names):
    return {k: dc.tensor(k).cpu().numpy().tobytes() for k in names}


def _recv_storage(capacity, n):
    """storage tensors in ReceiverReplay's layout, every element the marker"""
    import torch
    mk = lambda shape, dt: torch.full((capacity,) + shape, MARK, dtype=dt, device=_dev())   # noqa: E731
    return {'xe': mk((n, 16), torch.float32), 'xe_next': mk((n, 16), torch.float32), 'recv': mk((n,), torch.int32),
            'action': mk((n,), torch.int32), 'reward': mk((), torch.float64)}


def _adjacency(dest):
    """Agent.adjacency (BS_brain.py:441-445) of receivers [E, n] -> [E, n, n]"""
    E, n = dest.shape
    adj = np.ones((E, n, n)) - np.eye(n)[None]
    adj[np.arange(E)[:, None], dest, np.arange(n)[None, :]] = 0
    return adj


def start_channels_recv(E, n, st):
    """start_channels with the observation in receiver form (any link count up to 128)"""
    dc = DeviceChannels(E, n, RB)
    dc.set_grid(LANES, WIDTH, HEIGHT, 0.01)
    for name, a in st.items():
        dc.upload(name, a)
    dc.stream(mobility=False)
    dc.step(dc.tensor('u'))
    dc.observe_recv()
    dc.upload('mtpos', st['mtpos'])
    return dc


def _host_observation(dc, dest):
    """v2xsim_observe on the channels `dc` holds -> (state [E, n, 13] float64, xe [E, n, 16] float32, adjacency)"""
    v2v, v2i = dc.download('v2v_ff', 'v2i_ff')
    state, adj = native_sim.observe(dest, v2v, v2i, dc.constants['p_v2v'], RB)
    xe = np.zeros(state.shape[:2] + (16,), np.float32)
    xe[:, :, :state.shape[2]] = state.astype(np.float32)
    return state, xe, adj


# ------------------------------------------------------------------------------ 1. the observation against the existing kernel
@pytest.mark.parametrize("n", [3, 5, 20, 31])
def test_observation_in_receiver_form_is_the_existing_observation(n):
    rng = np.random.default_rng(n)
    E, rb = 4, min(RB, n)
    dest = ((np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n).astype(np.int64)
    dest[1, n // 2] = n // 2                                             # a link that is its own receiver
    dest[2, 0], dest[2, n - 1] = -1, n                                   # receivers outside [0, n): below and above
    dest[3, n - 1] = n - 1
    dest[3, 0] = 0
    old, new = DeviceChannels(E, n, rb), DeviceChannels(E, n, rb)
    v2v = rng.normal(100.0, 12.0, size=(E, n, n, rb))
    v2i = rng.normal(95.0, 10.0, size=(E, n, rb))
    for dc in (old, new):
        dc.upload('v2v_ff', v2v)
        dc.upload('v2i_ff', v2i)
    old.observe(dest)
    new.observe_recv(dest)
    a, b = _bytes(old, 'state', 'xe', 'interf_db'), _bytes(new, 'state', 'xe', 'interf_db')
    for k in a:
        assert a[k] == b[k], (k, n)
    regular = old.download('regular').astype(bool)
    xe, recv, flags = new.fetch_observation_recv()
    assert regular.tolist() == [True, False, False, False]
    assert np.array_equal((flags & FLAG_OWN) != 0, ~regular)
    assert ((flags & FLAG_BAD) != 0).tolist() == [False, False, True, False]
    good = [0, 1, 3]
    assert recv.dtype == np.int32 and np.array_equal(recv[good], dest[good])
    assert np.array_equal(recv[2], np.arange(n))                         # the bad state: every link its own receiver ...
    state = new.download('state')
    assert np.isnan(state[2]).all() and np.isnan(new.download('interf_db')[2]).all() and not np.isnan(state[good]).any()
    assert np.isnan(xe[2, :, :3 * rb + 1]).all() and (xe[2, :, 3 * rb + 1:] == 0).all()
    assert new._own[0].tolist() == [0, 1, 0, 2] and new._own[1].tolist() == [False, False, True, False]


# ------------------------------------------------------------------------------ 2. the observation beyond the mask
def _host_channels(n, E, seed):
    """fast-fading arrays of a host BatchedEnviron after a reset, cut to n links (n need not be a multiple of 4)"""
    env = start_env_batched(-(-n // 4) * 4, E, seed, lookahead=False)
    v2v = np.ascontiguousarray(env.V2V_channels_with_fastfading[:, :n, :n, :])
    v2i = np.ascontiguousarray(env.V2I_channels_with_fastfading[:, :n, :])
    return v2v, v2i, float(env.V2V_power_dB_List[env.fixed_v2v_power_index])


@pytest.mark.parametrize("n", [32, 33, 64, 65, 128])
def test_observation_beyond_31_links_is_the_host_librarys(n):
    E = 2
    rng = np.random.default_rng(7 * n)
    v2v, v2i, power = _host_channels(n, E, 40 + n)
    dest = ((np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n).astype(np.int64)
    dest[1, [0, 31, n - 1]] = [0, 31, n - 1]                             # own receivers at both ends and at the old mask's last bit
    dc = DeviceChannels(E, n, RB)
    dc.upload('v2v_ff', v2v)
    dc.upload('v2i_ff', v2i)
    dc.observe_recv(dest, power=power)
    state, adj = native_sim.observe(dest, v2v, v2i, power, RB)
    xe, recv, flags = dc.fetch_observation_recv()
    assert dc.download('state').tobytes() == state.tobytes()
    want = np.zeros((E, n, 16), np.float32)
    want[:, :, :13] = state.astype(np.float32)
    assert xe.tobytes() == want.tobytes()
    ref_recv, ref_own = receivers_from_adjacency(adj)
    assert np.array_equal(recv, ref_recv) and flags.tolist() == [0, FLAG_OWN] and ref_own.tolist() == [0, len({0, 31, n - 1})]
    itf = native_sim.interference_db(dest, v2v, dc.constants['p_v2i'], dc.constants['veh_gain'], dc.constants['veh_nf'], dc.constants['sig2'])
    assert np.allclose(dc.download('interf_db'), itf.reshape(E, n, RB), rtol=1e-11, atol=0)      # (log10 / pow of two math libraries)


# ------------------------------------------------------------------------------ 3. the CSR of resident graphs
@pytest.mark.parametrize("n", [3, 32, 65, 128])
def test_csr_of_resident_graphs_is_the_host_packers(n):
    import torch
    E, G, GUARD = 2, 5, 64
    rng = np.random.default_rng(n)
    dest = ((np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n).astype(np.int64)
    dest[1, [0, n - 1]] = [0, n - 1]                                     # state 1: two own-receiver links
    dc = DeviceChannels(E, n, min(RB, n))
    dc.upload('v2v_ff', rng.normal(100.0, 10.0, size=dc.shapes()['v2v_ff']))
    dc.upload('v2i_ff', rng.normal(100.0, 10.0, size=dc.shapes()['v2i_ff']))
    dc.observe_recv(dest)
    adj = _adjacency(dest)
    # with edge_base: graphs 0..4 on states 0, 1, 0, 1, 0
    ref_rp, ref_col, _ = adj_to_csr(adj[np.arange(G) % E])
    own = np.array([0, 2])[np.arange(G) % E]
    eb = np.concatenate([[0], np.cumsum(n * (n - 2) + own)]).astype(np.int32)
    assert eb[-1] == len(ref_col)
    rp = torch.full((G * n + 1 + GUARD,), -MARK, dtype=torch.int32, device=_dev())
    col = torch.full((int(eb[-1]) + GUARD,), -MARK, dtype=torch.int32, device=_dev())
    dc.csr_from_recv(G, rp, col, edge_base=torch.from_numpy(eb).to(_dev()))
    rp_h, col_h = rp.cpu().numpy(), col.cpu().numpy()
    assert np.array_equal(rp_h[:G * n + 1], ref_rp) and np.array_equal(col_h[:eb[-1]], ref_col)
    assert (rp_h[G * n + 1:] == -MARK).all() and (col_h[eb[-1]:] == -MARK).all()
    # without: every graph regular (state 0 alone, G graphs of it)
    dc1 = DeviceChannels(1, n, min(RB, n))
    dc1.upload('v2v_ff', rng.normal(100.0, 10.0, size=dc1.shapes()['v2v_ff']))
    dc1.upload('v2i_ff', rng.normal(100.0, 10.0, size=dc1.shapes()['v2i_ff']))
    dc1.observe_recv(dest[:1])
    ref_rp, ref_col, _ = adj_to_csr(adj[np.zeros(G, int)])
    rp.fill_(-MARK)
    col.fill_(-MARK)
    dc1.csr_from_recv(G, rp, col)
    rp_h, col_h = rp.cpu().numpy(), col.cpu().numpy()
    ne = G * n * (n - 2)
    assert np.array_equal(rp_h[:G * n + 1], ref_rp) and np.array_equal(col_h[:ne], ref_col)
    assert (rp_h[G * n + 1:] == -MARK).all() and (col_h[ne:] == -MARK).all()
    # a regular call on a state that is not: nothing is stored beyond a regular graph's n (n - 2) edges
    col.fill_(-MARK)
    dc.csr_from_recv(2, rp, col)
    assert (col.cpu().numpy()[2 * n * (n - 2):] == -MARK).all()


# ------------------------------------------------------------------------------ 4. against the existing call, where both apply
def _policy(E, n, T, rng):
    explore = (rng.random((T, E)) < 0.5).astype(np.uint8)
    explore[:, 0] = 0                                                    # at least one greedy state per step
    explore[0, -1] = 1
    if T >= 2:
        explore[1] = 0
    return explore, rng.integers(0, RB, size=(T, E, n)).astype(np.int32)


@pytest.mark.parametrize("E,n,T", [(3, 5, 3), (1, 20, 4)])
def test_one_call_in_receiver_form_is_the_wide_call_into_the_existing_memory(E, n, T):
    K, cap = T * E, T * E + 5
    rng = np.random.default_rng(10 * n + E)
    st = start_state(E, n, 500 + n, [(0, 623, 624)[e % 3] for e in range(E)])
    explore, rand = _policy(E, n, T, rng)
    eng = _engine(n)
    old_dc, new_dc = start_channels(E, n, RB, st), start_channels_recv(E, n, st)
    old, new = DeviceReplay(cap, n), ReceiverReplay(cap, n, device_writes=True)
    head = old.reserve(K)
    r_old = old_dc.rollout_steps(explore, rand, old.storage(), head, old.capacity, 1.0, 0.1, engine=eng, row_ptr=old.row_ptr(K),
                                 walk='wide')
    old.commit(K, r_old)
    assert new.reserve(K) == head
    r_new = new_dc.rollout_steps_recv(explore, rand, new.storage(), head, new.capacity, 1.0, 0.1, engine=eng)
    new.commit(K, np.zeros(K, np.int32))
    assert r_new.resolve().reward.tobytes() == r_old.resolve().reward.tobytes()
    assert np.array_equal(r_new.regular, r_old.regular) and r_new.flags.shape == (T, 2, E) and not r_new.flags.any()
    for k in ('xe', 'xe_next', 'action', 'reward'):
        assert getattr(new, k)[:K].cpu().numpy().tobytes() == getattr(old, k)[:K].cpu().numpy().tobytes(), k
    assert np.array_equal(new.recv[:K].cpu().numpy(), np.tile(st['dest'], (T, 1)))
    a, b = _bytes(old_dc, *SHARED), _bytes(new_dc, *SHARED)
    for k in SHARED:
        assert a[k] == b[k], k
    assert np.array_equal(new_dc.download('recv'), st['dest']) and not new_dc.download('flags').any()
    idx = rng.integers(0, K, size=7)
    so, sn = old.sample(idx), new.sample(idx)
    for name in ('xe', 'row_ptr', 'col_idx'):
        for j in (0, 1):
            assert getattr(sn[j], name).cpu().numpy().tobytes() == getattr(so[j], name).cpu().numpy().tobytes(), (name, j)
    assert sn[2].cpu().numpy().tobytes() == so[2].cpu().numpy().tobytes() and sn[3].cpu().numpy().tobytes() == so[3].cpu().numpy().tobytes()
    eng.close()


# ------------------------------------------------------------------------------ 5. beyond 31 links
@pytest.mark.parametrize("n", [32, 33, 60, 61, 64, 65, 128])
def test_one_call_beyond_31_links_is_the_single_step_calls_the_host_observation_and_the_engine(n):
    """n + rb = 64 | 65 at 60 | 61 links (one wave of rate threads and one past it), the wave boundary of the 128-thread
    observation at 64 | 65, the limits 32 and 128.  33 links: state 1 has own-receiver links and is greedy at every step.
    60 links: the block starts at capacity - 2 and wraps."""
    import torch
    E, T, w_v2v, w_v2i = 2, 3, 1.0, 0.1
    K, cap = T * E, T * E + 3
    rng = np.random.default_rng(n)
    st = start_state(E, n, 700 + n, [623, 0])
    if n == 33:
        st['dest'][1, [0, 32]] = [0, 32]
    head = cap - 2 if n == 60 else 1
    explore, rand = _policy(E, n, T, rng)
    if n == 33:
        explore[:, 1] = 0
    eng = _engine(n)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    storage = _recv_storage(cap, n)
    res = A.rollout_steps_recv(explore, rand, storage, head, cap, w_v2v, w_v2i, engine=eng).resolve()
    io = A.rollout_steps_recv_buffers(T)
    o = io['offsets']['traj_xe']
    traj_xe = io['workspace'][o:o + 4 * (T + 1) * E * n * 16].view(torch.float32).cpu().numpy().reshape(T + 1, E, n, 16)
    slots = (head + np.arange(K)) % cap
    got = {k: v.cpu().numpy() for k, v in storage.items()}
    actions = got['action'][slots].reshape(T, E, n)
    adj = _adjacency(st['dest'])
    states = []
    for t in range(T):
        state, xe, adj_t = _host_observation(B, st['dest'])
        assert np.array_equal(adj_t, adj)
        assert traj_xe[t].tobytes() == xe.tobytes(), ('entry', t)
        states.append(state)
        B.rates(actions[t])
        r = B.fetch_rates()
        reward = w_v2v * r['v2v_rate'].reshape(E, n, 1).sum(axis=(1, 2)) + w_v2i * r['v2i_rate'].sum(axis=1)
        assert got['reward'][slots[t * E:(t + 1) * E]].tobytes() == reward.tobytes() == res.reward[t].tobytes(), ('reward', t)
        B.stream(mobility=True)
        B.step(B.tensor('u'))
    _, xe, _ = _host_observation(B, st['dest'])
    assert traj_xe[T].tobytes() == xe.tobytes()
    B.observe_recv()
    names = WALKED + ('interf_db', 'state', 'xe', 'recv', 'flags', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf',
                      'actions')
    a, b = _bytes(A, *names), _bytes(B, *names)
    for k in names:
        assert a[k] == b[k], k
    # what was stored: the observations of entries t and t + 1, the receivers, the actions
    assert got['xe'][slots].tobytes() == traj_xe[:T].tobytes() and got['xe_next'][slots].tobytes() == traj_xe[1:].tobytes()
    assert np.array_equal(got['recv'][slots], np.tile(st['dest'], (T, 1)))
    own = (st['dest'] == np.arange(n)).sum(axis=1)
    assert np.array_equal(res.flags, np.broadcast_to((own > 0).astype(np.uint8), (T, 2, E)))
    # the picks: the uploaded draws where a state explores, elsewhere the first maximiser of the engine's Q-values
    all_states = np.concatenate(states)                                  # [T E, n, 13], t major
    q = eng.forward(PackedBatch.from_dense(all_states[:, :, :9].astype(np.float32), all_states[:, :, 9:].astype(np.float32),
                                           np.tile(adj, (T, 1, 1)))).reshape(T, E, n, RB)
    want = np.where(explore[:, :, None] != 0, rand, np.argmax(q, axis=3))
    assert np.array_equal(actions, want)
    assert (explore == 0).any(axis=1).all() and (n != 33 or own.tolist() == [0, 2])
    # nothing outside the block was written
    rest = np.setdiff1d(np.arange(cap), slots)
    for k, v in got.items():
        assert (v[rest] == MARK).all(), k
    eng.close()


# ------------------------------------------------------------------------------ 6. refusals before the first launch
def test_a_refused_call_leaves_state_and_storage_alone():
    import torch
    E, n, T, cap = 2, 36, 2, 8
    lib = load_library()
    st = start_state(E, n, 77, [600, 610])
    dc = start_channels_recv(E, n, st)
    storage = _recv_storage(cap, n)
    names = WALKED + ('xe', 'recv', 'flags', 'state', 'interf_db', 'actions', 'v2v_rate')

    def snapshot():
        torch.cuda.synchronize()
        snap = _bytes(dc, *names)
        snap.update({'rep_' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
        return snap

    before = snapshot()
    io = dc.rollout_steps_recv_buffers(T)
    ws = io['workspace']

    def call(change, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel()):
        r = dc.rollout_steps_recv_struct(T, storage, 0, cap, 1.0, 0.1)
        change(r)
        rc = lib.v2x_rollout_steps_recv(ctypes.byref(r), ws_ptr, ws_bytes, dc._stream())
        return rc, lib.v2x_last_error(None).decode()

    def links(v):
        def change(r):
            r.step.problem.n = v
        return change

    cases = [(links(129), {}, "n = 129"), (links(2), {}, "n = 2"), (lambda r: setattr(r, 'T', 0), {}, "T = 0"),
             (lambda r: setattr(r, 'capacity', T * E - 1), {}, "T E <= capacity"), (lambda r: None, dict(ws_bytes=ws.numel() - 256), "needs"),
             (lambda r: setattr(r, 'rep_recv', None), {}, "rep_recv")]
    for change, kw, word in cases:
        rc, text = call(change, **kw)
        assert rc == V2X_EINVAL and word in text, (word, rc, text)
        assert snapshot() == before, word
    # ... and the Python layer refuses a state whose receivers it has seen to be out of range
    bad = st['dest'].copy()
    bad[0, 3] = n
    dc.observe_recv(bad)
    with pytest.raises(ValueError, match="receiver outside"):
        dc.rollout_steps_recv(np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int32), storage, 0, cap, 1.0, 0.1)


# ------------------------------------------------------------------------------ 7. the agent
def _agent(n, E, seed, replay, backend='trajectory'):
    import random
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, E, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 16, 1, 0.1)
    agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay=replay, rollout_backend=backend,
                  trajectory_walk='wide')
    assert type(env) is DeviceBatchedEnviron
    return env, agent


def test_agent_on_the_receiver_memory_is_the_agent_on_the_existing_memory_at_20_links():
    runs = {}
    for replay in (True, 'receivers'):
        env, agent = _agent(20, 2, 91, replay)
        out = agent.train(1, 2)
        runs[replay] = (out[0].tobytes(), out[1].tobytes(), out[2].tobytes(), agent.brain.model.engine.get_flat().tobytes(),
                        agent.num_step, len(agent.memory.samples), env.device_channels.walk_calls['wide'])
        assert np.isfinite(out[0]).all()
        agent.brain.close()
    assert type(agent.device_replay) is ReceiverReplay
    for i, what in enumerate(('losses', 'rewards per step', 'rewards per episode', 'weights', 'num_step', 'fifo', 'wide calls')):
        assert runs[True][i] == runs['receivers'][i], what
    assert runs[True][4] == 100 and runs[True][6] == 2


@pytest.mark.parametrize("E", [1, 3])
def test_agent_at_40_links_rolls_out_in_one_resident_call_per_train_step(E):
    env, agent = _agent(40, E, 17 + E, 'receivers')
    host_calls = []
    for obj, name in ((agent, '_packed_iteration'), (agent, '_predict'), (env, 'act'), (env, 'observe')):
        inner = getattr(obj, name)
        setattr(obj, name, (lambda inner, name: lambda *a, **k: (host_calls.append(name), inner(*a, **k))[1])(inner, name))
    resident = []
    inner_call = env.rollout_steps_recv
    env.rollout_steps_recv = lambda ex, *a, **k: (resident.append(np.shape(ex)), inner_call(ex, *a, **k))[1]
    loss, reward_step = agent.train(1, 2)[:2]
    per_step = -(-50 // E) * E
    rep = agent.device_replay
    assert host_calls == [] and resident == [(per_step // E, E)] * 2
    assert (rep.size, rep.head, agent.num_step) == (2 * per_step, 2 * per_step, 2 * per_step)
    assert len(agent.memory.samples) == 2 * per_step and all(s is None for s in agent.memory.samples)
    assert np.isfinite(loss).all() and np.isfinite(reward_step).all() and len(set(reward_step.reshape(-1).tolist())) > per_step
    assert not rep._own[:rep.size].any() and np.array_equal(rep.recv[:E].cpu().numpy(), env.dest)
    agent.brain.close()


def test_agent_refuses_the_one_iteration_rollout_on_the_receiver_memory():
    env = start_env_batched(40, 2, 5, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 16, 1, 0.1)
    with pytest.raises(ValueError, match="'trajectory'"):
        Agent(40, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=5, device_replay='receivers', rollout_backend='device')
