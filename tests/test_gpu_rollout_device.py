"""GPU: the device-resident DQN rollout iteration (v2x_rollout_pick / v2x_rollout_store / v2x_rollout_step of csrc/v2xsimdev.hip,
DeviceChannels.rollout_step, Agent(rollout_backend='device')).  The reference everywhere is the existing path --
Agent._packed_iteration on DeviceBatchedEnviron(streams='device'), the calls the iteration chains issued one by one -- or
numpy; everything is compared byte for byte (the kernels copy, compare and add in numpy's order: no tolerance applies)."""
import ctypes
import random

import numpy as np
import pytest

from v2xgnn import GnnEngine, GnnSpec
from v2xgnn.lib import load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device('cuda', 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _storage(capacity, n, fill):
    """replay storage tensors of `capacity` slots, every element `fill`"""
    import torch
    mk = lambda shape, dt: torch.full((capacity,) + shape, fill, dtype=dt, device=_dev())   # noqa: E731
    return {'xe': mk((n, 16), torch.float32), 'xe_next': mk((n, 16), torch.float32), 'col': mk((n * (n - 2),), torch.int32),
            'mask': mk((n,), torch.int32), 'action': mk((n,), torch.int32), 'reward': mk((), torch.float64)}


# ------------------------------------------------------------------------------------------------------- 1. pick alone
def crafted_q(E, n, C, rng):
    """Q rows that exercise np.argmax's rule: the maximum tied at every subset of positions, -inf rows, NaN at every position
    (with a larger number before and after it), +inf, ordinary rows"""
    q = rng.normal(size=(E * n, C)).astype(np.float32)
    for r in range(E * n):
        kind = r % 6
        if kind == 0:                                                    # ties: the maximum at the positions of a bit pattern
            bits = (r // 6) % (1 << C) or (1 << C) - 1
            q[r] = np.where([(bits >> c) & 1 for c in range(C)], np.float32(1.5), np.float32(-0.25))
        elif kind == 1:
            q[r] = -np.inf
        elif kind == 2:                                                  # the first NaN wins over any number, +inf included
            q[r, (r // 6) % C] = np.nan
            q[r, (r // 6 + 1) % C] = np.inf
            if C > 2:
                q[r, (r // 6 + 2) % C] = np.nan
        elif kind == 3:
            q[r] = np.nan
        elif kind == 4:
            q[r, (r // 6) % C] = np.inf
            q[r, C - 1 - (r // 6) % C] = np.inf
    return q


@pytest.mark.parametrize("E,n,C", [(1, 3, 1), (3, 4, 4), (2, 8, 4), (70, 20, 4), (2, 31, 5)])
def test_pick_is_np_argmax_or_the_random_action_and_copies_the_observation_to_its_slots(E, n, C):
    import torch
    lib = load_library()
    rng = np.random.default_rng(1000 + 31 * E + n)
    q = crafted_q(E, n, C, rng)
    explore = (np.arange(E) % 3 == 1).astype(np.uint8)                  # a mix (E = 1: greedy)
    rand = rng.integers(0, C, size=(E, n)).astype(np.int32)
    xe = rng.normal(size=(E, n, 16)).astype(np.float32)
    xe[0, 0, :3] = [np.nan, -0.0, np.inf]                               # copied as bytes, whatever they are
    col = rng.integers(0, n, size=(E, n * (n - 2))).astype(np.int32)
    mask = rng.integers(0, 1 << n, size=(E, n)).astype(np.int32)
    regular = (np.arange(E) % 4 != 2).astype(np.uint8)
    capacity = E + 3
    want_a = np.where(explore[:, None] != 0, rand, np.argmax(q.reshape(E, n, C), axis=2).astype(np.int32))
    for head, use_q in ((0, True), (capacity - 1, True), (capacity - 2, False)):         # the last two wrap (E >= 2 / E >= 3)
        st = _storage(capacity, n, 7)
        actions = torch.full((E, n), -5, dtype=torch.int32, device=_dev())
        reg_out = torch.full((E,), 9, dtype=torch.uint8, device=_dev())
        d = [_t(a) for a in (q, explore, rand, xe, col, mask, regular)]
        rc = lib.v2x_rollout_pick(E, n, C, d[0].data_ptr() if use_q else None, d[1].data_ptr(), d[2].data_ptr(), actions.data_ptr(),
                                  d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), st['xe'].data_ptr(),
                                  st['col'].data_ptr(), st['mask'].data_ptr(), head, capacity, reg_out.data_ptr(), _stream())
        assert rc == 0, lib.v2x_last_error(None)
        torch.cuda.synchronize()
        tag = (head, use_q)
        assert actions.cpu().numpy().tobytes() == (want_a if use_q else rand).tobytes(), tag
        assert reg_out.cpu().numpy().tobytes() == regular.tobytes(), tag
        slots = (head + np.arange(E)) % capacity
        rest = np.setdiff1d(np.arange(capacity), slots)
        for name, src in (('xe', xe), ('col', col), ('mask', mask)):
            got = st[name].cpu().numpy()
            assert got[slots].tobytes() == src.tobytes(), (tag, name)
            assert np.all(got[rest] == 7), (tag, name)                   # no other slot was touched
        for name in ('xe_next', 'action', 'reward'):
            assert bool((st[name] == 7).all()), (tag, name)


# ------------------------------------------------------------------------------------------------------- 2. store alone
def _rates(E, n, m, rng):
    """rates of very different sizes (a sum's rounding depends on the order), a few exact zeros"""
    v2v = rng.random((E, n)) * rng.choice([1e-4, 1e-2, 1.0, 12.0], size=(E, n))
    v2i = rng.random((E, m)) * rng.choice([1e-3, 1.0, 9.0], size=(E, m))
    v2v[0, 0] = 0.0
    return v2v, v2i


@pytest.mark.parametrize("n", [3, 7, 8, 9, 15, 16, 20, 31])
def test_store_reward_is_the_numpy_expression_bit_for_bit(n):
    import torch
    lib = load_library()
    E, capacity = 5, 9
    rng = np.random.default_rng(50 + n)
    for rb in ((1, 5) if n >= 5 else (1, 3)):
        m = min(rb, n)
        v2v, v2i = _rates(E, n, m, rng)
        xe = rng.normal(size=(E, n, 16)).astype(np.float32)
        actions = rng.integers(0, rb, size=(E, n)).astype(np.int32)
        regular = (np.arange(E) % 2).astype(np.uint8)
        for w_v2v, w_v2i in ((1.0, 0.1), (0.0, 1.0), (1.0, 0.0)):
            want = w_v2v * v2v.reshape(E, n, 1).sum(axis=(1, 2)) + w_v2i * v2i.sum(axis=1)         # Agent._packed_iteration's line
            st = _storage(capacity, n, 7)
            r_out = torch.full((E,), -1.0, dtype=torch.float64, device=_dev())
            g_out = torch.full((E,), 9, dtype=torch.uint8, device=_dev())
            d = [_t(a) for a in (v2v, v2i, xe, actions, regular)]
            rc = lib.v2x_rollout_store(E, n, rb, d[0].data_ptr(), d[1].data_ptr(), w_v2v, w_v2i, d[2].data_ptr(), d[3].data_ptr(),
                                       d[4].data_ptr(), st['xe_next'].data_ptr(), st['action'].data_ptr(), st['reward'].data_ptr(),
                                       2, capacity, r_out.data_ptr(), g_out.data_ptr(), _stream())
            assert rc == 0, lib.v2x_last_error(None)
            torch.cuda.synchronize()
            tag = (n, rb, w_v2v, w_v2i)
            assert r_out.cpu().numpy().tobytes() == want.tobytes(), (tag, r_out.cpu().numpy() - want)
            assert st['reward'].cpu().numpy()[2:2 + E].tobytes() == want.tobytes(), tag
            assert g_out.cpu().numpy().tobytes() == regular.tobytes(), tag


def test_store_writes_next_observation_action_and_reward_to_slots_that_wrap():
    import torch
    lib = load_library()
    E, n, rb, capacity = 3, 4, 4, 7
    rng = np.random.default_rng(77)
    st = _storage(capacity, n, 7)
    want = {k: st[k].cpu().numpy() for k in st}
    head = 0
    for block in range(3):                                               # slots 0 1 2 | 3 4 5 | 6 0 1
        v2v, v2i = _rates(E, n, rb, rng)
        xe = rng.normal(size=(E, n, 16)).astype(np.float32)
        actions = rng.integers(0, rb, size=(E, n)).astype(np.int32)
        regular = np.ones(E, np.uint8)
        r_out = torch.zeros(E, dtype=torch.float64, device=_dev())
        g_out = torch.zeros(E, dtype=torch.uint8, device=_dev())
        d = [_t(a) for a in (v2v, v2i, xe, actions, regular)]
        rc = lib.v2x_rollout_store(E, n, rb, d[0].data_ptr(), d[1].data_ptr(), 1.0, 0.1, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                   st['xe_next'].data_ptr(), st['action'].data_ptr(), st['reward'].data_ptr(), head, capacity,
                                   r_out.data_ptr(), g_out.data_ptr(), _stream())
        assert rc == 0, lib.v2x_last_error(None)
        torch.cuda.synchronize()
        slots = (head + np.arange(E)) % capacity
        want['xe_next'][slots], want['action'][slots] = xe, actions
        want['reward'][slots] = 1.0 * v2v.reshape(E, n, 1).sum(axis=(1, 2)) + 0.1 * v2i.sum(axis=1)
        for k in st:                                                     # (xe / col / mask are the pick's: untouched)
            assert st[k].cpu().numpy().tobytes() == want[k].tobytes(), (block, k)
        head = (head + E) % capacity
    assert head == 2


# ------------------------------------------------------------------------------------------------------- 3. the call against its parts
STATE = ('keys', 'mtpos', 'pos', 'dirs', 'v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff', 'interf_db', 'state',
         'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf', 'actions')


def _engine(n, seed=5):
    eng = GnnEngine(GnnSpec(n_nodes=n, feat_dim=16, n_mp_layers=2))
    eng.set_flat(np.random.default_rng(seed).normal(0, 0.3, size=eng.n_params).astype(np.float32))
    return eng


def _resident(n, E, seed):
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, E, seed, backend="device", streams="device")
    env.observe_packed(4)                                                # the observation of the reset, on the device
    return env, env.device_channels


def _policies(E, n, rng, steps):
    out = []
    for k in range(steps):
        explore = (rng.random(E) < 0.5).astype(np.uint8)
        if k == 1:
            explore[:] = 0
        out.append((explore, rng.integers(0, 4, size=(E, n)).astype(np.int32)))
    return out


def _set_policy(dc, explore, rand):
    raw = np.zeros(dc.rollout_policy_bytes, np.uint8)
    raw[:rand.nbytes] = rand.reshape(-1).view(np.uint8)
    raw[rand.nbytes:rand.nbytes + explore.size] = explore
    dc.rollout_buffers()['policy_dev'].copy_(_t(raw))


def _snapshot(dc, st):
    import torch
    torch.cuda.synchronize()
    snap = {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}
    snap.update({'rep_' + k: v.cpu().numpy().tobytes() for k, v in st.items()})
    snap['result'] = dc.rollout_buffers()['result_dev'].cpu().numpy()[:10 * dc.E].tobytes()
    return snap


@pytest.mark.parametrize("n,E", [(4, 3), (20, 2)])
def test_rollout_step_is_forward_pick_advance_store_issued_separately_and_replays_from_a_graph(n, E):
    import torch
    lib = load_library()
    capacity, steps = 2 * E + 1, 4                                       # the third block wraps
    eng = _engine(n)
    pol = _policies(E, n, np.random.default_rng(9), steps)
    row_ptr = (torch.arange(E * n + 1, dtype=torch.int32, device=_dev()) * (n - 2))

    # the parts, one by one
    env_a, dc = _resident(n, E, 41)
    st_a = _storage(capacity, n, 7)
    io, T = dc.rollout_buffers(), dc.tensor
    parts, head = [], 0
    for explore, rand in pol:
        _set_policy(dc, explore, rand)
        base, res = io['policy_dev'].data_ptr(), io['result_dev'].data_ptr()
        eng.forward(dc.rollout_batch(row_ptr), out=io['q'])
        rc = lib.v2x_rollout_pick(E, n, 4, io['q'].data_ptr(), base + 4 * E * n, base, T('actions').data_ptr(), T('xe').data_ptr(),
                                  T('col').data_ptr(), T('mask').data_ptr(), T('regular').data_ptr(), st_a['xe'].data_ptr(),
                                  st_a['col'].data_ptr(), st_a['mask'].data_ptr(), head, capacity, res + 8 * E, _stream())
        assert rc == 0, lib.v2x_last_error(None)
        dc.advance(T('actions'))
        rc = lib.v2x_rollout_store(E, n, 4, T('v2v_rate').data_ptr(), T('v2i_rate').data_ptr(), 1.0, 0.1, T('xe').data_ptr(),
                                   T('actions').data_ptr(), T('regular').data_ptr(), st_a['xe_next'].data_ptr(),
                                   st_a['action'].data_ptr(), st_a['reward'].data_ptr(), head, capacity, res, res + 9 * E, _stream())
        assert rc == 0, lib.v2x_last_error(None)
        parts.append(_snapshot(dc, st_a))
        head = (head + E) % capacity
    greedy_rows = np.frombuffer(parts[1]['actions'], np.int32)
    assert not np.array_equal(greedy_rows, pol[1][1].reshape(-1))        # the all-greedy step took the network's actions

    # the one call
    env_b, dc = _resident(n, E, 41)
    st_b = _storage(capacity, n, 7)
    head = 0
    for k, (explore, rand) in enumerate(pol):
        row = dc.rollout_step(explore, rand, st_b, head, capacity, 1.0, 0.1, engine=eng, row_ptr=row_ptr)
        got = _snapshot(dc, st_b)
        for name in parts[k]:
            assert got[name] == parts[k][name], (k, name)
        row.resolve()
        assert row.reward.tobytes() == parts[k]['result'][:8 * E] and row.regular.all()
        head = (head + E) % capacity

    # once more, replayed from a captured graph on a side stream (the workspaces of the forward exist: eager calls came first)
    env_c, dc = _resident(n, E, 41)
    st_c = _storage(capacity, n, 7)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        head, graphs = 0, []
        for k in range(steps):                                           # (head is an argument: one captured call per block position)
            r = dc.rollout_struct(st_c, head, capacity, 1.0, 0.1, engine=eng, row_ptr=row_ptr)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):                       # capture runs nothing
                rc = lib.v2x_rollout_step(ctypes.byref(r), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.v2x_last_error(None)
            graphs.append((g, r))
            head = (head + E) % capacity
        for k, (explore, rand) in enumerate(pol):
            _set_policy(dc, explore, rand)
            graphs[k][0].replay()
            got = _snapshot(dc, st_c)
            for name in parts[k]:
                assert got[name] == parts[k][name], ("graph", k, name)
    eng.close()


# ------------------------------------------------------------------------------------------------------- 4. the agent
def _agent(n, E, seed, backend, irregular=None, num_step=400):
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, E, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 64, 1, 0.1)
    agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay=True, rollout_backend=backend)
    assert type(env) is DeviceBatchedEnviron and agent.rollout_backend == backend
    if irregular is not None:                                            # a link that is its own receiver: new receivers go up, the
        e, k = irregular                                                 # cached observation is of the old ones
        env.dest[e, k] = k
        env._static_dirty = True
        env._dev_obs = None
    agent.num_Train_Step, agent.num_step = 20, num_step                  # epsilon = 1 - 0.99 * num_step / 800: both branches occur
    return env, agent


def _memory(agent):
    import torch
    rep = agent.device_replay
    rep.flush()
    flags = rep.regular_flags()
    torch.cuda.synchronize()
    out = {k: getattr(rep, k)[:rep.size].cpu().numpy().tobytes() for k in ('xe', 'xe_next', 'col', 'mask', 'action', 'reward')}
    out.update(regular=flags[:rep.size].tobytes(), head=rep.head, size=rep.size, fifo=len(agent.memory.samples))
    return out


def _same_rng(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("n,E", [(4, 3), (20, 2)])
def test_agent_with_the_device_rollout_is_the_host_rollout_bit_for_bit(n, E):
    runs = {}
    for backend in ('host', 'device'):
        env, agent = _agent(n, E, 33, backend)
        dc = env.device_channels
        rewards = agent.generate_d2d_transition(5 * E).copy()           # five iterations, no replay
        eps = agent.epsilon
        mem, rng_state = _memory(agent), np.random.get_state()
        v2i_interf, v2v_interf = env.V2I_Interference.copy(), env.V2V_Interference.copy()       # (device: the first read downloads)
        stream_state = (env.pos.copy(), env._mt_keys.copy(), env._mt_pos.copy())
        out = agent.train(1, 2)
        runs[backend] = dict(rewards=rewards, eps=eps, mem=mem, rng=rng_state, interf=(v2i_interf, v2v_interf), streams=stream_state,
                             out=out, weights=agent.brain.model.engine.get_flat(), mem_after=_memory(agent), rng_after=np.random.get_state(),
                             steps=agent.num_step)
    h, d = runs['host'], runs['device']
    assert 0.3 < h['eps'] < 0.6 and h['eps'] == d['eps']
    assert d['rewards'].tobytes() == h['rewards'].tobytes() and np.all(np.isfinite(h['rewards'])) and h['rewards'].shape == (5 * E,)
    assert h['mem']['size'] == 5 * E
    for k in h['mem']:
        assert d['mem'][k] == h['mem'][k], k
    assert _same_rng(d['rng'], h['rng'])
    for g, w in zip(d['interf'] + d['streams'], h['interf'] + h['streams']):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()
    # Agent.train(1, 2): losses, rewards, Q statistics, final weights, memory, draws
    for i in (0, 1, 2, 3, 4):
        assert np.asarray(d['out'][i]).tobytes() == np.asarray(h['out'][i]).tobytes(), i
        assert np.all(np.isfinite(np.asarray(h['out'][i])))
    assert d['weights'].tobytes() == h['weights'].tobytes()
    for k in h['mem_after']:
        assert d['mem_after'][k] == h['mem_after'][k], k
    assert _same_rng(d['rng_after'], h['rng_after']) and d['steps'] == h['steps'] > 0


def test_an_irregular_state_goes_through_the_host_iteration_with_the_same_draws():
    n, E = 4, 3
    runs = {}
    for backend in ('host', 'device'):
        # epsilon 0.8: about half of the iterations explore everywhere (the device call stores the irregular state itself), the
        # others score somebody (the host iteration takes over)
        env, agent = _agent(n, E, 58, backend, irregular=(1, 2), num_step=160)
        rewards = agent.generate_d2d_transition(6 * E).copy()
        runs[backend] = (rewards, _memory(agent), np.random.get_state())
    (r_h, m_h, s_h), (r_d, m_d, s_d) = runs['host'], runs['device']
    assert r_d.tobytes() == r_h.tobytes() and _same_rng(s_d, s_h)
    for k in m_h:
        assert m_d[k] == m_h[k], k
    flags = np.frombuffer(m_d['regular'], bool).reshape(6, E)
    assert not flags[:, 1].any() and flags[:, [0, 2]].all()              # the slots of state 1 are not regular, the others are


def test_a_device_iteration_uploads_the_policy_buffer_and_downloads_one_result_row():
    n, E = 4, 3
    env, agent = _agent(n, E, 12, 'device')
    dc = env.device_channels
    agent.generate_d2d_transition(E)                                     # (after a reset the flags may come down with the observation)
    assert dc.rollout_policy_bytes == 4 * E * n + E + 1 and dc.rollout_result_bytes == 32
    for k in range(8):
        before, step0 = dict(dc.traffic), agent.num_step
        agent.generate_d2d_transition(E)
        assert agent.num_step == step0 + E
        assert dc.traffic['bytes_up'] - before['bytes_up'] == dc.rollout_policy_bytes, k
        assert dc.traffic['bytes_down'] - before['bytes_down'] == dc.rollout_result_bytes, k
    assert len(agent.memory.samples) == 9 * E == agent.device_replay.size
