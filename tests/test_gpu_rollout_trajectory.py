"""GPU: all T iterations of a DQN rollout in one call (v2x_rollout_steps: k_sim_trajectory, one forward, k_rollout_finish of
csrc/v2xsimdev.hip; DeviceChannels.rollout_steps; Agent(rollout_backend='trajectory')).  The reference everywhere is the
per-iteration path on an identically initialised second state -- T calls of v2x_rollout_step, or
Agent(rollout_backend='device') -- and everything is compared byte for byte: the same device functions run the same
expressions in the same order, so no tolerance applies anywhere.  Positions, directions and the MT19937 streams are also
compared with the host library (exact integer / exactly rounded arithmetic).

The engine scores 4 channels only, so the cases with rb = 1 and rb = 5 run without a model (model = NULL, everybody explores),
on both paths; the others mix exploring and greedy states per (t, e), with one all-greedy iteration when T >= 2."""
import ctypes
import random

import numpy as np
import pytest

from v2xgnn import GnnEngine, GnnSpec
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config, native_sim
from v2xgnn.rl.device_sim import uniforms_per_step
from v2xgnn.rl.replay import DeviceReplay
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

# the project's lane grid (rl/train.py start_env_batched), tables in the order of native_sim.positions: up, down, left, right
UP = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
DOWN = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
LEFT = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
RIGHT = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
LANES = (UP, DOWN, LEFT, RIGHT)
WIDTH, HEIGHT = 750.0, 1299.0

# every resident tensor a step writes (and the uniforms of the last step)
STATE = ('keys', 'mtpos', 'pos', 'dirs', 'u', 'v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff', 'interf_db', 'state',
         'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf', 'actions')
MARK = 7


def _dev():
    import torch
    return torch.device('cuda', 0)


def _storage(capacity, n):
    """replay storage tensors of `capacity` slots, every element the marker"""
    import torch
    mk = lambda shape, dt: torch.full((capacity,) + shape, MARK, dtype=dt, device=_dev())   # noqa: E731
    return {'xe': mk((n, 16), torch.float32), 'xe_next': mk((n, 16), torch.float32), 'col': mk((n * (n - 2),), torch.int32),
            'mask': mk((n,), torch.int32), 'action': mk((n,), torch.int32), 'reward': mk((), torch.float64)}


def _engine(n, seed=5):
    eng = GnnEngine(GnnSpec(n_nodes=n, feat_dim=16, n_mp_layers=2))
    eng.set_flat(np.random.default_rng(seed).normal(0, 0.3, size=eng.n_params).astype(np.float32))
    return eng


def _row_ptr(graphs, n):
    import torch
    return torch.arange(graphs * n + 1, dtype=torch.int32, device=_dev()) * (n - 2)


def start_state(E, n, seed, mtpos=None):
    """keys of seeded generators, vehicles spread over the map with most of them within a few steps of a crossing lane (so the
    walks draw) and every fifth about to leave the map, receivers that are never the link itself, shadowing states"""
    rng = np.random.default_rng(seed)
    keys = np.ascontiguousarray(np.stack([np.random.RandomState(seed + 11 * e).get_state()[1] for e in range(E)]).astype(np.uint32))
    xy, dirs = np.zeros((E, n, 2)), np.zeros((E, n), np.int8)
    vel = rng.integers(10, 16, size=(E, n)).astype(np.float64)
    for e in range(E):
        for v in range(n):
            d = int(rng.integers(0, 4))
            sg, ax, dv = (1.0 if d in (0, 3) else -1.0), (1 if d < 2 else 0), vel[e, v] * 0.01
            if v % 5 == 4:
                a = ((WIDTH, HEIGHT)[ax] - 1.5 * dv) if sg > 0 else 1.5 * dv
            else:
                tabs = (LEFT + RIGHT) if ax == 1 else (UP + DOWN)
                a = tabs[int(rng.integers(0, len(tabs)))] - sg * float(rng.random()) * 4.0 * dv
            xy[e, v, ax], xy[e, v, 1 - ax], dirs[e, v] = a, float(rng.random()) * (WIDTH, HEIGHT)[1 - ax], d
    dest = ((np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n).astype(np.int64)
    assert np.all(dest != np.arange(n))
    pos = np.array([600 + 5 * e for e in range(E)], np.int32) if mtpos is None else np.asarray(mtpos, np.int32)
    return dict(keys=keys, mtpos=pos, pos=xy, dirs=dirs, vel=vel, dest=dest, v2i_shadow=rng.normal(0.0, 8.0, (E, n)),
                v2v_shadow=rng.normal(0.0, 3.0, (E, n, n)))


def start_channels(E, n, rb, st):
    """a DeviceChannels holding the state `st` after one channel update and its observation; the streams then stand at
    st['mtpos'] again (the positions a case wants the rollout to START from)"""
    dc = DeviceChannels(E, n, rb)
    dc.set_grid(LANES, WIDTH, HEIGHT, 0.01)
    for name, a in st.items():
        dc.upload(name, a)
    dc.stream(mobility=False)
    dc.step(dc.tensor('u'))
    dc.observe()
    dc.upload('mtpos', st['mtpos'])
    return dc


def _policy(E, n, rb, T, rng, greedy_possible):
    explore = (rng.random((T, E)) < 0.5).astype(np.uint8)
    if T >= 2:
        explore[1] = 0                                                   # one iteration where everybody is greedy
    explore[0, 0] = 1
    if T * E > 1:
        explore[-1, -1] = 0
    if not greedy_possible:
        explore[:] = 1
    return explore, rng.integers(0, rb, size=(T, E, n)).astype(np.int32)


def _snapshot(dc, st):
    import torch
    torch.cuda.synchronize()
    snap = {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}
    snap.update({'rep_' + k: v.cpu().numpy().tobytes() for k, v in st.items()})
    return snap


def _heads(E, T, capacity):
    """the block inside the ring; wrapping between two iterations (T >= 2); wrapping inside one iteration's E slots (E >= 2)"""
    return (0, capacity - E * max(1, T // 2), capacity - E * (T // 2) - 1)


CASES = [(1, 3, 1, 1), (1, 3, 1, 4), (3, 4, 4, 3), (2, 15, 4, 3), (2, 16, 4, 3), (5, 20, 4, 10), (1, 20, 4, 50), (2, 31, 5, 2)]


@pytest.mark.parametrize("E,n,rb,T", CASES)
def test_one_call_leaves_what_T_single_iterations_leave(E, n, rb, T):
    K = T * E
    capacity = K + 3
    eng = _engine(n) if rb == 4 else None                                # (the engine scores 4 channels: see the module's docstring)
    rp_one, rp_all = _row_ptr(E, n), _row_ptr(K, n)
    rng = np.random.default_rng(100 * n + 10 * E + T)
    heads = _heads(E, T, capacity)
    if T >= 2:
        assert heads[1] + K > capacity and (capacity - heads[1]) % E == 0          # wraps, at an iteration's boundary
    if E >= 2:
        assert heads[2] + K > capacity and (capacity - heads[2]) % E != 0          # wraps inside an iteration's slots
    runs = [(v, head, True) for v, head in enumerate(heads)] + ([(0, 1, False)] if eng is not None else [])
    for variant, head, use_model in runs:
        # stream positions 0, 623 (the first double straddles two blocks) and 624 (the block is used up at entry), rotating
        # over the states from run to run
        mtpos = [(0, 623, 624)[(e + variant) % 3] for e in range(E)]
        st = start_state(E, n, 300 + n + variant, mtpos)
        explore, rand = _policy(E, n, rb, T, rng, eng is not None and use_model)
        model = eng if use_model else None
        tag = (variant, head, use_model)

        ref, st_ref = start_channels(E, n, rb, st), _storage(capacity, n)
        rows = [ref.rollout_step(explore[t], rand[t], st_ref, (head + t * E) % capacity, capacity, 1.0, 0.1, engine=model, row_ptr=rp_one)
                for t in range(T)]
        want = _snapshot(ref, st_ref)
        want_reward = np.stack([r.resolve().reward for r in rows])
        want_regular = np.stack([r.resolve().regular for r in rows])

        dc, st_got = start_channels(E, n, rb, st), _storage(capacity, n)
        block = dc.rollout_steps(explore, rand, st_got, head, capacity, 1.0, 0.1, engine=model, row_ptr=rp_all if model else None)
        got = _snapshot(dc, st_got)
        for name in want:
            assert got[name] == want[name], (tag, name)
        block.resolve()
        assert block.reward.shape == (T, E) and block.reward.tobytes() == want_reward.tobytes(), tag
        assert block.regular.shape == (T, 2, E) and block.regular.tobytes() == want_regular.tobytes() and block.regular.all(), tag
        assert np.all(np.isfinite(want_reward)), tag

        # the written slots are the block's, every other slot still holds the marker
        slots = (head + np.arange(K)) % capacity
        rest = np.setdiff1d(np.arange(capacity), slots)
        assert len(rest) == 3
        for name, t in st_got.items():
            assert np.all(t.cpu().numpy()[rest] == MARK), (tag, name)
        assert not np.any(st_got['reward'].cpu().numpy()[slots] == MARK), tag
        acts = st_got['action'].cpu().numpy()[slots].reshape(T, E, n)
        assert np.array_equal(acts[explore != 0], rand[explore != 0]), tag
        assert np.array_equal(np.frombuffer(got['actions'], np.int32).reshape(E, n), acts[-1]), tag
        if model is not None and T >= 2:                                 # the all-greedy iteration took the network's actions
            assert not np.array_equal(acts[1], rand[1]), tag
        assert dc.traffic['bytes_down'] == dc.rollout_steps_result_bytes(T) == -(-10 * K // 8) * 8, tag   # one block came down
    if eng is not None:
        eng.close()


@pytest.mark.parametrize("E,n,rb,T", [(3, 4, 4, 3), (1, 20, 4, 50)])
def test_positions_directions_and_streams_are_the_host_librarys_after_T_steps(E, n, rb, T):
    st = start_state(E, n, 900 + n)
    n_u = uniforms_per_step(n, rb)
    h = {k: np.ascontiguousarray(st[k]).copy() for k in ('keys', 'mtpos', 'pos', 'dirs')}
    native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)                   # start_channels' channel update (no walk) ...
    h['mtpos'][:] = st['mtpos']                                          # ... after which the positions are set back
    before = h['pos'].copy()
    for _ in range(T):
        native_sim.positions(h['keys'], h['mtpos'], h['pos'], h['dirs'], st['vel'], 0.01, LANES, WIDTH, HEIGHT)
        native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)
    assert np.all(np.any(h['pos'] != before, axis=2))                    # every vehicle moved
    dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
    rng = np.random.default_rng(5)
    explore, rand = _policy(E, n, rb, T, rng, False)
    dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1).resolve()
    for name in ('keys', 'mtpos', 'pos', 'dirs'):
        got = dc.download(name)
        assert got.shape == h[name].shape and got.tobytes() == np.ascontiguousarray(h[name]).tobytes(), name


def test_a_refused_call_leaves_the_state_and_the_storage_alone():
    import torch
    lib = load_library()
    E, n, rb, T = 3, 4, 4, 3
    st = start_state(E, n, 77)
    dc, storage = start_channels(E, n, rb, st), _storage(T * E + 2, n)
    eng = _engine(n)
    before = _snapshot(dc, storage)
    r = dc.rollout_steps_struct(T, storage, 0, T * E + 2, 1.0, 0.1, engine=eng, row_ptr=_row_ptr(T * E, n))
    r.r.capacity = T * E - 1                                             # T E > capacity
    assert lib.v2x_rollout_steps(ctypes.byref(r), torch.cuda.current_stream().cuda_stream) == V2X_EINVAL
    assert "T E <= capacity" in lib.v2x_last_error(None).decode()
    r.r.capacity = T * E + 2
    r.r.batch.n_graphs = E                                               # the batch of a single iteration: not this block's
    assert lib.v2x_rollout_steps(ctypes.byref(r), torch.cuda.current_stream().cuda_stream) == V2X_EINVAL
    assert "graphs" in lib.v2x_last_error(None).decode()
    after = _snapshot(dc, storage)
    for name in before:
        assert after[name] == before[name], name
    with pytest.raises(ValueError, match="capacity"):
        dc.rollout_steps(np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int32), storage, 0, T * E - 1, 1.0, 0.1)
    assert _snapshot(dc, storage) == before
    eng.close()


@pytest.mark.parametrize("use_model", [False, True])
def test_blocks_and_single_iterations_mixed_on_one_state_leave_what_five_single_iterations_leave(use_model):
    """rollout_steps (T = 2), rollout_step, rollout_steps (T = 2) on ONE DeviceChannels -- the two entry points share their host
    path, and their buffers must neither alias nor be made twice -- against five rollout_step calls on a twin: E = 3, n = 4,
    rb = 4, the smallest shape with more than one state, an odd E and a ring that wraps inside the single iteration."""
    E, n, rb, T = 3, 4, 4, 2
    capacity, head = 5 * E + 3, 3 * E + 2                                # slots 11..16 | 17, 0, 1 | 2..7
    eng = _engine(n) if use_model else None
    rp_one, rp_all = _row_ptr(E, n), _row_ptr(T * E, n)
    explore, rand = _policy(E, n, rb, 5, np.random.default_rng(41), use_model)
    if use_model:
        explore[2] = (0, 1, 0)                                           # the single iteration scores somebody too
        assert not explore[:2].all() and not explore[3:].all()
    st = start_state(E, n, 512, [0, 623, 624])
    at = lambda t: (head + t * E) % capacity                             # noqa: E731

    ref, st_ref = start_channels(E, n, rb, st), _storage(capacity, n)
    rows = [ref.rollout_step(explore[t], rand[t], st_ref, at(t), capacity, 1.0, 0.1, engine=eng, row_ptr=rp_one) for t in range(5)]
    want = _snapshot(ref, st_ref)
    want_reward = np.stack([r.resolve().reward for r in rows])
    want_regular = np.stack([r.resolve().regular for r in rows])

    dc, st_got = start_channels(E, n, rb, st), _storage(capacity, n)
    before = dict(dc.traffic)
    first = dc.rollout_steps(explore[:2], rand[:2], st_got, at(0), capacity, 1.0, 0.1, engine=eng, row_ptr=rp_all if eng else None)
    ptrs = {k: dc.rollout_steps_buffers(T)[k].data_ptr() for k in ('policy_dev', 'result_dev', 'workspace', 'q')}
    one = dc.rollout_step(explore[2], rand[2], st_got, at(2), capacity, 1.0, 0.1, engine=eng, row_ptr=rp_one)
    last = dc.rollout_steps(explore[3:], rand[3:], st_got, at(3), capacity, 1.0, 0.1, engine=eng, row_ptr=rp_all if eng else None)
    got = _snapshot(dc, st_got)
    for name in want:
        assert got[name] == want[name], name
    got_reward = np.concatenate([first.resolve().reward, one.resolve().reward[None], last.resolve().reward])
    got_regular = np.concatenate([first.regular, one.regular[None], last.regular])
    assert first.reward.shape == last.reward.shape == (T, E) and one.reward.shape == (E,) and one.regular.shape == (2, E)
    assert got_reward.tobytes() == want_reward.tobytes() and got_regular.tobytes() == want_regular.tobytes()
    assert np.all(np.isfinite(want_reward)) and len(set(want_reward.reshape(-1).tolist())) == 5 * E
    for res, t0 in ((first, 0), (one, 2), (last, 3)):
        k = res.stored_regular.size // E
        assert np.array_equal(res.stored_regular, want_regular[t0:t0 + k, 0].reshape(-1))
        assert np.array_equal(res.resident_regular, want_regular[t0 + k - 1, 1])
    # the second block reused the first one's buffers, and the single iteration has its own
    again, single = dc.rollout_steps_buffers(T), dc.rollout_buffers()
    assert {k: again[k].data_ptr() for k in ptrs} == ptrs
    assert not set(ptrs.values()) & {single[k].data_ptr() for k in ('policy_dev', 'result_dev', 'q')}
    assert {k: dc.traffic[k] - before[k] for k in before} == {
        'bytes_up': 2 * dc.rollout_steps_policy_bytes(T) + dc.rollout_policy_bytes,
        'bytes_down': 2 * dc.rollout_steps_result_bytes(T) + dc.rollout_result_bytes}
    rest = np.setdiff1d(np.arange(capacity), (head + np.arange(5 * E)) % capacity)
    assert len(rest) == 3 and all(np.all(t.cpu().numpy()[rest] == MARK) for t in st_got.values())
    if eng is not None:
        acts = st_got['action'].cpu().numpy()[(head + np.arange(5 * E)) % capacity].reshape(5, E, n)
        assert np.array_equal(acts[explore != 0], rand[explore != 0]) and not np.array_equal(acts[1], rand[1])
        eng.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _agent(E, seed, backend, n=4, capacity=None, irregular=None):
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, E, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay=True, rollout_backend=backend)
    assert type(env) is DeviceBatchedEnviron and agent.rollout_backend == backend
    if capacity is not None:                                             # a ring small enough to wrap during the run
        agent.device_replay = DeviceReplay(capacity, n, device=agent.brain.model.engine.device)
        agent.memory.capacity = capacity
    if irregular is not None:                                            # a link that is its own receiver: new receivers go up, the
        e, k = irregular                                                 # cached observation is of the old ones
        env.dest[e, k] = k
        env._static_dirty = True
        env._dev_obs = None
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


def _trained(E, backend, capacity=None):
    env, agent = _agent(E, 33, backend, capacity=capacity)
    calls = []
    if backend == 'trajectory':                                          # count the whole-rollout calls the run makes
        inner = env.rollout_steps
        env.rollout_steps = lambda *a, **k: (calls.append(np.asarray(a[0]).shape), inner(*a, **k))[1]
    out = agent.train(1, 3)
    run = dict(out=out, mem=_memory(agent), online=agent.brain.model.engine.get_flat(), target=agent.brain.target_model.engine.get_flat(),
               rng=np.random.get_state(), num_step=agent.num_step, epsilon=agent.epsilon,
               streams=[np.array(a).copy() for a in (env.pos, env.dirs, env._mt_keys, env._mt_pos)], calls=calls)
    agent.brain.close()
    return run


def _assert_same_run(d, t, tag):
    for i in range(5):                                                   # losses, reward_step, reward_episode, Q mean, Q max
        assert np.asarray(t['out'][i]).tobytes() == np.asarray(d['out'][i]).tobytes(), (tag, i)
        assert np.all(np.isfinite(np.asarray(d['out'][i]))), (tag, i)
    for k in d['mem']:
        assert t['mem'][k] == d['mem'][k], (tag, k)
    assert t['online'].tobytes() == d['online'].tobytes() and t['target'].tobytes() == d['target'].tobytes(), tag
    assert _same_rng(t['rng'], d['rng']) and t['num_step'] == d['num_step'] and t['epsilon'] == d['epsilon'], tag
    for g, w in zip(t['streams'], d['streams']):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), tag


@pytest.mark.parametrize("E", [1, 5])
def test_agent_with_the_trajectory_rollout_is_the_device_rollout_bit_for_bit(E):
    d, t = _trained(E, 'device'), _trained(E, 'trajectory')
    _assert_same_run(d, t, E)
    assert d['num_step'] == 150 and d['mem']['size'] == 150 and d['epsilon'] == 0.01
    assert t['calls'] == [(50 // E, E)] * 3                              # one call per train step, every iteration in it
    assert len(set(np.asarray(d['out'][1]).reshape(-1).tolist())) > 100  # (rewards that differ from transition to transition)


def test_agent_trajectory_rollout_with_a_replay_ring_that_wraps_during_the_run():
    d, t = _trained(5, 'device', capacity=120), _trained(5, 'trajectory', capacity=120)
    _assert_same_run(d, t, 'ring')
    assert d['mem']['size'] == 120 and d['mem']['head'] == 30 and d['mem']['fifo'] == 120 and len(t['calls']) == 3


def test_an_irregular_state_with_somebody_greedy_takes_the_per_iteration_path_and_still_equals_device():
    E = 3
    runs = {}
    for backend in ('device', 'trajectory'):
        env, agent = _agent(E, 58, backend, irregular=(1, 2))
        agent.num_Train_Step, agent.num_step = 20, 160                   # epsilon about 0.8: some iterations score somebody
        calls = []
        if backend == 'trajectory':
            inner = env.rollout_steps
            env.rollout_steps = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
        rewards = agent.generate_d2d_transition(6 * E).copy()
        runs[backend] = (rewards, _memory(agent), np.random.get_state(), agent.num_step, agent.epsilon)
        assert not calls                                                 # the whole-rollout call was not made
        agent.brain.close()
    (r_d, m_d, s_d, n_d, e_d), (r_t, m_t, s_t, n_t, e_t) = runs['device'], runs['trajectory']
    assert r_t.tobytes() == r_d.tobytes() and _same_rng(s_t, s_d) and n_t == n_d == 160 + 6 * E and e_t == e_d
    for k in m_d:
        assert m_t[k] == m_d[k], k
    flags = np.frombuffer(m_d['regular'], bool).reshape(6, E)
    assert not flags[:, 1].any() and flags[:, [0, 2]].all()              # the slots of state 1 are not regular, the others are


def test_a_direct_rollout_of_fifty_transitions_on_one_simulator_returns_the_device_rollouts_rewards():
    runs = {}
    for backend in ('device', 'trajectory'):
        env, agent = _agent(1, 21, backend)
        agent.num_Train_Step, agent.num_step = 20, 400                   # epsilon about 0.5: both branches occur
        dc = env.device_channels
        first = agent.generate_d2d_transition(50).copy()                 # (after a reset the flags may come down with the observation)
        before = dict(dc.traffic)
        rewards = agent.generate_d2d_transition(50).copy()
        traffic = {k: dc.traffic[k] - before[k] for k in before}
        runs[backend] = (first, rewards, _memory(agent), np.random.get_state(), traffic, dc)
        agent.brain.close()
    d, t = runs['device'], runs['trajectory']
    assert t[0].shape == (50,) and t[0].tobytes() == d[0].tobytes() and t[1].tobytes() == d[1].tobytes()
    assert np.all(np.isfinite(d[1])) and len(set(d[1].tolist())) == 50
    for k in d[2]:
        assert t[2][k] == d[2][k], k
    assert _same_rng(t[3], d[3])
    # one upload of the policy block and one download of the result block, against fifty of each
    dc = t[5]
    assert t[4] == {'bytes_up': dc.rollout_steps_policy_bytes(50), 'bytes_down': dc.rollout_steps_result_bytes(50)}
    assert d[4] == {'bytes_up': 50 * dc.rollout_policy_bytes, 'bytes_down': 50 * dc.rollout_result_bytes}
