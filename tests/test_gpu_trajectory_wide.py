"""GPU: the wide trajectory walk (v2x_rollout_steps_wide / v2x_eval_steps_wide: k_traj_stream, k_traj_terms, k_traj_scan,
k_traj_observe of csrc/v2xsimdev.hip; DeviceChannels.rollout_steps(walk='wide') / eval_steps(walk='wide');
Agent(trajectory_walk='wide')).  The reference is the per-iteration path on an identically initialised second state (T calls
of v2x_rollout_step) and the serial walk (k_sim_trajectory); everything is compared byte for byte: every expression of the
wide walk is a piece of the serial one's, cut where that one rounds to a double, so no tolerance applies anywhere.

The engine scores 4 channels only, so the cases with rb = 1 and rb = 5 run without a model (everybody explores)."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_eval_device import _agent as _eval_agent
from test_gpu_rollout_trajectory import (LANES, STATE, WIDTH, HEIGHT, _agent, _assert_same_run, _engine, _memory, _policy,
                                         _row_ptr, _same_rng, _snapshot, _storage, start_channels, start_state)
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import native_sim
from v2xgnn.rl.device_sim import uniforms_per_step, wide_workspace_layout

pytestmark = pytest.mark.gpu

# the minimum (no snapshot beyond 0); exactly one intermediate snapshot; strides over t and e; 240 and 272 elements, either side
# of a 256-thread block; the rollout shapes of 20 links; the limits
WIDE_CASES = [(1, 3, 1, 1), (1, 3, 1, 2), (3, 4, 4, 3), (2, 15, 4, 3), (2, 16, 4, 3), (5, 20, 4, 10), (1, 20, 4, 50), (2, 31, 5, 2)]
WORKSPACE = ('traj_xe', 'traj_col', 'traj_mask', 'traj_regular', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs')


def _trajectory(dc, E, n, rb, T):
    """the seven arrays of the trajectory workspace as bytes (without the padding between them)"""
    import torch
    torch.cuda.synchronize()
    io = dc.rollout_steps_buffers(T)
    ws, offs = io['workspace'].cpu().numpy(), io['offsets']
    size = dict(traj_xe=4 * (T + 1) * E * n * 16, traj_col=4 * (T + 1) * E * n * (n - 2), traj_mask=4 * (T + 1) * E * n,
                traj_regular=(T + 1) * E, traj_v2v_ff=8 * T * E * n * n * rb, traj_v2i_ff=8 * T * E * n * rb, traj_v2i_abs=8 * T * E * n)
    return {k: ws[offs[k]:offs[k] + size[k]].tobytes() for k in WORKSPACE}


@pytest.mark.parametrize("E,n,rb,T", WIDE_CASES)
def test_the_wide_walk_leaves_what_T_single_iterations_leave(E, n, rb, T):
    K = T * E
    capacity = K + 3
    eng = _engine(n) if rb == 4 else None
    rp_one, rp_all = _row_ptr(E, n), _row_ptr(K, n)
    rng = np.random.default_rng(100 * n + 10 * E + T)
    head = capacity - max(1, min(K - 1, E * (T // 2) + 1))               # a head that wraps the ring (inside an iteration's slots for E >= 2)
    assert K == 1 or head + K > capacity
    runs = [(0, True), (1, True), (2, False)]                            # (without a model everybody explores; rb != 4: no model anyway)
    calls = 0
    for variant, use_model in runs:
        # stream positions 0, 623 (the first double straddles two blocks) and 624 (the block is used up at entry), rotating
        # over the states from run to run
        mtpos = [(0, 623, 624)[(e + variant) % 3] for e in range(E)]
        st = start_state(E, n, 300 + n + variant, mtpos)
        explore, rand = _policy(E, n, rb, T, rng, eng is not None and use_model)
        model = eng if use_model else None
        tag = (variant, use_model)

        ref, st_ref = start_channels(E, n, rb, st), _storage(capacity, n)
        rows = [ref.rollout_step(explore[t], rand[t], st_ref, (head + t * E) % capacity, capacity, 1.0, 0.1, engine=model, row_ptr=rp_one)
                for t in range(T)]
        want = _snapshot(ref, st_ref)
        want_reward = np.stack([r.resolve().reward for r in rows])
        want_regular = np.stack([r.resolve().regular for r in rows])

        serial, st_ser = start_channels(E, n, rb, st), _storage(capacity, n)
        serial.rollout_steps(explore, rand, st_ser, head, capacity, 1.0, 0.1, engine=model, row_ptr=rp_all if model else None).resolve()
        want_traj = _trajectory(serial, E, n, rb, T)

        dc, st_got = start_channels(E, n, rb, st), _storage(capacity, n)
        block = dc.rollout_steps(explore, rand, st_got, head, capacity, 1.0, 0.1, engine=model, row_ptr=rp_all if model else None,
                                 walk='wide')
        calls += 1
        got = _snapshot(dc, st_got)
        for name in want:
            assert got[name] == want[name], (tag, name)
        block.resolve()
        assert block.reward.shape == (T, E) and block.reward.tobytes() == want_reward.tobytes(), tag
        assert block.regular.shape == (T, 2, E) and block.regular.tobytes() == want_regular.tobytes() and block.regular.all(), tag
        assert np.all(np.isfinite(want_reward)), tag
        got_traj = _trajectory(dc, E, n, rb, T)
        for name in WORKSPACE:
            assert got_traj[name] == want_traj[name], (tag, name)
        assert dc.walk_calls == {'serial': 0, 'wide': 1} and serial.walk_calls == {'serial': 1, 'wide': 0}, tag
        assert ref.walk_calls == {'serial': 0, 'wide': 0}, tag                        # (a single iteration is no trajectory call)
        assert dc.traffic == serial.traffic, tag                                      # the wide workspace never crosses the bus
        assert dc.rollout_steps_buffers(T)['wide_workspace'].numel() == max(256, wide_workspace_layout(E, n, rb, T)[1])
        if model is not None and T >= 2:                                 # the all-greedy iteration took the network's actions
            slots = (head + np.arange(K)) % capacity
            assert not np.array_equal(st_got['action'].cpu().numpy()[slots].reshape(T, E, n)[1], rand[1]), tag
    assert calls == len(runs)
    if eng is not None:
        eng.close()


@pytest.mark.parametrize("E,n,rb,T", [(3, 4, 4, 3), (1, 20, 4, 50)])
def test_positions_directions_and_streams_are_the_host_librarys_after_the_wide_walk(E, n, rb, T):
    st = start_state(E, n, 900 + n)
    n_u = uniforms_per_step(n, rb)
    h = {k: np.ascontiguousarray(st[k]).copy() for k in ('keys', 'mtpos', 'pos', 'dirs')}
    native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)                   # start_channels' channel update (no walk) ...
    h['mtpos'][:] = st['mtpos']                                          # ... after which the positions are set back
    before = h['pos'].copy()
    u = None
    for _ in range(T):
        native_sim.positions(h['keys'], h['mtpos'], h['pos'], h['dirs'], st['vel'], 0.01, LANES, WIDTH, HEIGHT)
        u = native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)
    assert np.all(np.any(h['pos'] != before, axis=2))                    # every vehicle moved
    dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
    explore, rand = _policy(E, n, rb, T, np.random.default_rng(5), False)
    dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, walk='wide').resolve()
    for name in ('keys', 'mtpos', 'pos', 'dirs'):
        got = dc.download(name)
        assert got.shape == h[name].shape and got.tobytes() == np.ascontiguousarray(h[name]).tobytes(), name
    if u is not None:                                                    # the resident uniforms are those of step T - 1
        assert dc.download('u').tobytes() == np.ascontiguousarray(u, np.float64).tobytes()
    assert dc.walk_calls['wide'] == 1


def test_irregular_and_out_of_range_receivers_are_the_serial_walks_in_every_entry():
    """State 0 has a link that is its own receiver, state 1 a receiver outside [0, n): everybody explores, no model.  The NaN
    rows, the zero col rows and regular == 0 of every entry are the serial walk's (k_traj_observe reads a receiver through
    sim_observe_entry alone, which never forms an index from one outside [0, n): its comment says so, and this test would
    read garbage or fault otherwise)."""
    E, n, rb, T = 2, 4, 4, 3
    st = start_state(E, n, 640, [623, 0])
    st['dest'][0, 2] = 2
    st['dest'][1, 1] = n + 3
    explore, rand = np.ones((T, E), np.uint8), np.random.default_rng(8).integers(0, rb, size=(T, E, n)).astype(np.int32)
    out = {}
    for walk in ('serial', 'wide'):
        dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
        res = dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, walk=walk).resolve()
        out[walk] = (_snapshot(dc, storage), _trajectory(dc, E, n, rb, T), res.regular.copy(), res.reward.tobytes())
    (s_state, s_traj, s_reg, s_rew), (w_state, w_traj, w_reg, w_rew) = out['serial'], out['wide']
    for name in s_state:
        assert w_state[name] == s_state[name], name
    for name in WORKSPACE:
        assert w_traj[name] == s_traj[name], name
    assert w_rew == s_rew and np.array_equal(w_reg, s_reg) and not w_reg.any()
    regular = np.frombuffer(w_traj['traj_regular'], np.uint8).reshape(T + 1, E)
    col = np.frombuffer(w_traj['traj_col'], np.int32).reshape(T + 1, E, n * (n - 2))
    xe = np.frombuffer(w_traj['traj_xe'], np.float32).reshape(T + 1, E, n, 16)
    assert not regular.any() and not col.any()
    assert np.all(np.isnan(xe[:, 1, :, :3 * rb + 1])) and np.all(np.isfinite(xe[:, 0]))      # NaN rows: the out-of-range state alone
    state = np.frombuffer(w_state['state'], np.float64).reshape(E, n, 3 * rb + 1)
    assert np.all(np.isnan(state[1])) and np.all(np.isfinite(state[0]))


@pytest.mark.parametrize("use_model", [False, True])
def test_a_wide_block_two_single_iterations_and_a_serial_block_leave_what_single_iterations_leave(use_model):
    E, n, rb, T = 3, 4, 4, 2
    total = 2 * T + 2
    capacity, head = total * E + 3, 4 * E + 2
    eng = _engine(n) if use_model else None
    rp_one, rp_all = _row_ptr(E, n), _row_ptr(T * E, n)
    explore, rand = _policy(E, n, rb, total, np.random.default_rng(43), use_model)
    if use_model:
        explore[2], explore[3] = (0, 1, 0), (1, 0, 1)
        assert not explore[:2].all() and not explore[4:].all()
    st = start_state(E, n, 513, [624, 0, 623])
    at = lambda t: (head + t * E) % capacity                             # noqa: E731
    kw = lambda block: dict(engine=eng, row_ptr=(rp_all if block else rp_one) if eng else None)    # noqa: E731

    ref, st_ref = start_channels(E, n, rb, st), _storage(capacity, n)
    rows = [ref.rollout_step(explore[t], rand[t], st_ref, at(t), capacity, 1.0, 0.1, **kw(False)) for t in range(total)]
    want = _snapshot(ref, st_ref)
    want_reward = np.stack([r.resolve().reward for r in rows])

    dc, st_got = start_channels(E, n, rb, st), _storage(capacity, n)
    first = dc.rollout_steps(explore[:2], rand[:2], st_got, at(0), capacity, 1.0, 0.1, walk='wide', **kw(True))
    ones = [dc.rollout_step(explore[t], rand[t], st_got, at(t), capacity, 1.0, 0.1, **kw(False)) for t in (2, 3)]
    last = dc.rollout_steps(explore[4:], rand[4:], st_got, at(4), capacity, 1.0, 0.1, walk='serial', **kw(True))
    got = _snapshot(dc, st_got)
    for name in want:
        assert got[name] == want[name], name
    got_reward = np.concatenate([first.resolve().reward] + [o.resolve().reward[None] for o in ones] + [last.resolve().reward])
    assert got_reward.tobytes() == want_reward.tobytes() and np.all(np.isfinite(want_reward))
    assert dc.walk_calls == {'serial': 1, 'wide': 1}
    if eng is not None:
        eng.close()


@pytest.mark.parametrize("E,n,rb,T", [(1, 4, 4, 3), (1, 20, 4, 50)])
def test_the_wide_evaluation_is_the_serial_one_in_every_byte(E, n, rb, T):
    import torch
    eng = _engine(n)
    rng = np.random.default_rng(7 * n + T)
    st = start_state(E, n, 410 + n, [623])
    explore, rand = _policy(E, n, rb, T, rng, True)
    baseline = rng.integers(0, rb, size=(T, E, n)).astype(np.int32)
    out = {}
    for walk in ('serial', 'wide'):
        dc = start_channels(E, n, rb, st)
        res = dc.eval_steps(explore, rand, baseline, 1.0, 0.1, engine=eng, walk=walk).resolve()
        torch.cuda.synchronize()
        block = dc.rollout_steps_buffers(T)['eval_result_dev'][:dc.eval_steps_result_bytes(T, 2)].cpu().numpy().tobytes()
        out[walk] = (block, {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}, _trajectory(dc, E, n, rb, T), res, dc)
    (s_block, s_state, s_traj, s_res, s_dc), (w_block, w_state, w_traj, w_res, w_dc) = out['serial'], out['wide']
    assert w_block == s_block and len(s_block) == s_dc.eval_steps_result_bytes(T, 2)
    for name in STATE:
        assert w_state[name] == s_state[name], name
    for name in WORKSPACE:
        assert w_traj[name] == s_traj[name], name
    assert np.all(np.isfinite(w_res.reward)) and w_res.regular.all() and w_res.actions.shape == (2, T, E, n)
    assert np.array_equal(w_res.actions[1], baseline) and not np.array_equal(w_res.actions[0], rand)
    assert w_dc.walk_calls == {'serial': 0, 'wide': 1} and s_dc.walk_calls == {'serial': 1, 'wide': 0}
    assert w_dc.traffic == s_dc.traffic
    eng.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _trained(E, walk):
    env, agent = _agent(E, 33, 'trajectory')
    agent.trajectory_walk = walk                                         # (the fixture of the existing file constructs the agent)
    out = agent.train(1, 3)
    run = dict(out=out, mem=_memory(agent), online=agent.brain.model.engine.get_flat(), target=agent.brain.target_model.engine.get_flat(),
               rng=np.random.get_state(), num_step=agent.num_step, epsilon=agent.epsilon,
               streams=[np.array(a).copy() for a in (env.pos, env.dirs, env._mt_keys, env._mt_pos)],
               walks=dict(env.device_channels.walk_calls))
    agent.brain.close()
    return run


@pytest.mark.parametrize("E", [1, 5])
def test_agent_with_the_wide_walk_is_the_serial_run_bit_for_bit(E):
    s, w = _trained(E, 'serial'), _trained(E, 'wide')
    _assert_same_run(s, w, E)
    assert s['num_step'] == 150 and s['mem']['size'] == 150
    assert w['walks'] == {'serial': 0, 'wide': 3} and s['walks'] == {'serial': 3, 'wide': 0}


def test_the_agent_takes_the_walk_at_construction():
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(3)
    np.random.seed(3)
    env = start_env_batched(4, 2, 3, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=3, device_replay=True, rollout_backend='trajectory',
                  trajectory_walk='wide')
    assert agent.trajectory_walk == 'wide'
    rewards = agent.generate_d2d_transition(6)
    assert rewards.shape == (6,) and np.all(np.isfinite(rewards)) and env.device_channels.walk_calls == {'serial': 0, 'wide': 1}
    with pytest.raises(ValueError, match="trajectory_walk must be one of"):
        Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=agent.brain, device_replay=True, rollout_backend='trajectory',
              trajectory_walk='sideways')
    # E = 2: eval_backend='device' cannot run, and without trajectory rollouts nothing would ever take the wide walk
    with pytest.raises(ValueError, match="trajectory_walk='wide' needs") as exc:
        Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=agent.brain, device_replay=True, rollout_backend='device',
              trajectory_walk='wide')
    assert "ONE simulator" in str(exc.value)
    agent.brain.close()


def test_test_run_on_the_device_with_the_wide_walk_equals_the_serial_books():
    runs = {}
    for walk in ('serial', 'wide'):
        env, agent = _eval_agent(4, 31)
        agent.trajectory_walk = walk
        out = agent.test_run(1, 3, False, eval_backend='device')
        runs[walk] = dict(out=[np.asarray(a).copy() for a in out], rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step,
                          streams=[np.array(a).copy() for a in (env._mt_keys, env._mt_pos, env.pos, env.dirs)],
                          stats=dict(agent.eval_stats), walks=dict(env.device_channels.walk_calls))
        agent.brain.close()
    s, w = runs['serial'], runs['wide']
    assert len(s['out']) == len(w['out']) > 0
    for i, (a, b) in enumerate(zip(s['out'], w['out'])):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), i
    assert _same_rng(s['rng'], w['rng']) and s['py'] == w['py'] and s['num_step'] == w['num_step'] > 0
    for a, b in zip(s['streams'], w['streams']):
        assert a.tobytes() == b.tobytes()
    assert s['stats'] == w['stats'] == {'device_episodes': 1, 'host_episodes': 0}
    assert w['walks'] == {'serial': 0, 'wide': 1} and s['walks'] == {'serial': 1, 'wide': 0}


# ------------------------------------------------------------------------------------------------------- a refused call
def test_a_refused_wide_call_leaves_the_state_and_the_storage_alone():
    import torch
    lib = load_library()
    E, n, rb, T = 3, 4, 4, 3
    st = start_state(E, n, 77)
    dc, storage = start_channels(E, n, rb, st), _storage(T * E + 2, n)
    eng = _engine(n)
    before = _snapshot(dc, storage)
    r = dc.rollout_steps_struct(T, storage, 0, T * E + 2, 1.0, 0.1, engine=eng, row_ptr=_row_ptr(T * E, n))
    _, need = wide_workspace_layout(E, n, rb, T)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=storage['xe'].device)
    stream = torch.cuda.current_stream().cuda_stream
    for ptr, size, word in ((None, need, "null wide-walk workspace"), (ws.data_ptr(), need - 1, "needs %d bytes" % need)):
        assert lib.v2x_rollout_steps_wide(ctypes.byref(r), ptr, size, stream) == V2X_EINVAL
        assert word in lib.v2x_last_error(None).decode()
    r.r.capacity = T * E - 1                                             # a check of the serial call, with a good workspace
    assert lib.v2x_rollout_steps_wide(ctypes.byref(r), ws.data_ptr(), need, stream) == V2X_EINVAL
    assert "T E <= capacity" in lib.v2x_last_error(None).decode()
    ev = dc.eval_steps_struct(T, 1.0, 0.1, engine=eng)
    assert lib.v2x_eval_steps_wide(ctypes.byref(ev), ws.data_ptr(), need - 1, stream) == V2X_EINVAL
    assert "needs %d bytes" % need in lib.v2x_last_error(None).decode()
    after = _snapshot(dc, storage)
    for name in before:
        assert after[name] == before[name], name
    torch.cuda.synchronize()
    assert bool((ws == 7).all())                                          # the workspace was not written either
    with pytest.raises(ValueError, match="walk must be"):
        dc.rollout_steps(np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int32), storage, 0, T * E + 2, 1.0, 0.1, walk='sideways')
    assert _snapshot(dc, storage) == before and dc.walk_calls == {'serial': 0, 'wide': 0}
    eng.close()
