"""GPU: the split stream phase of the wide walk (v2x_rollout_steps_split / v2x_eval_steps_split: k_traj_words, k_traj_walk,
k_traj_uniforms of csrc/v2xsimdev.hip in k_traj_stream's place; DeviceChannels.rollout_steps / eval_steps(walk='wide',
stream_phase='split'); Agent(trajectory_walk='wide', trajectory_streams='split')).  The references are the wide walk as it
stands (stream_phase='chain'), the serial walk (k_sim_trajectory) and the host library native_sim; everything is compared
byte for byte: the split form does integer and exactly rounded arithmetic only, so no tolerance applies anywhere.

The engine scores 4 channels only, so the cases with rb = 1 and rb = 5 run without a model (everybody explores).

The offsets of a step's uniforms depend on the words the walks before it drew.  That the cases really exercise this is asserted
on the host (test_the_cases_*): with start_state(E, n, 300 + n + variant) and entry positions 0 / 623 / 624 rotating over the
states, the host walk draws in 6-8 of 9 (step, state) pairs at (3,4,4,3), in 5-6 of 6 at (2,15,4,3), in all 6 at (2,16,4,3),
in 19-20 of 50 at (5,20,4,10) and in 10-11 of 50 at (1,20,4,50); per-step word counts run over 0, 2, ..., 16 (22 once at
n = 31); most states entering at 623 draw in step 0, so a walk double straddles two blocks.  start_state puts every vehicle
within four steps of a lane, so in a long case the draws sit in the first steps and the later offsets all follow from them:
31 of the 150 pairs of (1,20,4,50) draw.  The cases with T >= 10 therefore run two more states each (_spread_state: vehicle v
reaches its first lane at step v min(T, 25) / n and, going straight on, the next one 23 to 35 steps later, so the walks draw
all along the T steps: 31 and 26 of 50 at (1,20,4,50), 88 of 250 with the three runs above), and
test_the_cases_draw_in_a_third_of_their_step_state_pairs asks a third of all (step, state) pairs of a case, over its runs."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_eval_device import _agent as _eval_agent
from test_gpu_rollout_trajectory import (DOWN, LANES, LEFT, RIGHT, STATE, UP, WIDTH, HEIGHT, _agent, _assert_same_run, _engine, _memory, _policy,
                                         _row_ptr, _same_rng, _snapshot, _storage, start_channels, start_state)
from test_gpu_trajectory_wide import WORKSPACE, _trajectory
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import native_sim
from v2xgnn.rl.device_sim import split_workspace_layout, uniforms_per_step, wide_workspace_layout

pytestmark = pytest.mark.gpu

SPLIT_CASES = [(1, 3, 1, 1), (1, 3, 1, 2), (3, 4, 4, 3), (2, 15, 4, 3), (2, 16, 4, 3), (5, 20, 4, 10), (1, 20, 4, 50), (2, 31, 5, 2)]
VARIANTS = (0, 1, 2)
SPREAD_VARIANTS = (3, 4)                                 # the two further runs of the cases with T >= 10


def _variants(T):
    return VARIANTS + (SPREAD_VARIANTS if T >= 10 else ())


def _spread_state(E, n, T, seed, mtpos):
    """start_state with the vehicles placed so that vehicle v reaches the first lane ahead of it at step v min(T, 25) / n (it
    stands half a step before the lane at the start of that step), nothing else on its way there; who goes straight on meets
    the next lane 3.5 m on, 23 to 35 steps later: the walks draw all along the T steps.  The lanes: the outermost of the four
    that lie together in the middle of the map (no lane lies within 7.5 m, the most a vehicle moves in 50 steps, before them)."""
    st = start_state(E, n, seed, mtpos)
    first = {(1, 1.0): RIGHT[0], (1, -1.0): LEFT[3], (0, 1.0): DOWN[0], (0, -1.0): UP[3]}    # (axis, sign) -> the lane ahead
    for e in range(E):
        for v in range(n):
            d = int(st['dirs'][e, v])
            sg, ax, dv = (1.0 if d in (0, 3) else -1.0), (1 if d < 2 else 0), st['vel'][e, v] * 0.01
            st['pos'][e, v, ax] = first[(ax, sg)] - sg * ((v * min(T, 25)) // n + 0.5) * dv
    return st


def _case_state(E, n, variant, T=0):
    """stream positions 0, 623 (the first double straddles two blocks) and 624 (the block is used up at entry), rotating over
    the states from run to run"""
    mtpos = [(0, 623, 624)[(e + variant) % 3] for e in range(E)]
    if variant in SPREAD_VARIANTS:
        return _spread_state(E, n, T, 300 + n + variant, mtpos)
    return start_state(E, n, 300 + n + variant, mtpos)


def _host_walk(st, n, rb, T, lanes=LANES):
    """T steps of the host library on the state start_channels(st) leaves -> (keys / mtpos / pos / dirs after them, the
    uniforms of the last step, words the walk of (t, e) drew [T, E], the position each walk entered at [T, E])"""
    E, n_u = st['keys'].shape[0], uniforms_per_step(n, rb)
    h = {k: np.ascontiguousarray(st[k]).copy() for k in ('keys', 'mtpos', 'pos', 'dirs')}
    native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)                   # start_channels' channel update (no walk) ...
    h['mtpos'][:] = st['mtpos']                                          # ... after which the positions are set back
    drawn, entry, u = np.zeros((T, E), np.int64), np.zeros((T, E), np.int64), None
    for t in range(T):
        entry[t] = h['mtpos']
        native_sim.positions(h['keys'], h['mtpos'], h['pos'], h['dirs'], st['vel'], 0.01, lanes, WIDTH, HEIGHT)
        drawn[t] = (h['mtpos'] - entry[t]) % 624                         # (a walk draws far fewer than 624 words)
        u = native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)
    return h, u, drawn, entry


# ------------------------------------------------------------------------------------------------------- the preconditions
def test_the_cases_hold_a_straddling_walk_double_an_entry_at_624_and_varying_word_counts():
    straddles, at_624, counts = 0, 0, set()
    for E, n, rb, T in SPLIT_CASES:
        for variant in _variants(T):
            _, _, drawn, entry = _host_walk(_case_state(E, n, variant, T), n, rb, T)
            straddles += int(np.sum((entry[0] == 623) & (drawn[0] >= 2)))     # words 623 and 0 of the next block: one double
            at_624 += int(np.sum(entry[0] == 624))
            assert np.all(drawn % 2 == 0)
            counts |= set(drawn.ravel().tolist())
    assert straddles >= 1 and at_624 >= 1
    assert set(range(0, 18, 2)) <= counts                                # 0, 2, ..., 16 words per step all occur


@pytest.mark.parametrize("E,n,rb,T", [c for c in SPLIT_CASES if c[3] >= 3])
def test_the_cases_draw_in_a_third_of_their_step_state_pairs(E, n, rb, T):
    """of all (step, state) pairs of the case, over its runs, at least a third draw; where T >= 10 the two spread runs draw in
    at least a third of their own pairs as well, and in the second half of the steps too"""
    drawing, pairs = 0, 0
    for variant in _variants(T):
        _, _, drawn, _ = _host_walk(_case_state(E, n, variant, T), n, rb, T)
        k = int(np.sum(drawn > 0))
        print("E=%d n=%d rb=%d T=%d run %d: walk draws in %d of %d (step, state) pairs" % (E, n, rb, T, variant, k, drawn.size))
        drawing, pairs = drawing + k, pairs + drawn.size
        if variant in SPREAD_VARIANTS:
            assert 3 * k >= drawn.size and np.any(drawn[T // 2:] > 0), variant
    assert 3 * drawing >= pairs, (drawing, pairs)


# ------------------------------------------------------------------------------------------------------- split == wide == serial
def _run_block(E, n, rb, T, st, explore, rand, head, capacity, model, rp_all, **form):
    dc, storage = start_channels(E, n, rb, st), _storage(capacity, n)
    res = dc.rollout_steps(explore, rand, storage, head, capacity, 1.0, 0.1, engine=model, row_ptr=rp_all if model else None, **form)
    snap = _snapshot(dc, storage)
    res.resolve()
    return dc, snap, _trajectory(dc, E, n, rb, T), res


@pytest.mark.parametrize("E,n,rb,T", SPLIT_CASES)
def test_the_split_form_leaves_every_byte_the_wide_and_the_serial_walk_leave(E, n, rb, T):
    K = T * E
    capacity = K + 3
    eng = _engine(n) if rb == 4 else None
    rp_all = _row_ptr(K, n)
    rng = np.random.default_rng(100 * n + 10 * E + T)
    head = capacity - max(1, min(K - 1, E * (T // 2) + 1))               # a head that wraps the ring
    for variant, use_model in ((0, True), (1, True), (2, False), (3, True), (4, False))[:len(_variants(T))]:
        st = _case_state(E, n, variant, T)
        explore, rand = _policy(E, n, rb, T, rng, eng is not None and use_model)
        model = eng if use_model else None
        tag = (variant, use_model)
        args = (E, n, rb, T, st, explore, rand, head, capacity, model, rp_all)
        s_dc, s_state, s_traj, s_res = _run_block(*args)
        w_dc, w_state, w_traj, w_res = _run_block(*args, walk='wide')
        dc, state, traj, res = _run_block(*args, walk='wide', stream_phase='split')
        for name in s_state:                                             # STATE and the replay storage
            assert state[name] == w_state[name], (tag, name, 'wide')
            assert state[name] == s_state[name], (tag, name, 'serial')
        for name in WORKSPACE:                                           # the seven trajectory arrays
            assert traj[name] == w_traj[name] == s_traj[name], (tag, name)
        assert res.reward.shape == (T, E) and res.reward.tobytes() == w_res.reward.tobytes() == s_res.reward.tobytes(), tag
        assert res.regular.shape == (T, 2, E) and res.regular.tobytes() == w_res.regular.tobytes() == s_res.regular.tobytes(), tag
        assert res.regular.all() and np.all(np.isfinite(res.reward)), tag
        assert dc.walk_calls == w_dc.walk_calls == {'serial': 0, 'wide': 1} and s_dc.walk_calls == {'serial': 1, 'wide': 0}, tag
        assert dc.stream_phase_calls == {'chain': 0, 'split': 1} and w_dc.stream_phase_calls == {'chain': 1, 'split': 0}, tag
        assert s_dc.stream_phase_calls == {'chain': 0, 'split': 0}, tag
        assert dc.traffic == w_dc.traffic == s_dc.traffic, tag           # neither workspace crosses the bus
        io = dc.rollout_steps_buffers(T)
        assert io['wide_workspace'].numel() == max(256, wide_workspace_layout(E, n, rb, T)[1])
        assert io['split_workspace'].numel() == split_workspace_layout(E, n, rb, T, 6)[1]
        assert 'split_workspace' not in w_dc.rollout_steps_buffers(T)
    if eng is not None:
        eng.close()


# ------------------------------------------------------------------------------------------------------- a heavy walk
@pytest.mark.parametrize("n_lanes", [6, 64])
def test_a_heavy_walk_every_vehicle_reaching_every_lane_of_both_tables(n_lanes):
    """All vehicles head up from y = 100.0 and reach every lane of the left and the right table in step 0: the walk draws one
    double per reached lane until the vehicle turns, far more words than a chunk of 64, from entry position 623."""
    E, n, rb, T = 2, 20, 4, 3
    left = 100.0 + 0.001 * (np.arange(n_lanes) + 1)
    lanes = (np.asarray(LANES[0])[:1].repeat(n_lanes) + np.arange(n_lanes) * 3.5, np.asarray(LANES[1])[:1].repeat(n_lanes) +
             np.arange(n_lanes) * 3.5, left, left + 0.0005)
    st = start_state(E, n, 77, [623, 623])
    st['dirs'][:] = 0                                                    # up: the moving coordinate is y, the tables left / right
    st['pos'][:, :, 1] = 100.0
    st['pos'][:, :, 0] = 10.0 + 30.0 * np.arange(n)[None, :]
    assert np.all(st['vel'] * 0.01 >= 0.1) and np.all(left + 0.0005 < 100.1)      # every lane lies within the first move

    def channels():
        dc = start_channels(E, n, rb, st)
        dc.set_grid(lanes, WIDTH, HEIGHT, 0.01)
        return dc

    h, u, drawn, entry = _host_walk(st, n, rb, T, lanes)
    print("heavy walk, %d lanes: words drawn per (step, state): %s" % (n_lanes, drawn.tolist()))
    assert np.all(drawn[0] >= 2 * n) and np.all(entry[0] == 623)     # (92 and 116 words with these keys: more than a chunk of 64)
    explore, rand = _policy(E, n, rb, T, np.random.default_rng(3), False)
    out = {}
    for phase in ('chain', 'split'):
        dc, storage = channels(), _storage(T * E, n)
        res = dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, walk='wide', stream_phase=phase).resolve()
        out[phase] = (_snapshot(dc, storage), _trajectory(dc, E, n, rb, T), res.reward.tobytes(), res.regular.tobytes(), dc)
    c, s = out['chain'], out['split']
    for name in c[0]:
        assert s[0][name] == c[0][name], name
    for name in WORKSPACE:
        assert s[1][name] == c[1][name], name
    assert s[2] == c[2] and s[3] == c[3]
    dc = s[4]
    for name in ('keys', 'mtpos', 'pos', 'dirs'):
        assert dc.download(name).tobytes() == np.ascontiguousarray(h[name]).tobytes(), name
    assert dc.download('u').tobytes() == np.ascontiguousarray(u, np.float64).tobytes()
    assert dc.rollout_steps_buffers(T)['split_workspace'].numel() == split_workspace_layout(E, n, rb, T, n_lanes)[1]
    assert dc.stream_phase_calls == {'chain': 0, 'split': 1}


# ------------------------------------------------------------------------------------------------------- the block boundary
def test_a_stream_that_ends_exactly_on_a_block_boundary_leaves_position_624():
    E, n, rb, T = 1, 3, 1, 2
    found = None
    for p in range(625):
        st = start_state(E, n, 303, [p])
        h, u, _, _ = _host_walk(st, n, rb, T)
        if h['mtpos'][0] == 624:
            found = (p, st, h, u)
            break
    assert found is not None, "no entry position of (1, 3, 1, 2) ends the stream on a block boundary"
    p, st, h, u = found
    dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
    explore, rand = _policy(E, n, rb, T, np.random.default_rng(5), False)
    dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, walk='wide', stream_phase='split').resolve()
    assert int(dc.download('mtpos')[0]) == 624
    assert dc.download('keys').tobytes() == h['keys'].tobytes()
    for name in ('pos', 'dirs'):
        assert dc.download(name).tobytes() == np.ascontiguousarray(h[name]).tobytes(), name
    assert dc.download('u').tobytes() == np.ascontiguousarray(u, np.float64).tobytes()


# ------------------------------------------------------------------------------------------------------- the host library
@pytest.mark.parametrize("E,n,rb,T", [(3, 4, 4, 3), (1, 20, 4, 50)])
def test_positions_directions_and_streams_are_the_host_librarys_after_the_split_walk(E, n, rb, T):
    st = start_state(E, n, 900 + n)
    before = st['pos'].copy()
    h, u, _, _ = _host_walk(st, n, rb, T)
    assert np.all(np.any(h['pos'] != before, axis=2))                    # every vehicle moved
    dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
    explore, rand = _policy(E, n, rb, T, np.random.default_rng(5), False)
    dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, walk='wide', stream_phase='split').resolve()
    for name in ('keys', 'mtpos', 'pos', 'dirs'):
        got = dc.download(name)
        assert got.shape == h[name].shape and got.tobytes() == np.ascontiguousarray(h[name]).tobytes(), name
    assert dc.download('u').tobytes() == np.ascontiguousarray(u, np.float64).tobytes()      # the uniforms of step T - 1
    assert dc.walk_calls['wide'] == 1 and dc.stream_phase_calls['split'] == 1


def test_irregular_and_out_of_range_receivers_are_the_serial_walks_in_every_entry():
    """State 0 has a link that is its own receiver, state 1 a receiver outside [0, n): everybody explores, no model.  The NaN
    rows, the zero col rows and regular == 0 of every entry are the serial walk's."""
    E, n, rb, T = 2, 4, 4, 3
    st = start_state(E, n, 640, [623, 0])
    st['dest'][0, 2] = 2
    st['dest'][1, 1] = n + 3
    explore, rand = np.ones((T, E), np.uint8), np.random.default_rng(8).integers(0, rb, size=(T, E, n)).astype(np.int32)
    out = {}
    for tag, form in (('serial', {}), ('split', dict(walk='wide', stream_phase='split'))):
        dc, storage = start_channels(E, n, rb, st), _storage(T * E, n)
        res = dc.rollout_steps(explore, rand, storage, 0, T * E, 1.0, 0.1, **form).resolve()
        out[tag] = (_snapshot(dc, storage), _trajectory(dc, E, n, rb, T), res.regular.copy(), res.reward.tobytes())
    (s_state, s_traj, s_reg, s_rew), (w_state, w_traj, w_reg, w_rew) = out['serial'], out['split']
    for name in s_state:
        assert w_state[name] == s_state[name], name
    for name in WORKSPACE:
        assert w_traj[name] == s_traj[name], name
    assert w_rew == s_rew and np.array_equal(w_reg, s_reg) and not w_reg.any()
    regular = np.frombuffer(w_traj['traj_regular'], np.uint8).reshape(T + 1, E)
    col = np.frombuffer(w_traj['traj_col'], np.int32).reshape(T + 1, E, n * (n - 2))
    xe = np.frombuffer(w_traj['traj_xe'], np.float32).reshape(T + 1, E, n, 16)
    assert not regular.any() and not col.any()
    assert np.all(np.isnan(xe[:, 1, :, :3 * rb + 1])) and np.all(np.isfinite(xe[:, 0]))


# ------------------------------------------------------------------------------------------------------- mixing the forms
@pytest.mark.parametrize("use_model", [False, True])
def test_a_split_block_two_single_iterations_a_chain_block_and_a_serial_block_leave_what_single_iterations_leave(use_model):
    E, n, rb, T = 3, 4, 4, 2
    total = 3 * T + 2
    capacity, head = total * E + 3, 4 * E + 2
    eng = _engine(n) if use_model else None
    rp_one, rp_all = _row_ptr(E, n), _row_ptr(T * E, n)
    explore, rand = _policy(E, n, rb, total, np.random.default_rng(43), use_model)
    if use_model:
        explore[2], explore[3] = (0, 1, 0), (1, 0, 1)
        explore[4], explore[5] = (0, 0, 1), (1, 0, 0)
        assert not explore[:2].all() and not explore[4:6].all() and not explore[6:].all()
    st = start_state(E, n, 513, [624, 0, 623])
    at = lambda t: (head + t * E) % capacity                             # noqa: E731
    kw = lambda block: dict(engine=eng, row_ptr=(rp_all if block else rp_one) if eng else None)    # noqa: E731

    ref, st_ref = start_channels(E, n, rb, st), _storage(capacity, n)
    rows = [ref.rollout_step(explore[t], rand[t], st_ref, at(t), capacity, 1.0, 0.1, **kw(False)) for t in range(total)]
    want = _snapshot(ref, st_ref)
    want_reward = np.stack([r.resolve().reward for r in rows])

    dc, st_got = start_channels(E, n, rb, st), _storage(capacity, n)
    first = dc.rollout_steps(explore[:2], rand[:2], st_got, at(0), capacity, 1.0, 0.1, walk='wide', stream_phase='split', **kw(True))
    ones = [dc.rollout_step(explore[t], rand[t], st_got, at(t), capacity, 1.0, 0.1, **kw(False)) for t in (2, 3)]
    mid = dc.rollout_steps(explore[4:6], rand[4:6], st_got, at(4), capacity, 1.0, 0.1, walk='wide', stream_phase='chain', **kw(True))
    last = dc.rollout_steps(explore[6:], rand[6:], st_got, at(6), capacity, 1.0, 0.1, walk='serial', **kw(True))
    got = _snapshot(dc, st_got)
    for name in want:
        assert got[name] == want[name], name
    got_reward = np.concatenate([first.resolve().reward] + [o.resolve().reward[None] for o in ones] +
                                [mid.resolve().reward, last.resolve().reward])
    assert got_reward.tobytes() == want_reward.tobytes() and np.all(np.isfinite(want_reward))
    assert dc.walk_calls == {'serial': 1, 'wide': 2} and dc.stream_phase_calls == {'chain': 1, 'split': 1}
    if eng is not None:
        eng.close()


# ------------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("E,n,rb,T", [(1, 4, 4, 3), (1, 20, 4, 50)])
def test_the_split_evaluation_is_the_serial_one_in_every_byte(E, n, rb, T):
    import torch
    eng = _engine(n)
    rng = np.random.default_rng(7 * n + T)
    st = start_state(E, n, 410 + n, [623])
    explore, rand = _policy(E, n, rb, T, rng, True)
    baseline = rng.integers(0, rb, size=(T, E, n)).astype(np.int32)
    out = {}
    for tag, form in (('serial', {}), ('split', dict(walk='wide', stream_phase='split'))):
        dc = start_channels(E, n, rb, st)
        res = dc.eval_steps(explore, rand, baseline, 1.0, 0.1, engine=eng, **form).resolve()
        torch.cuda.synchronize()
        block = dc.rollout_steps_buffers(T)['eval_result_dev'][:dc.eval_steps_result_bytes(T, 2)].cpu().numpy().tobytes()
        out[tag] = (block, {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}, _trajectory(dc, E, n, rb, T), res, dc)
    (s_block, s_state, s_traj, s_res, s_dc), (w_block, w_state, w_traj, w_res, w_dc) = out['serial'], out['split']
    assert w_block == s_block and len(s_block) == s_dc.eval_steps_result_bytes(T, 2)
    for name in STATE:
        assert w_state[name] == s_state[name], name
    for name in WORKSPACE:
        assert w_traj[name] == s_traj[name], name
    assert np.all(np.isfinite(w_res.reward)) and w_res.regular.all() and w_res.actions.shape == (2, T, E, n)
    assert np.array_equal(w_res.actions[1], baseline) and not np.array_equal(w_res.actions[0], rand)
    assert w_dc.walk_calls == {'serial': 0, 'wide': 1} and s_dc.walk_calls == {'serial': 1, 'wide': 0}
    assert w_dc.stream_phase_calls == {'chain': 0, 'split': 1} and s_dc.stream_phase_calls == {'chain': 0, 'split': 0}
    assert w_dc.traffic == s_dc.traffic
    eng.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _trained(E, walk, streams):
    env, agent = _agent(E, 33, 'trajectory')
    agent.trajectory_walk, agent.trajectory_streams = walk, streams      # (the fixture of the existing file constructs the agent)
    out = agent.train(1, 3)
    run = dict(out=out, mem=_memory(agent), online=agent.brain.model.engine.get_flat(), target=agent.brain.target_model.engine.get_flat(),
               rng=np.random.get_state(), num_step=agent.num_step, epsilon=agent.epsilon,
               streams=[np.array(a).copy() for a in (env.pos, env.dirs, env._mt_keys, env._mt_pos)],
               walks=dict(env.device_channels.walk_calls), phases=dict(env.device_channels.stream_phase_calls))
    agent.brain.close()
    return run


@pytest.mark.parametrize("E", [1, 5])
def test_agent_with_the_split_stream_phase_is_the_serial_run_bit_for_bit(E):
    s, w = _trained(E, 'serial', 'chain'), _trained(E, 'wide', 'split')
    _assert_same_run(s, w, E)
    assert s['num_step'] == 150 and s['mem']['size'] == 150
    assert w['walks'] == {'serial': 0, 'wide': 3} and s['walks'] == {'serial': 3, 'wide': 0}
    assert w['phases'] == {'chain': 0, 'split': 3} and s['phases'] == {'chain': 0, 'split': 0}


def test_the_agent_takes_the_stream_phase_at_construction():
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.train import start_env_batched
    random.seed(3)
    np.random.seed(3)
    env = start_env_batched(4, 2, 3, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=3, device_replay=True, rollout_backend='trajectory',
                  trajectory_walk='wide', trajectory_streams='split')
    assert agent.trajectory_walk == 'wide' and agent.trajectory_streams == 'split'
    rewards = agent.generate_d2d_transition(6)
    assert rewards.shape == (6,) and np.all(np.isfinite(rewards))
    assert env.device_channels.walk_calls == {'serial': 0, 'wide': 1} and env.device_channels.stream_phase_calls == {'chain': 0, 'split': 1}
    with pytest.raises(ValueError, match="trajectory_streams must be one of"):
        Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=agent.brain, device_replay=True, rollout_backend='trajectory',
              trajectory_walk='wide', trajectory_streams='sideways')
    with pytest.raises(ValueError, match="trajectory_streams='split' needs trajectory_walk='wide'"):
        Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, brain=agent.brain, device_replay=True, rollout_backend='trajectory',
              trajectory_streams='split')
    agent.brain.close()


def test_test_run_on_the_device_with_the_split_stream_phase_equals_the_serial_books():
    runs = {}
    for tag, walk, streams in (('serial', 'serial', 'chain'), ('split', 'wide', 'split')):
        env, agent = _eval_agent(4, 31)
        agent.trajectory_walk, agent.trajectory_streams = walk, streams
        out = agent.test_run(1, 3, False, eval_backend='device')
        runs[tag] = dict(out=[np.asarray(a).copy() for a in out], rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step,
                         streams=[np.array(a).copy() for a in (env._mt_keys, env._mt_pos, env.pos, env.dirs)],
                         stats=dict(agent.eval_stats), walks=dict(env.device_channels.walk_calls),
                         phases=dict(env.device_channels.stream_phase_calls))
        agent.brain.close()
    s, w = runs['serial'], runs['split']
    assert len(s['out']) == len(w['out']) > 0
    for i, (a, b) in enumerate(zip(s['out'], w['out'])):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), i
    assert _same_rng(s['rng'], w['rng']) and s['py'] == w['py'] and s['num_step'] == w['num_step'] > 0
    for a, b in zip(s['streams'], w['streams']):
        assert a.tobytes() == b.tobytes()
    assert s['stats'] == w['stats'] == {'device_episodes': 1, 'host_episodes': 0}
    assert w['walks'] == {'serial': 0, 'wide': 1} and s['walks'] == {'serial': 1, 'wide': 0}
    assert w['phases'] == {'chain': 0, 'split': 1} and s['phases'] == {'chain': 0, 'split': 0}


# ------------------------------------------------------------------------------------------------------- a refused call
def test_a_refused_split_call_leaves_the_state_the_storage_and_both_workspaces_alone():
    import torch
    lib = load_library()
    E, n, rb, T = 3, 4, 4, 3
    st = start_state(E, n, 77)
    dc, storage = start_channels(E, n, rb, st), _storage(T * E + 2, n)
    eng = _engine(n)
    before = _snapshot(dc, storage)
    r = dc.rollout_steps_struct(T, storage, 0, T * E + 2, 1.0, 0.1, engine=eng, row_ptr=_row_ptr(T * E, n))
    _, wide = wide_workspace_layout(E, n, rb, T)
    _, need = split_workspace_layout(E, n, rb, T, 6)
    assert lib.v2x_traj_split_workspace_bytes(E, n, rb, T, 6) == need
    ws = torch.full((wide,), 7, dtype=torch.uint8, device=storage['xe'].device)
    ss = torch.full((need,), 9, dtype=torch.uint8, device=storage['xe'].device)
    stream = torch.cuda.current_stream().cuda_stream
    W, S = ws.data_ptr(), ss.data_ptr()
    for a, word in (((None, wide, S, need), "null wide-walk workspace"), ((W, wide - 1, S, need), "needs %d bytes" % wide),
                    ((W, wide, None, need), "null split-stream workspace"), ((W, wide, S, need - 1), "needs %d bytes" % need)):
        assert lib.v2x_rollout_steps_split(ctypes.byref(r), a[0], a[1], a[2], a[3], stream) == V2X_EINVAL
        assert word in lib.v2x_last_error(None).decode()
    r.r.capacity = T * E - 1                                             # a check of the serial call, with good workspaces
    assert lib.v2x_rollout_steps_split(ctypes.byref(r), W, wide, S, need, stream) == V2X_EINVAL
    assert "T E <= capacity" in lib.v2x_last_error(None).decode()
    ev = dc.eval_steps_struct(T, 1.0, 0.1, engine=eng)
    assert lib.v2x_eval_steps_split(ctypes.byref(ev), W, wide, S, need - 1, stream) == V2X_EINVAL
    assert "needs %d bytes" % need in lib.v2x_last_error(None).decode()
    after = _snapshot(dc, storage)
    for name in before:
        assert after[name] == before[name], name
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((ss == 9).all())               # neither workspace was written
    ex, ra = np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int32)
    with pytest.raises(ValueError, match="stream_phase must be"):
        dc.rollout_steps(ex, ra, storage, 0, T * E + 2, 1.0, 0.1, walk='wide', stream_phase='sideways')
    with pytest.raises(ValueError, match="stream_phase='split' needs walk='wide'"):
        dc.rollout_steps(ex, ra, storage, 0, T * E + 2, 1.0, 0.1, stream_phase='split')
    assert _snapshot(dc, storage) == before and dc.walk_calls == {'serial': 0, 'wide': 0}
    assert dc.stream_phase_calls == {'chain': 0, 'split': 0}
    eng.close()
