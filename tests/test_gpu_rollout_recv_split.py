"""GPU: the receiver-form rollout with the split stream phase (v2x_rollout_steps_recv_split: k_traj_words_recv,
k_traj_walk_recv -- one wave, two vehicles per lane, up to 128 vehicles -- and k_traj_uniforms in k_traj_stream_recv's place;
DeviceChannels.rollout_steps_recv(stream_phase='split'); Agent(receiver_streams='split')).  The reference everywhere is the
chain form (v2x_rollout_steps_recv) on a twin DeviceChannels built from the same state, and every comparison is byte for byte:
integer and exactly rounded arithmetic only, so no tolerance applies anywhere.  What a case needs of its inputs (who walks,
how many words a step draws, where the stream stands) is established by a replay on the host library first and asserted before
anything is compared.  The engine scores 4 channels: rb = 4 throughout."""
import ctypes

import numpy as np
import pytest

from test_gpu_rollout_recv import MARK, RB, WALKED, _bytes, _policy, _recv_storage, start_channels_recv
from test_gpu_rollout_trajectory import DOWN, HEIGHT, LANES, LEFT, RIGHT, UP, WIDTH, _engine, start_state
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, RL_Config, native_sim
from v2xgnn.rl.device_sim import RECV_SECTIONS, split_workspace_layout, uniforms_per_step, wide_workspace_layout
from v2xgnn.rl.replay import ReceiverReplay
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

# every resident tensor the call writes: streams, positions, uniforms, shadowing, channels, observation, actions, rates
RESIDENT = WALKED + ('interf_db', 'state', 'xe', 'recv', 'flags', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf',
                     'actions')
REENTRY = {0: 3, 1: 2, 2: 0, 3: 1}                       # the direction a vehicle re-enters the map with (sim_stream_walk)


# ------------------------------------------------------------------------------------------------------- the host replay
def _reaches(pos, dirs, vel):
    """[E, n] bool: the vehicle reaches a lane of one of its two tables in the next step (sim_stream_walk's masks, non-empty)"""
    E, n = dirs.shape
    out = np.zeros((E, n), bool)
    for e in range(E):
        for v in range(n):
            d = int(dirs[e, v])
            ax, sg, dv = (1 if d < 2 else 0), (1.0 if d in (0, 3) else -1.0), vel[e, v] * 0.01
            av = pos[e, v, ax]
            tabs = np.asarray((LEFT + RIGHT) if ax == 1 else (UP + DOWN))
            out[e, v] = bool(np.any((av <= tabs) & (av + dv >= tabs)) if sg > 0 else np.any((av >= tabs) & (av - dv <= tabs)))
    return out


def _leaves(pos, dirs, vel):
    """[E, n] bool: a straight move takes the vehicle off the map in the next step"""
    ax = (dirs < 2).astype(int)
    sg = np.where((dirs == 0) | (dirs == 3), 1.0, -1.0)
    av = np.take_along_axis(pos, ax[:, :, None], axis=2)[:, :, 0] + sg * vel * 0.01
    return (av < 0) | (av > np.where(ax == 1, HEIGHT, WIDTH))


def _inside(pos, margin=5.0):
    return ((pos[:, :, 0] > margin) & (pos[:, :, 0] < WIDTH - margin) & (pos[:, :, 1] > margin) & (pos[:, :, 1] < HEIGHT - margin))


def _host_replay(st, n, T):
    """T steps of the host library on the state start_channels_recv(st) leaves -> a dict: keys / mtpos / pos / dirs after them,
    and per step [T, E(, n)]: drawn (words of the walk), entry (the position the walk entered at), walkers (who reaches a
    lane), turned (walkers well inside the map that left their axis: a turn, not a re-entry), reentered (non-walkers whose
    straight move leaves the map and that came back with the re-entry direction)"""
    E, n_u = st['keys'].shape[0], uniforms_per_step(n, RB)
    h = {k: np.ascontiguousarray(st[k]).copy() for k in ('keys', 'mtpos', 'pos', 'dirs')}
    native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)                   # start_channels_recv's channel update (no walk) ...
    h['mtpos'][:] = st['mtpos']                                          # ... after which the positions are set back
    rec = {k: [] for k in ('drawn', 'entry', 'walkers', 'turned', 'reentered')}
    for t in range(T):
        before_pos, before_dirs = h['pos'].copy(), h['dirs'].copy()
        walkers, leaves = _reaches(before_pos, before_dirs, st['vel']), _leaves(before_pos, before_dirs, st['vel'])
        entry = h['mtpos'].copy()
        native_sim.positions(h['keys'], h['mtpos'], h['pos'], h['dirs'], st['vel'], 0.01, LANES, WIDTH, HEIGHT)
        drawn = (h['mtpos'] - np.minimum(entry, 624)) % 624              # (none of these walks draws 624 words)
        native_sim.mt_uniforms(h['keys'], h['mtpos'], n_u)
        off_axis = (before_dirs < 2) != (h['dirs'] < 2)
        rec['drawn'].append(drawn)
        rec['entry'].append(entry)
        rec['walkers'].append(walkers)
        rec['turned'].append(walkers & off_axis & _inside(before_pos))
        rec['reentered'].append(~walkers & leaves & (h['dirs'] == np.vectorize(REENTRY.get)(before_dirs)))
    h.update({k: np.stack(v) for k, v in rec.items()})
    return h


# (axis, sign) -> lanes ahead that lie well inside the map with no other lane within 3.5 m before them
INNER = {(1, 1.0): (RIGHT[0], RIGHT[2]), (1, -1.0): (LEFT[3], LEFT[5]), (0, 1.0): (DOWN[0], DOWN[2]), (0, -1.0): (UP[3], UP[5])}


def _place_before_a_lane(st, e, v, rng):
    """vehicle v of state e half a velocity step before one of the INNER lanes ahead of it, 20 m or more from the map's edges"""
    d = int(st['dirs'][e, v])
    sg, ax, dv = (1.0 if d in (0, 3) else -1.0), (1 if d < 2 else 0), st['vel'][e, v] * 0.01
    st['pos'][e, v, ax] = INNER[(ax, sg)][int(rng.integers(0, 2))] - sg * 0.5 * dv
    st['pos'][e, v, 1 - ax] = 20.0 + float(rng.random()) * ((WIDTH, HEIGHT)[1 - ax] - 40.0)


# ------------------------------------------------------------------------------------------------------- one call, everything it leaves
def _run(dc, phase, T, explore, rand, storage, head, cap, eng):
    """one rollout_steps_recv of the form `phase` on dc -> every byte it leaves, by name"""
    import torch
    E, n = dc.E, dc.n
    res = dc.rollout_steps_recv(explore, rand, storage, head, cap, 1.0, 0.1, engine=eng, stream_phase=phase).resolve()
    torch.cuda.synchronize()
    out = {'resident ' + k: v for k, v in _bytes(dc, *RESIDENT).items()}
    out.update({'replay ' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
    io = dc.rollout_steps_recv_buffers(T)
    ws, offs = io['workspace'].cpu().numpy(), io['offsets']
    ends = [offs[k] for k in RECV_SECTIONS[1:]] + [offs['wide']]
    for k, end in zip(RECV_SECTIONS, ends):                              # the eight trajectory sections, padding included
        out['workspace ' + k] = ws[offs[k]:end].tobytes()
    w = wide_workspace_layout(E, n, RB, T)[0]
    out['workspace u_all'] = ws[offs['wide'] + w['u_all']:offs['wide'] + w['xy_all']].tobytes()
    out['workspace xy_all'] = ws[offs['wide'] + w['xy_all']:offs['wide'] + w['pl']].tobytes()
    out['result reward'], out['result flags'], out['result regular'] = res.reward.tobytes(), res.flags.tobytes(), res.regular.tobytes()
    assert res.reward.shape == (T, E) and res.flags.shape == (T, 2, E) and np.all(np.isfinite(res.reward))
    return out


def _assert_same(got, want, tag):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (tag, name)


def _both(E, n, T, st, eng, rng, head=None, own=False):
    """the chain call and the split call on twins of `st` -> (what each leaves, the two DeviceChannels)"""
    K = T * E
    cap = K + 3
    head = cap - max(1, min(K - 1, E * (T // 2) + 1)) if head is None else head          # a block that wraps the ring
    explore, rand = _policy(E, n, T, rng)
    if own:
        explore[:, 1] = 0                                                # the state with own-receiver links is greedy throughout
    out, dcs = {}, {}
    for phase in ('chain', 'split'):
        dcs[phase] = start_channels_recv(E, n, st)
        out[phase] = _run(dcs[phase], phase, T, explore, rand, _recv_storage(cap, n), head, cap, eng)
    assert dcs['chain'].stream_phase_calls == {'chain': 1, 'split': 0} and dcs['split'].stream_phase_calls == {'chain': 0, 'split': 1}
    assert dcs['chain'].walk_calls == dcs['split'].walk_calls == {'serial': 0, 'wide': 1}
    assert dcs['chain'].traffic == dcs['split'].traffic                  # the split workspace never crosses the bus
    io = dcs['split'].rollout_steps_recv_buffers(T)
    assert io['split_workspace'].numel() == split_workspace_layout(E, n, RB, T, 6)[1] and io['split_workspace'].data_ptr() % 256 == 0
    assert 'split_workspace' not in dcs['chain'].rollout_steps_recv_buffers(T)
    return out, dcs


# ------------------------------------------------------------------------------------------------------- (a) split == chain
SHAPES = [(3, 5, 3), (1, 20, 4), (2, 63, 3), (2, 64, 3), (2, 65, 3), (1, 127, 2), (1, 128, 3), (1, 40, 1)]


@pytest.mark.parametrize("E,n,T", SHAPES)
def test_the_split_call_leaves_every_byte_the_chain_call_leaves(E, n, T):
    """with a model (greedy and exploring states mixed) and without one; stream positions 0 / 623 / 624 rotating over the states.
    start_state puts most vehicles within four steps of a lane, and beyond 64 links vehicle 64 -- at 65 links the whole high
    half -- stands half a step before one: the host replay shows that the walks draw, in the high half too."""
    eng = _engine(n)
    rng = np.random.default_rng(100 * n + 10 * E + T)
    for variant, model in ((0, eng), (1, None)):
        st = start_state(E, n, 300 + n + variant, [(0, 623, 624)[(e + variant) % 3] for e in range(E)])
        for e in range(E if n > 64 else 0):
            _place_before_a_lane(st, e, 64, rng)
        h = _host_replay(st, n, T)
        assert np.all(h['drawn'].sum(axis=0) > 0) and (n <= 64 or h['walkers'][0, :, 64].all()), (variant, h['drawn'].tolist())
        out, dcs = _both(E, n, T, st, model, rng)
        _assert_same(out['split'], out['chain'], (variant, model is not None))
        for name in ('keys', 'mtpos', 'pos', 'dirs'):                    # ... and the streams and positions are the host library's
            assert dcs['split'].download(name).tobytes() == np.ascontiguousarray(h[name]).tobytes(), (variant, name)
    eng.close()


# ------------------------------------------------------------------------------------------------------- (b) the walk is exercised
def _busy_state(E, n, seed):
    """start_state with every vehicle but each fifth (those leave the map in step 1) placed half a velocity step before a lane
    well inside the map: all of them walk in step 0, far more than 64 words; who went straight meets the next lane 3.5 m on,
    23 steps later at the least, so the steps after that have few walkers or none"""
    st = start_state(E, n, seed, [623] + [5] * (E - 1))
    rng = np.random.default_rng(seed + 1)
    for e in range(E):
        for v in range(n):
            if v % 5 != 4:
                _place_before_a_lane(st, e, v, rng)
    return st


def test_both_halves_walk_turn_reload_the_chunk_rest_and_re_enter_alike_in_both_forms():
    """128 vehicles, E = 2, T = 4, seed 41.  Asserted from the host replay of the chain form's inputs before anything is compared
    (counts with this seed: 23 and 13 turns by vehicles of index >= 64 in step 0 of the two states, 20 and 21 by the others;
    103 walkers of both halves and 206 words in step 0 of either state, the chunk of 64 loaded four times; one walker in steps
    1 and 2 of state 0, none in step 3 and none in steps 1 to 3 of state 1; 25 re-entries in step 1 of either state, 13 of them
    in the high half)."""
    E, n, T = 2, 128, 4
    st = _busy_state(E, n, 41)
    h = _host_replay(st, n, T)
    print("turns by vehicles >= 64 per (step, state): %s; words drawn: %s; re-entries: %s"
          % (h['turned'][:, :, 64:].sum(axis=2).tolist(), h['drawn'].tolist(), h['reentered'].sum(axis=2).tolist()))
    assert h['turned'][:, :, 64:].any()                                  # 1. a turn by a vehicle of index >= 64
    assert np.any(h['walkers'][:, :, :64].any(axis=2) & h['walkers'][:, :, 64:].any(axis=2))     # 2. both halves draw in one step
    assert np.any((h['drawn'] == 0) & ~h['walkers'].any(axis=2))         # 3. a step with no walker
    assert np.any(h['drawn'] > 64)                                       # 4. off[t + 1] - off[t] - 2 n_u > 64: the chunk is reloaded
    assert h['reentered'].any() and h['reentered'][:, :, 64:].any()      # 5. a re-entry at the map edge, in the high half too
    assert h['turned'][:, :, :64].any() and np.all(h['drawn'] % 2 == 0)
    eng = _engine(n)
    out, dcs = _both(E, n, T, st, eng, np.random.default_rng(9))
    _assert_same(out['split'], out['chain'], 'busy')
    for name in ('keys', 'mtpos', 'pos', 'dirs'):
        assert dcs['chain'].download(name).tobytes() == np.ascontiguousarray(h[name]).tobytes(), name
    eng.close()


# ------------------------------------------------------------------------------------------------------- (c) stream positions at entry
@pytest.mark.parametrize("mtpos", [(0, 1, 623), (624, 9999, 1), (623, -7, 624)])
def test_every_entry_position_three_different_ones_in_one_call(mtpos):
    """n = 5: a step consumes 540 words and the walk's; T = 4 crosses at least three 624-word blocks.  A position outside
    [0, 624] reads as 624 (the block is used up), in both forms."""
    E, n, T = 3, 5, 4
    st = start_state(E, n, 77, list(mtpos))
    assert T * 2 * uniforms_per_step(n, RB) >= 3 * 624
    out, dcs = _both(E, n, T, st, None, np.random.default_rng(3))
    _assert_same(out['split'], out['chain'], mtpos)
    as_624 = dict(st, mtpos=np.array([p if 0 <= p <= 624 else 624 for p in mtpos], np.int32))
    ref, _ = _both(E, n, T, as_624, None, np.random.default_rng(3))
    _assert_same(out['split'], ref['chain'], (mtpos, 'read as 624'))
    h = _host_replay(as_624, n, T)
    assert dcs['split'].download('keys').tobytes() == h['keys'].tobytes() and np.array_equal(dcs['split'].download('mtpos'), h['mtpos'])


def test_a_stream_whose_last_consumed_word_is_the_last_of_a_block_leaves_position_624():
    E, n, T = 1, 5, 2
    found = None
    for p in range(625):                                                 # (host replays of two steps of five links: milliseconds)
        st = start_state(E, n, 303, [p])
        h = _host_replay(st, n, T)
        if h['mtpos'][0] == 624:
            found = (p, st, h)
            break
    assert found is not None, "no entry position of (1, 5, 2) ends the stream on a block boundary"
    p, st, h = found
    out, dcs = _both(E, n, T, st, None, np.random.default_rng(5), head=0)
    _assert_same(out['split'], out['chain'], p)
    assert int(dcs['split'].download('mtpos')[0]) == 624 and dcs['split'].download('keys').tobytes() == h['keys'].tobytes()


# ------------------------------------------------------------------------------------------------------- (d) continuation
@pytest.mark.parametrize("E,n,T", [(2, 65, 3), (3, 5, 3)])
def test_the_two_forms_continue_each_other(E, n, T):
    """split then chain and chain then split leave what chain then chain leaves: the key block and the position the split walk
    writes back are the chain form's"""
    K = T * E
    cap = 2 * K + 1
    st = start_state(E, n, 500 + n, [(620, 0, 624)[e % 3] for e in range(E)])
    eng = _engine(n)
    rng = np.random.default_rng(n)
    blocks = [_policy(E, n, T, rng) for _ in range(2)]
    runs = {}
    for order in (('chain', 'chain'), ('split', 'chain'), ('chain', 'split'), ('split', 'split')):
        dc, storage = start_channels_recv(E, n, st), _recv_storage(cap, n)
        for j, phase in enumerate(order):
            out = _run(dc, phase, T, blocks[j][0], blocks[j][1], storage, j * K, cap, eng)
        runs[order] = out
        assert dc.stream_phase_calls == {p: order.count(p) for p in ('chain', 'split')}
    for order in runs:
        _assert_same(runs[order], runs[('chain', 'chain')], order)
    eng.close()


# ------------------------------------------------------------------------------------------------------- (e) own-receiver states
def test_a_state_with_own_receiver_links_and_a_regular_state_at_33_links():
    E, n, T = 2, 33, 3
    st = start_state(E, n, 733, [623, 0])
    st['dest'][1, [0, 32]] = [0, 32]
    eng = _engine(n)
    out, dcs = _both(E, n, T, st, eng, np.random.default_rng(n), own=True)
    _assert_same(out['split'], out['chain'], 'own')
    assert dcs['split']._own[0].tolist() == [0, 2]                       # the batch took edge_base in both calls
    flags = np.frombuffer(out['split']['result flags'], np.uint8).reshape(T, 2, E)
    assert np.array_equal(flags, np.broadcast_to(np.array([0, 1], np.uint8), (T, 2, E)))
    eng.close()


# ------------------------------------------------------------------------------------------------------- (f) refusals
def test_a_refused_split_call_leaves_state_and_storage_alone():
    import torch
    E, n, T, cap = 2, 36, 2, 8
    lib = load_library()
    st = start_state(E, n, 77, [600, 610])
    dc = start_channels_recv(E, n, st)
    storage = _recv_storage(cap, n)

    def snapshot():
        torch.cuda.synchronize()
        snap = _bytes(dc, *RESIDENT)
        snap.update({'rep_' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
        return snap

    before = snapshot()
    ws = dc.rollout_steps_recv_buffers(T)['workspace']
    sws = dc._recv_split_workspace(T)
    assert sws.numel() == lib.v2x_rollout_recv_split_workspace_bytes(E, n, RB, T, 6)
    for split_ptr, split_bytes, word in ((None, sws.numel(), "split-stream workspace is null"),
                                         (sws.data_ptr(), sws.numel() - 256, "needs"),
                                         (sws.data_ptr() + 64, sws.numel(), "256-byte aligned")):
        r = dc.rollout_steps_recv_struct(T, storage, 0, cap, 1.0, 0.1)
        rc = lib.v2x_rollout_steps_recv_split(ctypes.byref(r), ws.data_ptr(), ws.numel(), split_ptr, split_bytes, dc._stream())
        text = lib.v2x_last_error(None).decode()
        assert rc == V2X_EINVAL and word in text and text.startswith("rollout_steps_recv_split"), (word, rc, text)
        assert snapshot() == before, word
    for k, v in storage.items():
        assert (v == MARK).all(), k


# ------------------------------------------------------------------------------------------------------- (g) the agent
def _trained(E, streams, steps=3):
    import random
    seed = 17 + E
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(40, E, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 16, 1, 0.1)
    agent = Agent(40, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay='receivers', rollout_backend='trajectory',
                  receiver_streams=streams)
    assert type(env) is DeviceBatchedEnviron and type(agent.device_replay) is ReceiverReplay
    out = agent.train(1, steps)
    rep = agent.device_replay
    run = {'losses': out[0].tobytes(), 'rewards per step': out[1].tobytes(), 'weights': agent.brain.model.engine.get_flat().tobytes(),
           'size': (rep.size, rep.head, agent.num_step)}
    for k in ('xe', 'xe_next', 'recv', 'action', 'reward'):
        run['replay ' + k] = getattr(rep, k)[:rep.size].cpu().numpy().tobytes()
    calls = dict(env.device_channels.stream_phase_calls)
    assert np.isfinite(out[0]).all()
    agent.brain.close()
    return run, calls


@pytest.mark.parametrize("E", [1, 3])
def test_agent_with_the_split_stream_phase_is_the_agent_with_the_chain_form(E):
    chain, chain_calls = _trained(E, 'chain')
    split, split_calls = _trained(E, 'split')
    assert chain_calls == {'chain': 3, 'split': 0} and split_calls == {'chain': 0, 'split': 3}
    _assert_same(split, chain, E)
    assert chain['size'][0] == 3 * -(-50 // E) * E
