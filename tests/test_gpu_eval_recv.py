"""GPU: an evaluation episode of 3..128 links on the receiver-form resident state (v2x_eval_steps_recv / _split: the front of
the receiver-form rollout -- wide walk in chain or split form, k_traj_observe_recv, v2x_csr_from_recv, one forward -- and
k_eval_finish_recv; DeviceChannels.eval_steps_recv, DeviceBatchedEnviron.evaluate_steps beyond 31 links, Agent.test_run with
eval_backend='device').  Every comparison is byte for byte.  Up to 31 links the reference is the existing call
(v2x_eval_steps_wide); beyond them the single-step device calls that already serve 128 links (v2x_sim_stream, v2x_sim_channels,
v2x_sim_rates), the host library's observation, the host packer and the engine's forward, and for the agent the host loop on a
twin environment with the same seeds.  The engine scores 4 channels: rb = 4 throughout."""
import ctypes
import functools
import random

import numpy as np
import pytest

from test_gpu_rollout_recv import RB, SHARED, WALKED, _adjacency, _bytes, _host_observation, _policy, start_channels_recv
from test_gpu_rollout_trajectory import _engine, _same_rng, start_channels, start_state
from v2xgnn import PackedBatch
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.device_sim import FLAG_OWN, RECV_SECTIONS, EvalResult, RecvEvalResult, eval_result_layout
from v2xgnn.rl.optimum import OptimalAllocation
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

W_V2V, W_V2I = 1.0, 0.1
MARK = 7
RATES = ('v2v_rate', 'v2i_rate', 'interference')
SECTIONS = RATES + ('reward', 'actions')
RESIDENT = WALKED + ('interf_db', 'state', 'xe', 'recv', 'flags', 'v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf',
                     'actions')


def _left(dc, T, res=None):
    """every byte an evaluation call of block length T left on dc, by name: the result block on the device (whole, padding
    included), the resident tensors, the first eight workspace sections (padding included), and the resolved result"""
    import torch
    torch.cuda.synchronize()
    io = dc.eval_steps_recv_buffers(T)
    out = {'resident ' + k: v for k, v in _bytes(dc, *RESIDENT).items()}
    out['result block'] = io['eval_result_dev'].cpu().numpy().tobytes()
    ws, offs = io['workspace'].cpu().numpy(), io['offsets']
    ends = [offs[k] for k in RECV_SECTIONS[1:]] + [offs['wide']]
    for k, end in zip(RECV_SECTIONS, ends):
        out['workspace ' + k] = ws[offs[k]:end].tobytes()
    if res is not None:
        for k in SECTIONS + ('flags', 'regular'):
            out['result ' + k] = getattr(res, k).tobytes()
    return out


def _assert_same(got, want, tag):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (tag, name)


# ------------------------------------------------------------------------------ (a) up to 31 links: the existing call
@pytest.mark.parametrize("E,n,T", [(3, 5, 3), (1, 20, 4)])
def test_receiver_form_up_to_31_links_is_the_existing_wide_call(E, n, T):
    rng = np.random.default_rng(10 * n + E)
    st = start_state(E, n, 500 + n, [(0, 623, 624)[e % 3] for e in range(E)])
    explore, rand = _policy(E, n, T, rng)
    baseline = rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    eng = _engine(n)
    old_dc, new_dc = start_channels(E, n, RB, st), start_channels_recv(E, n, st)
    old = old_dc.eval_steps(explore, rand, baseline, W_V2V, W_V2I, engine=eng, walk='wide').resolve()
    new = new_dc.eval_steps_recv(explore, rand, baseline, W_V2V, W_V2I, engine=eng).resolve()
    assert type(old) is EvalResult and type(new) is RecvEvalResult
    for k in SECTIONS:
        a, b = getattr(old, k), getattr(new, k)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert new.actions.shape == (2, T, E, n) and np.all(np.isfinite(new.reward)) and np.array_equal(new.actions[1], baseline)
    assert new.flags.shape == (T + 1, E) and new.flags.dtype == np.uint8 and not new.flags.any()
    assert np.array_equal(new.regular, new.flags == 0) and np.array_equal(new.regular, old.regular)
    a, b = _bytes(old_dc, *SHARED), _bytes(new_dc, *SHARED)
    for k in SHARED:
        assert a[k] == b[k], k
    assert np.array_equal(new_dc.download('recv'), st['dest']) and not new_dc.download('flags').any()
    assert new_dc.walk_calls == {'serial': 0, 'wide': 1} and new_dc.stream_phase_calls == {'chain': 1, 'split': 0}
    # the snapshots of either form are one stacked problem with the same channels
    po, pn = old_dc.trajectory_states(T).problem_tensors()[0], new_dc.trajectory_states(T).problem_tensors()[0]
    for x, y in zip(po, pn):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    eng.close()


# ------------------------------------------------------------------------------ (b) beyond 31 links
@pytest.mark.parametrize("n", [32, 33, 60, 61, 64, 65, 128])
def test_one_call_beyond_31_links_is_the_single_step_calls_the_host_observation_and_the_engine(n):
    """n + rb = 64 | 65 rate threads at 60 | 61 links (one wave and one thread past it: k_eval_finish_recv's second wave), the
    wave boundary of the 128-thread observation at 64 | 65, the limits 32 and 128.  33 links: state 1 has own-receiver links
    and is greedy at every step."""
    import torch
    E, T = 2, 3
    K = T * E
    rng = np.random.default_rng(n)
    st = start_state(E, n, 700 + n, [623, 0])
    if n == 33:
        st['dest'][1, [0, 32]] = [0, 32]
    explore, rand = _policy(E, n, T, rng)
    if n == 33:
        explore[:, 1] = 0
    baseline = rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    eng = _engine(n)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    res = A.eval_steps_recv(explore, rand, baseline, W_V2V, W_V2I, engine=eng).resolve()
    assert res.actions.shape == (2, T, E, n) and res.reward.shape == (2, T, E) and res.v2i_rate.shape == (2, T, E, RB)
    assert np.array_equal(res.actions[1], baseline)                      # the baseline's actions are the uploaded ones
    io = A.eval_steps_recv_buffers(T)
    o = io['offsets']['traj_xe']
    traj_xe = io['workspace'][o:o + 4 * (T + 1) * E * n * 16].view(torch.float32).cpu().numpy().reshape(T + 1, E, n, 16)
    adj = _adjacency(st['dest'])
    states = []
    for t in range(T):
        state, xe, adj_t = _host_observation(B, st['dest'])
        assert np.array_equal(adj_t, adj) and traj_xe[t].tobytes() == xe.tobytes(), ('entry', t)
        states.append(state)
        for s in (1, 0):                                                 # the baseline first: the policy's rates stay resident
            B.rates(res.actions[s, t])
            r = B.fetch_rates()
            for k in RATES:
                assert getattr(res, k)[s, t].tobytes() == r[k].reshape(getattr(res, k)[s, t].shape).tobytes(), (k, s, t)
            reward = W_V2V * r['v2v_rate'].reshape(E, n, 1).sum(axis=(1, 2)) + W_V2I * r['v2i_rate'].sum(axis=1)
            assert res.reward[s, t].tobytes() == reward.tobytes(), ('reward', s, t)
        B.stream(mobility=True)
        B.step(B.tensor('u'))
    assert np.all(np.isfinite(res.reward)) and len(set(res.reward.reshape(-1).tolist())) == 2 * K
    _, xe, _ = _host_observation(B, st['dest'])
    assert traj_xe[T].tobytes() == xe.tobytes()
    # the policy's picks: the uploaded draws where a state explores, elsewhere the first maximiser of the engine's Q-values
    all_states = np.concatenate(states)                                  # [T E, n, 13], t major
    q = eng.forward(PackedBatch.from_dense(all_states[:, :, :9].astype(np.float32), all_states[:, :, 9:].astype(np.float32),
                                           np.tile(adj, (T, 1, 1)))).reshape(T, E, n, RB)
    assert np.array_equal(res.actions[0], np.where(explore[:, :, None] != 0, rand, np.argmax(q, axis=3)))
    assert (explore == 0).any(axis=1).all() and not np.array_equal(res.actions[0], rand)
    # the flags of entries 0..T
    own = (st['dest'] == np.arange(n)).sum(axis=1)
    assert res.flags.shape == (T + 1, E) and np.array_equal(res.flags, np.broadcast_to((own > 0).astype(np.uint8) * FLAG_OWN, (T + 1, E)))
    assert np.array_equal(res.regular, res.flags == 0) and (n != 33 or own.tolist() == [0, 2])
    # the resident state: the twin advanced T times under the policy's actions
    B.observe_recv()
    a, b = _bytes(A, *RESIDENT), _bytes(B, *RESIDENT)
    for k in RESIDENT:
        assert a[k] == b[k], k
    # the snapshots as one stacked problem: its rates() of either scheme's actions are the result rows
    ts = A.trajectory_states(T)
    assert (ts.E, ts.n_Veh, ts.n_RB) == (K, n, RB)
    for s in (0, 1):
        got = ts.rates(res.actions[s].reshape(K, n))
        for k, g in zip(RATES, got):
            assert g.tobytes() == getattr(res, k)[s].tobytes(), (k, s)
    eng.close()


# ------------------------------------------------------------------------------ (c) one scheme, no engine
def test_one_scheme_without_an_engine_reads_no_q_and_writes_the_one_scheme_layout_only():
    import torch
    E, n, T = 2, 61, 3
    K = T * E
    rng = np.random.default_rng(5)
    st = start_state(E, n, 761, [623, 0])
    explore, rand = np.ones((T, E), np.uint8), rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    baseline = rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    io = A.eval_steps_recv_buffers(T)
    io['q'].fill_(float('nan'))
    io['eval_result_dev'].fill_(MARK)
    one = A.eval_steps_recv(explore, rand, None, W_V2V, W_V2I, engine=None).resolve()
    assert one.schemes == 1 and one.actions.shape == (1, T, E, n) and one.reward.shape == (1, T, E) and one.flags.shape == (T + 1, E)
    assert np.array_equal(one.actions[0], rand) and np.all(np.isfinite(one.reward)) and np.all(np.isfinite(one.v2v_rate))
    offs, size = eval_result_layout(E, n, RB, T, 1)
    end = offs['regular'] + (T + 1) * E                                  # the last byte of the S = 1 layout, before its padding
    block = io['eval_result_dev'].cpu().numpy()
    assert size < block.size and (block[end:] == MARK).all() and not (block[offs['regular']:end] == MARK).any()
    assert torch.isnan(io['q']).all()                                    # nobody was greedy: q was neither read nor written
    # the two-scheme call on a twin: its policy scheme is this one, its baseline the uploaded actions
    two = B.eval_steps_recv(explore, rand, baseline, W_V2V, W_V2I, engine=None).resolve()
    for k in SECTIONS:
        assert getattr(two, k)[0].tobytes() == getattr(one, k)[0].tobytes(), k
    assert np.array_equal(two.actions[1], baseline) and np.array_equal(two.flags, one.flags)
    assert not np.array_equal(two.reward[1], two.reward[0])
    a, b = _bytes(A, *RESIDENT), _bytes(B, *RESIDENT)
    for k in RESIDENT:
        assert a[k] == b[k], k
    assert A.traffic['bytes_down'] < B.traffic['bytes_down']             # one scheme's block came down, not two


# ------------------------------------------------------------------------------ (d) split is chain
def _eval(dc, phase, T, explore, rand, baseline, eng):
    res = dc.eval_steps_recv(explore, rand, baseline, W_V2V, W_V2I, engine=eng, stream_phase=phase).resolve()
    return _left(dc, T, res)


@pytest.mark.parametrize("E,n", [(2, 33), (2, 65), (2, 128), (3, 40)])
def test_the_split_call_leaves_every_byte_the_chain_call_leaves(E, n):
    T = 4
    rng = np.random.default_rng(3 * n + E)
    st = start_state(E, n, 800 + n, [(623, 0, 624)[e % 3] for e in range(E)])
    if n == 33:
        st['dest'][1, [0, 32]] = [0, 32]
    explore, rand = _policy(E, n, T, rng)
    baseline = rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    eng = _engine(n)
    out, dcs = {}, {}
    for phase in ('chain', 'split'):
        dcs[phase] = start_channels_recv(E, n, st)
        out[phase] = _eval(dcs[phase], phase, T, explore, rand, baseline, eng)
    _assert_same(out['split'], out['chain'], (E, n))
    assert dcs['chain'].stream_phase_calls == {'chain': 1, 'split': 0} and dcs['split'].stream_phase_calls == {'chain': 0, 'split': 1}
    assert dcs['chain'].walk_calls == dcs['split'].walk_calls == {'serial': 0, 'wide': 1}
    assert dcs['chain'].traffic == dcs['split'].traffic                  # the split workspace never crosses the bus
    assert 'split_workspace' in dcs['split'].eval_steps_recv_buffers(T) and 'split_workspace' not in dcs['chain'].eval_steps_recv_buffers(T)
    eng.close()


def test_a_chain_call_and_a_split_call_continue_each_other_on_one_state():
    E, n, T = 2, 36, 3
    rng = np.random.default_rng(36)
    st = start_state(E, n, 836, [623, 0])
    draws = [(_policy(E, n, T, rng), rng.integers(0, RB, size=(T, E, n)).astype(np.int32)) for _ in range(2)]
    eng = _engine(n)
    left = {}
    for forms in (('chain', 'chain'), ('chain', 'split')):
        dc = start_channels_recv(E, n, st)
        for phase, ((explore, rand), baseline) in zip(forms, draws):
            left[forms] = _eval(dc, phase, T, explore, rand, baseline, eng)
        assert dc.walk_calls['wide'] == 2 and dc.stream_phase_calls['chain'] + dc.stream_phase_calls['split'] == 2
    _assert_same(left[('chain', 'split')], left[('chain', 'chain')], 'continued')
    eng.close()


# ------------------------------------------------------------------------------ (e) refusals before the first launch
def test_a_refused_call_leaves_the_state_and_the_result_block_alone():
    E, n, T = 2, 36, 2
    lib = load_library()
    st = start_state(E, n, 77, [600, 610])
    dc = start_channels_recv(E, n, st)
    io = dc.eval_steps_recv_buffers(T)
    io['eval_result_dev'].fill_(MARK)
    before = _left(dc, T)
    ws = io['workspace']
    sws = dc._recv_split_workspace(T)

    def call(change, split=False, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), sws_ptr=sws.data_ptr(), sws_bytes=sws.numel()):
        r = dc.eval_steps_recv_struct(T, W_V2V, W_V2I)
        change(r)
        if split:
            rc = lib.v2x_eval_steps_recv_split(ctypes.byref(r), ws_ptr, ws_bytes, sws_ptr, sws_bytes, dc._stream())
        else:
            rc = lib.v2x_eval_steps_recv(ctypes.byref(r), ws_ptr, ws_bytes, dc._stream())
        return rc, lib.v2x_last_error(None).decode()

    def links(v):
        def change(r):
            r.step.problem.n = v
        return change

    same = lambda r: None                                                # noqa: E731
    cases = [(links(129), {}, "n = 129"), (links(2), {}, "n = 2"), (lambda r: setattr(r, 'T', 0), {}, "T = 0"),
             (same, dict(ws_bytes=ws.numel() - 256), "needs"), (lambda r: setattr(r, 'traj_recv', r.traj_xe), {}, "first eight sections"),
             (lambda r: setattr(r, 'result_reward', None), {}, "null result"), (lambda r: (setattr(r, 'model', 1), setattr(r, 'q', None)), {}, "a model needs the Q workspace"),
             (same, dict(split=True, sws_ptr=None), "split-stream workspace is null"),
             (same, dict(split=True, sws_ptr=sws.data_ptr() + 64), "256-byte aligned"),
             (same, dict(split=True, sws_bytes=sws.numel() - 256), "split-stream workspace of")]
    for change, kw, word in cases:
        rc, text = call(change, **kw)
        assert rc == V2X_EINVAL and word in text, (word, rc, text)
        assert _left(dc, T) == before, word
    # ... and the Python layer refuses a state whose receivers it has seen to be out of range
    bad = st['dest'].copy()
    bad[0, 3] = n
    dc.observe_recv(bad)
    with pytest.raises(ValueError, match="receiver outside"):
        dc.eval_steps_recv(np.ones((T, E), np.uint8), np.zeros((T, E, n), np.int32), None, W_V2V, W_V2I)


# ------------------------------------------------------------------------------ (f)-(h) the agent
def _agent(n, seed, own=(), **kw):
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, 1, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay=False, **kw)       # an untrained, seeded brain
    assert type(env) is DeviceBatchedEnviron
    if len(own):                                                         # after every reset: links that are their own receiver
        inner = env.new_random_game

        def reset(n_Veh=0):
            inner(n_Veh)
            env.dest[0, list(own)] = list(own)
            env._static_dirty = True
            env._dev_obs = None
        env.new_random_game = reset
    return env, agent


def _run(n, seed, backend, episodes, steps, own=(), opt=None, **kw):
    """test_run on a fresh seeded agent -> what it returned and left, with the host calls it made, the observations its host
    loop scored (one-graph forwards) and the local searches it ran"""
    env, agent = _agent(n, seed, own, **kw)
    host_calls, resident, scored, searches = [], [], [], []
    for obj, name in ((agent, '_predict'), (env, 'act'), (env, 'observe')):
        inner = getattr(obj, name)
        setattr(obj, name, (lambda inner, name: lambda *a, **k: (host_calls.append(name), inner(*a, **k))[1])(inner, name))
    predict = agent._predict
    agent._predict = lambda s, a, **k: (lambda q: (scored.append((np.array(s), np.array(a), np.array(q))), q)[1])(predict(s, a, **k))
    inner_eval = env.evaluate_steps
    env.evaluate_steps = lambda ex, *a, **k: (resident.append((np.shape(ex), k.get('walk'), k.get('stream_phase'))), inner_eval(ex, *a, **k))[1]
    inner_search = OptimalAllocation.search_local

    def search(self, *a, **k):
        out = inner_search(self, *a, **k)
        searches.append((np.array(out[0]), np.array(out[1])))
        return out
    OptimalAllocation.search_local = search
    try:
        out = agent.test_run(episodes, steps, opt is not None, eval_backend=backend,
                             **(dict(opt_backend='local', opt_restarts=opt) if opt is not None else {}))
    finally:
        OptimalAllocation.search_local = inner_search
    run = dict(out=[np.asarray(a).copy() for a in out], rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step,
               streams=[np.array(a).copy() for a in (env._mt_keys, env._mt_pos, env.pos, env.dirs)], stats=dict(agent.eval_stats),
               host_calls=list(host_calls), resident=list(resident), scored=scored, searches=searches, dest=np.array(env.dest),
               calls=dict(env.device_channels.walk_calls), phases=dict(env.device_channels.stream_phase_calls))
    if scored:                                                           # the five-graph forward of what the host loop scored one by one
        last = scored[-steps:]
        run['q_stacked'] = np.array(predict(np.concatenate([s for s, _, _ in last]), np.concatenate([a for _, a, _ in last])))
        run['q_single'] = np.concatenate([q for _, _, q in last], axis=1)
    if backend == 'device':                                              # the last episode's snapshots and observations, as left
        ts = env.trajectory_states(steps)
        io = env.device_channels.eval_steps_recv_buffers(steps)
        xe = io['xe'].cpu().numpy().reshape(steps, n, 16)[:, :, :13].astype(np.float64)
        adj = np.tile(_adjacency(np.array(env.dest)), (steps, 1, 1))
        q = np.array(predict(xe, adj))                                   # [n, T, C]: the five-graph Q-values of the device's observations
        acts = np.argmax(q, axis=2).T.astype(np.int64)                   # [T, n]
        run['requoted'] = ts.rates(acts)
    agent.brain.close()
    return run


@functools.lru_cache(maxsize=None)
def _host40():
    return _run(40, 41, 'host', 2, 5)


@functools.lru_cache(maxsize=None)
def _device40(stream):
    return _run(40, 41, 'device', 2, 5, **({} if stream == 'chain' else dict(receiver_streams=stream)))


def _runs40(stream='chain'):
    """test_run(2, 5) at 40 links, E = 1, on twins with the same seeds: the host loop and the device episodes (computed once)"""
    return _host40(), _device40(stream)


def _assert_same_walk(h, d, episodes):
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] > 0
    for a, b in zip(h['streams'], d['streams']):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert d['stats'] == {'device_episodes': episodes, 'host_episodes': 0}      # no fallback
    assert h['stats'] == {'device_episodes': 0, 'host_episodes': episodes}


@pytest.mark.parametrize("stream", ['chain', 'split'])
def test_test_run_at_40_links_on_the_device_books_the_random_scheme_of_the_host_loop(stream):
    """the channels do not depend on the actions, so the random scheme's books are the host loop's whatever the network says"""
    h, d = _runs40(stream)
    assert len(h['out']) == len(d['out']) == 10
    for i in range(5, 10):                                               # the `ra` books: return, reward, V2V rates, V2I rates, interference
        assert h['out'][i].shape == d['out'][i].shape and h['out'][i].tobytes() == d['out'][i].tobytes(), i
        assert np.all(np.isfinite(d['out'][i])), i
    assert len(set(d['out'][6].reshape(-1).tolist())) == 10
    _assert_same_walk(h, d, 2)
    assert d['host_calls'] == [] and d['resident'] == [((5, 1), 'wide', stream)] * 2
    assert d['calls'] == {'serial': 0, 'wide': 2} and d['phases'][stream] == 2 and sum(d['phases'].values()) == 2
    assert h['host_calls'].count('_predict') == 10 and h['host_calls'].count('act') == 10 and h['resident'] == []


def test_test_run_at_40_links_on_the_device_books_the_policy_scheme_of_the_host_loop():
    """The host loop scores one graph per step, the device call all five at once.  Where the engine's one-graph forwards are its
    five-graph forward byte for byte (what the tests up to 31 links rely on) the `rl` books must be the host loop's bit for bit;
    where they are not, the rows that differ are named and the device's books must be those recomputed from the five-graph
    Q-values on the call's own snapshots."""
    h, d = _runs40()
    single, stacked = h['q_single'], h['q_stacked']                      # [n, 5, C] each
    assert single.shape == stacked.shape == (40, 5, 4)
    differ = np.argwhere((single.view(np.uint32) != stacked.view(np.uint32)).any(axis=2))
    print("one-graph against five-graph forward at 40 links: %d of %d (link, step) rows differ" % (len(differ), 40 * 5))
    if len(differ) == 0:
        for i in range(5):                                               # the `rl` books
            assert h['out'][i].tobytes() == d['out'][i].tobytes(), i
    else:
        v2v, v2i, intf = d['requoted']
        want = [W_V2V * np.sum(v2v[t][:, None]) + W_V2I * np.sum(v2i[t]) for t in range(5)]
        assert d['out'][1][-1].tobytes() == np.array(want).tobytes(), \
            "one-graph and five-graph forwards differ in (link, step) rows %s" % differ.tolist()
        assert d['out'][2][-1].tobytes() == v2v.tobytes() and d['out'][3][-1].tobytes() == v2i.tobytes()
        assert d['out'][4][-1].tobytes() == intf.tobytes()
    assert np.all(np.isfinite(d['out'][1])) and len(set(d['out'][1].reshape(-1).tolist())) == 10


def test_own_receiver_links_run_on_the_device_and_the_stacked_local_search_is_the_host_loops():
    """36 links (the simulator places vehicles in groups of four: the nearest size above 33) with links 2 and 35 their own
    receivers after every reset: the episode runs on the device, and the multi-start local search over the stacked snapshots
    (8 restarts, seeded by restart and link alone) returns per snapshot the allocation and reward the host loop's single-state
    searches return -- rewards_of() of the allocation on the snapshot, which is what search_local hands back."""
    own = (2, 35)
    h = _run(36, 43, 'host', 2, 3, own=own, opt=8)
    d = _run(36, 43, 'device', 2, 3, own=own, opt=8)
    assert np.array_equal(d['dest'][0, list(own)], own) and np.array_equal(h['dest'], d['dest'])
    _assert_same_walk(h, d, 2)
    assert d['host_calls'] == [] and d['resident'] == [((3, 1), 'wide', 'chain')] * 2
    assert len(h['searches']) == 6 and len(d['searches']) == 2           # one search per step | one stacked search per episode
    for ep in range(2):
        acts, rewards = d['searches'][ep]
        assert acts.shape == (3, 36) and rewards.shape == (3,)
        for t in range(3):
            a, r = h['searches'][3 * ep + t]
            assert np.array_equal(a[0], acts[t]) and r.tobytes() == rewards[t:t + 1].tobytes(), (ep, t)
    assert len(h['out']) == len(d['out']) == 15
    for i in range(5, 15):                                               # the `ra` and the `opt` books
        assert h['out'][i].tobytes() == d['out'][i].tobytes(), i
    assert np.all(d['out'][11] > 0) and np.all(np.isfinite(d['out'][11]))
