"""GPU: K networks scored on the same walked episode of 3..128 links on the receiver-form resident state (v2x_eval_sweep_recv /
_split: the front of v2x_eval_steps_recv once, K - 1 further forwards of the one batch, k_eval_finish_sweep_recv;
DeviceChannels.eval_sweep_recv, DeviceBatchedEnviron.evaluate_sweep, Agent.evaluate_training_sweep(eval_backend='device')).
Every comparison is byte for byte.  The reference is v2x_eval_steps_recv with one network at a time on a twin holding the same
state, and for the agent the host definition (Agent.evaluate_training_sweep(eval_backend='host')) on a twin environment with
the same seeds.  The engine scores 4 channels: rb = 4 throughout; T is 1..4 and K at most 3."""
import ctypes
import os
import random

import numpy as np
import pytest

from test_gpu_eval_recv import MARK, RESIDENT, SECTIONS, W_V2I, W_V2V, _agent
from test_gpu_rollout_recv import RB, WALKED, _bytes, _policy, start_channels_recv
from test_gpu_rollout_trajectory import _engine, _same_rng, start_state
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl.device_sim import RECV_SECTIONS, RecvEvalResult, eval_result_layout

pytestmark = pytest.mark.gpu


def _engines(n, K, first=5):
    return [_engine(n, first + k) for k in range(K)]


def _close(engines):
    for e in engines:
        e.close()


def _left(dc, T, res=None, block=None):
    """every byte a call of block length T left on dc, by name: the resident tensors, the first eight workspace sections
    (padding included), the resolved result, and `block` (a result block on the device, whole)"""
    import torch
    torch.cuda.synchronize()
    io = dc.eval_steps_recv_buffers(T)
    out = {'resident ' + k: v for k, v in _bytes(dc, *RESIDENT).items()}
    ws, offs = io['workspace'].cpu().numpy(), io['offsets']
    ends = [offs[k] for k in RECV_SECTIONS[1:]] + [offs['wide']]
    for k, end in zip(RECV_SECTIONS, ends):
        out['workspace ' + k] = ws[offs[k]:end].tobytes()
    if res is not None:
        for k in SECTIONS + ('flags', 'regular'):
            out['result ' + k] = getattr(res, k).tobytes()
    if block is not None:
        out['result block'] = block.cpu().numpy().tobytes()
    return out


def _assert_same(got, want, tag, skip=()):
    assert sorted(got) == sorted(want)
    for name in want:
        if not name.startswith(skip or ('\0',)):
            assert got[name] == want[name], (tag, name)


def _assert_is_the_single_calls(sweep, singles, K, baseline, tag):
    """scheme k of the sweep is scheme 0 of single call k, scheme K their scheme 1, the flags theirs"""
    assert type(sweep) is RecvEvalResult and sweep.schemes == K + (1 if baseline else 0)
    for k, one in enumerate(singles):
        for name in SECTIONS:
            a, b = getattr(sweep, name)[k], getattr(one, name)[0]
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, name, 'network', k)
        assert sweep.flags.tobytes() == one.flags.tobytes(), (tag, 'flags', k)
    if baseline:
        for name in SECTIONS:
            assert getattr(sweep, name)[K].tobytes() == getattr(singles[-1], name)[1].tobytes(), (tag, name, 'baseline')
    assert np.all(np.isfinite(sweep.reward))


def _case(E, n, T, K, seed, own=False, greedy=None, baseline=True, phase='chain'):
    rng = np.random.default_rng(seed)
    st = start_state(E, n, 900 + n, [(623, 0, 624)[e % 3] for e in range(E)])
    if own:                                                              # the last state: links 0 and n - 1 their own receivers
        st['dest'][E - 1, [0, n - 1]] = [0, n - 1]
    explore, rand = _policy(E, n, T, rng)
    if own:
        explore[:, E - 1] = 0
    if greedy is not None:
        explore[:] = 0 if greedy else 1
    base = rng.integers(0, RB, size=(T, E, n)).astype(np.int32) if baseline else None
    return st, explore, rand, base


def _singles(E, n, T, st, explore, rand, base, engines, phase='chain'):
    """v2x_eval_steps_recv with engine k on a twin of the state, for every k -> (results, what the last call left)"""
    out, left = [], None
    for eng in engines:
        dc = start_channels_recv(E, n, st)
        res = dc.eval_steps_recv(explore, rand, base, W_V2V, W_V2I, engine=eng, stream_phase=phase).resolve()
        out.append(res)
        left = _left(dc, T)
    return out, left


# ------------------------------------------------------------------------------ (a) the sweep is K single calls from one state
@pytest.mark.parametrize("E,n", [(2, 5), (1, 33), (2, 65), (1, 128)])
def test_the_sweep_is_k_single_calls_from_the_same_state(E, n):
    """below the form switch, the first size past a 32-bit mask, past one wave of links, the maximum (n + rb = 132 of the 192
    threads compute a rate)"""
    T, K = 3, 3
    st, explore, rand, base = _case(E, n, T, K, 11 * n + E)
    engines = _engines(n, K)
    singles, left_last = _singles(E, n, T, st, explore, rand, base, engines)
    dc = start_channels_recv(E, n, st)
    sweep = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines).resolve()
    assert sweep.actions.shape == (K + 1, T, E, n) and np.array_equal(sweep.actions[K], base)
    _assert_is_the_single_calls(sweep, singles, K, True, (E, n))
    # the networks differ, at the last step too: the resident actions tell network K - 1 from the others
    picks = [s.actions[0] for s in singles]
    assert not np.array_equal(picks[0], picks[K - 1]) and not np.array_equal(picks[1], picks[K - 1])
    assert not np.array_equal(picks[0][T - 1], picks[K - 1][T - 1]) and (explore[T - 1] == 0).any()
    _assert_same(_left(dc, T), left_last, (E, n))
    assert np.array_equal(np.asarray(dc.download('actions')).reshape(E, n), picks[K - 1][T - 1])
    assert dc.walk_calls == {'serial': 0, 'wide': 1} and dc.stream_phase_calls == {'chain': 1, 'split': 0}
    # the snapshots serve the stacked search: rates() of any scheme's actions on them are that scheme's rows
    ts = dc.trajectory_states(T)
    assert (ts.E, ts.n_Veh, ts.n_RB) == (T * E, n, RB)
    for s in (0, K - 1, K):
        for name, got in zip(('v2v_rate', 'v2i_rate', 'interference'), ts.rates(sweep.actions[s].reshape(T * E, n))):
            assert got.tobytes() == getattr(sweep, name)[s].tobytes(), (name, s)
    _close(engines)


# ------------------------------------------------------------------------------ (b) K = 1 is the single call outright
def test_one_network_is_the_single_call_result_block_included():
    E, n, T = 2, 33, 3
    st, explore, rand, base = _case(E, n, T, 1, 33)
    engines = _engines(n, 1)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    one = A.eval_steps_recv(explore, rand, base, W_V2V, W_V2I, engine=engines[0]).resolve()
    got = B.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines).resolve()
    _, sw, q = B._recv_sweep_io(T, 2, 1)
    want = _left(A, T, one, A.eval_steps_recv_buffers(T)['eval_result_dev'])
    _assert_same(_left(B, T, got, sw['dev']), want, 'K = 1')
    assert q.shape == (1, T * E * n, RB) and q[0].cpu().numpy().tobytes() == A.eval_steps_recv_buffers(T)['q'].cpu().numpy().tobytes()
    assert A.traffic == B.traffic
    _close(engines)


# ------------------------------------------------------------------------------ (c) own-receiver links (the edge_base path)
def test_own_receiver_links_are_swept_like_the_others():
    E, n, T, K = 2, 33, 3, 2
    st, explore, rand, base = _case(E, n, T, K, 34, own=True)
    assert (st['dest'][1] == np.arange(n)).sum() == 2 and not (st['dest'][0] == np.arange(n)).any()
    engines = _engines(n, K)
    singles, left_last = _singles(E, n, T, st, explore, rand, base, engines)
    dc = start_channels_recv(E, n, st)
    sweep = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines).resolve()
    _assert_is_the_single_calls(sweep, singles, K, True, 'own')
    _assert_same(_left(dc, T), left_last, 'own')
    assert sweep.flags[:, 1].all() and not sweep.flags[:, 0].any()
    assert not np.array_equal(singles[0].actions[0][:, 1], singles[1].actions[0][:, 1])     # the irregular state is scored, per network
    _close(engines)


# ------------------------------------------------------------------------------ (d) shapes
def test_one_step():
    E, n, T, K = 1, 33, 1, 2
    st, explore, rand, base = _case(E, n, T, K, 35, greedy=True)
    engines = _engines(n, K)
    singles, left_last = _singles(E, n, T, st, explore, rand, base, engines)
    dc = start_channels_recv(E, n, st)
    sweep = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines).resolve()
    assert sweep.reward.shape == (K + 1, 1, 1) and sweep.flags.shape == (2, 1)
    _assert_is_the_single_calls(sweep, singles, K, True, 'T = 1')
    _assert_same(_left(dc, T), left_last, 'T = 1')
    _close(engines)


def test_everybody_greedy():
    E, n, T, K = 2, 36, 2, 3
    st, explore, rand, base = _case(E, n, T, K, 36, greedy=True)
    engines = _engines(n, K)
    singles, left_last = _singles(E, n, T, st, explore, rand, base, engines)
    dc = start_channels_recv(E, n, st)
    sweep = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines).resolve()
    _assert_is_the_single_calls(sweep, singles, K, True, 'greedy')
    _assert_same(_left(dc, T), left_last, 'greedy')
    assert not any(np.array_equal(sweep.actions[k], rand) for k in range(K))
    _close(engines)


def test_no_baseline_writes_the_layout_of_k_schemes_only():
    """S = K: the call is made on a marker-filled block larger than its layout; everything past the layout keeps the marker"""
    import torch
    E, n, T, K = 2, 33, 2, 2
    st, explore, rand, _ = _case(E, n, T, K, 37, baseline=False)
    engines = _engines(n, K)
    singles, left_last = _singles(E, n, T, st, explore, rand, None, engines)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    sweep = A.eval_sweep_recv(explore, rand, None, W_V2V, W_V2I, engines=engines).resolve()
    assert sweep.schemes == K and sweep.actions.shape == (K, T, E, n)
    _assert_is_the_single_calls(sweep, singles, K, False, 'S = K')
    _assert_same(_left(A, T), left_last, 'S = K')
    # the same call through the library on a twin, its results in a larger block
    lib = load_library()
    offs, size = eval_result_layout(E, n, RB, T, K)
    end = offs['regular'] + (T + 1) * E
    big = torch.full((size + 4096,), MARK, dtype=torch.uint8, device=B.device)
    T_, ex, ra, ba, own, K_ = B.check_eval_sweep_recv(explore, rand, None, engines, None, None)
    io, _, _ = B._recv_sweep_io(T, K, K)
    B._eval_upload(io, T, ex, ra, ba)
    s = B.eval_sweep_recv_struct(T, K, W_V2V, W_V2I, engines, baseline=False)
    for name, o in offs.items():
        setattr(s.base, 'result_' + ('flags' if name == 'regular' else name), big.data_ptr() + o)
    ws = io['workspace']
    assert lib.v2x_eval_sweep_recv(ctypes.byref(s), ws.data_ptr(), ws.numel(), B._stream()) == 0, lib.v2x_last_error(None)
    torch.cuda.synchronize()
    block = big.cpu().numpy()
    assert (block[end:] == MARK).all() and not (block[offs['regular']:end] == MARK).any()
    _, sw, _ = A._recv_sweep_io(T, K, K)
    assert block[:end].tobytes() == sw['dev'].cpu().numpy()[:end].tobytes()
    _close(engines)


def test_everybody_explores_without_models_reads_no_q_and_writes_no_csr():
    import torch
    E, n, T, K = 2, 61, 2, 3
    st, explore, rand, base = _case(E, n, T, K, 38, greedy=False)
    A, B = start_channels_recv(E, n, st), start_channels_recv(E, n, st)
    one = A.eval_steps_recv(explore, rand, base, W_V2V, W_V2I, engine=None).resolve()
    io, sw, q = B._recv_sweep_io(T, K + 1, K)
    q.fill_(float('nan'))
    io['q'].fill_(float('nan'))
    io['row_ptr'].fill_(MARK)
    io['col_any'].fill_(MARK)
    A.eval_steps_recv_buffers(T)['row_ptr'].fill_(MARK)
    A.eval_steps_recv_buffers(T)['col_any'].fill_(MARK)
    A.eval_steps_recv_buffers(T)['q'].fill_(float('nan'))
    sweep = B.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=None, K=K).resolve()
    assert sweep.schemes == K + 1
    _assert_is_the_single_calls(sweep, [one] * K, K, True, 'explore')
    assert all(np.array_equal(sweep.actions[k], rand) for k in range(K))
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(io['q']).all()
    assert (io['row_ptr'] == MARK).all() and (io['col_any'] == MARK).all()
    _assert_same(_left(B, T), _left(A, T), 'explore')


# ------------------------------------------------------------------------------ (e) split is chain
@pytest.mark.parametrize("E,n", [(2, 33), (1, 128)])
def test_the_split_sweep_leaves_every_byte_the_chain_sweep_leaves(E, n):
    T, K = 4, 2
    st, explore, rand, base = _case(E, n, T, K, 3 * n + E, own=(n == 33))
    engines = _engines(n, K)
    left, dcs = {}, {}
    for phase in ('chain', 'split'):
        dc = dcs[phase] = start_channels_recv(E, n, st)
        res = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines, stream_phase=phase).resolve()
        left[phase] = _left(dc, T, res, dc._recv_sweep_io(T, K + 1, K)[1]['dev'])
    _assert_same(left['split'], left['chain'], (E, n))
    assert dcs['chain'].stream_phase_calls == {'chain': 1, 'split': 0} and dcs['split'].stream_phase_calls == {'chain': 0, 'split': 1}
    assert dcs['chain'].traffic == dcs['split'].traffic
    _close(engines)


def test_a_chain_sweep_and_a_split_sweep_continue_each_other_on_one_state():
    E, n, T, K = 2, 36, 3, 2
    rng = np.random.default_rng(36)
    st = start_state(E, n, 936, [623, 0])
    draws = [(_policy(E, n, T, rng), rng.integers(0, RB, size=(T, E, n)).astype(np.int32)) for _ in range(2)]
    engines = _engines(n, K)
    left = {}
    for forms in (('chain', 'chain'), ('chain', 'split'), ('split', 'chain')):
        dc = start_channels_recv(E, n, st)
        for phase, ((explore, rand), base) in zip(forms, draws):
            res = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines, stream_phase=phase).resolve()
        left[forms] = _left(dc, T, res, dc._recv_sweep_io(T, K + 1, K)[1]['dev'])
        assert dc.walk_calls['wide'] == 2
    _assert_same(left[('chain', 'split')], left[('chain', 'chain')], 'chain, split')
    _assert_same(left[('split', 'chain')], left[('chain', 'chain')], 'split, chain')
    _close(engines)


# ------------------------------------------------------------------------------ (f) refusals before the first launch
def test_a_refused_sweep_leaves_the_state_the_workspace_and_the_result_block_alone():
    """(the ABI carries no size of q, so a q too short cannot be told from one that fits: the q the library can refuse is the
    absent one)"""
    E, n, T, K = 2, 36, 2, 2
    lib = load_library()
    st = start_state(E, n, 77, [600, 610])
    dc = start_channels_recv(E, n, st)
    engines = _engines(n, K)
    from v2xgnn import GnnEngine, GnnSpec
    other = _engine(40)
    wider = GnnEngine(GnnSpec(n_nodes=n, feat_dim=32, n_mp_layers=2))
    deeper = GnnEngine(GnnSpec(n_nodes=n, feat_dim=16, n_mp_layers=3))
    io, sw, q = dc._recv_sweep_io(T, K + 1, K)
    dc.eval_steps_recv_buffers(T)
    sw['dev'].fill_(MARK)
    q.fill_(MARK)
    before = _left(dc, T, None, sw['dev'])
    q_before = q.cpu().numpy().tobytes()
    ws, sws = io['workspace'], dc._recv_split_workspace(T)

    def call(change, engines_=engines, split=False, sws_ptr=sws.data_ptr(), sws_bytes=sws.numel(), ws_bytes=ws.numel()):
        s = dc.eval_sweep_recv_struct(T, K, W_V2V, W_V2I, engines_)
        change(s)
        if split:
            rc = lib.v2x_eval_sweep_recv_split(ctypes.byref(s), ws.data_ptr(), ws_bytes, sws_ptr, sws_bytes, dc._stream())
        else:
            rc = lib.v2x_eval_sweep_recv(ctypes.byref(s), ws.data_ptr(), ws_bytes, dc._stream())
        return rc, lib.v2x_last_error(None).decode()

    def sixty_five(s):
        s._many = (ctypes.c_void_p * 65)(*[engines[0]._h] * 65)
        s.models, s.K = s._many, 65

    same = lambda s: None                                                # noqa: E731
    cases = [
        (same, dict(engines_=[engines[0], other]), "models[1]: a fixed-size model of 36 links and 4 channels needed, got 40 links"),
        (same, dict(engines_=[other, engines[0]]), "models[0]: a fixed-size model of 36 links"),
        (same, dict(engines_=[engines[0], wider]), "models[1] has 4 channels, feature width 32"),
        (same, dict(engines_=[engines[0], deeper]), "models[1] has 4 channels, feature width 16, 3 layers"),
        (lambda s: setattr(s, 'q', None), {}, "models need the Q workspace"),
        (sixty_five, {}, "1..64 networks supported, got K = 65"),
        (lambda s: setattr(s, 'K', 0), {}, "got K = 0"),
        (lambda s: setattr(s.base, 'T', 0), {}, "T = 0"),
        (lambda s: setattr(s.base, 'result_reward', None), {}, "null result"),
        (lambda s: setattr(s.base, 'explore', None), {}, "explore"),
        (same, dict(ws_bytes=ws.numel() - 256), "needs"),
        (same, dict(split=True, sws_ptr=sws.data_ptr() + 64), "256-byte aligned"),
        (same, dict(split=True, sws_ptr=None), "split-stream workspace is null"),
        (same, dict(split=True, sws_bytes=sws.numel() - 256), "split-stream workspace of"),
    ]
    for change, kw, word in cases:
        rc, text = call(change, **kw)
        assert rc == V2X_EINVAL and word in text, (word, rc, text)
        assert text.startswith(("eval_sweep_recv", "rollout_steps_recv", "sim_")), text
        assert _left(dc, T, None, sw['dev']) == before and q.cpu().numpy().tobytes() == q_before, word
    # the Python layer's refusals come before any device work of the call, too
    with pytest.raises(ValueError, match="engine 1 has another spec"):
        dc.eval_sweep_recv(np.zeros((T, E), np.uint8), np.zeros((T, E, n), np.int32), None, W_V2V, W_V2I, engines=[engines[0], wider])
    with pytest.raises(ValueError, match="fixed-size engines of 36 links"):
        dc.eval_sweep_recv(np.zeros((T, E), np.uint8), np.zeros((T, E, n), np.int32), None, W_V2V, W_V2I, engines=[other])
    assert _left(dc, T, None, sw['dev']) == before
    assert dc.walk_calls == {'serial': 0, 'wide': 0}
    _close(engines + [other, wider, deeper])


# ------------------------------------------------------------------------------ (g) the agent
STATE_AFTER = WALKED + ('actions', 'v2v_rate', 'v2i_rate', 'interference')


def _sweep_run(backend, engines, epsilon, opt_flag=False, stream='chain', n=36, seed=43, T=3, trials=2, **how):
    """evaluate_training_sweep on a fresh seeded agent -> what it returned and left"""
    env, agent = _agent(n, seed, **({} if stream == 'chain' else dict(receiver_streams=stream)))
    calls = []
    inner = env.evaluate_sweep
    env.evaluate_sweep = lambda ex, *a, **k: (calls.append((np.shape(ex), k.get('K'), k.get('stream_phase'),
                                                            k.get('engines') is not None)), inner(ex, *a, **k))[1]
    random.seed(seed + 1)
    np.random.seed(seed + 1)
    kw = dict(engines=engines) if engines is not None else {}
    kw.update(how)
    out = agent.evaluate_training_sweep(5 * (len(engines) if engines is not None else 2), T, opt_flag, epsilon, trials,
                                        opt_backend='local', opt_restarts=8, eval_backend=backend, **kw)
    import torch
    torch.cuda.synchronize()
    dc = env.device_channels
    run = dict(out=[np.asarray(a).copy() for a in out], rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step,
               stats=dict(agent.eval_stats), state=_bytes(dc, *STATE_AFTER), calls=calls, walks=dict(dc.walk_calls),
               phases=dict(dc.stream_phase_calls), dest=np.array(env.dest))
    agent.brain.close()
    return run


def _assert_device_is_host(h, d, trials, stream, n_out):
    assert len(h['out']) == len(d['out']) == n_out
    for i, (a, b) in enumerate(zip(h['out'], d['out'])):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), ('array', i, '%d of %d entries differ' % ((a != b).sum(), a.size))
        assert np.all(np.isfinite(b))
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] > 0
    for k in STATE_AFTER:
        assert h['state'][k] == d['state'][k], ('resident', k)
    assert d['stats'] == {'device_episodes': trials, 'host_episodes': 0}
    assert h['stats'] == {'device_episodes': 0, 'host_episodes': trials}
    assert d['walks'] == {'serial': 0, 'wide': trials}                   # ONE walk per trial, whatever K
    assert d['phases'][stream] == trials and sum(d['phases'].values()) == trials
    assert h['calls'] == [] and len(d['calls']) == trials and all(c[:3] == ((3, 1), 2, stream) for c in d['calls'])


@pytest.mark.parametrize("stream", ['chain', 'split'])
@pytest.mark.parametrize("epsilon", [0.0, 0.5])
def test_the_agents_device_sweep_is_the_host_definition(epsilon, stream):
    engines = _engines(36, 2, first=21)
    h = _sweep_run('host', engines, epsilon, stream=stream)
    d = _sweep_run('device', engines, epsilon, stream=stream)
    _assert_device_is_host(h, d, 2, stream, 5)
    ret, rew = d['out'][1], d['out'][2]
    assert ret.shape == (2, 2) and rew.shape == (2, 2, 3) and np.all(d['out'][0] > 0)
    assert not np.array_equal(rew[:, 0], rew[:, 1])                      # two networks, two rows
    assert d['out'][4][:, 0].tobytes() == d['out'][4][:, 1].tobytes()    # one random scheme
    _close(engines)


def test_the_agents_device_sweep_with_the_optimum_is_the_host_definition():
    engines = _engines(36, 2, first=21)
    h = _sweep_run('host', engines, 0.5, opt_flag=True)
    d = _sweep_run('device', engines, 0.5, opt_flag=True)
    _assert_device_is_host(h, d, 2, 'chain', 9)
    opt_reward, opt_v2v = d['out'][5], d['out'][6]
    assert opt_reward.shape == (2, 2, 3) and opt_v2v.shape == (2, 2, 3, 36) and np.all(opt_reward > 0)
    assert np.all(opt_reward >= d['out'][1] - 1e-9) and np.all(opt_reward >= d['out'][3] - 1e-9)      # the search's floor
    _close(engines)


# ------------------------------------------------------------------------------ (h) the checkpoints train() writes
def test_the_sweep_scores_the_files_train_writes(tmp_path):
    from v2xgnn import GnnEngine
    from v2xgnn.bs_brain import load_weight_file
    n, seed = 36, 47
    env, trainer = _agent(n, seed)
    trainer.train(10, 1, save_dir=str(tmp_path), save_interval=5)
    names = ['Q-Network_model_weights-Episode-%d-Step-1-Batch-32.h5' % ep for ep in (5, 10)]
    assert all(os.path.exists(os.path.join(str(tmp_path), name)) for name in names)
    spec = trainer.brain.model.spec
    final = trainer.brain.model.get_weights()
    trainer.brain.close()
    by_hand = []
    for name in names:
        eng = GnnEngine(spec)
        eng.set_weights(load_weight_file(os.path.join(str(tmp_path), name)))
        by_hand.append(eng)
    for a, b in zip(by_hand[1].get_weights(), final):                    # the last file holds the trained network
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert any(np.asarray(a).tobytes() != np.asarray(b).tobytes() for a, b in zip(by_hand[0].get_weights(), by_hand[1].get_weights()))
    files = _sweep_run('device', None, 0.0, trials=1, model_dir=str(tmp_path), num_train_steps=1)
    hand = _sweep_run('device', by_hand, 0.0, trials=1)
    assert len(files['out']) == len(hand['out']) == 5 and files['out'][1].shape == (1, 2)
    for i, (a, b) in enumerate(zip(files['out'], hand['out'])):
        assert a.tobytes() == b.tobytes(), i
    for k in STATE_AFTER:
        assert files['state'][k] == hand['state'][k], k
    assert files['calls'] == hand['calls'] == [((3, 1), 2, 'chain', True)]
    _close(by_hand)
