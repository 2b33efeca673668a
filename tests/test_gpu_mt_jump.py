"""GPU: the split stream phase's words drawn in chunks by jump-ahead (v2x_rollout_steps_recv_jump, v2x_eval_steps_recv_jump,
v2x_eval_sweep_recv_jump: k_traj_words_recv stopped at `first`, k_traj_jump_seeds, k_traj_jump_chunks;
DeviceChannels.*_recv(stream_words='jump'); Agent(receiver_words='jump')).  The reference everywhere is the _split call on a
twin DeviceChannels built from the same state, and every comparison is byte for byte: the jump form writes the same word array,
and everything behind the words is the same code.  The engine scores 4 channels: rb = 4 throughout."""
import ctypes

import numpy as np
import pytest

from test_gpu_eval_recv import W_V2I, W_V2V
from test_gpu_eval_recv import _left as _eval_left
from test_gpu_eval_sweep_recv import _case, _close, _engines
from test_gpu_eval_sweep_recv import _left as _sweep_left
from test_gpu_rollout_recv import MARK, RB, _bytes, _policy, _recv_storage, start_channels_recv
from test_gpu_rollout_recv_split import RESIDENT, _assert_same
from test_gpu_rollout_trajectory import _engine, start_state
from v2xgnn.lib import MtJump, V2X_EINVAL, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.device_sim import (JUMP_FIRST, JUMP_SLICES, JUMP_STRIDE, RECV_SECTIONS, jump_plan, split_stream_blocks,
                                  split_workspace_layout, wide_workspace_layout)
from v2xgnn.rl.replay import ReceiverReplay
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

N_LANES = 6                                              # start_state's lane grid
MIN_FIRST = 20561
GUARD, GUARD_BYTE = 1024, 0xA5


def _nbw(n, T):
    return split_stream_blocks(n, RB, T, N_LANES) * 624


def _guarded(nbytes):
    """a device buffer of nbytes behind and before a guard band of GUARD marked bytes -> (whole tensor, the 256-byte aligned
    pointer of the payload)"""
    import torch
    whole = torch.full((nbytes + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device='cuda')
    lead = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    return whole, lead


def _guards_intact(whole, lead, nbytes):
    host = whole.cpu().numpy()
    return bool((host[:lead] == GUARD_BYTE).all() and (host[lead + nbytes:] == GUARD_BYTE).all())


class _Table:
    """v2x_mt_jump of (first, stride, count) for E states with guard bands around the polynomials and the scratch"""

    def __init__(self, lib, E, first, stride, count):
        import torch
        host = np.zeros((max(count, 1), 624), np.uint32)
        if count:
            assert lib.v2x_mt_jump_polys(first, stride, count, host.ctypes.data) == 0, lib.v2x_last_error(None)
        self.poly_bytes = 4 * 624 * max(count, 1)
        self.polys, self.poly_lead = _guarded(self.poly_bytes)
        self.polys[self.poly_lead:self.poly_lead + self.poly_bytes] = torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda()
        self.host = host
        self.scratch_bytes = max(int(lib.v2x_mt_jump_scratch_bytes(E, count)), 256)
        assert lib.v2x_mt_jump_scratch_bytes(E, count) == (4 * E * count * JUMP_SLICES * 624 + 255) // 256 * 256
        self.scratch, self.scratch_lead = _guarded(self.scratch_bytes)
        self.struct = MtJump(first=first, stride=stride, count=count, pad_=0, polys=self.polys.data_ptr() + self.poly_lead,
                             scratch=self.scratch.data_ptr() + self.scratch_lead, scratch_bytes=self.scratch_bytes)
        assert self.struct.polys % 256 == 0 and self.struct.scratch % 256 == 0

    def intact(self):
        """the guard bands hold and the polynomials are what went up"""
        import torch
        torch.cuda.synchronize()
        table = self.polys[self.poly_lead:self.poly_lead + self.poly_bytes].cpu().numpy().tobytes()
        return (_guards_intact(self.polys, self.poly_lead, self.poly_bytes) and table == self.host.tobytes()
                and _guards_intact(self.scratch, self.scratch_lead, self.scratch_bytes))


def _raw_call(lib, dc, T, storage, cap, table=None):
    """v2x_rollout_steps_recv_split (table None) or _jump of dc's resident state without a model, straight through the C ABI ->
    every byte it leaves, the split workspace (words, the band behind them, off) included"""
    import torch
    ws = dc.rollout_steps_recv_buffers(T)['workspace']
    sws = dc._recv_split_workspace(T)
    r = dc.rollout_steps_recv_struct(T, storage, 0, cap, 1.0, 0.1)
    if table is None:
        rc = lib.v2x_rollout_steps_recv_split(ctypes.byref(r), ws.data_ptr(), ws.numel(), sws.data_ptr(), sws.numel(), dc._stream())
    else:
        rc = lib.v2x_rollout_steps_recv_jump(ctypes.byref(r), ws.data_ptr(), ws.numel(), sws.data_ptr(), sws.numel(),
                                             ctypes.byref(table.struct), dc._stream())
    assert rc == 0, lib.v2x_last_error(None).decode()
    torch.cuda.synchronize()
    out = {'resident ' + k: v for k, v in _bytes(dc, *RESIDENT).items()}
    out.update({'replay ' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
    out['split workspace'] = sws.cpu().numpy().tobytes()
    out['workspace'] = ws.cpu().numpy()[:dc.rollout_steps_recv_buffers(T)['offsets']['wide']].tobytes()
    return out


# ------------------------------------------------------------------------------------------------------- the words array
E_W, N_W, T_W = 2, 32, 4
NBW_W = _nbw(N_W, T_W)
REST_W = NBW_W - MIN_FIRST
# (first, stride, count): strides that are no multiple of 227 and one that is; a last chunk of 100 words (fewer than a round and
# fewer than its own 624 seeds), one of 700, one of a single word behind the last legal `first`; fewer chunks than would fit
PLANS_W = [(MIN_FIRST, 624, -(-REST_W // 624)), (MIN_FIRST, 1000, -(-REST_W // 1000)), (MIN_FIRST, 227 * 64, -(-REST_W // (227 * 64))),
           (MIN_FIRST, REST_W - 100, 2), (MIN_FIRST, REST_W - 700, 2), (NBW_W - 1001, 1000, 2), (JUMP_FIRST, 227 * 64, 2)]


@pytest.fixture(scope="module")
def words_reference():
    """the split call's bytes at (2, 32, 4, 4), once per entry position: state 0 enters at 624 or 0, state 1 mid-block"""
    lib = load_library()
    ref = {}
    for entry in ((624, 300), (0, 623)):
        st = start_state(E_W, N_W, 410, list(entry))
        dc = start_channels_recv(E_W, N_W, st)
        ref[entry] = (st, _raw_call(lib, dc, T_W, _recv_storage(E_W * T_W + 1, N_W), E_W * T_W + 1))
    return ref


@pytest.mark.parametrize("entry", [(624, 300), (0, 623)])
@pytest.mark.parametrize("first,stride,count", PLANS_W)
def test_the_words_array_of_the_jump_form_is_the_split_forms(words_reference, entry, first, stride, count):
    assert NBW_W > 70000 and first + (count - 1) * stride < NBW_W
    lib = load_library()
    st, want = words_reference[entry]
    dc = start_channels_recv(E_W, N_W, st)
    table = _Table(lib, E_W, first, stride, count)
    got = _raw_call(lib, dc, T_W, _recv_storage(E_W * T_W + 1, N_W), E_W * T_W + 1, table)
    offs, size = split_workspace_layout(E_W, N_W, RB, T_W, N_LANES)
    assert len(got['split workspace']) == size and offs['off'] >= 4 * E_W * NBW_W
    words = lambda o: np.frombuffer(o['split workspace'], np.uint32, E_W * NBW_W).reshape(E_W, NBW_W)     # noqa: E731
    bad = np.argwhere(words(got) != words(want))
    assert bad.size == 0, "first differing word (state, index): %s of %d" % (bad[0].tolist(), len(bad))
    _assert_same(got, want, (entry, first, stride, count))               # words, the band behind them, off, and everything after
    assert table.intact()


def test_one_short_chunk_at_the_boundary():
    """(1, 5, 4, 50): the prefix ends 50 words before the array does, and one chunk of 50 words follows; then the default plan"""
    E, n, T = 1, 5, 50
    nbw = _nbw(n, T)
    assert MIN_FIRST < nbw < 2 * MIN_FIRST
    lib = load_library()
    st = start_state(E, n, 55, [311])
    want = _raw_call(lib, start_channels_recv(E, n, st), T, _recv_storage(T + 1, n), T + 1)
    for plan in ((nbw - 50, 624, 1), (MIN_FIRST, 624, 1), jump_plan(nbw)):
        table = _Table(lib, E, *plan)
        got = _raw_call(lib, start_channels_recv(E, n, st), T, _recv_storage(T + 1, n), T + 1, table)
        _assert_same(got, want, plan)
        assert table.intact()


def test_an_array_the_prefix_covers_runs_the_serial_launch():
    """(1, 4, 4, 5): nbw < first (the receiver form needs rb <= n, so 4 links are the fewest that carry these tests' 4 channels).
    The Python path plans no chunk; a table with chunks is legal too and is not read."""
    E, n, T = 1, 4, 5
    nbw = _nbw(n, T)
    assert nbw < MIN_FIRST and jump_plan(nbw) == (JUMP_FIRST, JUMP_STRIDE, 0)
    lib = load_library()
    st = start_state(E, n, 56, [17])
    want = _raw_call(lib, start_channels_recv(E, n, st), T, _recv_storage(T + 1, n), T + 1)
    for plan in ((JUMP_FIRST, JUMP_STRIDE, 0), (MIN_FIRST, 624, 3)):
        table = _Table(lib, E, *plan)
        got = _raw_call(lib, start_channels_recv(E, n, st), T, _recv_storage(T + 1, n), T + 1, table)
        _assert_same(got, want, plan)
        assert table.intact()
    explore, rand = _policy(E, n, T, np.random.default_rng(1))
    runs = {}
    for words in ('serial', 'jump'):
        dc = start_channels_recv(E, n, st)
        runs[words] = _run(dc, words, T, explore, rand, _recv_storage(T + 1, n), 0, T + 1, None)
        assert dc.stream_words_calls == {'serial': int(words == 'serial'), 'jump': int(words == 'jump')}
        assert dc._recv_jump_table(T).count == 0 and dc._recv_jump_table(T).polys is None
    _assert_same(runs['jump'], runs['serial'], 'fallback')


def test_a_first_one_past_the_last_legal_value_is_refused_and_nothing_is_written():
    import torch
    E, n, T, cap = 2, 32, 4, 9
    nbw, stride = _nbw(n, T), 1000
    lib = load_library()
    dc = start_channels_recv(E, n, start_state(E, n, 77, [600, 610]))
    storage = _recv_storage(cap, n)
    ws = dc.rollout_steps_recv_buffers(T)['workspace']
    sws = dc._recv_split_workspace(T)

    def snapshot():
        torch.cuda.synchronize()
        snap = _bytes(dc, *RESIDENT)
        snap.update({'rep_' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
        snap['split workspace'], snap['workspace'] = sws.cpu().numpy().tobytes(), ws.cpu().numpy().tobytes()
        return snap

    before = snapshot()
    table = _Table(lib, E, nbw - stride, stride, 2)                      # chunk 2 would begin at nbw: empty
    r = dc.rollout_steps_recv_struct(T, storage, 0, cap, 1.0, 0.1)
    rc = lib.v2x_rollout_steps_recv_jump(ctypes.byref(r), ws.data_ptr(), ws.numel(), sws.data_ptr(), sws.numel(),
                                         ctypes.byref(table.struct), dc._stream())
    text = lib.v2x_last_error(None).decode()
    assert rc == V2X_EINVAL and text.startswith("rollout_steps_recv_jump") and "last chunk is empty" in text, (rc, text)
    assert snapshot() == before and table.intact()
    for k, v in storage.items():
        assert (v == MARK).all(), k


# ------------------------------------------------------------------------------------------------------- end to end
def _small_plan(nbw):
    """several chunks at the small shapes of these tests: a stride that is no multiple of 227"""
    stride = 5000
    return MIN_FIRST, stride, (-(-(nbw - MIN_FIRST) // stride) if nbw > MIN_FIRST else 0)


def _run(dc, words, T, explore, rand, storage, head, cap, eng):
    """one rollout_steps_recv with the split stream phase and the words launch `words` on dc -> every byte it leaves, by name"""
    import torch
    E, n = dc.E, dc.n
    res = dc.rollout_steps_recv(explore, rand, storage, head, cap, 1.0, 0.1, engine=eng, stream_phase='split',
                                stream_words=words).resolve()
    torch.cuda.synchronize()
    out = {'resident ' + k: v for k, v in _bytes(dc, *RESIDENT).items()}
    out.update({'replay ' + k: v.cpu().numpy().tobytes() for k, v in storage.items()})
    io = dc.rollout_steps_recv_buffers(T)
    ws, offs = io['workspace'].cpu().numpy(), io['offsets']
    ends = [offs[k] for k in RECV_SECTIONS[1:]] + [offs['wide']]
    for k, end in zip(RECV_SECTIONS, ends):
        out['workspace ' + k] = ws[offs[k]:end].tobytes()
    w = wide_workspace_layout(E, n, RB, T)[0]
    out['workspace u_all'] = ws[offs['wide'] + w['u_all']:offs['wide'] + w['xy_all']].tobytes()
    out['workspace xy_all'] = ws[offs['wide'] + w['xy_all']:offs['wide'] + w['pl']].tobytes()
    out['split workspace'] = io['split_workspace'].cpu().numpy().tobytes()
    out['result reward'], out['result flags'], out['result regular'] = res.reward.tobytes(), res.flags.tobytes(), res.regular.tobytes()
    assert res.reward.shape == (T, E) and np.all(np.isfinite(res.reward))
    return out


@pytest.mark.parametrize("E,n,T", [(3, 33, 3), (1, 64, 4)])
def test_two_rollouts_in_a_row_leave_every_byte_the_split_form_leaves(E, n, T):
    K = T * E
    cap = 2 * K + 1
    st = start_state(E, n, 640 + n, [(620, 0, 624)[e % 3] for e in range(E)])
    eng = _engine(n)
    rng = np.random.default_rng(n)
    blocks = [_policy(E, n, T, rng) for _ in range(2)]
    runs = {}
    for words in ('serial', 'jump'):
        dc, storage = start_channels_recv(E, n, st), _recv_storage(cap, n)
        dc.jump_plan = _small_plan
        runs[words] = [_run(dc, words, T, blocks[j][0], blocks[j][1], storage, j * K, cap, eng) for j in range(2)]
        assert dc.stream_phase_calls == {'chain': 0, 'split': 2}
        assert dc.stream_words_calls == {'serial': 2 * int(words == 'serial'), 'jump': 2 * int(words == 'jump')}
        if words == 'jump':
            jump = dc._recv_jump_table(T)
            assert jump.count == _small_plan(_nbw(n, T))[2] >= 5 and len(dc._jump_tables) == 1      # one table, built once
    for j in range(2):
        _assert_same(runs['jump'][j], runs['serial'][j], (E, n, T, 'call', j))
    eng.close()


def test_an_evaluation_episode_at_40_links():
    E, n, T = 2, 40, 4
    rng = np.random.default_rng(3 * n + E)
    st = start_state(E, n, 840, [623, 0])
    explore, rand = _policy(E, n, T, rng)
    baseline = rng.integers(0, RB, size=(T, E, n)).astype(np.int32)
    eng = _engine(n)
    out = {}
    for words in ('serial', 'jump'):
        dc = start_channels_recv(E, n, st)
        dc.jump_plan = _small_plan
        res = dc.eval_steps_recv(explore, rand, baseline, W_V2V, W_V2I, engine=eng, stream_phase='split', stream_words=words).resolve()
        out[words] = _eval_left(dc, T, res)
        out[words]['split workspace'] = dc.eval_steps_recv_buffers(T)['split_workspace'].cpu().numpy().tobytes()
        assert dc.stream_words_calls == {'serial': int(words == 'serial'), 'jump': int(words == 'jump')}
    _assert_same(out['jump'], out['serial'], 'episode')
    eng.close()


def test_a_sweep_of_two_networks_at_33_links():
    E, n, T, K = 2, 33, 4, 2
    st, explore, rand, base = _case(E, n, T, K, 3 * n + E, own=True)
    engines = _engines(n, K)
    left = {}
    for words in ('serial', 'jump'):
        dc = start_channels_recv(E, n, st)
        dc.jump_plan = _small_plan
        res = dc.eval_sweep_recv(explore, rand, base, W_V2V, W_V2I, engines=engines, stream_phase='split', stream_words=words).resolve()
        left[words] = _sweep_left(dc, T, res, dc._recv_sweep_io(T, K + 1, K)[1]['dev'])
        left[words]['split workspace'] = dc.eval_steps_recv_buffers(T)['split_workspace'].cpu().numpy().tobytes()
        assert dc.stream_words_calls == {'serial': int(words == 'serial'), 'jump': int(words == 'jump')}
    _assert_same(left['jump'], left['serial'], 'sweep')
    _close(engines)


# ------------------------------------------------------------------------------------------------------- the agent
def _trained(words, steps=2):
    import random
    seed = 18
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(40, 1, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 16, 1, 0.1)
    agent = Agent(40, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay='receivers', rollout_backend='trajectory',
                  receiver_streams='split', receiver_words=words)
    assert type(env) is DeviceBatchedEnviron and type(agent.device_replay) is ReceiverReplay
    out = agent.train(1, steps)
    rep = agent.device_replay
    run = {'losses': out[0].tobytes(), 'rewards per step': out[1].tobytes(), 'weights': agent.brain.model.engine.get_flat().tobytes(),
           'size': (rep.size, rep.head, agent.num_step)}
    for k in ('xe', 'xe_next', 'recv', 'action', 'reward'):
        run['replay ' + k] = getattr(rep, k)[:rep.size].cpu().numpy().tobytes()
    dc = env.device_channels
    calls = (dict(dc.stream_phase_calls), dict(dc.stream_words_calls))
    assert np.isfinite(out[0]).all()
    agent.brain.close()
    return run, calls


def test_agent_with_jump_words_is_the_agent_with_serial_words():
    serial, serial_calls = _trained('serial')
    jump, jump_calls = _trained('jump')
    assert serial_calls == ({'chain': 0, 'split': 2}, {'serial': 2, 'jump': 0})
    assert jump_calls == ({'chain': 0, 'split': 2}, {'serial': 0, 'jump': 2})
    _assert_same(jump, serial, 'agent')
