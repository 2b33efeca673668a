"""GPU: the mixed wide walk (v2x_rollout_steps_mixed_wide / v2x_eval_steps_mixed_wide: k_traj_words_mixed, k_traj_walk_mixed,
k_traj_uniforms_mixed, k_traj_terms_mixed, k_traj_scan_mixed and k_traj_observe_mixed of csrc/v2xsimdev.hip in the place of
k_sim_trajectory_mixed; rl/device_sim.py rollout_steps_mixed / eval_steps_mixed with walk='wide';
MixedAgent(trajectory_walk='wide')).  Everything is compared byte for byte.  The independent reference of a pool is its own
twin DeviceChannels stepped by its own SERIAL rollout_steps / eval_steps (k_sim_trajectory: other kernels, another launch
geometry); the pool's wide and split workspaces are compared with those its own single-size split call leaves."""
import ctypes
import random

import numpy as np
import pytest

import test_gpu_eval_mixed as em
import test_gpu_rollout_mixed as rm
from test_gpu_eval_device import W_V2I, W_V2V
from test_gpu_rollout_trajectory import MARK, STATE, _same_rng
from v2xgnn.lib import V2X_EINVAL, EvalMixed, RolloutMixed, TrajWs, load_library
from v2xgnn.rl import DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.device_sim import (eval_steps_mixed, mixed_rollout_buffers, rollout_steps_mixed, split_workspace_layout,
                                  wide_workspace_layout)
from v2xgnn.rl.mixed import MixedAgent
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

RB, LANES = rm.RB, 6
CASES = {
    'a_one_block_next_to_many': ([(1, 4), (3, 5), (2, 31)], 3),          # unequal E, the largest pool first, n (n - 2) > 256
    'b_one_pool_T1': ([(2, 4)], 1),                                      # zero-length ob_state / ob_interf, the last entry only
    'c_one_pool_T4': ([(2, 4)], 4),                                      # a stream crossing block boundaries at 4 links
    'd_eight_pools': ([(1, n) for n in range(4, 12)], 2),                # the full table against the argument limit
    'e_two_pools': ([(1, 8), (5, 20)], 2),
}
BATCH = ('xe', 'graph_off', 'row_ptr', 'col_idx', 'q')


def _workspaces(dc, T):
    """the arrays of the pool's wide and split workspaces (wide_workspace_layout / split_workspace_layout), as bytes"""
    import torch
    torch.cuda.synchronize()
    io = dc.rollout_steps_buffers(T)
    out = {}
    for key, (offs, size) in (('wide_workspace', wide_workspace_layout(dc.E, dc.n, dc.rb, T)),
                              ('split_workspace', split_workspace_layout(dc.E, dc.n, dc.rb, T, LANES))):
        raw = io[key].cpu().numpy()
        assert raw.size == max(size, 256 if key == 'wide_workspace' else 0)
        names = sorted(offs, key=offs.get)
        for name, end in zip(names, [offs[x] for x in names[1:]] + [size]):
            out[name] = raw[offs[name]:end].tobytes()
    assert sorted(out) == ['gs', 'ob_interf', 'ob_state', 'off', 'pl', 'u_all', 'words', 'xy_all']
    return out


def _assert_counts(chans, calls=1):
    for dc in chans:
        assert dc.walk_calls == {'serial': 0, 'wide': calls} and dc.stream_phase_calls == {'chain': 0, 'split': calls}


# ------------------------------------------------------------------------------------------------------- explore only
@pytest.mark.parametrize("case", sorted(CASES))
def test_explore_only_rollout_every_pool_is_left_as_its_own_serial_rollout_steps_leaves_it(case):
    spec, T = CASES[case]
    for variant in range(3):
        pools = rm._pools(spec, T, variant, 100 + variant)
        explore = [np.ones((T, p['E']), np.uint8) for p in pools]
        actions = [p['policy'][1] for p in pools]
        args = lambda k, p, st: (explore[k], actions[k], st[k], p['head'], p['capacity'], 1.0, 0.1)     # noqa: E731
        ref_c, ref_s = rm._start(pools)
        want_rows = [dc.rollout_steps(*args(k, p, ref_s)) for k, (dc, p) in enumerate(zip(ref_c, pools))]
        split_c, split_s = rm._start(pools)
        for k, (dc, p) in enumerate(zip(split_c, pools)):
            dc.rollout_steps(*args(k, p, split_s), walk='wide', stream_phase='split')
        got_c, got_s = rm._start(pools)
        got_rows = rollout_steps_mixed(got_c, explore, actions, got_s, [p['head'] for p in pools], [p['capacity'] for p in pools],
                                       1.0, 0.1, walk='wide')
        # every resident tensor (keys and mtpos among them), the trajectory workspace, the replay storage with its markers, the rows
        rm._assert_same(pools, T, list(zip(got_c, got_s)), list(zip(ref_c, ref_s)), got_rows, want_rows, (case, variant))
        for k, p in enumerate(pools):
            got, want = _workspaces(got_c[k], T), _workspaces(split_c[k], T)
            for name in want:
                assert got[name] == want[name], (case, variant, k, name)
            assert any(want['words']) and (T == 1) == (want['ob_state'] == b'')
            assert 'wide_workspace' not in ref_c[k].rollout_steps_buffers(T)
        _assert_counts(got_c)


@pytest.mark.parametrize("case", sorted(CASES))
def test_explore_only_evaluation_every_pool_is_left_as_its_own_serial_eval_steps_leaves_it(case):
    spec, T = CASES[case]
    for S, variant in ((2, 0), (1, 1), (2, 2)):
        pools = em._pools(spec, T, variant, 100 + variant)
        explore = [np.ones((T, p['E']), np.uint8) for p in pools]
        rand = [p['policy'][1] for p in pools]
        base = [p['baseline'] if S == 2 else None for p in pools]
        ref = em._start(pools)
        want_rows = [dc.eval_steps(explore[k], rand[k], base[k], W_V2V, W_V2I) for k, dc in enumerate(ref)]
        split = em._start(pools)
        for k, dc in enumerate(split):
            dc.eval_steps(explore[k], rand[k], base[k], W_V2V, W_V2I, walk='wide', stream_phase='split')
        got = em._start(pools)
        got_rows = eval_steps_mixed(got, explore, rand, base, W_V2V, W_V2I, walk='wide')
        em._assert_same(pools, T, S, got, ref, got_rows, want_rows, (case, S, variant))
        for k in range(len(pools)):
            a, b = _workspaces(got[k], T), _workspaces(split[k], T)
            for name in b:
                assert a[name] == b[name], (case, S, variant, k, name)
        _assert_counts(got)


# ------------------------------------------------------------------------------------------------------- greedy
def _batch(chans, T):
    import torch
    torch.cuda.synchronize()
    buf = mixed_rollout_buffers(chans, T)
    return {name: buf[name].cpu().numpy().copy() for name in BATCH}


def _host_actions(spec, T, q, explore, rand):
    expected, row = [], 0
    for k, (E, n) in enumerate(spec):
        qk = q[row:row + T * E * n].reshape(T, E, n, RB)
        row += T * E * n
        greedy = np.argmax(qk, axis=3).astype(np.int32)
        assert np.any(greedy[explore[k] == 0] != rand[k][explore[k] == 0]), k               # otherwise the pool shows nothing
        expected.append(np.ascontiguousarray(np.where(explore[k][:, :, None] != 0, rand[k], greedy), np.int32))
    return expected


@pytest.mark.parametrize("case", ['a_one_block_next_to_many', 'e_two_pools'])
def test_greedy_rollout_the_batch_and_q_are_the_serial_mixed_calls(case):
    spec, T = CASES[case]
    eng = rm._ragged_engine()
    pools = rm._pools(spec, T, 1, 41)
    explore, rand = [p['policy'][0] for p in pools], [p['policy'][1] for p in pools]
    assert all(ex.any() and not ex.all() for ex in explore)
    ser_c, ser_s = rm._start(pools)
    ser_rows = rm._mixed_call(pools, ser_c, ser_s, explore, rand, engine=eng)
    want = _batch(ser_c, T)
    got_c, got_s = rm._start(pools)
    got_rows = rollout_steps_mixed(got_c, explore, rand, got_s, [p['head'] for p in pools], [p['capacity'] for p in pools], 1.0, 0.1,
                                   engine=eng, walk='wide')
    got = _batch(got_c, T)
    for name in BATCH:
        assert got[name].tobytes() == want[name].tobytes() and got[name].size, (case, name)
    assert np.all(np.isfinite(got['q']))
    rm._assert_same(pools, T, list(zip(got_c, got_s)), list(zip(ser_c, ser_s)), got_rows, ser_rows, (case, 'serial mixed'))
    # twins that explore the actions computed on the host from q, through their own serial rollout_steps
    expected = _host_actions(spec, T, got['q'], explore, rand)
    ref_c, ref_s = rm._start(pools)
    want_rows = [dc.rollout_steps(np.ones((T, p['E']), np.uint8), expected[k], ref_s[k], p['head'], p['capacity'], 1.0, 0.1)
                 for k, (dc, p) in enumerate(zip(ref_c, pools))]
    rm._assert_same(pools, T, list(zip(got_c, got_s)), list(zip(ref_c, ref_s)), got_rows, want_rows, (case, 'twins'))
    for k, p in enumerate(pools):
        assert np.array_equal(got_c[k].download('actions').reshape(p['E'], p['n']), expected[k][-1]), k
    _assert_counts(got_c)
    eng.close()


@pytest.mark.parametrize("S", [2, 1])
@pytest.mark.parametrize("case", ['a_one_block_next_to_many', 'e_two_pools'])
def test_greedy_evaluation_the_batch_and_q_are_the_serial_mixed_calls(case, S):
    spec, T = CASES[case]
    eng = rm._ragged_engine()
    pools = em._pools(spec, T, 1, 41)
    explore, rand = [p['policy'][0] for p in pools], [p['policy'][1] for p in pools]
    base = [p['baseline'] if S == 2 else None for p in pools]
    assert all(ex.any() and not ex.all() for ex in explore)
    ser = em._start(pools)
    ser_rows = eval_steps_mixed(ser, explore, rand, base, W_V2V, W_V2I, engine=eng)
    want = _batch(ser, T)
    got_c = em._start(pools)
    got_rows = eval_steps_mixed(got_c, explore, rand, base, W_V2V, W_V2I, engine=eng, walk='wide')
    got = _batch(got_c, T)
    for name in BATCH:
        assert got[name].tobytes() == want[name].tobytes() and got[name].size, (case, name)
    em._assert_same(pools, T, S, got_c, ser, got_rows, ser_rows, (case, 'serial mixed'))
    expected = _host_actions(spec, T, got['q'], explore, rand)
    ref = em._start(pools)
    want_rows = [dc.eval_steps(np.ones((T, p['E']), np.uint8), expected[k], base[k], W_V2V, W_V2I) for k, (dc, p) in enumerate(zip(ref, pools))]
    em._assert_same(pools, T, S, got_c, ref, got_rows, want_rows, (case, 'twins'))
    for k, p in enumerate(pools):
        assert np.array_equal(got_rows[k].resolve().actions[0], expected[k]), k
        assert np.array_equal(got_c[k].download('actions').reshape(p['E'], p['n']), expected[k][-1]), k
    _assert_counts(got_c)
    eng.close()


# ------------------------------------------------------------------------------------------------------- refusals
def test_a_refused_call_names_the_pool_and_leaves_state_storage_and_workspaces_alone():
    import torch
    lib = load_library()
    spec, T = [(2, 4), (3, 5)], 2
    pools = rm._pools(spec, T, 0, 9)
    chans, stores = rm._start(pools)
    for dc in chans:
        dc._eval_io(T)['eval_result_dev'].fill_(7)
    stream = torch.cuda.current_stream().cuda_stream
    dev = stores[0]['xe'].device
    sizes = [(wide_workspace_layout(E, n, RB, T)[1], split_workspace_layout(E, n, RB, T, LANES)[1]) for E, n in spec]
    ws = [(torch.full((w,), 5, dtype=torch.uint8, device=dev), torch.full((s,), 9, dtype=torch.uint8, device=dev)) for w, s in sizes]
    other_lanes = split_workspace_layout(3, 5, RB, T, 1)[1]               # pool 1's split workspace for one lane per direction:
    assert other_lanes < sizes[1][1]                                     # a block of words per state fewer than for six

    def table(change=()):
        t = (TrajWs * len(spec))()
        for k, ((w, s), (wb, sb)) in enumerate(zip(ws, sizes)):
            t[k] = TrajWs(w.data_ptr(), wb, s.data_ptr(), sb)
        for (k, field), value in dict(change).items():
            setattr(t[k], field, value)
        return t

    def snap():
        torch.cuda.synchronize()
        return ([rm._snap(dc, st, T) for dc, st in zip(chans, stores)], [em._snap(dc, T)['result'] for dc in chans],
                [(bool((w == 5).all()), bool((s == 9).all())) for w, s in ws])
    before = snap()
    assert all(a and b for a, b in before[2])
    rt, et = rm._table(chans, stores, pools, T), em._table(chans, T)
    calls = (("rollout_steps_mixed_wide", lib.v2x_rollout_steps_mixed_wide, RolloutMixed(n_pools=2, T=T, pools=rt, model=None)),
             ("eval_steps_mixed_wide", lib.v2x_eval_steps_mixed_wide, EvalMixed(n_pools=2, T=T, pools=et, model=None)))
    refusals = ((None, None, "null workspace table"),
                (table({(1, 'wide_ws_bytes'): sizes[1][0] - 1}), 1, "needs %d bytes, got %d" % (sizes[1][0], sizes[1][0] - 1)),
                (table({(0, 'split_ws'): None}), 0, "null split-stream workspace"),
                (table({(1, 'split_ws_bytes'): other_lanes}), 1, "n_lanes = %d needs %d bytes, got %d" % (LANES, sizes[1][1], other_lanes)),
                (table({(0, 'wide_ws'): None}), 0, "null wide-walk workspace"))
    for who, fn, m in calls:
        for t, pool, text in refusals:
            assert fn(ctypes.byref(m), t, stream) == V2X_EINVAL, (who, text)
            err = lib.v2x_last_error(None).decode()
            assert err.startswith(who + ": ") and text in err, (who, text, err)
            if pool is not None:
                assert "pool %d (%d links): " % (pool, spec[pool][1]) in err, (who, text, err)
        # a check of the serial mixed call, with good workspaces: the checks are the shared ones
        m.T = T + 1
        assert fn(ctypes.byref(m), table(), stream) == V2X_EINVAL
        assert "pool 0 (4 links) walks T = 2 steps, the call T = 3" in lib.v2x_last_error(None).decode()
        m.T = T
    assert snap() == before
    for st in stores:
        assert all(np.all(v.cpu().numpy() == MARK) for v in st.values())
    # the Python entry points refuse an unknown walk before any device work
    explore, rand = [p['policy'][0] for p in pools], [p['policy'][1] for p in pools]
    with pytest.raises(ValueError, match="walk must be one of 'serial', 'wide', got 'auto'"):
        rollout_steps_mixed(chans, explore, rand, stores, [0, 0], [p['capacity'] for p in pools], 1.0, 0.1, walk='auto')
    with pytest.raises(ValueError, match="walk must be one of 'serial', 'wide', got 'split'"):
        eval_steps_mixed(chans, explore, rand, [None, None], W_V2V, W_V2I, walk='split')
    assert snap() == before
    assert all(dc.walk_calls == {'serial': 0, 'wide': 0} and dc.stream_phase_calls == {'chain': 0, 'split': 0} for dc in chans)


# ------------------------------------------------------------------------------------------------------- the agent
def _agent(sizes, Es, seed, rollout, walk, num_step=0, schedule=20):
    random.seed(seed)
    np.random.seed(seed)
    envs = [start_env_batched(n, E, seed + 1000 * k, backend="device", streams="device") for k, (n, E) in enumerate(zip(sizes, Es))]
    assert all(type(e) is DeviceBatchedEnviron for e in envs)
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = MixedAgent(envs, cfg, 16, seed=seed, capacity=256, rollout=rollout, trajectory_walk=walk)
    agent.num_Episodes, agent.num_Train_Step, agent.num_step = 1, schedule, num_step
    return agent


def _trained(walk):
    """two train steps of sizes (4, 8) with E = (2, 3): T = 10 iterations per call, some simulators greedy"""
    import torch
    agent = _agent((4, 8), (2, 3), 12, 'trajectory', walk, num_step=300)
    assert agent.trajectory_walk == walk
    rewards, losses = [], []
    for _ in range(2):
        rewards.append({n: np.array(r).tobytes() for n, r in agent.generate_transitions().items()})
        losses.append(agent.replay())
    mem = {}
    for n, pool in agent.memory.pools.items():
        pool.flush()
        torch.cuda.synchronize()
        mem[n] = {k: getattr(pool, k)[:pool.size].cpu().numpy().tobytes() for k in ('xe', 'xe_next', 'col', 'mask', 'action', 'reward')}
        mem[n].update(size=pool.size, head=pool.head)
    run = dict(rewards=rewards, losses=losses, mem=mem, num_step=agent.num_step, rng=np.random.get_state(),
               stats=dict(agent.rollout_stats), online=agent.online.get_flat().tobytes(), target=agent.target.get_flat().tobytes(),
               walks=[dict(e._dc.walk_calls) for e in agent.envs], phases=[dict(e._dc.stream_phase_calls) for e in agent.envs])
    agent.close()
    return run


def test_agent_with_the_wide_walk_is_the_serial_run_bit_for_bit():
    s, w = _trained('serial'), _trained('wide')
    assert s['stats'] == w['stats'] == {'trajectory': 2, 'host': 0}
    assert w['walks'] == [{'serial': 0, 'wide': 2}] * 2 and w['phases'] == [{'chain': 0, 'split': 2}] * 2
    assert s['walks'] == [{'serial': 2, 'wide': 0}] * 2 and s['phases'] == [{'chain': 0, 'split': 0}] * 2
    assert _same_rng(s['rng'], w['rng']) and s['num_step'] == w['num_step'] == 300 + 100
    assert s['rewards'] == w['rewards'] and s['losses'] == w['losses'] and s['mem'] == w['mem']
    assert all(m['size'] > 0 for m in s['mem'].values())
    assert s['online'] == w['online'] and s['target'] == w['target'] and s['online'] != s['target']


def _evaluated(walk):
    import torch
    agent = _agent((4, 8, 12), (2, 1, 3), 33, 'host', walk)
    envs = agent.envs
    books = agent.test_run(envs, 2, 5, opt_flag=False, fixed_epsilon=0.5, eval_backend='device')
    torch.cuda.synchronize()
    run = dict(books=books, rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step, stats=dict(agent.eval_stats),
               rollouts=dict(agent.rollout_stats),
               streams=[[np.array(a).copy() for a in (e._mt_keys, e._mt_pos, e.pos, e.dirs)] for e in envs],
               resident=[{k: e._dc.tensor(k).cpu().numpy().tobytes() for k in STATE} for e in envs],
               walks=[dict(e._dc.walk_calls) for e in envs], phases=[dict(e._dc.stream_phase_calls) for e in envs])
    agent.close()
    return run


def test_test_run_on_the_device_with_the_wide_walk_equals_the_serial_books():
    """trajectory_walk='wide' with rollout='host': it applies to the evaluation"""
    s, w = _evaluated('serial'), _evaluated('wide')
    assert s['stats'] == w['stats'] == {'device_episodes': 2, 'host_episodes': 0}
    assert w['walks'] == [{'serial': 0, 'wide': 2}] * 3 and w['phases'] == [{'chain': 0, 'split': 2}] * 3
    assert s['walks'] == [{'serial': 2, 'wide': 0}] * 3
    assert sorted(s['books']) == sorted(w['books']) == [4, 8, 12]
    for n in s['books']:
        assert sorted(s['books'][n]) == sorted(w['books'][n]) == ['gnn', 'random']
        for scheme in s['books'][n]:
            for a, b in zip(s['books'][n][scheme], w['books'][n][scheme]):
                assert a.shape == b.shape and a.tobytes() == b.tobytes() and np.all(np.isfinite(a)), (n, scheme)
        assert s['books'][n]['gnn'][1].tobytes() != s['books'][n]['random'][1].tobytes(), n
    assert _same_rng(s['rng'], w['rng']) and s['py'] == w['py'] and s['num_step'] == w['num_step'] == 2 * 5 * 6
    for a, b in zip(s['streams'], w['streams']):
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
    for k, (a, b) in enumerate(zip(s['resident'], w['resident'])):
        for name in STATE:
            assert a[name] == b[name], (k, name)
