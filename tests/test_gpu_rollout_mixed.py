"""GPU: the rollouts of several link counts in one call (v2x_rollout_steps_mixed: k_sim_trajectory_mixed, k_traj_assemble_mixed,
one ragged forward, k_rollout_finish_mixed of csrc/v2xsimdev.hip; rl/device_sim.py rollout_steps_mixed;
MixedAgent(rollout='trajectory')).  The reference is an identically initialised twin state per pool stepped by that pool's own
DeviceChannels.rollout_steps -- the kernels share their __device__ functions, so everything is compared byte for byte: every
resident tensor, the whole trajectory workspace, the replay storage and the result row."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_rollout_trajectory import MARK, _heads, _policy, _same_rng, _snapshot, _storage, start_channels, start_state
from v2xgnn import GnnEngine, GnnSpec
from v2xgnn.engine import DeviceBatch
from v2xgnn.lib import V2X_EINVAL, RolloutMixed, RolloutTraj, load_library
from v2xgnn.rl import DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.device_sim import mixed_rollout_bases, mixed_rollout_buffers, rollout_steps_mixed
from v2xgnn.rl.mixed import MixedAgent
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

RB = 4
CASES = {
    'smallest_and_largest': ([(1, 4), (3, 5), (2, 31)], 3),              # n = 31: n + rb = 35 lanes, n (n - 2) = 899 > 256; unequal E
    'one_pool_T1': ([(2, 4)], 1),
    'one_pool_T4': ([(2, 4)], 4),
    'eight_pools': ([(1, n) for n in range(4, 12)], 1),                  # the full table against the argument limit
    'two_pools': ([(1, 8), (5, 20)], 2),
}


def _ragged_engine(seed=5, n_channels=RB):
    eng = GnnEngine(GnnSpec(n_nodes=1, n_channels=n_channels, feat_dim=16, n_mp_layers=2, share_weights=True, variable_graphs=True))
    eng.set_flat(np.random.default_rng(seed).normal(0, 0.3, size=eng.n_params).astype(np.float32))
    return eng


def _snap(dc, storage, T):
    """every resident tensor, the replay storage and the whole trajectory workspace, as bytes"""
    snap = _snapshot(dc, storage)
    snap['workspace'] = dc.rollout_steps_buffers(T)['workspace'].cpu().numpy().tobytes()
    return snap


def _pools(pools, T, variant, seed):
    """per pool: the start state, capacity, head (variant 0: 0; 1: wraps between two iterations; 2: wraps inside one) and policy"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (E, n) in enumerate(pools):
        capacity = T * E + 3
        mtpos = [(0, 623, 624)[(e + variant + k) % 3] for e in range(E)]
        out.append(dict(E=E, n=n, capacity=capacity, head=_heads(E, T, capacity)[variant],
                        state=start_state(E, n, 500 + 7 * n + variant, mtpos), policy=_policy(E, n, RB, T, rng, True)))
    return out


def _start(pools):
    chans = [start_channels(p['E'], p['n'], RB, p['state']) for p in pools]
    stores = [_storage(p['capacity'], p['n']) for p in pools]
    return chans, stores


def _mixed_call(pools, chans, stores, explore, actions, engine=None):
    return rollout_steps_mixed(chans, explore, actions, stores, [p['head'] for p in pools], [p['capacity'] for p in pools], 1.0, 0.1,
                               engine=engine)


def _assert_same(pools, T, got_cs, want_cs, got_rows, want_rows, tag):
    for k, p in enumerate(pools):
        (gc, gs), (wc, ws) = got_cs[k], want_cs[k]
        got, want = _snap(gc, gs, T), _snap(wc, ws, T)
        for name in want:
            assert got[name] == want[name], (tag, k, name)
        g, w = got_rows[k].resolve(), want_rows[k].resolve()
        assert g.reward.shape == (T, p['E']) and g.reward.tobytes() == w.reward.tobytes(), (tag, k)
        assert g.regular.shape == (T, 2, p['E']) and g.regular.tobytes() == w.regular.tobytes() and g.regular.all(), (tag, k)
        assert np.all(np.isfinite(w.reward)), (tag, k)
        slots = (p['head'] + np.arange(T * p['E'])) % p['capacity']
        rest = np.setdiff1d(np.arange(p['capacity']), slots)
        assert len(rest) == 3
        for name, t in gs.items():                                       # every other slot still holds the marker
            assert np.all(t.cpu().numpy()[rest] == MARK), (tag, k, name)
        assert not np.any(gs['reward'].cpu().numpy()[slots] == MARK), (tag, k)


@pytest.mark.parametrize("case", sorted(CASES))
def test_explore_only_every_pool_is_left_as_its_own_rollout_steps_leaves_it(case):
    spec, T = CASES[case]
    for variant in range(3):
        pools = _pools(spec, T, variant, 100 + variant)
        if variant and T >= 2:
            assert any(p['head'] + T * p['E'] > p['capacity'] for p in pools)              # some pool's block wraps its ring
        explore = [np.ones((T, p['E']), np.uint8) for p in pools]
        actions = [p['policy'][1] for p in pools]
        ref_c, ref_s = _start(pools)
        want_rows = [dc.rollout_steps(explore[k], actions[k], ref_s[k], p['head'], p['capacity'], 1.0, 0.1)
                     for k, (dc, p) in enumerate(zip(ref_c, pools))]
        got_c, got_s = _start(pools)
        got_rows = _mixed_call(pools, got_c, got_s, explore, actions)
        _assert_same(pools, T, list(zip(got_c, got_s)), list(zip(ref_c, ref_s)), got_rows, want_rows, (case, variant))
        for k, p in enumerate(pools):
            acts = got_s[k]['action'].cpu().numpy()[(p['head'] + np.arange(T * p['E'])) % p['capacity']].reshape(T, p['E'], p['n'])
            assert np.array_equal(acts, actions[k]), (case, variant, k)


@pytest.mark.parametrize("case", ['smallest_and_largest', 'two_pools'])
def test_greedy_one_ragged_forward_scores_every_pool(case):
    import torch
    spec, T = CASES[case]
    eng = _ragged_engine()
    pools = _pools(spec, T, 1, 41)
    explore = [p['policy'][0] for p in pools]
    rand = [p['policy'][1] for p in pools]
    for ex in explore:                                                   # both values in every pool, iteration 1 all greedy
        assert ex.any() and not ex.all() and not ex[1].any()
    got_c, got_s = _start(pools)
    got_rows = _mixed_call(pools, got_c, got_s, explore, rand, engine=eng)
    torch.cuda.synchronize()

    # (i) the ragged batch is the concatenation of the pools' trajectory prefixes, the offsets are closed-form
    buf = mixed_rollout_buffers(got_c, T)
    gbase, rbase, ebase, (B, R, Ed) = mixed_rollout_bases(spec, T)
    assert buf['sizes'] == (B, R, Ed)
    ios = [dc.rollout_steps_buffers(T) for dc in got_c]
    want_xe = np.concatenate([io['xe'].cpu().numpy() for io in ios])
    want_col = np.concatenate([io['col'].cpu().numpy() for io in ios])
    want_off = np.concatenate([rbase[k] + np.arange(T * E) * n for k, (E, n) in enumerate(spec)] + [[R]]).astype(np.int32)
    want_rp = np.concatenate([ebase[k] + np.arange(T * E * n) * (n - 2) for k, (E, n) in enumerate(spec)] + [[Ed]]).astype(np.int32)
    assert want_xe.shape == (R, 16) and want_col.shape == (Ed,)
    assert buf['xe'].cpu().numpy().tobytes() == want_xe.tobytes() and buf['col_idx'].cpu().numpy().tobytes() == want_col.tobytes()
    assert np.array_equal(buf['graph_off'].cpu().numpy(), want_off) and np.array_equal(buf['row_ptr'].cpu().numpy(), want_rp)

    # (ii) q is a second forward of that same device batch, bitwise
    n_max = spec[-1][1]
    db = DeviceBatch.from_tensors(B, 0, buf['xe'], buf['row_ptr'], buf['col_idx'], n_max * (n_max - 2), graph_off=buf['graph_off'],
                                  max_nodes=n_max)
    q = buf['q'].cpu().numpy().copy()
    again = eng.forward(db).cpu().numpy()
    assert q.shape == (R, RB) and np.all(np.isfinite(q)) and q.tobytes() == again.tobytes()

    # (iii) the twins explore the actions computed on the host from q: the same bytes everywhere, the resident actions included
    expected = []
    for k, (E, n) in enumerate(spec):
        qk = q[rbase[k]:rbase[k] + T * E * n].reshape(T, E, n, RB)
        greedy = np.argmax(qk, axis=3).astype(np.int32)
        acts = np.where(explore[k][:, :, None] != 0, rand[k], greedy)
        assert np.any(greedy[explore[k] == 0] != rand[k][explore[k] == 0]), k           # otherwise the pool shows nothing
        expected.append(np.ascontiguousarray(acts, np.int32))
    ref_c, ref_s = _start(pools)
    want_rows = [dc.rollout_steps(np.ones((T, p['E']), np.uint8), expected[k], ref_s[k], p['head'], p['capacity'], 1.0, 0.1)
                 for k, (dc, p) in enumerate(zip(ref_c, pools))]
    _assert_same(pools, T, list(zip(got_c, got_s)), list(zip(ref_c, ref_s)), got_rows, want_rows, case)
    for k, p in enumerate(pools):
        assert np.array_equal(got_c[k].download('actions').reshape(p['E'], p['n']), expected[k][-1]), k
    eng.close()


# ------------------------------------------------------------------------------------------------------- refusals
def _table(chans, stores, pools, T):
    table = (RolloutTraj * len(chans))()
    for k, (dc, p) in enumerate(zip(chans, pools)):
        table[k] = dc.rollout_steps_struct(T, stores[k], p['head'], p['capacity'], 1.0, 0.1)
    return table


def test_a_refused_call_names_the_pool_and_leaves_every_state_and_storage_alone():
    import torch
    lib = load_library()
    spec, T = [(2, 4), (3, 5)], 2
    pools = _pools(spec, T, 0, 9)
    chans, stores = _start(pools)
    other = start_channels(3, 5, 3, pools[1]['state'])                   # the second pool with another channel count
    other0 = start_channels(2, 4, 3, pools[0]['state'])                  # ... and the first one (kept: the structs point into them)
    eng, fixed = _ragged_engine(), GnnEngine(GnnSpec(n_nodes=4, feat_dim=16, n_mp_layers=2))
    buf = mixed_rollout_buffers(chans, T)
    before = [_snap(dc, st, T) for dc, st in zip(chans, stores)]
    stream = torch.cuda.current_stream().cuda_stream

    def refused(text, pool=None, model=None, n_pools=None, call_T=T, table=None, **null):
        table = _table(chans, stores, pools, T) if table is None else table
        m = RolloutMixed(n_pools=len(spec) if n_pools is None else n_pools, T=call_T, pools=table, model=model)
        if model is not None:
            for name in ('xe', 'graph_off', 'row_ptr', 'col_idx', 'q'):
                setattr(m, name, None if null.get(name) else buf[name].data_ptr())
        assert lib.v2x_rollout_steps_mixed(ctypes.byref(m), stream) == V2X_EINVAL, text
        err = lib.v2x_last_error(None).decode()
        assert err.startswith("rollout_steps_mixed: ") and text in err, (text, err)
        if pool is not None:
            assert "pool %d" % pool in err, (text, err)

    refused("1..8 pools", n_pools=0)
    refused("1..8 pools", n_pools=9)
    t = _table(chans, stores, pools, T)
    t[0], t[1] = _table(chans, stores, pools, T)[1], _table(chans, stores, pools, T)[0]
    refused("the link counts must ascend strictly", pool=1, table=t)
    t = _table(chans, stores, pools, T)
    t[1].T = T + 1
    refused("walks T = 3 steps, the call T = 2", pool=1, table=t)
    t = _table(chans, stores, pools, T)
    t[0].r.model = eng._h
    refused("has a model of its own", pool=0, table=t)
    t = _table(chans, stores, pools, T)
    t[1].r.capacity = T * 3 - 1                                          # what v2x_rollout_steps refuses of a pool: T E > capacity
    refused("T E <= capacity", pool=1, table=t)
    t = _table(chans, stores, pools, T)
    t[0].r.step.problem.n = 32                                           # ... and more than 31 links
    refused("3..31 links", pool=0, table=t)
    t = _table(chans, stores, pools, T)
    t[1].traj_xe = None                                                  # ... and a null workspace
    refused("null trajectory workspace pointer", pool=1, table=t)
    t = _table(chans, stores, pools, T)
    t[1] = other.rollout_steps_struct(T, stores[1], 0, pools[1]['capacity'], 1.0, 0.1)
    refused("one channel count for all pools", pool=1, table=t)
    refused("a variable_graphs model of 4 channels needed, got fixed-size graphs", model=fixed._h)
    t = _table(chans, stores, pools, T)                                  # every pool with 3 channels: the model's 4 are not rb
    t[0] = other0.rollout_steps_struct(T, stores[0], 0, pools[0]['capacity'], 1.0, 0.1)
    t[1] = other.rollout_steps_struct(T, stores[1], 0, pools[1]['capacity'], 1.0, 0.1)
    refused("a variable_graphs model of 3 channels needed, got variable graphs, 4 channels", model=eng._h, table=t)
    for name in ('xe', 'graph_off', 'row_ptr', 'col_idx'):
        refused("a model needs the ragged batch's xe / graph_off / row_ptr / col_idx", model=eng._h, **{name: True})
    refused("a model needs the Q workspace", model=eng._h, q=True)
    t = _table(chans, stores, pools, T)                                  # what v2x_rollout_steps refuses of a pool that is SCORED
    t[1].r.explore = None
    refused("Q-values need the explore flags", pool=1, model=eng._h, table=t)
    # R and Ed beyond int32: two pools that v2x_rollout_steps would each take (T E n (n - 2) < 2^31), together too many.  Nothing
    # is launched, so the structs may claim a T the buffers behind them do not have
    big = 2300000
    wide = [start_channels(1, 30, RB, start_state(1, 30, 3)), start_channels(1, 31, RB, start_state(1, 31, 4))]
    wide_s = [_storage(4, 30), _storage(4, 31)]
    wide_before = [_snapshot(dc, st) for dc, st in zip(wide, wide_s)]
    t = (RolloutTraj * 2)()
    for k, dc in enumerate(wide):
        t[k] = dc.rollout_steps_struct(1, wide_s[k], 0, 4, 1.0, 0.1)
        t[k].T, t[k].r.capacity = big, big
    refused("exceed the 32-bit sizes of a batch", call_T=big, table=t)

    after = [_snap(dc, st, T) for dc, st in zip(chans, stores)]
    for b, a in zip(before, after):
        for name in b:
            assert a[name] == b[name], name
    assert [_snapshot(dc, st) for dc, st in zip(wide, wide_s)] == wide_before
    for st in stores + wide_s:
        assert all(np.all(v.cpu().numpy() == MARK) for v in st.values())
    # the Python entry point refuses before any device work, too
    with pytest.raises(ValueError, match="ascend strictly"):
        rollout_steps_mixed(chans[::-1], [None] * 2, [None] * 2, stores, [0, 0], [7, 9], 1.0, 0.1)
    with pytest.raises(ValueError, match="variable_graphs engine"):
        _mixed_call(pools, chans, stores, [p['policy'][0] for p in pools], [p['policy'][1] for p in pools], engine=fixed)
    assert [_snap(dc, st, T) for dc, st in zip(chans, stores)] == before
    eng.close()
    fixed.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _agent(sizes, Es, seed, rollout, num_step, schedule, irregular=None, capacity=256):
    random.seed(seed)
    np.random.seed(seed)
    envs = [start_env_batched(n, E, seed + 1000 * k, backend="device", streams="device") for k, (n, E) in enumerate(zip(sizes, Es))]
    assert all(type(e) is DeviceBatchedEnviron for e in envs)
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = MixedAgent(envs, cfg, 16, seed=seed, capacity=capacity, rollout=rollout)
    agent.num_Episodes, agent.num_Train_Step, agent.num_step = 1, schedule, num_step        # (epsilon falls over 40 x schedule steps)
    if irregular is not None:                                            # a link that is its own receiver, in one environment
        k, e, link = irregular
        envs[k].dest[e, link] = link
        envs[k]._static_dirty = True
        envs[k]._dev_obs = None
    return agent


def _run(sizes, Es, seed, rollout, num_step, schedule, train_steps, irregular=None):
    import torch
    agent = _agent(sizes, Es, seed, rollout, num_step, schedule, irregular)
    rewards, losses, greedy_count = [], [], []
    draws = agent._policy_draws

    def counted(step_no):                                                # the greedy simulators of every iteration, on the host
        out = draws(step_no)
        greedy_count.append(sum(len(g) for g in out[1]))
        return out
    agent._policy_draws = counted
    for _ in range(train_steps):
        rewards.append({n: np.array(r) for n, r in agent.generate_transitions().items()})
        losses.append(agent.replay())
    mem = {}
    for n, pool in agent.memory.pools.items():
        pool.flush()
        flags = pool.regular_flags()
        torch.cuda.synchronize()
        mem[n] = {k: getattr(pool, k)[:pool.size].cpu().numpy().tobytes() for k in ('xe', 'xe_next', 'col', 'mask', 'action', 'reward')}
        mem[n].update(size=pool.size, head=pool.head, regular=flags[:pool.size].tobytes())
    run = dict(rewards=rewards, losses=losses, mem=mem, num_step=agent.num_step, epsilon=agent.epsilon, rng=np.random.get_state(),
               stats=dict(agent.rollout_stats), greedy=sum(greedy_count), dropped=dict(agent.memory.dropped_irregular),
               online=agent.online.get_flat())
    agent.close()
    return run


def _assert_same_run(h, t):
    assert t['num_step'] == h['num_step'] and t['epsilon'] == h['epsilon'] and _same_rng(t['rng'], h['rng'])
    assert t['greedy'] == h['greedy'] and t['dropped'] == h['dropped']
    for rh, rt in zip(h['rewards'], t['rewards']):
        assert sorted(rh) == sorted(rt)
        for n in rh:
            assert rt[n].shape == rh[n].shape and rt[n].tobytes() == rh[n].tobytes() and np.all(np.isfinite(rh[n])), n
    for n in h['mem']:
        for k in h['mem'][n]:
            assert t['mem'][n][k] == h['mem'][n][k], (n, k)
    assert t['losses'] == h['losses'] and t['online'].tobytes() == h['online'].tobytes()


def test_agent_one_iteration_per_rollout_with_greedy_simulators_equals_the_host_rollout():
    """sizes (4, 8, 12) x 17 simulators: 51 transitions per iteration, T = 1 -- both forms score the same batch"""
    h = _run((4, 8, 12), (17, 17, 17), 33, 'host', 400, 20, 2)
    t = _run((4, 8, 12), (17, 17, 17), 33, 'trajectory', 400, 20, 2)
    assert 0 < h['greedy'] < 2 * 51                                      # some simulators are greedy, some explore
    _assert_same_run(h, t)
    assert h['stats'] == {'trajectory': 0, 'host': 2} and t['stats'] == {'trajectory': 2, 'host': 0}
    assert h['num_step'] == 400 + 2 * 51 and all(m['size'] == 34 for m in h['mem'].values())


def test_agent_ten_iterations_in_one_call_with_nobody_greedy_equals_the_host_rollout():
    """sizes (4, 8) with E = (2, 3): T = 10.  Nobody is greedy (asserted), so the check does not lean on a ragged forward being
    independent of what else is in the batch"""
    h = _run((4, 8), (2, 3), 12, 'host', 0, 2000, 2)                      # epsilon stays above 0.998 over the 100 draws
    t = _run((4, 8), (2, 3), 12, 'trajectory', 0, 2000, 2)
    assert h['greedy'] == 0 and t['greedy'] == 0
    _assert_same_run(h, t)
    assert t['stats'] == {'trajectory': 2, 'host': 0}
    assert h['mem'][4]['size'] == 40 and h['mem'][8]['size'] == 60 and h['num_step'] == 100


def test_agent_an_irregular_graph_takes_the_host_path_and_equals_the_host_agent():
    h = _run((4, 8), (2, 3), 12, 'host', 300, 20, 1, irregular=(1, 2, 5))
    t = _run((4, 8), (2, 3), 12, 'trajectory', 300, 20, 1, irregular=(1, 2, 5))
    assert h['greedy'] > 0                                               # (the host path scores the irregular graph, too)
    _assert_same_run(h, t)
    assert t['stats'] == {'trajectory': 0, 'host': 1}
    assert h['dropped'] == {4: 0, 8: 10} and h['mem'][8]['size'] == 20   # simulator 2 of the 8-link environment stores nothing
