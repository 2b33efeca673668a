"""GPU: an evaluation episode of several link counts in one call (v2x_eval_steps_mixed: k_sim_trajectory_mixed,
k_traj_assemble_mixed, one ragged forward, k_eval_finish_mixed of csrc/v2xsimdev.hip; rl/device_sim.py eval_steps_mixed /
resident_evaluate_steps_mixed; MixedAgent.test_run(eval_backend='device'); MixedAgent.save_weights / load_weights).  The
reference is an identically initialised twin state per pool run through that pool's own DeviceChannels.eval_steps -- the kernels
share their __device__ functions, so everything is compared byte for byte: every resident tensor, the whole trajectory
workspace and the whole result block -- or the agent's host loop on twin environments.

Of the refusals of the library, one cannot be reached and is not exercised: a pool holds T E_k <= 65535 states, so 8 pools of 31
links hold 16 R = 16 * 8 * 65535 * 31 = 2.6e8 floats and Ed = 8 * 65535 * 31 * 29 = 4.7e8 edges at most, both below 2^31."""
import ctypes
import os
import random

import numpy as np
import pytest

from test_gpu_eval_device import W_V2I, W_V2V
from test_gpu_rollout_mixed import CASES, RB, _agent, _ragged_engine
from test_gpu_rollout_trajectory import STATE, _policy, _same_rng, start_channels, start_state
from v2xgnn import GnnEngine, GnnSpec
from v2xgnn.engine import DeviceBatch
from v2xgnn.lib import V2X_EINVAL, Eval, EvalMixed, load_library
from v2xgnn.rl import mixed
from v2xgnn.rl.device_sim import (eval_result_layout, eval_steps_mixed, mixed_rollout_bases, mixed_rollout_buffers,
                                  resident_evaluate_steps_mixed)
from v2xgnn.rl.run import weight_file_names
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

RATES = ('v2v_rate', 'v2i_rate', 'interference', 'reward')


def _pools(spec, T, variant, seed, rb=RB):
    """per pool: the start state (streams at 0, 623 and 624, rotating over states, pools and variants), the policy and a baseline"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (E, n) in enumerate(spec):
        mtpos = [(0, 623, 624)[(e + variant + k) % 3] for e in range(E)]
        out.append(dict(E=E, n=n, state=start_state(E, n, 500 + 7 * n + variant, mtpos), policy=_policy(E, n, rb, T, rng, True),
                        baseline=rng.integers(0, rb, size=(T, E, n)).astype(np.int32)))
    return out


def _start(pools, rb=RB):
    return [start_channels(p['E'], p['n'], rb, p['state']) for p in pools]


def _snap(dc, T):
    """every resident tensor, the whole trajectory workspace and the whole result block, as bytes"""
    import torch
    torch.cuda.synchronize()
    snap = {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}
    snap['workspace'] = dc.rollout_steps_buffers(T)['workspace'].cpu().numpy().tobytes()
    snap['result'] = dc._eval_io(T)['eval_result_dev'].cpu().numpy().tobytes()
    return snap


def _assert_same(pools, T, S, got_c, want_c, got_rows, want_rows, tag):
    for k, p in enumerate(pools):
        got, want = _snap(got_c[k], T), _snap(want_c[k], T)
        for name in want:
            assert got[name] == want[name], (tag, k, name)
        g, w = got_rows[k].resolve(), want_rows[k].resolve()
        assert g.actions.shape == (S, T, p['E'], p['n']) and g.actions.tobytes() == w.actions.tobytes(), (tag, k)
        for name in RATES:
            a, b = getattr(g, name), getattr(w, name)
            assert a.shape == b.shape and a.tobytes() == b.tobytes() and np.all(np.isfinite(b)), (tag, k, name)
        assert g.regular.shape == (T + 1, p['E']) and np.array_equal(g.regular, w.regular) and g.regular.all(), (tag, k)


def _explore_only(spec, T, rb, tag):
    for S in (1, 2):
        for variant in range(3):
            pools = _pools(spec, T, variant, 100 + variant, rb)
            explore = [np.ones((T, p['E']), np.uint8) for p in pools]
            rand = [p['policy'][1] for p in pools]
            base = [p['baseline'] if S == 2 else None for p in pools]
            ref = _start(pools, rb)
            want_rows = [dc.eval_steps(explore[k], rand[k], base[k], W_V2V, W_V2I) for k, dc in enumerate(ref)]
            got = _start(pools, rb)
            got_rows = eval_steps_mixed(got, explore, rand, base, W_V2V, W_V2I)
            _assert_same(pools, T, S, got, ref, got_rows, want_rows, (tag, S, variant))
            for k, p in enumerate(pools):
                r = got_rows[k].resolve()
                assert np.array_equal(r.actions[0], rand[k]) and (S == 1 or np.array_equal(r.actions[1], base[k])), (tag, S, variant, k)
                assert got[k].trajectory_states(T).E == T * p['E']
                if S == 1:                                               # ... and the block has the single-size layout of ONE scheme
                    _, size = eval_result_layout(p['E'], p['n'], rb, T, 1)
                    assert got[k].eval_steps_result_bytes(T, 1) == size


@pytest.mark.parametrize("case", sorted(CASES))
def test_explore_only_every_pool_is_left_as_its_own_eval_steps_leaves_it(case):
    spec, T = CASES[case]
    _explore_only(spec, T, RB, case)


def test_explore_only_with_five_resource_blocks_and_36_lanes():
    """n + rb = 31 + 5 = 36 lanes at work in the finish.  The observation needs rb <= links (block r's V2I transmitter is vehicle
    r), so the small pool next to the 31-link one has 5 links, the fewest that five resource blocks admit; a pool of 4 links
    with five resource blocks is refused by the library like by v2x_eval_steps, with the pool's name."""
    import torch
    _explore_only([(1, 5), (2, 31)], 2, 5, 'rb5')
    pools = _pools([(1, 5), (2, 31)], 2, 0, 3, 5)
    chans = _start(pools, 5)
    table = _table(chans, 2)
    table[0].step.problem.n = 4
    m = EvalMixed(n_pools=2, T=2, pools=table, model=None)
    lib = load_library()
    assert lib.v2x_eval_steps_mixed(ctypes.byref(m), torch.cuda.current_stream().cuda_stream) == V2X_EINVAL
    err = lib.v2x_last_error(None).decode()
    assert err.startswith("eval_steps_mixed: pool 0 (4 links): ") and "1 <= C <= n" in err and "got n = 4, C = 5" in err, err


def test_a_baseline_channel_outside_the_range_makes_exactly_its_state_nan():
    spec, T = CASES['smallest_and_largest']
    pools = _pools(spec, T, 1, 17)
    explore = [np.ones((T, p['E']), np.uint8) for p in pools]
    rand = [p['policy'][1] for p in pools]
    good = [p['baseline'] for p in pools]
    k0, t0, e0 = 1, 1, 2                                                 # pool 1 (3 states of 5 links), step 1, state 2
    bad = [b.copy() for b in good]
    bad[k0][t0, e0, 3] = RB
    ref = _start(pools)
    want_rows = [dc.eval_steps(explore[k], rand[k], good[k], W_V2V, W_V2I).resolve() for k, dc in enumerate(ref)]
    got = _start(pools)
    got_rows = [r.resolve() for r in eval_steps_mixed(got, explore, rand, bad, W_V2V, W_V2I)]
    for k, p in enumerate(pools):
        hit = np.zeros((2, T, p['E']), bool)
        if k == k0:
            hit[1, t0, e0] = True
        for name in RATES:
            g, w = getattr(got_rows[k], name), getattr(want_rows[k], name)
            assert np.all(np.isnan(g[hit])) and g[~hit].tobytes() == w[~hit].tobytes() and np.all(np.isfinite(w)), (k, name)
        assert np.array_equal(got_rows[k].actions[1], bad[k]) and np.array_equal(got_rows[k].actions[0], rand[k]), k
        assert np.array_equal(got_rows[k].regular, want_rows[k].regular), k
        a, b = _snap(got[k], T), _snap(ref[k], T)
        for name in b:
            if name != 'result':
                assert a[name] == b[name], (k, name)


@pytest.mark.parametrize("case", ['smallest_and_largest', 'two_pools'])
def test_greedy_one_ragged_forward_scores_every_pool(case):
    import torch
    spec, T = CASES[case]
    eng = _ragged_engine()
    pools = _pools(spec, T, 1, 41)
    explore = [p['policy'][0] for p in pools]
    rand = [p['policy'][1] for p in pools]
    base = [p['baseline'] for p in pools]
    for ex in explore:                                                   # both flag values in every pool
        assert ex.any() and not ex.all()
    got = _start(pools)
    got_rows = eval_steps_mixed(got, explore, rand, base, W_V2V, W_V2I, engine=eng)
    torch.cuda.synchronize()

    # (1) the ragged batch is the concatenation of the pools' trajectory prefixes, the offsets are closed-form
    buf = mixed_rollout_buffers(got, T)
    gbase, rbase, ebase, (B, R, Ed) = mixed_rollout_bases(spec, T)
    assert buf['sizes'] == (B, R, Ed)
    ios = [dc.rollout_steps_buffers(T) for dc in got]
    want_xe = np.concatenate([io['xe'].cpu().numpy() for io in ios])
    want_col = np.concatenate([io['col'].cpu().numpy() for io in ios])
    want_off = np.concatenate([rbase[k] + np.arange(T * E) * n for k, (E, n) in enumerate(spec)] + [[R]]).astype(np.int32)
    want_rp = np.concatenate([ebase[k] + np.arange(T * E * n) * (n - 2) for k, (E, n) in enumerate(spec)] + [[Ed]]).astype(np.int32)
    assert want_xe.shape == (R, 16) and want_col.shape == (Ed,)
    assert buf['xe'].cpu().numpy().tobytes() == want_xe.tobytes() and buf['col_idx'].cpu().numpy().tobytes() == want_col.tobytes()
    assert np.array_equal(buf['graph_off'].cpu().numpy(), want_off) and np.array_equal(buf['row_ptr'].cpu().numpy(), want_rp)

    # (2) q is a second forward of that same device batch, bitwise
    n_max = spec[-1][1]
    db = DeviceBatch.from_tensors(B, 0, buf['xe'], buf['row_ptr'], buf['col_idx'], n_max * (n_max - 2), graph_off=buf['graph_off'],
                                  max_nodes=n_max)
    q = buf['q'].cpu().numpy().copy()
    again = eng.forward(db).cpu().numpy()
    assert q.shape == (R, RB) and np.all(np.isfinite(q)) and q.tobytes() == again.tobytes()

    # (3) the policy's actions are where(explore, random, argmax(q)), computed on the host
    expected = []
    for k, (E, n) in enumerate(spec):
        qk = q[rbase[k]:rbase[k] + T * E * n].reshape(T, E, n, RB)
        greedy = np.argmax(qk, axis=3).astype(np.int32)
        acts = np.ascontiguousarray(np.where(explore[k][:, :, None] != 0, rand[k], greedy), np.int32)
        assert np.any(greedy[explore[k] == 0] != rand[k][explore[k] == 0]), k           # otherwise the pool shows nothing
        assert np.array_equal(got_rows[k].resolve().actions[0], acts), k
        expected.append(acts)

    # (4) twins that explore those actions through their own eval_steps: the same bytes everywhere
    ref = _start(pools)
    want_rows = [dc.eval_steps(np.ones((T, p['E']), np.uint8), expected[k], base[k], W_V2V, W_V2I) for k, (dc, p) in enumerate(zip(ref, pools))]
    _assert_same(pools, T, 2, got, ref, got_rows, want_rows, case)
    for k, p in enumerate(pools):
        assert np.array_equal(got[k].download('actions').reshape(p['E'], p['n']), expected[k][-1]), k
    eng.close()


# ------------------------------------------------------------------------------------------------------- refusals
def _table(chans, T, baseline=True):
    table = (Eval * len(chans))()
    for k, dc in enumerate(chans):
        table[k] = dc.eval_steps_struct(T, W_V2V, W_V2I, baseline=baseline)
    return table


def test_a_refused_call_names_the_pool_and_leaves_every_state_and_result_alone():
    import torch
    lib = load_library()
    spec, T = [(2, 4), (3, 5)], 2
    pools = _pools(spec, T, 0, 9)
    chans = _start(pools)
    other = start_channels(3, 5, 3, pools[1]['state'])                   # the second pool with another channel count
    other0 = start_channels(2, 4, 3, pools[0]['state'])                  # ... and the first one (kept: the structs point into them)
    eng, fixed = _ragged_engine(), GnnEngine(GnnSpec(n_nodes=4, feat_dim=16, n_mp_layers=2))
    buf = mixed_rollout_buffers(chans, T)
    for dc in chans:
        dc._eval_io(T)['eval_result_dev'].fill_(7)
    before = [_snap(dc, T) for dc in chans]
    stream = torch.cuda.current_stream().cuda_stream

    def refused(text, pool=None, model=None, n_pools=None, call_T=T, table=None, no_table=False, xe_shift=0, **null):
        table = _table(chans, T) if table is None else table
        m = EvalMixed(n_pools=len(spec) if n_pools is None else n_pools, T=call_T, model=model)
        if not no_table:
            m.pools = table
        if model is not None:
            for name in ('xe', 'graph_off', 'row_ptr', 'col_idx', 'q'):
                setattr(m, name, None if null.get(name) else buf[name].data_ptr() + (xe_shift if name == 'xe' else 0))
        assert lib.v2x_eval_steps_mixed(ctypes.byref(m), stream) == V2X_EINVAL, text
        err = lib.v2x_last_error(None).decode()
        assert err.startswith("eval_steps_mixed: ") and text in err, (text, err)
        if pool is not None:
            assert "pool %d" % pool in err, (text, err)

    refused("1..8 pools", n_pools=0)
    refused("1..8 pools", n_pools=9)
    refused("non-null pool table", no_table=True)
    t = _table(chans, T)
    t[0], t[1] = _table(chans, T)[1], _table(chans, T)[0]
    refused("the link counts must ascend strictly", pool=1, table=t)
    t = _table(chans, T)
    t[1].T = T + 1
    refused("walks T = 3 steps, the call T = 2", pool=1, table=t)
    t = _table(chans, T)
    t[0].model = eng._h
    refused("has a model of its own", pool=0, table=t)
    t = _table(chans, T)                                                 # what v2x_eval_steps refuses of a pool: T E > 65535 ...
    big = 65535 // 3 + 1
    t[0].T = t[1].T = big                                                # (nothing is launched: the buffers need not hold that T)
    refused("T E <= 65535", pool=1, call_T=big, table=t)
    t = _table(chans, T)
    t[0].step.problem.n = 32                                             # ... more than 31 links
    refused("3..31 links", pool=0, table=t)
    t = _table(chans, T)
    t[1].traj_xe = None                                                  # ... a null workspace
    refused("null trajectory workspace pointer", pool=1, table=t)
    t = _table(chans, T)
    t[1].result_reward = None                                            # ... a null result
    refused("null result pointer", pool=1, table=t)
    t = _table(chans, T)
    t[1] = other.eval_steps_struct(T, W_V2V, W_V2I)
    refused("one channel count for all pools", pool=1, table=t)
    t = _table(chans, T)
    t[1].baseline_actions = None
    refused("one number of schemes for all pools", pool=1, table=t)
    refused("a variable_graphs model of 4 channels needed, got fixed-size graphs", model=fixed._h)
    t = _table(chans, T)                                                 # every pool with 3 channels: the model's 4 are not rb
    t[0], t[1] = other0.eval_steps_struct(T, W_V2V, W_V2I), other.eval_steps_struct(T, W_V2V, W_V2I)
    refused("a variable_graphs model of 3 channels needed, got variable graphs, 4 channels", model=eng._h, table=t)
    for name in ('xe', 'graph_off', 'row_ptr', 'col_idx'):
        refused("a model needs the ragged batch's xe / graph_off / row_ptr / col_idx", model=eng._h, **{name: True})
    refused("a model needs the Q workspace", model=eng._h, q=True)
    t = _table(chans, T)                                                 # what v2x_eval_steps refuses of a pool that is SCORED
    t[1].explore = None
    refused("Q-values need the explore flags", pool=1, model=eng._h, table=t)
    refused("the ragged batch's xe must be 16-byte aligned", model=eng._h, xe_shift=4)
    t = _table(chans, T)
    t[1].traj_xe += 4
    refused("traj_xe must be 16-byte aligned to be scored", pool=1, model=eng._h, table=t)

    assert [_snap(dc, T) for dc in chans] == before
    # the Python entry points refuse before any device work, too
    explore, rand, base = ([p['policy'][0] for p in pools], [p['policy'][1] for p in pools], [p['baseline'] for p in pools])
    with pytest.raises(ValueError, match="ascend strictly"):
        eval_steps_mixed(chans[::-1], explore[::-1], rand[::-1], base[::-1], W_V2V, W_V2I)
    with pytest.raises(ValueError, match="variable_graphs engine"):
        eval_steps_mixed(chans, explore, rand, base, W_V2V, W_V2I, engine=fixed)
    with pytest.raises(ValueError, match="one number of schemes for all pools"):
        eval_steps_mixed(chans, explore, rand, [base[0], None], W_V2V, W_V2I)
    with pytest.raises(ValueError, match=r"pool 1 \(5 links\) has a block of 3 steps, pool 0 of 2"):
        eval_steps_mixed(chans, [explore[0], np.ones((3, 3), np.uint8)], rand, base, W_V2V, W_V2I)
    with pytest.raises(ValueError, match=r"pool 1 \(5 links\): policy_random: an array of shape"):
        eval_steps_mixed(chans, explore, [rand[0], rand[1][:, :, :4]], base, W_V2V, W_V2I)
    with pytest.raises(ValueError, match="one channel count for all pools"):
        eval_steps_mixed([chans[0], other], explore, rand, base, W_V2V, W_V2I)
    with pytest.raises(ValueError, match="one explore per pool"):
        eval_steps_mixed(chans, explore[:1], rand, base, W_V2V, W_V2I)
    with pytest.raises(ValueError, match="1..8 pools"):
        eval_steps_mixed([], [], [], [], W_V2V, W_V2I)
    host_env = start_env_batched(4, 2, 5, backend="device", streams="host")
    with pytest.raises(ValueError, match="needs streams='device' in every environment"):
        resident_evaluate_steps_mixed([host_env], explore[:1], rand[:1], base[:1], W_V2V, W_V2I)
    with pytest.raises(ValueError, match="one policy_random per environment"):
        resident_evaluate_steps_mixed([host_env], explore[:1], rand, base[:1], W_V2V, W_V2I)
    assert [_snap(dc, T) for dc in chans] == before
    eng.close()
    fixed.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _force_irregular(env, e, link):
    """after every reset: link `link` of simulator e is its own receiver"""
    inner = env.new_random_game

    def reset(n_Veh=0):
        inner(n_Veh)
        env.dest[e, link] = link
        env._static_dirty = True
        env._dev_obs = None
    env.new_random_game = reset


def _eval_run(monkeypatch, sizes, Es, seed, backend, episodes, steps, eps, opt=False, irregular=None, eval_sizes=None, eval_Es=None):
    import torch
    # (irregular: the rollout test's helper marks the link once; test_run resets every episode, so the reset marks it again)
    agent = _agent(sizes, Es, seed, 'host', 0, 20, irregular)
    envs = agent.envs
    if eval_sizes is not None:
        envs = [start_env_batched(n, E, seed + 77 * k, backend="device", streams="device") for k, (n, E) in enumerate(zip(eval_sizes, eval_Es))]
    if irregular is not None:
        _force_irregular(envs[irregular[0]], irregular[1], irregular[2])
    flags, scored = [], []
    step, score = mixed.draw_eval_step, agent.score

    def spy(*a):                                                         # (taking the draws ahead calls draw_eval_step itself)
        out = step(*a)
        flags.extend(np.asarray(x).reshape(-1) for x in out[1])
        return out
    monkeypatch.setattr(mixed, 'draw_eval_step', spy)
    agent.score = lambda *a, **k: (scored.append(1), score(*a, **k))[1]
    books = agent.test_run(envs, episodes, steps, opt_flag=opt, opt_backend='device', fixed_epsilon=eps, eval_backend=backend)
    monkeypatch.setattr(mixed, 'draw_eval_step', step)
    torch.cuda.synchronize()
    run = dict(books=books, rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step, stats=dict(agent.eval_stats),
               explore=np.concatenate(flags), scored=len(scored),
               streams=[[np.array(a).copy() for a in (e._mt_keys, e._mt_pos, e.pos, e.dirs)] for e in envs],
               resident=[{k: e._dc.tensor(k).cpu().numpy().tobytes() for k in STATE} for e in envs])
    agent.close()
    return run


def _assert_same_run(h, d, sizes, Es, episodes, steps, schemes=('gnn', 'random')):
    assert sorted(h['books']) == sorted(d['books']) == sorted(sizes)
    for n, E in zip(sizes, Es):
        assert sorted(h['books'][n]) == sorted(d['books'][n]) == sorted(schemes)
        for s in schemes:
            shapes = [(episodes, E), (episodes, E, steps), (episodes, E, steps, n), (episodes, E, steps, RB), (episodes, E, steps, RB)]
            for a, b, shape in zip(h['books'][n][s], d['books'][n][s], shapes):
                assert a.shape == b.shape == shape and a.tobytes() == b.tobytes() and np.all(np.isfinite(a)), (n, s)
            assert np.all(h['books'][n][s][1] > 0), (n, s)
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] == episodes * steps * sum(Es)
    assert np.array_equal(h['explore'], d['explore'])
    for a, b in zip(h['streams'], d['streams']):
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
    for k, (a, b) in enumerate(zip(h['resident'], d['resident'])):
        for name in STATE:
            assert a[name] == b[name], (k, name)


def test_test_run_one_step_per_episode_with_everybody_greedy_equals_the_host_loop(monkeypatch):
    """sizes (4, 8, 12) with E = (2, 1, 3), T = 1: both forms score the same batch"""
    args = ((4, 8, 12), (2, 1, 3), 33)
    h = _eval_run(monkeypatch, *args, 'host', 3, 1, 0.0)
    d = _eval_run(monkeypatch, *args, 'device', 3, 1, 0.0)
    _assert_same_run(h, d, (4, 8, 12), (2, 1, 3), 3, 1)
    assert not h['explore'].any() and len(h['explore']) == 3 * 6 and h['scored'] == 3 and d['scored'] == 0
    assert h['stats'] == {'device_episodes': 0, 'host_episodes': 3} and d['stats'] == {'device_episodes': 3, 'host_episodes': 0}
    for n in (4, 8, 12):                                                 # the network's actions are not the baseline's
        assert h['books'][n]['gnn'][1].tobytes() != h['books'][n]['random'][1].tobytes()


@pytest.mark.parametrize("opt", [False, True])
def test_test_run_ten_steps_with_nobody_greedy_equals_the_host_loop(monkeypatch, opt):
    """sizes (4, 8) with E = (2, 3), T = 10, fixed_epsilon = 1: nobody is greedy (asserted), so the check does not lean on a ragged
    forward being independent of what else is in the batch; once with the optimum of every state (exhaustive search)"""
    args = ((4, 8), (2, 3), 12)
    h = _eval_run(monkeypatch, *args, 'host', 2, 10, 1.0, opt=opt)
    d = _eval_run(monkeypatch, *args, 'device', 2, 10, 1.0, opt=opt)
    schemes = ('gnn', 'random', 'optimal') if opt else ('gnn', 'random')
    _assert_same_run(h, d, (4, 8), (2, 3), 2, 10, schemes)
    assert h['explore'].all() and len(h['explore']) == 2 * 10 * 5 and h['scored'] == d['scored'] == 0
    assert d['stats'] == {'device_episodes': 2, 'host_episodes': 0}
    if opt:
        for n in (4, 8):
            best = h['books'][n]['optimal'][1]
            assert np.all(best >= h['books'][n]['gnn'][1] - 1e-9) and np.all(best >= h['books'][n]['random'][1] - 1e-9), n


def test_test_run_an_irregular_graph_takes_the_host_loop_and_equals_the_host_agent(monkeypatch):
    args = ((4, 8), (2, 3), 12)
    h = _eval_run(monkeypatch, *args, 'host', 1, 2, 0.0, irregular=(1, 2, 5))
    d = _eval_run(monkeypatch, *args, 'device', 1, 2, 0.0, irregular=(1, 2, 5))
    assert h['stats'] == d['stats'] == {'device_episodes': 0, 'host_episodes': 1}
    _assert_same_run(h, d, (4, 8), (2, 3), 1, 2)
    assert h['scored'] == d['scored'] == 2                               # (the host loop scores the irregular graph, too)


def test_test_run_on_link_counts_the_network_never_saw(monkeypatch):
    """evaluation sizes (4, 16) on an agent built for (8, 12)"""
    args = ((8, 12), (1, 1), 21)
    kw = dict(eval_sizes=(4, 16), eval_Es=(2, 1))
    h = _eval_run(monkeypatch, *args, 'host', 2, 1, 0.0, **kw)
    d = _eval_run(monkeypatch, *args, 'device', 2, 1, 0.0, **kw)
    _assert_same_run(h, d, (4, 16), (2, 1), 2, 1)
    assert d['stats'] == {'device_episodes': 2, 'host_episodes': 0}
    long = _eval_run(monkeypatch, *args, 'device', 1, 5, 0.0, **kw)       # several steps in one call: shapes and finite values
    for n, E in ((4, 2), (16, 1)):
        for s in ('gnn', 'random'):
            b = long['books'][n][s]
            assert [a.shape for a in b] == [(1, E), (1, E, 5), (1, E, 5, n), (1, E, 5, RB), (1, E, 5, RB)]
            assert all(np.all(np.isfinite(a)) for a in b) and np.all(b[1] > 0)
            assert np.allclose(b[0], b[1].sum(axis=2), rtol=1e-12)
    assert long['num_step'] == 5 * 3 and long['stats'] == {'device_episodes': 1, 'host_episodes': 0}


def test_test_run_refuses_host_simulators_before_any_draw_or_reset():
    agent = _agent((4, 8), (2, 3), 5, 'host', 0, 20)
    host_env = start_env_batched(4, 2, 5, backend="device", streams="host")
    np.random.seed(3)
    before = np.random.get_state()
    dest = [np.array(e.dest).copy() for e in agent.envs]
    with pytest.raises(ValueError, match="must be a DeviceBatchedEnviron with streams='device', got DeviceBatchedEnviron with streams='host'"):
        agent.test_run([host_env, agent.envs[1]], 1, 2, eval_backend='device')
    with pytest.raises(ValueError, match="opt_backend must be one of"):
        agent.test_run(agent.envs, 1, 2, opt_flag=True, opt_backend='host')
    assert _same_rng(np.random.get_state(), before) and agent.eval_stats == {'device_episodes': 0, 'host_episodes': 0}
    assert all(np.array_equal(e.dest, d) for e, d in zip(agent.envs, dest))
    agent.close()


# ------------------------------------------------------------------------------------------------------- weights
def test_saved_weights_load_into_a_freshly_seeded_agent(tmp_path):
    a, b = _agent((4, 8), (2, 3), 5, 'host', 0, 20), _agent((4, 8), (2, 3), 6, 'host', 0, 20)
    want = (a.online.get_flat().copy(), a.target.get_flat().copy())
    assert want[0].tobytes() != want[1].tobytes()
    assert b.online.get_flat().tobytes() != want[0].tobytes() and b.target.get_flat().tobytes() != want[1].tobytes()
    paths = a.save_weights(str(tmp_path / 'w'), 7, 3)
    assert [os.path.basename(p) for p in paths] == list(weight_file_names(7, 3, 32)) and all(os.path.exists(p) for p in paths)
    assert b.load_weights(str(tmp_path / 'w'), 7, 3) == paths
    assert b.online.get_flat().tobytes() == want[0].tobytes() and b.target.get_flat().tobytes() == want[1].tobytes()
    a.close()
    b.close()


def test_train_with_a_save_dir_writes_the_two_files(tmp_path):
    agent = _agent((4, 8), (2, 3), 5, 'host', 0, 20)
    folder = str(tmp_path / 'run')
    agent.train(1, 1, save_dir=folder)
    online, target = weight_file_names(1, 1, 32)
    assert sorted(os.listdir(folder)) == sorted([online, target])
    fresh = _agent((4, 8), (2, 3), 9, 'host', 0, 20)
    fresh.load_weights(folder, 1, 1)
    assert fresh.online.get_flat().tobytes() == agent.online.get_flat().tobytes()
    assert fresh.target.get_flat().tobytes() == agent.target.get_flat().tobytes()
    agent.close()
    fresh.close()
