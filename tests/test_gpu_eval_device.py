"""GPU: an evaluation episode on the resident state (v2x_eval_steps: k_sim_trajectory, one forward, k_eval_finish of
csrc/v2xsimdev.hip; DeviceChannels.eval_steps / trajectory_states; Agent.test_run / evaluate_training_diff_trials with
eval_backend='device').  The reference everywhere is the step-by-step path on an identically initialised twin -- rates() of
the baseline, rates() of the policy's actions, advance() -- or the agent's host loop on a twin environment, and everything is
compared byte for byte: the same device functions run the same expressions in the same order, so no tolerance applies, with
one exception that is stated where it is used (the mean over all joint actions, whose summation order follows the launch plan).

The engine scores 4 channels only, so the cases with rb = 1 and rb = 5 run without a model (everybody explores)."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_rollout_trajectory import STATE, _engine, _policy, _row_ptr, _same_rng, _storage, start_channels, start_state
from v2xgnn.lib import V2X_EINVAL, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, RL_Config
from v2xgnn.rl.optimum import OptimalAllocation, decode
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

W_V2V, W_V2I = 1.0, 0.1
RATES = ('v2v_rate', 'v2i_rate', 'interference')


def _snapshot(dc):
    import torch
    torch.cuda.synchronize()
    return {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}


def _np_reward(v2v, v2i):
    """w_v2v * sum(V2V rates) + w_v2i * sum(V2I rates) per state, as the agent's books compute it"""
    return np.array([W_V2V * np.sum(a) + W_V2I * np.sum(b) for a, b in zip(v2v, v2i)])


def _policy_actions(E, n, rb, T, st, explore, rand, eng):
    """the policy's actions [T, E, n]: a v2x_rollout_steps run on a twin of its own, into scratch storage"""
    dc, scratch = start_channels(E, n, rb, st), _storage(T * E, n)
    dc.rollout_steps(explore, rand, scratch, 0, T * E, W_V2V, W_V2I, engine=eng, row_ptr=_row_ptr(T * E, n) if eng else None).resolve()
    return scratch['action'].cpu().numpy().reshape(T, E, n).astype(np.int32)


def _walk(E, n, rb, T, st, baseline, policy):
    """the twin, step by step -> (rates of both schemes {name: [2, T, E, ...]}, regular [T + 1, E], its state afterwards, the twin)"""
    twin = start_channels(E, n, rb, st)
    got = {k: [[], []] for k in RATES}
    regular = [twin.download('regular').astype(bool)]
    for t in range(T):
        for s, acts in ((1, baseline[t]), (0, policy[t])):               # the baseline first: the policy's rates stay resident
            twin.rates(acts)
            r = twin.fetch_rates()
            for k in RATES:
                got[k][s].append(r[k])
        twin.advance()
        regular.append(twin.download('regular').astype(bool))
    return {k: np.array(v) for k, v in got.items()}, np.stack(regular), _snapshot(twin), twin


CASES = [(1, 3, 1, 1), (3, 4, 4, 3), (2, 16, 4, 3), (2, 31, 5, 2), (1, 20, 4, 10)]


@pytest.mark.parametrize("E,n,rb,T", CASES)
def test_one_call_returns_and_leaves_what_the_single_steps_do(E, n, rb, T):
    eng = _engine(n) if rb == 4 else None
    rng = np.random.default_rng(7 * n + 3 * E + T)
    mtpos = [(0, 623, 624)[e % 3] for e in range(E)]
    st = start_state(E, n, 410 + n, mtpos)
    explore, rand = _policy(E, n, rb, T, rng, eng is not None)
    baseline = rng.integers(0, rb, size=(T, E, n)).astype(np.int32)
    policy = _policy_actions(E, n, rb, T, st, explore, rand, eng)
    assert np.array_equal(policy[explore != 0], rand[explore != 0])
    if eng is not None and T >= 2:
        assert not np.array_equal(policy[1], rand[1])                    # the all-greedy step took the network's actions
    want, want_regular, want_state, _ = _walk(E, n, rb, T, st, baseline, policy)

    dc = start_channels(E, n, rb, st)
    before = dict(dc.traffic)
    res = dc.eval_steps(explore, rand, baseline, W_V2V, W_V2I, engine=eng).resolve()
    got_state = _snapshot(dc)
    assert res.actions.shape == (2, T, E, n) and np.array_equal(res.actions[0], policy) and np.array_equal(res.actions[1], baseline)
    for k in RATES:
        g = getattr(res, k)
        assert g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k
        assert np.all(np.isfinite(g)), k
    for s in range(2):
        for t in range(T):
            assert res.reward[s, t].tobytes() == _np_reward(want['v2v_rate'][s, t], want['v2i_rate'][s, t]).tobytes(), (s, t)
    assert res.regular.shape == (T + 1, E) and np.array_equal(res.regular, want_regular) and res.regular.all()
    for name in STATE:
        assert got_state[name] == want_state[name], name
    io = dc.rollout_steps_buffers(T)
    o = io['offsets']['traj_regular']
    assert io['workspace'][o:o + (T + 1) * E].cpu().numpy().astype(bool).tobytes() == want_regular.tobytes()
    assert {k: dc.traffic[k] - before[k] for k in before} == {'bytes_up': dc.eval_steps_policy_bytes(T),
                                                              'bytes_down': dc.eval_steps_result_bytes(T, 2)}

    # without a baseline scheme the policy's outputs and the state are the same
    alone = start_channels(E, n, rb, st)
    one = alone.eval_steps(explore, rand, None, W_V2V, W_V2I, engine=eng).resolve()
    assert one.actions.shape == (1, T, E, n) and one.reward.shape == (1, T, E)
    for k in RATES + ('reward', 'actions'):
        assert getattr(one, k)[0].tobytes() == getattr(res, k)[0].tobytes(), k
    assert np.array_equal(one.regular, res.regular) and _snapshot(alone) == want_state

    # a baseline channel equal to rb makes exactly that (scheme, t, e) NaN and nothing else
    t0, e0 = T - 1, E - 1
    bad = baseline.copy()
    bad[t0, e0, n // 2] = rb
    other = start_channels(E, n, rb, st)
    nan = other.eval_steps(explore, rand, bad, W_V2V, W_V2I, engine=eng).resolve()
    hit = np.zeros((2, T, E), bool)
    hit[1, t0, e0] = True
    for k in RATES + ('reward',):
        g, w = getattr(nan, k), getattr(res, k)
        assert np.all(np.isnan(g[hit])) and g[~hit].tobytes() == w[~hit].tobytes(), k
    assert np.array_equal(nan.actions[1], bad) and np.array_equal(nan.actions[0], policy) and _snapshot(other) == want_state
    if eng is not None:
        eng.close()


def test_the_stacked_search_returns_every_states_own_optimum():
    E, n, rb, T = 2, 4, 4, 3
    eng = _engine(n)
    rng = np.random.default_rng(12)
    st = start_state(E, n, 77, [623, 0])
    explore, rand = _policy(E, n, rb, T, rng, True)
    policy = _policy_actions(E, n, rb, T, st, explore, rand, eng)
    opt = OptimalAllocation()
    twin = start_channels(E, n, rb, st)
    want_index, want_reward, want_rates = [], [], {k: [] for k in RATES}
    for t in range(T):
        index, reward = opt.search(twin, W_V2V, W_V2I)
        want_index.append(index)
        want_reward.append(reward)
        twin.rates(decode(index, n, rb))
        r = twin.fetch_rates()
        for k in RATES:
            want_rates[k].append(r[k])
        twin.rates(policy[t])
        twin.advance()
    dc = start_channels(E, n, rb, st)
    dc.eval_steps(explore, rand, None, W_V2V, W_V2I, engine=eng).resolve()
    states = dc.trajectory_states(T)
    assert (states.E, states.n_Veh, states.n_RB) == (T * E, n, rb)
    tensors, _ = states.problem_tensors()
    ws = dc.rollout_steps_buffers(T)['workspace']
    assert tensors[0].data_ptr() == ws.data_ptr() + dc.rollout_steps_buffers(T)['offsets']['traj_v2v_ff']      # a view, no copy
    index, reward = opt.search(states, W_V2V, W_V2I)
    assert index.shape == (T * E,) and index.tobytes() == np.concatenate(want_index).tobytes()
    assert reward.tobytes() == np.concatenate(want_reward).tobytes() and len(set(index.tolist())) > 1
    got = states.rates(decode(index, n, rb))
    for g, k in zip(got, RATES):
        assert g.tobytes() == np.concatenate(want_rates[k]).tobytes(), k
    eng.close()


def test_a_refused_call_leaves_every_resident_tensor_alone():
    import torch
    lib = load_library()
    E, n, rb, T = 3, 4, 4, 3
    dc = start_channels(E, n, rb, start_state(E, n, 78))
    eng, wide = _engine(n), _engine(8)
    before = _snapshot(dc)
    stream = torch.cuda.current_stream().cuda_stream

    def refused(r, word):
        assert lib.v2x_eval_steps(ctypes.byref(r), stream) == V2X_EINVAL
        assert word in lib.v2x_last_error(None).decode(), lib.v2x_last_error(None).decode()

    r = dc.eval_steps_struct(T, W_V2V, W_V2I, engine=eng)
    r.T = 65535 // E + 1
    refused(r, "T E <= 65535")
    r = dc.eval_steps_struct(T, W_V2V, W_V2I, engine=eng)
    r.batch.xe = dc.tensor('xe').data_ptr()                              # the resident observation: not the trajectory's entries
    refused(r, "traj_xe / traj_col")
    r = dc.eval_steps_struct(T, W_V2V, W_V2I, engine=eng)
    r.model = wide._h
    refused(r, "a fixed-size model of 4 links and 4 channels needed, got 8 links")
    three = start_channels(E, n, 3, start_state(E, n, 79))               # three resource blocks: the model scores four channels
    refused(three.eval_steps_struct(T, W_V2V, W_V2I, engine=eng), "got 4 links, 4 channels")
    with pytest.raises(ValueError, match="T E <= 65535"):
        dc.eval_steps(np.ones((21846, E), np.uint8), np.zeros((21846, E, n), np.int8), None, W_V2V, W_V2I)
    assert _snapshot(dc) == before
    eng.close()
    wide.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _agent(n, seed, force_irregular=False):
    random.seed(seed)
    np.random.seed(seed)
    env = start_env_batched(n, 1, seed, lookahead=False, backend="device", streams="device")
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=seed, device_replay=False)
    assert type(env) is DeviceBatchedEnviron
    if force_irregular:                                                  # after every reset: a link that is its own receiver
        inner = env.new_random_game

        def reset(n_Veh=0):
            inner(n_Veh)
            env.dest[0, 2] = 2
            env._static_dirty = True
            env._dev_obs = None
        env.new_random_game = reset
    return env, agent


def _run(n, seed, call, force_irregular=False):
    env, agent = _agent(n, seed, force_irregular)
    out = call(agent)
    run = dict(out=[np.asarray(a).copy() for a in out], rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step,
               streams=[np.array(a).copy() for a in (env._mt_keys, env._mt_pos, env.pos, env.dirs)], stats=dict(agent.eval_stats),
               book={k: np.array(v).copy() for k, v in getattr(agent, 'rank_book', {}).items()})
    agent.brain.close()
    return run


def _assert_same(h, d, count, episodes):
    assert len(h['out']) == len(d['out']) == count
    for i, (a, b) in enumerate(zip(h['out'], d['out'])):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), i
        assert np.all(np.isfinite(a)), i
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] > 0
    for a, b in zip(h['streams'], d['streams']):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert d['stats'] == {'device_episodes': episodes, 'host_episodes': 0}      # no silent fallback: every episode was regular
    assert h['stats'] == {'device_episodes': 0, 'host_episodes': episodes}


@pytest.mark.parametrize("n,opt_backend,restarts", [(4, 'device', None), (8, 'bound', None), (8, 'local', 64), (4, 'host', None)])
def test_test_run_on_the_device_is_the_host_loop_bit_for_bit(n, opt_backend, restarts):
    call = lambda backend: (lambda a: a.test_run(2, 3, True, opt_backend=opt_backend, opt_restarts=restarts,      # noqa: E731
                                                 eval_backend=backend))
    h, d = _run(n, 31, call('host')), _run(n, 31, call('device'))
    _assert_same(h, d, 15, 2)
    assert h['num_step'] == 6
    assert np.all(h['out'][11] > 0) and len(set(h['out'][1].reshape(-1).tolist())) == 6       # optimum rewards; distinct policy rewards
    if opt_backend != 'local':                                           # (the local search is a lower bound on the optimum)
        assert np.all(h['out'][11] >= h['out'][1] - 1e-9) and np.all(h['out'][11] >= h['out'][6] - 1e-9)


def test_test_run_with_ranks_on_the_device_is_the_host_loop():
    n, M = 4, 4 ** 4
    call = lambda backend: (lambda a: a.test_run(2, 3, False, opt_rank=True, eval_backend=backend))      # noqa: E731
    h, d = _run(n, 32, call('host')), _run(n, 32, call('device'))
    _assert_same(h, d, 10, 2)
    for k in ('better', 'equal', 'ra_better', 'ra_equal', 'total'):
        assert h['book'][k].shape == (2, 3) and np.array_equal(h['book'][k], d['book'][k]), k
    assert np.all(h['book']['total'] == M) and np.all(h['book']['equal'] >= 1)
    # two orderings of an fp64 sum of M non-negative terms differ by at most 2 M 2^-53 relative (the landscape's sum follows the
    # launch plan, which differs between a stacked and a single-state call)
    a, b = h['book']['uniform_mean_reward'], d['book']['uniform_mean_reward']
    assert np.all(a > 0) and np.all(np.abs(a - b) <= 2 * M * 2.0 ** -53 * np.abs(a))


@pytest.mark.parametrize("opt_flag", [False, True])
def test_the_trials_on_the_device_are_the_host_loop_bit_for_bit(opt_flag):
    call = lambda backend: (lambda a: a.evaluate_training_diff_trials(5, 2, opt_flag, 0.5, 2, load=False,      # noqa: E731
                                                                       eval_backend=backend))
    h, d = _run(4, 33, call('host')), _run(4, 33, call('device'))
    _assert_same(h, d, 9 if opt_flag else 5, 2)
    assert h['num_step'] == 4


def test_an_irregular_episode_runs_on_the_host_loop():
    call = lambda backend: (lambda a: a.test_run(1, 2, False, eval_backend=backend))      # noqa: E731
    h, d = _run(4, 34, call('host'), True), _run(4, 34, call('device'), True)
    assert h['stats'] == d['stats'] == {'device_episodes': 0, 'host_episodes': 1}
    for a, b in zip(h['out'], d['out']):
        assert a.tobytes() == b.tobytes()
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] == 2
    for a, b in zip(h['streams'], d['streams']):
        assert a.tobytes() == b.tobytes()
