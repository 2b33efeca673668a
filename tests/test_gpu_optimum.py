"""GPU: the exhaustive optimal-allocation search (csrc/v2xopt.hip through v2xgnn.rl.optimum) against a float64 numpy
evaluation of the reward of every joint action, the reference's own evaluation runs (tests/golden) and the host brute force
of Agent._brute_force."""
import os
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import decode
from test_rl_agent import RecordingBrain
from test_rl_env import make_env
from util import GOLDEN

pytestmark = pytest.mark.gpu

W_V2V, W_V2I = 1.0, 0.1
TOL = 1e-12


def _tol(r):
    return TOL * np.maximum(1.0, np.abs(r))


class Stack(object):
    """E simulator states as the arrays BatchedEnviron exposes (what OptimalAllocation reads of a batched simulator)."""

    def __init__(self, envs):
        e0 = envs[0]
        self.E, self.n_Veh, self.n_RB, self.n_Neighbor = len(envs), len(e0.vehicles), e0.n_RB, 1
        self.V2V_channels_with_fastfading = np.stack([e.V2V_channels_with_fastfading for e in envs])
        self.V2I_channels_with_fastfading = np.stack([e.V2I_channels_with_fastfading for e in envs])
        self.V2I_channels_abs = np.stack([e.V2I_channels_abs for e in envs])
        self.dest = np.array([[v.destinations[0] for v in e.vehicles] for e in envs], np.int64)
        self.activate_links = np.ones((self.E, self.n_Veh, 1), bool)
        for k in ('V2V_power_dB_List', 'fixed_v2v_power_index', 'V2I_power_dB', 'vehAntGain', 'bsAntGain', 'bsNoiseFigure',
                  'vehNoiseFigure', 'sig2'):
            setattr(self, k, getattr(e0, k))

    def finish_step(self):
        pass


def make_state(n, rb, seed):
    """A simulator state of n links over rb RBs: the reference simulator of ceil(n / 4) * 4 vehicles, cut to n links with
    receivers redrawn among them when n is not a multiple of 4."""
    random.seed(seed)
    np.random.seed(seed)
    env = make_env()
    env.n_RB = rb
    env.new_random_game(-(-n // 4) * 4)
    if len(env.vehicles) != n:
        rng = np.random.default_rng(seed)
        env.vehicles = env.vehicles[:n]
        for i, v in enumerate(env.vehicles):
            v.destinations = [int((i + 1 + rng.integers(n - 1)) % n)]
        env.V2V_channels_with_fastfading = env.V2V_channels_with_fastfading[:n, :n].copy()
        env.V2I_channels_with_fastfading = env.V2I_channels_with_fastfading[:n].copy()
        env.V2I_channels_abs = env.V2I_channels_abs[:n].copy()
        env.activate_links = env.activate_links[:n].copy()
        env.n_Veh = n
    return env


def landscape(env, w_v2v=W_V2V, w_v2i=W_V2I, idx=None, chunk=1 << 15):
    """float64 reward of every joint action index (or of `idx`), written from the formula of the issue: chunked and
    vectorised over joint actions."""
    n, rb = len(env.vehicles), env.n_RB
    v2v, v2i, v2i_abs = env.V2V_channels_with_fastfading, env.V2I_channels_with_fastfading, env.V2I_channels_abs
    rx = np.array([v.destinations[0] for v in env.vehicles])
    p_v2v = env.V2V_power_dB_List[env.fixed_v2v_power_index]
    gain = 2 * env.vehAntGain - env.vehNoiseFigure
    bs_gain = env.vehAntGain + env.bsAntGain - env.bsNoiseFigure
    L, K, Cc = np.arange(n)[:, None, None], np.arange(n)[None, :, None], np.arange(rb)[None, None, :]
    sig = 10 ** ((p_v2v - v2v[np.arange(n)[:, None], rx[:, None], np.arange(rb)[None, :]] + gain) / 10)        # [l, c]
    cm = np.minimum(np.arange(rb), n - 1)
    tx = np.where(np.arange(rb)[None, :] < n,
                  10 ** ((env.V2I_power_dB - v2v[cm[None, :], rx[:, None], np.arange(rb)[None, :]] + gain) / 10), 0.0)
    cross = 10 ** ((p_v2v - v2v[K, rx[L], Cc] + gain) / 10)                                                  # [l, k, c]
    bs = 10 ** ((p_v2v - v2i + bs_gain) / 10)                                                                # [l, c]
    m = min(rb, n)
    v2i_sig = 10 ** ((env.V2I_power_dB - v2i_abs[:m] + bs_gain) / 10)
    idx = np.arange(rb ** n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
    out = np.empty(idx.size)
    eye = np.eye(n, dtype=bool)
    for s in range(0, idx.size, chunk):
        a = decode(idx[s:s + chunk], n, rb)                                                                  # [B, n]
        same = (a[:, :, None] == a[:, None, :]) & ~eye
        cv = cross[np.arange(n)[None, :, None], np.arange(n)[None, None, :], a[:, :, None]]                   # [B, l, k]
        intf = tx[np.arange(n)[None, :], a] + (cv * same).sum(axis=2) + env.sig2
        v2v_rate = np.log2(1 + sig[np.arange(n)[None, :], a] / intf)
        onehot = a[:, :, None] == np.arange(m)[None, None, :]
        at_bs = (bs[:, :m][None] * onehot).sum(axis=1)
        v2i_rate = np.log2(1 + v2i_sig[None, :] / (at_bs + env.sig2))
        out[s:s + chunk] = w_v2v * v2v_rate.sum(axis=1) + w_v2i * v2i_rate.sum(axis=1)
    return out


def env_reward(env, index, w_v2v=W_V2V, w_v2i=W_V2I):
    n, rb = len(env.vehicles), env.n_RB
    v2v, v2i, _ = env.compute_reward_with_channel_selection(decode(index, n, rb)[0].reshape(n, 1))
    return w_v2v * np.sum(v2v) + w_v2i * np.sum(v2i)


def test_oracle_matches_the_simulator_reward():
    rng = np.random.default_rng(3)
    for n, rb in ((4, 4), (5, 2), (8, 4), (4, 6), (10, 4)):
        env = make_state(n, rb, 40 + n)
        idx = rng.integers(0, rb ** n, size=64)
        got = landscape(env, idx=idx)
        want = np.array([env_reward(env, int(i)) for i in idx])
        assert np.all(np.abs(got - want) <= _tol(want)), (n, rb, np.abs(got - want).max())


def _check_landscape(opt, envs, E_call):
    """rewards() of every index against the oracle; search() against rewards(); the argmax against the oracle's."""
    stack = Stack(envs) if E_call > 1 else envs[0]
    gpu = opt.rewards(stack, W_V2V, W_V2I)
    index, reward = opt.search(stack, W_V2V, W_V2I)
    assert gpu.shape == (len(envs), envs[0].n_RB ** len(envs[0].vehicles))
    for e, env in enumerate(envs):
        ref = landscape(env)
        assert np.all(np.abs(gpu[e] - ref) <= _tol(ref)), np.abs(gpu[e] - ref).max()
        best = int(np.argmax(gpu[e]))
        assert index[e] == best and reward[e].tobytes() == gpu[e, best].tobytes()
        top = np.sort(ref)[::-1]
        if top[0] - top[1] > 1e-9 * abs(top[0]):
            assert index[e] == int(np.argmax(ref))


@pytest.mark.parametrize("n,rb", [(4, 4), (8, 4), (5, 2), (6, 3), (4, 6), (10, 4)])
def test_full_landscape_matches_numpy(n, rb):
    opt = OptimalAllocation()
    envs = [make_state(n, rb, 100 * n + rb + s) for s in range(1 if n >= 10 else 3)]
    _check_landscape(opt, envs[:1], 1)
    if len(envs) > 1:
        _check_landscape(opt, envs, len(envs))


def test_exact_ties_take_the_lowest_index():
    """Every gain equal and w_v2i = 0: a joint action's reward depends only on its sequence of per-link co-channel counts.
    GPU rewards are bitwise equal inside each group, and the search returns the smallest index of the best group."""
    n, rb = 6, 3
    env = make_state(n, rb, 7)
    env.V2V_channels_with_fastfading = np.full_like(env.V2V_channels_with_fastfading, 80.0)
    env.V2I_channels_with_fastfading = np.full_like(env.V2I_channels_with_fastfading, 80.0)
    env.V2I_channels_abs = np.full_like(env.V2I_channels_abs, 80.0)
    opt = OptimalAllocation()
    gpu = opt.rewards(env, 1.0, 0.0)[0]
    index, reward = opt.search(env, 1.0, 0.0)
    a = decode(np.arange(rb ** n), n, rb)
    counts = (a[:, :, None] == a[:, None, :]).sum(axis=2)                              # [idx, link]
    groups = {}
    for i, key in enumerate(map(bytes, counts.astype(np.int8))):
        groups.setdefault(key, []).append(i)
    best_val, best_first = None, None
    for key, members in groups.items():
        vals = gpu[members]
        assert np.all(vals.view(np.int64) == vals[0].view(np.int64)), key
        if best_val is None or vals[0] > best_val or (vals[0] == best_val and members[0] < best_first):
            best_val, best_first = vals[0], members[0]
    assert len(groups) > 3
    assert int(index[0]) == best_first and reward[0] == best_val


def test_twelve_links_beyond_the_host_cap():
    """4^12 = 16.7 M joint actions (the host path refuses them): search == max / first argmax of the device reward vector;
    the numpy oracle agrees at the returned index and at the 1,000 best GPU indices, none of which beats the optimum."""
    import torch
    env = make_state(12, 4, 12)
    opt = OptimalAllocation()
    vec = opt.rewards_device(env, W_V2V, W_V2I)[0]
    index, reward = opt.search(env, W_V2V, W_V2I)
    vmax = vec.max()
    assert reward[0].tobytes() == np.float64(vmax.item()).tobytes()
    assert int(index[0]) == int(torch.argmax(vec).item())
    top = torch.topk(vec, 1000).indices.cpu().numpy()
    idx = np.concatenate([[int(index[0])], top])
    ref = landscape(env, idx=idx)
    got = vec[torch.from_numpy(idx).to(vec.device)].cpu().numpy()
    assert np.all(np.abs(got - ref) <= _tol(ref))
    assert np.all(ref <= reward[0] + _tol(reward[0]))
    assert abs(env_reward(env, int(index[0])) - reward[0]) <= _tol(reward[0])


def _agent(env, n=None):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    n = env.n_Veh if n is None else n
    brain = RecordingBrain(n, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(n, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain), brain


def test_test_run_device_backend_reproduces_reference_run():
    """the setup of test_rl_agent.test_test_run_matches_reference_evaluation_loop with the optimum searched on the GPU"""
    g = np.load(os.path.join(GOLDEN, 'golden_testrun_n4.npz'))
    random.seed(int(g['seed']))
    np.random.seed(int(g['seed']))
    agent, _ = _agent(make_env())
    out = agent.test_run(int(g['episodes']), int(g['steps']), True, opt_backend='device')
    names = ['Expect_Return', 'Reward', 'Per_V2V_Rate', 'Per_V2I_Rate', 'Per_V2B_Interference']
    assert len(out) == 15
    for i, name in enumerate([p + n for p in ('', 'RA_', 'Opt_') for n in names]):
        assert out[i].shape == g[name].shape, name
        assert np.allclose(out[i], g[name], rtol=1e-9, atol=1e-12), name


def test_evaluate_training_diff_trials_device_backend_reproduces_reference_run(tmp_path):
    """the setup of test_rl_agent.test_evaluate_training_diff_trials_matches_reference_loop with opt_backend='device'"""
    import types
    g = np.load(os.path.join(GOLDEN, 'golden_evaltrials_n4.npz'))
    names_opt = ['Return', 'Reward', 'RA_Return', 'RA_Reward', 'Opt_Return', 'Opt_Reward', 'Opt_V2V', 'Opt_V2I', 'Opt_Interference']
    names_ra = ['Evaluated_Opt_Return', 'Return', 'Reward', 'RA_Return', 'RA_Reward']
    for opt_flag, names, tag in ((True, names_opt, 'opt/'), (False, names_ra, 'ra/')):
        random.seed(int(g['seed']))
        np.random.seed(int(g['seed']))
        env = make_env()
        agent, brain = _agent(env)
        brain.model = types.SimpleNamespace(load_weights=lambda p: None)
        brain.target_model = types.SimpleNamespace(load_weights=lambda p: None)
        out = agent.evaluate_training_diff_trials(int(g['episodes']), int(g['steps']), opt_flag, float(g['epsilon']),
                                                  int(g['trials']), model_dir=str(tmp_path), opt_backend='device')
        assert len(out) == len(names)
        for o, name in zip(out, names):
            assert o.shape == g[tag + name].shape, name
            assert np.allclose(o, g[tag + name], rtol=1e-9, atol=1e-12), name


def test_device_and_host_backends_agree_at_eight_links():
    outs = []
    for backend in ('host', 'device'):
        random.seed(808)
        np.random.seed(808)
        env = make_env()
        env.new_random_game(8)
        agent, _ = _agent(env, 8)
        outs.append(agent.test_run(1, 2, True, opt_backend=backend))
    for h, d in zip(*outs):
        assert np.array_equal(h, d)


def test_test_run_at_twelve_links_dominates_both_policies():
    random.seed(1212)
    np.random.seed(1212)
    env = make_env()
    env.new_random_game(12)
    agent, _ = _agent(env, 12)
    out = agent.test_run(1, 3, True, opt_backend='device')
    rl, ra, opt = out[1], out[6], out[11]
    assert np.all(opt > 0)
    assert np.all(opt >= np.maximum(rl, ra) - _tol(opt))


def test_batched_simulator_equals_single_state_searches():
    from v2xgnn.rl.train import start_env_batched
    env = start_env_batched(8, 8, seed=31, lookahead=False)
    opt = OptimalAllocation()
    index, reward = opt.search(env, W_V2V, W_V2I)
    assert index.shape == (8,) and reward.shape == (8,)
    for e in range(8):
        one = Stack.__new__(Stack)
        one.__dict__.update(E=1, n_Veh=env.n_Veh, n_RB=env.n_RB, n_Neighbor=1,
                            V2V_channels_with_fastfading=env.V2V_channels_with_fastfading[e:e + 1],
                            V2I_channels_with_fastfading=env.V2I_channels_with_fastfading[e:e + 1],
                            V2I_channels_abs=env.V2I_channels_abs[e:e + 1], dest=env.dest[e:e + 1],
                            activate_links=np.ones((1, env.n_Veh, 1), bool))
        for k in ('V2V_power_dB_List', 'fixed_v2v_power_index', 'V2I_power_dB', 'vehAntGain', 'bsAntGain', 'bsNoiseFigure',
                  'vehNoiseFigure', 'sig2'):
            setattr(one, k, getattr(env, k))
        i1, r1 = opt.search(one, W_V2V, W_V2I)
        assert i1[0] == index[e] and r1[0].tobytes() == reward[e].tobytes()
    # and the batched simulator's own numpy reward of the decoded optimum
    v2v, v2i, _ = env.compute_reward_with_channel_selection(decode(index, env.n_Veh, env.n_RB))
    host = W_V2V * v2v.reshape(8, -1).sum(axis=1) + W_V2I * v2i.sum(axis=1)
    assert np.all(np.abs(host - reward) <= _tol(reward))
