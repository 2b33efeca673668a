"""GPU: the reward landscape (v2x_opt_landscape through OptimalAllocation.landscape / rank_of, csrc/v2xopt.hip) against a
numpy histogram of OptimalAllocation.rewards() -- the reward of every joint action index, existing code -- and, for the
ranks at 3 x 3 and 4 x 4, against the float64 numpy landscape() of tests/test_gpu_optimum.py."""
import ctypes
import math
import random

import numpy as np
import pytest

from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import decode, encode, problem_arrays
from test_gpu_optimum import W_V2I, W_V2V, Stack, landscape, make_state
from test_rl_agent import RecordingBrain
from test_rl_env import make_env

pytestmark = pytest.mark.gpu


def histogram(edges, r):
    """the definition of the slots: np.searchsorted(edges, r, 'right'), NaN rewards in slot K + 1"""
    K = len(edges)
    nan = np.isnan(r)
    c = np.bincount(np.searchsorted(edges, r[~nan], side='right'), minlength=K + 2).astype(np.int64)
    c[K + 1] = nan.sum()
    return c


def spread_edges(r, K):
    """K ascending edges over the sorted rewards: alternately exactly ON a reward value and BETWEEN two neighbours"""
    s = np.sort(r)
    at = np.linspace(0, s.size - 2, K + 2)[1:-1].astype(np.int64)
    ed = np.where(np.arange(K) % 2 == 0, s[at], 0.5 * (s[at] + s[at + 1]))
    assert np.all(np.diff(ed) >= 0)
    return ed


@pytest.fixture(scope="module")
def opt():
    return OptimalAllocation()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_27_joint_actions_with_owner_lanes_that_have_no_work(opt, seed):
    """3 x 3: 27 prefixes in one wave of 64 lanes, the second wave of the workgroup has none -- and up to 64 lanes own a
    slot.  1, 2, 7 and 62 edges, on reward values and between them."""
    env = make_state(3, 3, seed)
    r = opt.rewards(env, W_V2V, W_V2I)[0]
    s = np.sort(r)
    assert r.size == 27 and np.all(np.diff(s) > 0)
    mid = 0.5 * (s[:-1] + s[1:])
    all62 = np.sort(np.concatenate([s, mid, [s[0] - 1.0, s[0] - 0.5, s[-1] + 0.5, s[-1] + 1.0], np.nextafter(s[:5], np.inf)]))
    for edges in ([s[13]], [mid[5], s[20]], [s[2], mid[3], s[8], mid[12], s[13], s[20], mid[25]], all62):
        edges = np.asarray(edges)
        counts, sums = opt.landscape(env, W_V2V, W_V2I, edges)
        assert counts.shape == (1, edges.size + 2) and counts.dtype == np.int64 and sums.shape == (1,)
        assert np.array_equal(counts[0], histogram(edges, r)), edges.size
        assert counts[0].sum() == 27 and counts[0, -1] == 0
        assert abs(sums[0] - math.fsum(r)) <= 1e-12 * abs(math.fsum(r))


@pytest.mark.parametrize("n,m", [(4, 0), (10, 1), (12, 3)])
def test_counts_and_sum_at_every_suffix_length(opt, n, m):
    """n x 4 as one state: opt_plan walks m = 0 / 1 / 3 suffix digits per thread (4^n, 4^9, 4^9 prefixes).  16 edges;
    the sum against math.fsum to 1e-12 relative (per thread at most 64 terms in sequence, then a tree of about 20 levels:
    below 1e-14), and bit-identical between two calls."""
    env = make_state(n, 4, 300 + n)
    r = opt.rewards(env, W_V2V, W_V2I)[0]
    edges = spread_edges(r, 16)
    counts, sums = opt.landscape(env, W_V2V, W_V2I, edges)
    assert np.array_equal(counts[0], histogram(edges, r))
    assert counts[0].sum() == 4 ** n
    want = math.fsum(r)
    print("n = %d: sum %r, fsum %r, relative error %.3g" % (n, sums[0], want, abs(sums[0] - want) / abs(want)))
    assert abs(sums[0] - want) <= 1e-12 * abs(want)
    counts2, sums2 = opt.landscape(env, W_V2V, W_V2I, edges)
    assert sums2.tobytes() == sums.tobytes() and np.array_equal(counts2, counts)


def test_fifty_stacked_states_with_their_own_edges(opt):
    envs = [make_state(8, 4, 500 + s) for s in range(50)]
    stack = Stack(envs)
    r = opt.rewards(stack, W_V2V, W_V2I)
    edges = np.stack([spread_edges(r[e], 9 + e % 5)[:9] for e in range(50)])
    assert len({row.tobytes() for row in edges}) == 50
    counts, sums = opt.landscape(stack, W_V2V, W_V2I, edges)
    assert counts.shape == (50, 11) and sums.shape == (50,)
    for e, env in enumerate(envs):
        one, one_sum = opt.landscape(env, W_V2V, W_V2I, edges[e])
        assert np.array_equal(counts[e], one[0]), e
        assert np.array_equal(counts[e], histogram(edges[e], r[e])), e
        assert abs(sums[e] - one_sum[0]) <= 1e-12 * abs(one_sum[0])


def test_three_hundred_stacked_states_take_a_second_partial_turn(opt):
    """300 stacked 5 x 16 states.  opt_plan: want = 2^19 / 300 = 1747 prefixes, m stops at 2 (three suffix digits would need
    72,832 bytes of LDS, over the 63 KiB cap), so 16^3 = 4,096 prefixes of 256 suffixes per state; the workgroups are capped
    at 8192 / 300 = 27 per state = 3,456 threads, so the grid-stride loop takes a second turn in which only 640 of them
    (5 workgroups) have a prefix."""
    envs = [make_state(5, 16, 900 + s) for s in range(300)]
    r0 = opt.rewards(envs[0], W_V2V, W_V2I)[0]
    edges = spread_edges(r0, 16)
    counts, sums = opt.landscape(Stack(envs), W_V2V, W_V2I, edges)
    assert counts.shape == (300, 18)
    assert np.all(counts.sum(axis=1) == 16 ** 5) and np.all(counts[:, -1] == 0)
    assert np.array_equal(counts[0], histogram(edges, r0))
    for e in (0, 149, 299):
        one, _ = opt.landscape(envs[e], W_V2V, W_V2I, edges)
        assert np.array_equal(counts[e], one[0]), e


def test_rank_of_the_optimum_and_of_a_flat_landscape(opt):
    for n, rb in ((4, 4), (8, 4), (5, 16)):
        env = make_state(n, rb, 40 + n)
        index, reward = opt.search(env, W_V2V, W_V2I)
        rk = opt.rank_of(env, W_V2V, W_V2I, decode(index, n, rb))
        assert rk['better'].shape == (1,) and rk['better'][0] == 0 and rk['equal'][0] >= 1
        assert rk['total'] == rb ** n and rk['reward'][0].tobytes() == reward[0].tobytes()
        r = opt.rewards(env, W_V2V, W_V2I)[0]
        assert abs(rk['mean_reward'][0] - math.fsum(r) / r.size) <= 1e-12 * abs(rk['mean_reward'][0])
        assert rk['equal'][0] == np.sum(r == reward[0])
        flat = opt.rank_of(env, 0.0, 0.0, np.zeros((1, 3, n), int) + np.arange(3)[None, :, None] % rb)
        assert np.all(flat['equal'] == rb ** n) and np.all(flat['better'] == 0) and flat['better'].shape == (1, 3)


@pytest.mark.parametrize("n,rb", [(4, 4), (3, 3)])
def test_ranks_match_the_numpy_landscape(opt, n, rb):
    """No two rewards of these states lie within 1e-9 relative of each other, and device and numpy rewards agree to 1e-12:
    the order of the numpy landscape is the order of the device rewards."""
    rng = np.random.default_rng(17 * n)
    for seed in range(3):
        env = make_state(n, rb, seed)
        ref = landscape(env)
        s = np.sort(ref)
        assert np.all(np.diff(s) > 1e-9 * s[1:])
        actions = rng.integers(0, rb, size=(1, 8, n))
        idx = encode(actions, rb)[0]
        rk = opt.rank_of(env, W_V2V, W_V2I, actions)
        assert np.array_equal(rk['better'][0], [(ref > ref[i]).sum() for i in idx])
        assert np.array_equal(rk['equal'][0], [(ref == ref[i]).sum() for i in idx])
        assert abs(rk['mean_reward'][0] - ref.mean()) <= 1e-11 * ref.mean()


def test_receiver_out_of_range_puts_every_action_in_the_nan_slot(opt):
    """through the C ABI (the Python wrapper refuses such a state): the link's table entries are NaN, so every reward is"""
    import torch
    from v2xgnn.lib import OptProblem, check
    env = make_state(4, 4, 3)
    v2v, v2i, v2i_abs, dest, const = problem_arrays(env)
    dest = dest.copy()
    dest[0, 2] = 4
    opt._init_device()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(opt.device) for a in (v2v, v2i, v2i_abs, dest)]
    prob = OptProblem(E=1, n=4, rb=4, pad_=0, v2v_ff=dev[0].data_ptr(), v2i_ff=dev[1].data_ptr(), v2i_abs=dev[2].data_ptr(),
                      dest=dev[3].data_ptr(), w_v2v=W_V2V, w_v2i=W_V2I, **const)
    lib = opt._lib
    need = int(lib.v2x_opt_landscape_workspace_bytes(ctypes.byref(prob), 3))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=opt.device)
    edges = torch.tensor([1.0, float('nan'), 1e9], dtype=torch.float64, device=opt.device)
    counts = torch.full((5,), -1, dtype=torch.int64, device=opt.device)
    sums = torch.zeros(1, dtype=torch.float64, device=opt.device)
    stream = torch.cuda.current_stream(opt.device).cuda_stream
    check(lib, lib.v2x_opt_landscape(ctypes.byref(prob), ws.data_ptr(), edges.data_ptr(), 3, counts.data_ptr(), sums.data_ptr(),
                                     stream))
    assert counts.cpu().tolist() == [0, 0, 0, 0, 256] and math.isnan(sums.item())
    # the argument checks of the entry point, and a null `sums`
    for bad in (0, 63):
        assert lib.v2x_opt_landscape_workspace_bytes(ctypes.byref(prob), bad) < 0
        assert lib.v2x_opt_landscape(ctypes.byref(prob), ws.data_ptr(), edges.data_ptr(), bad, counts.data_ptr(), None, stream) < 0
        assert b"n_edges" in lib.v2x_last_error(None)
    assert lib.v2x_opt_landscape(ctypes.byref(prob), ws.data_ptr(), None, 3, counts.data_ptr(), None, stream) < 0
    assert lib.v2x_opt_landscape(ctypes.byref(prob), ws.data_ptr(), edges.data_ptr(), 3, None, None, stream) < 0
    assert lib.v2x_opt_landscape(ctypes.byref(prob), None, edges.data_ptr(), 3, counts.data_ptr(), None, stream) < 0
    check(lib, lib.v2x_opt_landscape(ctypes.byref(prob), ws.data_ptr(), edges.data_ptr(), 3, counts.data_ptr(), None, stream))
    assert counts.cpu().tolist() == [0, 0, 0, 0, 256]


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def test_test_run_records_the_ranks_of_every_visited_state(opt):
    outs, seen = [], []
    for rank in (False, True):
        random.seed(4242)
        np.random.seed(4242)
        agent = _agent(make_env())
        if rank:                                   # the state each step acts in, as rewards() sees it (no RNG draw)
            act, draw, last = agent.act, agent.select_action_random, []

            def select_action_random(state):
                last[:] = [draw(state)]
                return last[0]

            def act_and_note(action):
                r = opt.rewards(agent.env, agent.v2v_weight, agent.v2i_weight)[0]
                seen.append((r, int(encode(np.asarray(action).reshape(1, -1), 4)[0]),
                             int(encode(np.asarray(last[0]).reshape(1, -1), 4)[0])))
                return act(action)

            agent.act, agent.select_action_random = act_and_note, select_action_random
        outs.append(agent.test_run(2, 3, opt_flag=True, opt_backend='device', opt_rank=rank))
    assert len(outs[0]) == len(outs[1]) == 15
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    book = agent.rank_book
    assert len(seen) == 6 and all(v.shape == (2, 3) for v in book.values())
    for k, (r, gnn, ra) in enumerate(seen):
        ep, st = divmod(k, 3)
        assert book['better'][ep, st] == np.sum(r > r[gnn]) and book['equal'][ep, st] == np.sum(r == r[gnn])
        assert book['ra_better'][ep, st] == np.sum(r > r[ra]) and book['ra_equal'][ep, st] == np.sum(r == r[ra])
        assert book['total'][ep, st] == 256
        assert abs(book['uniform_mean_reward'][ep, st] - math.fsum(r) / 256) <= 1e-12 * math.fsum(r) / 256
