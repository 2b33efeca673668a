"""CPU: the host side of the counting branch and bound (v2x_opt_count_bound of csrc/v2xopt.hip, OptimalAllocation.count_better,
rank_of(..., backend='bound'), rank_backend='bound' of Agent.test_run): the C ABI is declared, exported and bound alike, the
workspace formula, every refusal by its own message before any device work, and the 128-bit arithmetic behind `open` on
hand-made per-depth counts.  No GPU is needed: a call that passes the checks fails on a machine without one with RuntimeError
("needs a GPU"), never ValueError."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, OptProblem
from v2xgnn.rl import Agent, OptimalAllocation, RL_Config
from v2xgnn.rl.optimum import (DEFAULT_MAX_NODES, DEFAULT_RANK_MAX_NODES, MAX_THRESHOLDS, check_thresholds, join128,
                               open_leaves)
from test_rl_agent import RecordingBrain
from test_rl_env import make_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _L = C.c_void_p, C.c_int32, C.c_int64
_U = C.POINTER(C.c_uint64)
ABI = [("v2x_opt_count_bound_workspace_bytes", "int64_t", _L, [C.POINTER(OptProblem), _I, _L]),
       ("v2x_opt_count_bound", "int", C.c_int, [C.POINTER(OptProblem), _P, _P, _I, _L, _P, _P, _P, _P, C.POINTER(_L), _P]),
       ("v2x_opt_count_open_leaves", "int", C.c_int, [_U, _I, _I, _U, _U])]


def _env(links=4):
    random.seed(5)
    np.random.seed(5)
    env = make_env()
    if links != 4:
        env.new_random_game(links)
    return env


def _agent(env):
    cfg = RL_Config()
    cfg.set_train_value(16, 0.5, 32, 1, 0.1)
    brain = RecordingBrain(env.n_Veh, 3, 1, cfg.Num_Feedback, env.n_Neighbor, env.n_RB)
    return Agent(env.n_Veh, env.n_RB, env.n_Neighbor, cfg.Num_Feedback, env, cfg, brain=brain)


def _problem(E=1, n=20, rb=4, w_v2v=1.0, w_v2i=0.1):
    return OptProblem(E=E, n=n, rb=rb, pad_=0, w_v2v=w_v2v, w_v2i=w_v2i, sig2=1e-11)


@pytest.mark.parametrize("name,ret,restype,argtypes", ABI)
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, argtypes):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), hdr)
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == len(argtypes)
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and bound[name][1] == argtypes


@pytest.mark.parametrize("E,n,rb,A", [(1, 20, 4, 1), (1, 20, 4, 31), (6, 8, 4, 5), (50, 3, 3, 2), (1, 5, 16, 7), (8192, 12, 4, 31)])
def test_workspace_is_the_searchs_plus_the_per_depth_counts(E, n, rb, A):
    """include/v2xgnn.h: v2x_opt_bound_workspace_bytes + E * n_thr * (n + 1) * 8 rounded up to 256"""
    lib = vlib.load_library()
    p = _problem(E, n, rb)
    base = lib.v2x_opt_bound_workspace_bytes(C.byref(p), 1000)
    assert base > 0
    assert lib.v2x_opt_count_bound_workspace_bytes(C.byref(p), A, 1000) == base + -(-(E * A * (n + 1) * 8) // 256) * 256


def test_workspace_has_no_cap_on_the_joint_actions_but_the_lanes_lds():
    """32 x 4 = 2^64 joint actions have no 64-bit index (the search refuses them) but can be counted; 32 x 10 needs 330 LDS
    values per lane, more than the 318 a workgroup of 64 lanes has"""
    lib = vlib.load_library()
    p = _problem(1, 32, 4)
    assert lib.v2x_opt_bound_workspace_bytes(C.byref(p), 10) == V2X_EINVAL
    assert lib.v2x_opt_count_bound_workspace_bytes(C.byref(p), 2, 10) > 0
    OptimalAllocation.check_count(32, 4, 1.0, 0.1)
    OptimalAllocation.check_count(30, 10, 1.0, 0.1)                        # 310 values
    assert lib.v2x_opt_count_bound_workspace_bytes(C.byref(_problem(1, 30, 10)), 2, 10) > 0
    assert lib.v2x_opt_count_bound_workspace_bytes(C.byref(_problem(1, 32, 10)), 2, 10) == V2X_EINVAL
    assert b"bytes of LDS" in lib.v2x_last_error(None)
    with pytest.raises(ValueError, match=r"330 values per lane in LDS, 318 at most"):
        OptimalAllocation.check_count(32, 10, 1.0, 0.1)


@pytest.mark.parametrize("kw,A,max_nodes,text", [
    (dict(w_v2v=-1.0), 2, 10, b"weights"), (dict(w_v2i=-0.1), 2, 10, b"weights"), (dict(w_v2v=float('nan')), 2, 10, b"weights"),
    (dict(), 0, 10, b"n_thr = 0"), (dict(), 32, 10, b"n_thr = 32"), (dict(), 2, 0, b"max_nodes = 0"),
    (dict(n=33), 2, 10, b"n = 33 links"), (dict(rb=1), 2, 10, b"rb = 1 channels"), (dict(rb=17), 2, 10, b"rb = 17 channels"),
    (dict(E=65535), 5, 10, b"root items exceed the queue")])
def test_the_library_refuses_each_bad_argument_by_name(kw, A, max_nodes, text):
    """both entry points, before anything is launched: the pointers handed over are null and never dereferenced"""
    lib = vlib.load_library()
    p = _problem(**kw)
    assert lib.v2x_opt_count_bound_workspace_bytes(C.byref(p), A, max_nodes) == V2X_EINVAL
    assert text in lib.v2x_last_error(None)
    nodes = C.c_int64(-7)
    assert lib.v2x_opt_count_bound(C.byref(p), None, None, A, max_nodes, None, None, None, None, C.byref(nodes), None) == V2X_EINVAL
    assert text in lib.v2x_last_error(None) and nodes.value == -7


def test_the_library_refuses_null_thresholds_and_outputs():
    lib = vlib.load_library()
    p = _problem()
    one = C.c_void_p(8)                                                    # never dereferenced: the null checks come first
    assert lib.v2x_opt_count_bound(C.byref(p), one, None, 2, 10, one, one, one, one, None, None) == V2X_EINVAL
    assert b"null thresholds" in lib.v2x_last_error(None)
    for k in range(4):
        outs = [None if i == k else one for i in range(4)]
        assert lib.v2x_opt_count_bound(C.byref(p), one, one, 2, 10, *outs, None, None) == V2X_EINVAL
        assert b"null output" in lib.v2x_last_error(None)


def test_count_better_refuses_before_any_device_work():
    env, opt = _env(), OptimalAllocation()
    for w in ((-1.0, 0.1), (1.0, -0.1), (float('nan'), 0.1)):
        with pytest.raises(ValueError, match="counting search needs weights >= 0"):
            opt.count_better(env, w[0], w[1], [1.0])
    with pytest.raises(ValueError, match="a threshold is NaN"):
        opt.count_better(env, 1.0, 0.1, [1.0, float('nan')])
    with pytest.raises(ValueError, match="a threshold is NaN"):
        opt.count_better(env, 1.0, 0.1, [[float('nan')]])
    for A in (0, 32):
        with pytest.raises(ValueError, match=r"1..31 thresholds per state .*got %d" % A):
            opt.count_better(env, 1.0, 0.1, np.zeros(A))
    with pytest.raises(ValueError, match=r"thresholds of shape \[A\] or \[1, A\]"):
        opt.count_better(env, 1.0, 0.1, np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"thresholds of shape \[A\] or \[1, A\]"):
        opt.count_better(env, 1.0, 0.1, 1.0)
    for bad in (0, -5, 2.5):
        with pytest.raises(ValueError, match="max_nodes must be an integer >= 1"):
            opt.count_better(env, 1.0, 0.1, [1.0], max_nodes=bad)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels, got 33 x 4"):
        OptimalAllocation.check_count(33, 4, 1.0, 0.1)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels, got 4 x 1"):
        OptimalAllocation.check_count(4, 1, 1.0, 0.1)
    with pytest.raises(ValueError, match="1..32 links and 2..16 channels, got 4 x 17"):
        OptimalAllocation.check_count(4, 17, 1.0, 0.1)
    with pytest.raises(ValueError, match=r"65535 states x 5 thresholds exceed the 262144"):
        OptimalAllocation.check_count(20, 4, 1.0, 0.1, n_thr=5, E=65535)
    one = _env()
    one.n_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        opt.count_better(one, 1.0, 0.1, [1.0])
    assert opt.torch is None                                               # no device was touched
    OptimalAllocation.check_count(20, 4, 1.0, 0.1, DEFAULT_MAX_NODES, MAX_THRESHOLDS)
    OptimalAllocation.check_count(24, 4, 0.0, 0.0, 1, 1)
    th = check_thresholds([0.0, -1.0, float('inf')], 3)                    # one row serves every state; infinities are numbers
    assert th.shape == (3, 3) and th.dtype == np.float64 and th.flags['C_CONTIGUOUS'] and th.flags['WRITEABLE']


def test_rank_of_keeps_its_refusal_at_twenty_links_and_names_a_bad_backend():
    env, opt = _env(20), OptimalAllocation()
    with pytest.raises(ValueError, match=r"4\^20 = 1.1e\+12 joint actions exceeds the limit of 2\^36 \(estimated"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int))                 # no backend: the landscape, as before
    with pytest.raises(ValueError, match=r"4\^20 .*estimated"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int), backend='landscape')
    with pytest.raises(ValueError, match=r"backend must be one of \('landscape', 'bound'\), got 'nope'"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int), backend='nope')
    with pytest.raises(ValueError, match="counting search needs weights >= 0"):
        opt.rank_of(env, 1.0, -0.1, np.zeros((1, 20), int), backend='bound')
    with pytest.raises(ValueError, match="max_nodes must be an integer >= 1"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int), backend='bound', max_nodes=0)
    with pytest.raises(ValueError, match="1..31 joint actions"):
        opt.rank_of(env, 1.0, 0.1, np.zeros((1, 32, 20), int), backend='bound')
    with pytest.raises(ValueError, match=r"channel outside \[0, 4\)"):
        opt.rank_of(env, 1.0, 0.1, np.full((1, 20), 4), backend='bound')
    assert opt.torch is None
    assert 1 <= DEFAULT_RANK_MAX_NODES <= DEFAULT_MAX_NODES


def test_twenty_links_pass_the_checks_of_the_bound_backend():
    """every argument check passes: the call goes on to the device, where there is one"""
    env, opt = _env(20), OptimalAllocation()
    try:
        rk = opt.rank_of(env, 1.0, 0.1, np.zeros((1, 20), int), backend='bound', max_nodes=1)
    except ValueError:
        raise
    except RuntimeError as exc:
        assert "GPU" in str(exc) or "HIP" in str(exc) or "hip" in str(exc), exc
    else:
        assert rk['mean_reward'] is None and rk['total'] == 4 ** 20


def test_drivers_check_the_rank_backend_before_device_work():
    big = _agent(_env(20))
    assert big._check_rank_backend('bound', None) == DEFAULT_RANK_MAX_NODES
    assert big._check_rank_backend('bound', 1000) == 1000
    with pytest.raises(ValueError, match=r"4\^20"):
        big._check_rank_backend('landscape', None)
    with pytest.raises(ValueError, match=r"rank_backend must be one of \('landscape', 'bound'\), got 'nope'"):
        big.test_run(1, 1, False, opt_rank=True, rank_backend='nope')
    with pytest.raises(ValueError, match="max_nodes must be an integer >= 1"):
        big.test_run(1, 1, False, opt_rank=True, rank_backend='bound', rank_max_nodes=0)
    neg = _agent(_env())
    neg.v2i_weight = -0.1
    with pytest.raises(ValueError, match="counting search needs weights >= 0"):
        neg.test_run(1, 1, False, opt_rank=True, rank_backend='bound')
    two = _agent(_env())
    two.num_Neighbor = 2
    with pytest.raises(ValueError, match="one receiver"):
        two.test_run(1, 1, False, opt_rank=True, rank_backend='bound')
    book = big._new_rank_book((2, 3), 'bound')
    assert all(v.shape == (2, 3) for v in book.values())
    assert book['exact'].dtype == bool and book['ra_exact'].dtype == bool and not book['uniform_mean_reward'].any()
    assert all(book[k].dtype == object for k in ('total', 'better_max', 'ra_better_max'))
    assert set(big._new_rank_book((2, 3), 'landscape')) == {'better', 'equal', 'ra_better', 'ra_equal', 'total', 'uniform_mean_reward'}


def test_cli_takes_the_rank_backend_and_summarises_exact_and_bracketed_states():
    import contextlib
    import io
    from v2xgnn.rl import run
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(SystemExit):
        run.main(["--save-dir", "x", "--opt-rank", "--opt-rank-backend", "bound", "--opt-rank-max-nodes", "1000", "--no-such-option"])
    assert "no-such-option" in err.getvalue() and "invalid choice" not in err.getvalue()
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(SystemExit):
        run.main(["--save-dir", "x", "--opt-rank-backend", "bogus"])
    assert "invalid choice" in err.getvalue() and "'bound'" in err.getvalue()
    total = np.full((2, 2), 4 ** 20, object)
    book = {'better': np.array([[0, 5], [0, 20]]), 'better_max': np.array([[0, 5], [0, 4 ** 19]], object),
            'exact': np.array([[True, True], [True, False]]),
            'ra_better': np.array([[100, 200], [40, 60]]), 'ra_better_max': np.array([[4 ** 20, 4 ** 18], [40, 4 ** 19]], object),
            'ra_exact': np.array([[False, False], [True, False]]), 'total': total, 'uniform_mean_reward': np.zeros((2, 2))}
    s = run.rank_summary(book)
    assert s == {"share_states_gnn_ranked_exactly": 0.75, "share_exact_states_gnn_optimal": 2.0 / 3.0,
                 "median_share_better_gnn_exact_states": 0.0, "median_upper_share_better_gnn_bracketed_states": 0.25,
                 "share_states_random_ranked_exactly": 0.25, "median_share_better_random_exact_states": 40.0 / 4 ** 20,
                 "median_upper_share_better_random_bracketed_states": 0.25}
    book['exact'][:] = True
    book['ra_exact'][:] = False
    s = run.rank_summary(book)
    assert s["median_upper_share_better_gnn_bracketed_states"] is None and s["median_share_better_random_exact_states"] is None
    assert "mean_reward_uniform_exact" not in s


def _lib_open(counts, n, rb):
    lib = vlib.load_library()
    arr = (C.c_uint64 * (n + 1))(*counts)
    hi, lo = C.c_uint64(1), C.c_uint64(1)
    assert lib.v2x_opt_count_open_leaves(arr, n, rb, C.byref(hi), C.byref(lo)) == 0
    return hi.value, lo.value


def test_open_leaves_on_hand_made_per_depth_counts():
    """sum_k count[k] * rb^(n - k): worked by hand, then the library's two 64-bit words against Python's integers"""
    assert open_leaves([0, 0, 0], 2, 4) == 0 and _lib_open([0, 0, 0], 2, 4) == (0, 0)
    assert open_leaves([1, 0, 0], 2, 4) == 16 and open_leaves([0, 3, 5], 2, 4) == 17       # the root; 3 x 4 + 5 leaves
    assert _lib_open([0, 3, 5], 2, 4) == (0, 17)
    # 20 x 4, nothing examined: the root alone is 4^20 leaves; the same as a path of 3 untried siblings per level + one leaf
    assert open_leaves([1] + [0] * 20, 20, 4) == 4 ** 20 == open_leaves([0] + [3] * 20, 20, 4) + 1
    assert _lib_open([1] + [0] * 20, 20, 4) == (0, 4 ** 20)
    # across the 64-bit boundary: 16^16 = 2^64 exactly, and a carry out of the low word
    assert _lib_open([1] + [0] * 16, 16, 16) == (1, 0)
    assert _lib_open([0] * 16 + [2 ** 64 - 1], 16, 16) == (0, 2 ** 64 - 1)
    assert _lib_open([0] * 15 + [1, 2 ** 64 - 1], 16, 16) == (1, 15)                       # 16 + 2^64 - 1
    assert _lib_open([0, 2 ** 60] + [0] * 15, 16, 16) == (2 ** 56, 0)                      # 2^60 * 2^60 = 2^120
    # 32 x 8 = 2^96 joint actions, the largest the lanes' LDS takes at 32 links: every level at once
    rng = random.Random(3)
    for n, rb in ((32, 8), (32, 9), (20, 4), (18, 16), (30, 10), (3, 3)):
        counts = [rng.randrange(0, rb) if k else 0 for k in range(n + 1)]                  # untried siblings along ONE path
        counts[n] += 1
        want = open_leaves(counts, n, rb)
        assert 0 < want <= rb ** n
        hi, lo = _lib_open(counts, n, rb)
        assert (hi << 64) | lo == want, (n, rb)
        big = [rng.randrange(0, 2 ** 18 * 15) for _ in range(n + 1)]                       # as many items as a queue holds
        big[0] = 0
        want = open_leaves(big, n, rb)
        if want < 2 ** 128:
            hi, lo = _lib_open(big, n, rb)
            assert (hi << 64) | lo == want, (n, rb)
    assert open_leaves(np.array([0, 2 ** 63, 1], np.uint64), 2, 4) == 2 ** 65 + 1          # numpy words stay integers
    with pytest.raises(ValueError, match="3 non-negative per-depth counts"):
        open_leaves([1, 2], 2, 4)
    lib = vlib.load_library()
    assert lib.v2x_opt_count_open_leaves(None, 2, 4, None, None) == V2X_EINVAL
    arr, w = (C.c_uint64 * 40)(), C.c_uint64()
    assert lib.v2x_opt_count_open_leaves(arr, 33, 4, C.byref(w), C.byref(w)) == V2X_EINVAL
    assert lib.v2x_opt_count_open_leaves(arr, 4, 1, C.byref(w), C.byref(w)) == V2X_EINVAL


def test_join128_reads_signed_storage_as_unsigned_words():
    hi = np.array([[0, 1, -1]], np.int64)                                  # torch has no uint64 arithmetic: int64 storage
    lo = np.array([[5, -1, -2]], np.int64)
    got = join128(hi, lo)
    assert got.dtype == object and got.shape == (1, 3)
    assert got.tolist() == [[5, (1 << 64) | (2 ** 64 - 1), ((2 ** 64 - 1) << 64) | (2 ** 64 - 2)]]
    assert (got == 0).tolist() == [[False, False, False]] and (join128(np.zeros(2, np.int64), np.zeros(2, np.int64)) == 0).all()
