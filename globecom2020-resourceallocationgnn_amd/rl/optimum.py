"""Optimal channel allocation of a simulator state on the GPU: the brute-force baseline of the evaluation drivers
(BS_brain.py:1060-1100, :1286-1330, :1339-1380) as an exhaustive fp64 search in HIP (csrc/v2xopt.hip, the v2x_opt_*
entry points of include/v2xgnn.h).

Every joint action a in [0, C)^N of a state with N links (one receiver each, every link active) is scored with the reward
of `compute_reward_with_channel_selection` -- w_v2v * sum of the V2V rates + w_v2i * sum of the V2I rates -- and the
best one is returned as its index  idx = sum_l a_l * C^(N-1-l)  (link 0 most significant: itertools.product order);
among exactly equal rewards the lowest index wins, like np.argmax.

    opt = OptimalAllocation()
    index, reward = opt.search(env, agent.v2v_weight, agent.v2i_weight)      # env: Environ (E = 1) or BatchedEnviron
                                                                               # (or a DeviceChannels / DeviceBatchedEnviron of
                                                                               #  rl/device_sim.py: its device arrays, no upload)
    actions = opt.decode(index, n, C)                                          # [E, N]

`search` enumerates all C^N joint actions (C^N <= 2^36: 18 links x 4 channels).  `search_bound` finds the same pair by
branch and bound (v2x_opt_search_bound: a depth-first search that prunes with an upper bound on every completion of a
partial assignment), which reaches the 20 links x 4 channels the training loops run at, and beyond; its cost depends on
the state, so it takes a node budget and raises BoundBudgetExceeded with the best allocation found when that is spent.

Beyond 32 links (the 100-link wide path, the 8-128 links of the ragged one) no exact search applies.  `search_local` is the
baseline there: a multi-start best-response local search (v2x_opt_search_local, up to 128 links), which returns a LOWER
BOUND on the optimum -- a 1-opt allocation, in practice the optimum itself at the sizes where that can be checked
 -- as an array of channel numbers, not an index.  `rewards_of` scores given joint actions at any of those
sizes, and `search_bound(..., incumbent='local')` starts the exact search from the local search's result.

Where an allocation stands among ALL C^N joint actions of its state (C^N <= 2^36) is what `landscape` and `rank_of` answer:
a histogram of every reward over given edges and the rewards' sum, reduced on the device (v2x_opt_landscape), and from it
the number of joint actions strictly better than / exactly equal to given ones, and the exact mean of the landscape -- the
expectation of the random-action scheme.

At 20 links and beyond the landscape cannot be walked, but the same two numbers can still be had for a GOOD allocation:
`count_better` counts the joint actions above / exactly at given thresholds by branch and bound (v2x_opt_count_bound: the
tree of `search_bound` with the threshold in the incumbent's place, so only the neighbourhood of the better actions is
visited), and `rank_of(..., backend='bound')` ranks given actions with it.  A node budget ends in a certified bracket
[count, count + open], never in a refusal.
"""
import ctypes as C

import numpy as np

from ..lib import OptProblem, V2X_EBUDGET, check, load_library

MAX_SEARCH = 1 << 36                 # joint actions per state the search accepts (v2x_opt_search)
MAX_INDEX = 1 << 62                  # ... and the reward range (v2x_opt_rewards)
HOST_S_PER_ACTION = 57e-6            # one numpy reward of the host path (Agent._brute_force)
DEVICE_S_PER_ACTION = 2e-10          # search kernel time per joint action at 16 links on one MI355X: the estimate in errors

# Node budget of one search_bound call.  A single CPU thread needed 2.1e5 .. 1.9e6 search-tree nodes for 20 links x 4
# channels and 2.3e6 .. 9.6e7 for 24 x 4; the parallel search visits more than that, because subtrees start
# before the incumbent that would have pruned them is known: 4.8e4 .. 3.0e7 on ten seeded 20-link states, 1.7e6 .. 9.5e7 at
# 24 links.  2^32 = 4.3e9 is three orders of magnitude above the worst 20-link state of the prototype, 140 times the worst
# one measured on the GPU and 45 times the worst 24-link one; at the 2.7e7 nodes/s of the longest measured search it ends
# after about three minutes: a safety stop, not a tuning knob.
DEFAULT_MAX_NODES = 1 << 32


# Node budget of one rank_of(..., backend='bound') call and of a ranked step of the evaluation drivers.  Measured at 20 links
# x 4 channels (profiles/opt_count_bound_timing.json): an allocation at 97 % of the optimum has 2.7e4 .. 2.4e6
# strictly better joint actions and is counted exactly in 1.8e6 .. 1.5e7 nodes (4.5 .. 66 per better action), while a random
# action has more than 7e7 better ones and no budget ranks it.  2^26 = 6.7e7 nodes rank an allocation with a few million
# better ones exactly and bound the time spent on one that cannot be ranked to 2 .. 3.4 s; its rank comes back as a bracket.
DEFAULT_RANK_MAX_NODES = 1 << 26
MAX_THRESHOLDS = 31                 # thresholds per state of one count_better call (v2x_opt_count_bound)
MAX_COUNT_ROOTS = 1 << 18           # states x thresholds of one call: its root items fill the search's queue at most
MAX_COUNT_SLOTS = 318               # rb * (n + 1): the LDS slots of a lane (64 lanes x 8 bytes each within 159 KiB)
RANK_BACKENDS = ('landscape', 'bound')

MAX_LOCAL_LINKS = 128               # v2x_opt_search_local / v2x_opt_rewards_actions
MAX_LOCAL_RESTARTS = 65536
# Restarts of one search_local call.  Measured on ten seeded states per size (profiles/opt_local_timing.json):
# 128 restarts find the exact optimum in 10 / 8 / 9 / 10 of 10 states at 12 / 16 / 20 / 24 links, 1024 in 10 / 9 / 10 / 10; at 100
# links 1024 gain 0.4 % over 128 at the median (4 % at most) for 12.5 against 10.3 ms per state -- 128 waves leave half of
# an MI355X idle -- while 8192 cost 2.4 times more for another 0.3 %.
DEFAULT_LOCAL_RESTARTS = 1024
DEFAULT_MAX_SWEEPS = 64
_MASK64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def local_start(seed, r, n, rb):
    """-> int64 [n]: the joint action restart r of search_local starts from (the rule of v2x_opt_search_local): l mod rb
    for restart 0, else splitmix64((seed << 32) ^ (r << 8) ^ l) mod rb in unsigned 64-bit arithmetic.  It depends on
    neither the state nor its position in a batch."""
    seed, r = int(seed), int(r)
    if r == 0:
        return np.arange(n, dtype=np.int64) % rb
    return np.array([splitmix64((((seed << 32) & _MASK64) ^ ((r << 8) & _MASK64) ^ l) & _MASK64) % rb for l in range(n)],
                    np.int64)


def encode(actions, rb):
    """actions [..., n] -> int64 index [...]: the inverse of decode (link 0 most significant).  ValueError above
    rb^n = 2^62, where no 64-bit index exists."""
    a = np.asarray(actions)
    n = a.shape[-1]
    if int(rb) ** n > MAX_INDEX:
        raise ValueError("%d^%d joint actions exceed 2^62: such an action has no 64-bit index" % (rb, n))
    if a.size and (a.min() < 0 or a.max() >= rb):
        raise ValueError("channel outside [0, %d)" % rb)
    out = np.zeros(a.shape[:-1], np.int64)
    for l in range(n):
        out = out * int(rb) + a[..., l].astype(np.int64)
    return out


MAX_EDGES = 62                      # edges of one landscape call (v2x_opt_landscape: 64 slots, one per lane of a wave)
MAX_RANKED = MAX_EDGES // 2         # joint actions per state one rank_of call ranks (two edges each)


def check_edges(edges, E=None):
    """The argument checks of landscape (ValueError): edges [K] or [E, K] floats, 1 <= K <= 62, every row ascending (equal
    neighbours allowed) -> float64 [E, K] (or [1, K] for E None and a single row)."""
    ed = np.asarray(edges, np.float64)
    if ed.ndim not in (1, 2):
        raise ValueError("edges of shape [K] or [E, K] expected, got %s" % list(ed.shape))
    ed = np.atleast_2d(ed)
    K = ed.shape[1]
    if not 1 <= K <= MAX_EDGES:
        raise ValueError("the landscape takes 1..%d edges, got %d" % (MAX_EDGES, K))
    if np.any(ed[:, 1:] < ed[:, :-1]):
        raise ValueError("every row of edges must be ascending")
    if E is not None:
        if ed.shape[0] not in (1, E):
            raise ValueError("edges of shape [%d] or [%d, %d] expected, got %s" % (K, E, K, list(np.shape(edges))))
        ed = np.broadcast_to(ed, (E, K))
    return np.array(ed, np.float64, order='C')                              # a writable copy


def rank_edges(rewards):
    """rewards [E, A] (A <= 31) -> edges float64 [E, 2 A] for landscape(): per row the sorted distinct values of
    {v, nextafter(v, +inf)} over the row's rewards v, padded with +inf.  The bin [v, nextafter(v)) then holds exactly
    the joint actions whose reward equals v, and the bins above it those that are strictly better (rank_from_counts).
    NaN rewards get no edge."""
    r = np.atleast_2d(np.asarray(rewards, np.float64))
    E, A = r.shape
    if not 1 <= A <= MAX_RANKED:
        raise ValueError("1..%d rewards per state can be ranked in one call, got %d" % (MAX_RANKED, A))
    out = np.full((E, 2 * A), np.inf)
    for e in range(E):
        v = r[e][~np.isnan(r[e])]
        u = np.unique(np.concatenate([v, np.nextafter(v, np.inf)]))
        out[e, :u.size] = u
    return out


def rank_from_counts(counts, edges, rewards):
    """counts [E, K + 2] of landscape(edges = rank_edges(rewards)), edges [E, K], rewards [E, A] -> (better, equal) int64
    [E, A]: the joint actions of the state with a strictly larger / an exactly equal reward.  `equal` is the count of the
    bin [v, nextafter(v)), `better` the sum of the bins above it; the NaN slot is excluded.  -1 / -1 for a NaN reward."""
    c = np.atleast_2d(np.asarray(counts, np.int64))
    ed = np.atleast_2d(np.asarray(edges, np.float64))
    r = np.atleast_2d(np.asarray(rewards, np.float64))
    E, A = r.shape
    K = ed.shape[1]
    if c.shape != (E, K + 2) or ed.shape[0] != E:
        raise ValueError("counts [%d, %d] and edges [%d, %d] expected, got %s and %s"
                         % (E, K + 2, E, K, list(c.shape), list(ed.shape)))
    better, equal = np.full((E, A), -1, np.int64), np.full((E, A), -1, np.int64)
    for e in range(E):
        above = np.concatenate([np.cumsum(c[e, K::-1])[::-1], [0]])          # above[s] = counts of slots s .. K
        for a in range(A):
            if r[e, a] == r[e, a]:
                s = int(np.searchsorted(ed[e], r[e, a], side='right'))
                equal[e, a] = c[e, s]
                better[e, a] = above[s + 1]
    return better, equal


def open_leaves(depth_counts, n, rb):
    """depth_counts [n + 1] (entry k: open subtrees rooted at depth k, i.e. with k links assigned) -> the number of leaves
    below them, sum_k depth_counts[k] * rb^(n - k), as a Python int: the arithmetic behind `open` of count_better (the
    library does it in two 64-bit words: v2x_opt_count_open_leaves)."""
    c = [int(v) for v in (depth_counts.tolist() if hasattr(depth_counts, 'tolist') else depth_counts)]    # (no float on the way)
    if len(c) != n + 1 or min(c) < 0:
        raise ValueError("%d non-negative per-depth counts expected, got %r" % (n + 1, c))
    return sum(v * int(rb) ** (n - k) for k, v in enumerate(c))


def join128(hi, lo):
    """two arrays of 64-bit words (signed or unsigned storage) -> object array of Python ints hi * 2^64 + lo"""
    hi, lo = np.asarray(hi), np.asarray(lo)
    out = np.empty(hi.shape, object)
    for i in np.ndindex(*hi.shape):
        out[i] = ((int(hi[i]) & _MASK64) << 64) | (int(lo[i]) & _MASK64)
    return out


def check_thresholds(thresholds, E):
    """The argument checks of count_better (ValueError): thresholds [A] (for every state) or [E, A] floats, 1 <= A <= 31,
    none of them NaN -> float64 [E, A]."""
    th = np.asarray(thresholds, np.float64)
    if th.ndim not in (1, 2) or (th.ndim == 2 and th.shape[0] not in (1, E)):
        raise ValueError("thresholds of shape [A] or [%d, A] expected, got %s" % (E, list(th.shape)))
    th = np.atleast_2d(th)
    if not 1 <= th.shape[1] <= MAX_THRESHOLDS:
        raise ValueError("1..%d thresholds per state can be counted in one call, got %d" % (MAX_THRESHOLDS, th.shape[1]))
    if np.isnan(th).any():
        raise ValueError("a threshold is NaN (not a number): nothing can be counted against it")
    return np.array(np.broadcast_to(th, (E, th.shape[1])), np.float64, order='C')


class BoundBudgetExceeded(RuntimeError):
    """search_bound spent max_nodes before the optimum was proven.  `index` / `reward` ([E] host arrays; torch tensors
    from search_bound_device): the best joint action found so far in every state -- a lower bound on the optimum, with
    rewards(first=index, count=1) == reward; index is 2^63 - 1 where no leaf was reached.  `nodes_visited`: nodes spent."""

    def __init__(self, text, index, reward, nodes_visited):
        RuntimeError.__init__(self, text)
        self.index, self.reward, self.nodes_visited = index, reward, nodes_visited


def decode(index, n, rb):
    """index [E] (or a scalar) -> int64 actions [E, n]: digit l of the index in base rb, link 0 most significant."""
    idx = np.atleast_1d(np.asarray(index, dtype=np.int64))
    out = np.empty((idx.size, n), np.int64)
    rest = idx.copy()
    for l in range(n - 1, -1, -1):
        out[:, l] = rest % rb
        rest //= rb
    return out


def _seconds(s):
    if s < 120:
        return "%.3g s" % s
    if s < 2 * 86400:
        return "%.3g h" % (s / 3600.0)
    return "%.3g days" % (s / 86400.0)


def _sizes(env):
    return (env.n_Veh if hasattr(env, 'E') else len(env.vehicles)), env.n_RB


def problem_arrays(env):
    """-> (v2v_ff [E,n,n,rb], v2i_ff [E,n,rb], v2i_abs [E,n], dest [E,n] int64, constants dict) of a simulator, after the
    checks the search needs (ValueError: more than one receiver per link, an inactive link)."""
    if hasattr(env, 'E'):                                           # BatchedEnviron (rl/batched_env.py)
        env.finish_step()                                           # as its reward does: a pending step lands first
        n, rb = env.n_Veh, env.n_RB
        v2v = np.asarray(env.V2V_channels_with_fastfading, np.float64).reshape(env.E, n, n, rb)
        v2i = np.asarray(env.V2I_channels_with_fastfading, np.float64).reshape(env.E, n, rb)
        v2i_abs = np.asarray(env.V2I_channels_abs, np.float64).reshape(env.E, n)
        dest = np.asarray(env.dest, np.int64).reshape(env.E, n)
    else:
        n, rb = len(env.vehicles), env.n_RB
        v2v = np.asarray(env.V2V_channels_with_fastfading, np.float64).reshape(1, n, n, rb)
        v2i = np.asarray(env.V2I_channels_with_fastfading, np.float64).reshape(1, n, rb)
        v2i_abs = np.asarray(env.V2I_channels_abs, np.float64)[:n].reshape(1, n)
        dest = None
    if env.n_Neighbor != 1:
        raise ValueError("the optimal-allocation search supports one receiver per link (n_Neighbor = 1), got %d"
                         % env.n_Neighbor)
    active = np.asarray(getattr(env, 'activate_links', True))
    if not np.all(active):
        raise ValueError("the optimal-allocation search needs every link active (activate_links has %d inactive)"
                         % int(np.size(active) - np.count_nonzero(active)))
    if dest is None:
        dest = np.array([[v.destinations[0] for v in env.vehicles]], np.int64)
    if dest.min() < 0 or dest.max() >= n:
        raise ValueError("receiver index outside [0, %d)" % n)
    const = dict(p_v2v=float(env.V2V_power_dB_List[env.fixed_v2v_power_index]), p_v2i=float(env.V2I_power_dB),
                 veh_gain=float(env.vehAntGain), bs_gain=float(env.bsAntGain), bs_nf=float(env.bsNoiseFigure),
                 veh_nf=float(env.vehNoiseFigure), sig2=float(env.sig2))
    return v2v, v2i, v2i_abs, dest, const


class OptimalAllocation(object):
    """Owns the device workspace (grown on demand) and issues the search on torch's current stream of `device`.  The
    argument checks (ValueError) come before any device work."""

    def __init__(self, device=0):
        self.device_index = int(device)
        self.torch = None
        self._ws = None
        self._keep = None
        self.nodes_visited = 0                            # of the last search_bound
        self.local_info = None                            # of the last search_local: int32 [E, 2] (winning restart, converged)

    def _init_device(self):
        if self.torch is None:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("OptimalAllocation needs a GPU (there is no CPU fallback; the host path is "
                                   "Agent._brute_force)")
            self.torch = torch
            self.device = torch.device('cuda', self.device_index)
            self._lib = load_library()

    @staticmethod
    def check_size(n, rb, limit=MAX_SEARCH):
        if not 1 <= n <= 32 or not 2 <= rb <= 16:
            raise ValueError("the optimal-allocation search supports 1..32 links and 2..16 channels, got %d x %d" % (n, rb))
        total = rb ** n
        if total > limit:
            raise ValueError("the optimal-allocation search over %d^%d = %.3g joint actions exceeds the limit of 2^%d "
                             "(estimated %s per state on the GPU, %s on the host)"
                             % (rb, n, float(total), limit.bit_length() - 1, _seconds(total * DEVICE_S_PER_ACTION),
                                _seconds(total * HOST_S_PER_ACTION)))

    @staticmethod
    def check_bound(n, rb, v2v_weight=0.0, v2i_weight=0.0, max_nodes=DEFAULT_MAX_NODES):
        """The argument checks of search_bound (ValueError), before any device work: no cap on rb^n but the 64-bit index."""
        OptimalAllocation.check_size(n, rb, MAX_INDEX)
        if not (float(v2v_weight) >= 0.0 and float(v2i_weight) >= 0.0):
            raise ValueError("the branch-and-bound search needs weights >= 0 (its bound assumes interference can only "
                             "lower the reward), got %r / %r" % (v2v_weight, v2i_weight))
        if int(max_nodes) != max_nodes or int(max_nodes) < 1:
            raise ValueError("max_nodes must be an integer >= 1, got %r" % (max_nodes,))

    @staticmethod
    def check_count(n, rb, v2v_weight=0.0, v2i_weight=0.0, max_nodes=DEFAULT_MAX_NODES, n_thr=1, E=1):
        """The argument checks of count_better (ValueError), before any device work: the sizes of search_bound without
        its cap on rb^n (no joint action is named by an index), within the LDS of a lane."""
        OptimalAllocation.check_size(n, rb, 1 << 128)
        if rb * (n + 1) > MAX_COUNT_SLOTS:
            raise ValueError("the counting search keeps rb * (n + 1) = %d values per lane in LDS, %d at most (%d x %d)"
                             % (rb * (n + 1), MAX_COUNT_SLOTS, n, rb))
        if not (float(v2v_weight) >= 0.0 and float(v2i_weight) >= 0.0):
            raise ValueError("the counting search needs weights >= 0 (its bound assumes interference can only lower the "
                             "reward), got %r / %r" % (v2v_weight, v2i_weight))
        if int(max_nodes) != max_nodes or int(max_nodes) < 1:
            raise ValueError("max_nodes must be an integer >= 1, got %r" % (max_nodes,))
        if not 1 <= int(n_thr) <= MAX_THRESHOLDS:
            raise ValueError("1..%d thresholds per state can be counted in one call, got %d" % (MAX_THRESHOLDS, n_thr))
        if int(E) * int(n_thr) > MAX_COUNT_ROOTS:
            raise ValueError("%d states x %d thresholds exceed the %d (state, threshold) pairs of one call"
                             % (E, n_thr, MAX_COUNT_ROOTS))

    @staticmethod
    def check_local(n, rb, restarts=DEFAULT_LOCAL_RESTARTS, max_sweeps=DEFAULT_MAX_SWEEPS):
        """The argument checks of search_local / rewards_of (ValueError), before any device work."""
        if not 1 <= n <= MAX_LOCAL_LINKS or not 2 <= rb <= 16:
            raise ValueError("the local search supports 1..%d links and 2..16 channels, got %d x %d" % (MAX_LOCAL_LINKS, n, rb))
        if int(restarts) != restarts or not 1 <= int(restarts) <= MAX_LOCAL_RESTARTS:
            raise ValueError("restarts must be an integer in 1..%d, got %r" % (MAX_LOCAL_RESTARTS, restarts))
        if int(max_sweeps) != max_sweeps or int(max_sweeps) < 1:
            raise ValueError("max_sweeps must be an integer >= 1, got %r" % (max_sweeps,))

    @staticmethod
    def _check_actions(actions, E, n, rb):
        """host joint actions [E, K, n] or [E, n] -> (int32 [E, K, n], had K)"""
        a = np.asarray(actions)
        if a.dtype.kind not in 'iu':
            raise ValueError("joint actions must be integers, got dtype %s" % a.dtype)
        if a.ndim not in (2, 3) or a.shape[0] != E or a.shape[-1] != n or a.size == 0:
            raise ValueError("joint actions of shape [%d, K, %d] or [%d, %d] expected, got %s" % (E, n, E, n, list(a.shape)))
        if a.min() < 0 or a.max() >= rb:
            raise ValueError("channel outside [0, %d) in the joint actions" % rb)
        return np.ascontiguousarray(a.reshape(E, -1, n), np.int32), a.ndim == 3

    def _setup(self, env, v2v_weight, v2i_weight, limit, max_nodes=None, local=None, n_edges=None, n_thr=None):
        """max_nodes not None: the problem of search_bound (its checks, its workspace), with n_thr of count_better;
        local = (restarts, max_sweeps): of search_local / rewards_of; n_edges: of landscape."""
        on_device = hasattr(env, 'problem_tensors')       # DeviceChannels / DeviceBatchedEnviron (rl/device_sim.py): no upload
        if on_device:
            E, (n, rb) = env.E, _sizes(env)
        else:
            v2v, v2i, v2i_abs, dest, const = problem_arrays(env)
            E, n, rb = v2v.shape[0], v2v.shape[1], v2v.shape[3]
        if local is not None:
            self.check_local(n, rb, *local)
        elif n_thr is not None:
            self.check_count(n, rb, v2v_weight, v2i_weight, max_nodes, n_thr, E)
        elif max_nodes is None:
            self.check_size(n, rb, limit)
        else:
            self.check_bound(n, rb, v2v_weight, v2i_weight, max_nodes)
        self._init_device()
        t = self.torch
        if on_device:
            dev, const = env.problem_tensors(self.device)
        else:
            dev = [t.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (v2v, v2i, v2i_abs, dest)]
        prob = OptProblem(E=E, n=n, rb=rb, pad_=0, v2v_ff=dev[0].data_ptr(), v2i_ff=dev[1].data_ptr(),
                          v2i_abs=dev[2].data_ptr(), dest=dev[3].data_ptr(), w_v2v=float(v2v_weight),
                          w_v2i=float(v2i_weight), **const)
        if local is not None:
            need = int(self._lib.v2x_opt_local_workspace_bytes(C.byref(prob), int(local[0])))
        elif n_thr is not None:
            need = int(self._lib.v2x_opt_count_bound_workspace_bytes(C.byref(prob), int(n_thr), int(max_nodes)))
        elif n_edges is not None:
            need = int(self._lib.v2x_opt_landscape_workspace_bytes(C.byref(prob), int(n_edges)))
        elif max_nodes is None:
            need = int(self._lib.v2x_opt_workspace_bytes(C.byref(prob)))
        else:
            need = int(self._lib.v2x_opt_bound_workspace_bytes(C.byref(prob), int(max_nodes)))
        if need < 0:
            check(self._lib, need)
        if self._ws is None or self._ws.numel() < need:
            self._ws = t.empty(max(need, 1 << 20), dtype=t.uint8, device=self.device)
        self._keep = dev                                  # inputs stay alive until the next call (the launches are async)
        return prob, E, n, rb

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def search_device(self, env, v2v_weight, v2i_weight):
        """search() with the results left on the device: (index int64 [E], reward float64 [E]) torch tensors."""
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_SEARCH)
        t = self.torch
        index = t.empty(E, dtype=t.int64, device=self.device)
        reward = t.empty(E, dtype=t.float64, device=self.device)
        check(self._lib, self._lib.v2x_opt_search(C.byref(prob), self._ws.data_ptr(), index.data_ptr(), reward.data_ptr(),
                                                  self._stream()))
        return index, reward

    def search(self, env, v2v_weight, v2i_weight):
        """-> (index int64 [E], reward float64 [E]) host arrays: the optimum of every state of the simulator."""
        index, reward = self.search_device(env, v2v_weight, v2i_weight)
        return index.cpu().numpy(), reward.cpu().numpy()

    def search_bound_device(self, env, v2v_weight, v2i_weight, max_nodes=DEFAULT_MAX_NODES, incumbent=None,
                            restarts=DEFAULT_LOCAL_RESTARTS, seed=0):
        """search_bound() with the results left on the device: (index int64 [E], reward float64 [E]) torch tensors.
        `nodes_visited` of the object holds the nodes of the last call."""
        start = None
        if incumbent is not None:
            n, rb = _sizes(env)
            self.check_bound(n, rb, v2v_weight, v2i_weight, max_nodes)
            if isinstance(incumbent, str):
                if incumbent != 'local':
                    raise ValueError("incumbent must be None, 'local' or an [E, n] array of channels, got %r" % (incumbent,))
                self.check_local(n, rb, restarts)
                start = self.search_local_device(env, v2v_weight, v2i_weight, restarts=restarts, seed=seed)[0]
            else:
                E = env.E if hasattr(env, 'E') else 1
                start, had_k = self._check_actions(incumbent, E, n, rb)
                if had_k:
                    raise ValueError("incumbent: one joint action per state ([%d, %d]) expected, got %s"
                                     % (E, n, list(np.shape(incumbent))))
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_INDEX, max_nodes)
        t = self.torch
        if start is not None and not t.is_tensor(start):
            start = t.from_numpy(start).to(self.device)
        index = t.empty(E, dtype=t.int64, device=self.device)
        reward = t.empty(E, dtype=t.float64, device=self.device)
        nodes = C.c_int64(0)
        if start is None:
            rc = self._lib.v2x_opt_search_bound(C.byref(prob), self._ws.data_ptr(), int(max_nodes), index.data_ptr(),
                                                reward.data_ptr(), C.byref(nodes), self._stream())
        else:
            start = start.contiguous()
            rc = self._lib.v2x_opt_search_bound_seeded(C.byref(prob), self._ws.data_ptr(), int(max_nodes), start.data_ptr(),
                                                       index.data_ptr(), reward.data_ptr(), C.byref(nodes), self._stream())
        self.nodes_visited = int(nodes.value)
        if rc == V2X_EBUDGET:
            msg = self._lib.v2x_last_error(None)
            raise BoundBudgetExceeded(msg.decode() if msg else "node budget spent", index, reward, self.nodes_visited)
        check(self._lib, rc)
        return index, reward

    def search_bound(self, env, v2v_weight, v2i_weight, max_nodes=DEFAULT_MAX_NODES, incumbent=None,
                     restarts=DEFAULT_LOCAL_RESTARTS, seed=0):
        """The pair search() returns -- the largest reward and, among exactly equal rewards, the lowest index, bit for bit
        -- by branch and bound: 1..32 links, 2..16 channels, rb^n <= 2^62.  max_nodes: search-tree nodes the call may visit
        over all states of `env`; BoundBudgetExceeded (carrying the best allocation found) when they are spent.
        incumbent: None (the default: the unseeded call, unchanged), 'local' (search_local with `restarts` / `seed` runs first and its
        allocation is the first incumbent: v2x_opt_search_bound_seeded) or an [E, n] array of channels used as it is.  The
        result is the same pair either way; only the nodes visited change."""
        try:
            index, reward = self.search_bound_device(env, v2v_weight, v2i_weight, max_nodes, incumbent, restarts, seed)
        except BoundBudgetExceeded as exc:
            exc.index, exc.reward = exc.index.cpu().numpy(), exc.reward.cpu().numpy()
            raise
        return index.cpu().numpy(), reward.cpu().numpy()

    def search_local_device(self, env, v2v_weight, v2i_weight, restarts=DEFAULT_LOCAL_RESTARTS, seed=0,
                            max_sweeps=DEFAULT_MAX_SWEEPS, all_restarts=False):
        """search_local() with the results left on the device (torch tensors; actions int32, `local_info` a tensor too)."""
        if int(seed) != seed or not 0 <= int(seed) < (1 << 32):
            raise ValueError("seed must be an integer in [0, 2^32), got %r" % (seed,))
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_INDEX, local=(restarts, max_sweeps))
        t = self.torch
        R = int(restarts)
        actions = t.empty((E, n), dtype=t.int32, device=self.device)
        reward = t.empty(E, dtype=t.float64, device=self.device)
        info = t.empty((E, 2), dtype=t.int32, device=self.device)
        all_a = t.empty((E, R, n), dtype=t.int32, device=self.device) if all_restarts else None
        all_r = t.empty((E, R), dtype=t.float64, device=self.device) if all_restarts else None
        check(self._lib, self._lib.v2x_opt_search_local(
            C.byref(prob), self._ws.data_ptr(), R, int(seed), int(max_sweeps), actions.data_ptr(), reward.data_ptr(),
            info.data_ptr(), all_a.data_ptr() if all_restarts else None, all_r.data_ptr() if all_restarts else None,
            self._stream()))
        self.local_info = info
        return (actions, reward, all_a, all_r) if all_restarts else (actions, reward)

    def search_local(self, env, v2v_weight, v2i_weight, restarts=DEFAULT_LOCAL_RESTARTS, seed=0,
                     max_sweeps=DEFAULT_MAX_SWEEPS, all_restarts=False):
        """-> (actions int64 [E, n], reward float64 [E]): the best allocation a multi-start best-response local search
        finds in every state -- a LOWER BOUND on the optimum, not the optimum; 1..128 links, 2..16 channels.  `restarts`
        independent searches per state (restart r starts from local_start(seed, r, n, rb)), each sweeping the links in
        order until no single link can improve the reward by changing its channel (max_sweeps sweeps at most); the best
        restart wins, by (larger reward, else lexicographically lower action).  The reward is that of rewards_of(actions),
        bit for bit.  all_restarts: also (all_actions int64 [E, R, n], all_rewards float64 [E, R]).  `local_info` of the
        object: int32 [E, 2] -- the winning restart and whether its last sweep made no move."""
        out = self.search_local_device(env, v2v_weight, v2i_weight, restarts, seed, max_sweeps, all_restarts)
        self.local_info = self.local_info.cpu().numpy()
        host = [o.cpu().numpy() for o in out]
        host[0] = host[0].astype(np.int64)
        if all_restarts:
            host[2] = host[2].astype(np.int64)
        return tuple(host)

    def rewards_of_device(self, env, v2v_weight, v2i_weight, actions):
        """rewards_of() with the result left on the device.  actions: a host array (checked) or an int32 torch tensor on
        the device (a channel outside [0, rb) then gives NaN)."""
        n, rb = _sizes(env)
        self.check_local(n, rb)
        E = env.E if hasattr(env, 'E') else 1
        if hasattr(actions, 'data_ptr'):                                # a torch tensor
            if actions.dim() not in (2, 3) or actions.shape[0] != E or actions.shape[-1] != n or actions.numel() == 0:
                raise ValueError("joint actions of shape [%d, K, %d] or [%d, %d] expected, got %s"
                                 % (E, n, E, n, list(actions.shape)))
            had_k, host = actions.dim() == 3, None
        else:
            host, had_k = self._check_actions(actions, E, n, rb)
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_INDEX, local=(1, 1))
        t = self.torch
        dev = (t.from_numpy(host).to(self.device) if host is not None
               else actions.to(device=self.device, dtype=t.int32).reshape(E, -1, n).contiguous())
        K = dev.shape[1]
        out = t.empty((E, K), dtype=t.float64, device=self.device)
        check(self._lib, self._lib.v2x_opt_rewards_actions(C.byref(prob), self._ws.data_ptr(), dev.data_ptr(), K,
                                                           out.data_ptr(), self._stream()))
        self._keep = self._keep + [dev]
        return out if had_k else out[:, 0]

    def rewards_of(self, env, v2v_weight, v2i_weight, actions):
        """The reward of given joint actions: actions [E, K, n] -> float64 [E, K], or [E, n] -> [E]; channel numbers, at
        any size up to 128 links.  Up to 32 links bit for bit rewards(first=encode(action), count=1)."""
        return self.rewards_of_device(env, v2v_weight, v2i_weight, actions).cpu().numpy()

    def rewards_device(self, env, v2v_weight, v2i_weight, first=0, count=None):
        """The reward of every joint action index in [first, first + count) of every state: float64 [E, count] torch
        tensor on the device (count None: to the last index)."""
        n, rb = _sizes(env)
        self.check_size(n, rb, MAX_INDEX)
        total = rb ** n
        first = int(first)
        count = total - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > total:
            raise ValueError("index range [%d, %d) outside [0, %d)" % (first, first + count, total))
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_INDEX)
        t = self.torch
        out = t.empty((E, count), dtype=t.float64, device=self.device)
        check(self._lib, self._lib.v2x_opt_rewards(C.byref(prob), self._ws.data_ptr(), first, count, out.data_ptr(),
                                                   self._stream()))
        return out

    def rewards(self, env, v2v_weight, v2i_weight, first=0, count=None):
        """rewards_device() copied to the host: float64 [E, count] (the reference's Curr_Feasible_Reward vector)."""
        return self.rewards_device(env, v2v_weight, v2i_weight, first, count).cpu().numpy()

    def landscape_device(self, env, v2v_weight, v2i_weight, edges):
        """landscape() with the results left on the device: (counts int64 [E, K + 2], sums float64 [E]) torch tensors."""
        n, rb = _sizes(env)
        E = env.E if hasattr(env, 'E') else 1
        ed = check_edges(edges, E)
        self.check_size(n, rb)
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_SEARCH, n_edges=ed.shape[1])
        t = self.torch
        K = ed.shape[1]
        dev = t.from_numpy(ed).to(self.device)
        counts = t.empty((E, K + 2), dtype=t.int64, device=self.device)
        sums = t.empty(E, dtype=t.float64, device=self.device)
        check(self._lib, self._lib.v2x_opt_landscape(C.byref(prob), self._ws.data_ptr(), dev.data_ptr(), K, counts.data_ptr(),
                                                     sums.data_ptr(), self._stream()))
        self._keep = self._keep + [dev]
        return counts, sums

    def landscape(self, env, v2v_weight, v2i_weight, edges):
        """The histogram of ALL rb^n rewards of every state (rb^n <= 2^36, as search) over `edges` -- [K] for every state or
        [E, K], 1 <= K <= 62, rows ascending -- reduced on the device, never downloaded:
        -> (counts int64 [E, K + 2], sums float64 [E]).  counts[e, s] for s <= K: joint actions whose reward r has
        np.searchsorted(edges[e], r, side='right') == s, each reward with the bits rewards() returns; counts[e, K + 1]:
        NaN rewards; a row sums to rb^n.  sums[e]: the sum of the state's rewards, so sums / rb^n is the exact expectation
        of the random-action scheme (uniform, independent per link).  Counts are exact; the sum is reproducible call to
        call, but may differ in its last bits between a stacked and a single-state call."""
        counts, sums = self.landscape_device(env, v2v_weight, v2i_weight, edges)
        return counts.cpu().numpy(), sums.cpu().numpy()

    def count_better_device(self, env, v2v_weight, v2i_weight, thresholds, max_nodes=DEFAULT_MAX_NODES):
        """count_better() with the results left on the device: dict of torch tensors `better` / `equal` (int64 [E, A]),
        `open_hi` / `open_lo` (int64 [E, A] holding the two unsigned 64-bit words of `open`) and `exact` (bool [E, A]), and
        `nodes_visited` (int).  thresholds: a host array (checked) or a float64 torch tensor [E, A] on the device (a NaN in
        it is refused by the library: V2XInvalidArgument, a ValueError)."""
        n, rb = _sizes(env)
        E = env.E if hasattr(env, 'E') else 1
        if hasattr(thresholds, 'data_ptr'):                             # a torch tensor
            if thresholds.dim() != 2 or thresholds.shape[0] != E:
                raise ValueError("thresholds of shape [%d, A] expected, got %s" % (E, list(thresholds.shape)))
            A, host = int(thresholds.shape[1]), None
        else:
            host = check_thresholds(thresholds, E)
            A = host.shape[1]
        self.check_count(n, rb, v2v_weight, v2i_weight, max_nodes, A, E)
        prob, E, n, rb = self._setup(env, v2v_weight, v2i_weight, MAX_INDEX, max_nodes, n_thr=A)
        t = self.torch
        dev = (t.from_numpy(host).to(self.device) if host is not None
               else thresholds.to(device=self.device, dtype=t.float64).contiguous())
        out = {k: t.empty((E, A), dtype=t.int64, device=self.device) for k in ('better', 'equal', 'open_hi', 'open_lo')}
        nodes = C.c_int64(0)
        rc = self._lib.v2x_opt_count_bound(C.byref(prob), self._ws.data_ptr(), dev.data_ptr(), A, int(max_nodes),
                                           out['better'].data_ptr(), out['equal'].data_ptr(), out['open_hi'].data_ptr(),
                                           out['open_lo'].data_ptr(), C.byref(nodes), self._stream())
        self._keep = self._keep + [dev]
        self.nodes_visited = int(nodes.value)
        if rc != V2X_EBUDGET:                                           # a spent budget is a result: the bracket
            check(self._lib, rc)
        out['exact'] = (out['open_hi'] == 0) & (out['open_lo'] == 0)
        out['nodes_visited'] = self.nodes_visited
        return out

    def count_better(self, env, v2v_weight, v2i_weight, thresholds, max_nodes=DEFAULT_MAX_NODES):
        """How many joint actions of every state score above / exactly at given thresholds, by branch and bound
        (v2x_opt_count_bound) -- no cap on rb^n: 1..32 links, 2..16 channels with rb * (n + 1) <= 318, weights >= 0.
        thresholds [A] (for every state) or [E, A], 1 <= A <= 31, no NaN.  -> dict: `better` / `equal` (int64 [E, A]: joint
        actions with a reward > / == the threshold, each reward with the bits rewards() returns: what rank_from_counts
        yields from a landscape), `open` (object [E, A] of Python ints: leaves the search did not examine), `exact` (bool
        [E, A]: open == 0) and `nodes_visited`.  max_nodes: search-tree nodes the call may visit over all states and
        thresholds.  A spent budget does not raise: better / equal are then certified lower bounds and the true counts lie
        in [better, better + open] and [equal, equal + open].  The counts of an exact entry are the same in every run."""
        out = self.count_better_device(env, v2v_weight, v2i_weight, thresholds, max_nodes)
        better, equal = out['better'].cpu().numpy(), out['equal'].cpu().numpy()
        opened = join128(out['open_hi'].cpu().numpy(), out['open_lo'].cpu().numpy())
        return dict(better=better, equal=equal, open=opened, exact=np.array(opened == 0, bool),
                    nodes_visited=out['nodes_visited'])

    def rank_of(self, env, v2v_weight, v2i_weight, actions, backend='landscape', max_nodes=DEFAULT_RANK_MAX_NODES):
        """Where given joint actions stand among all rb^n of their state: actions [E, A, n] (A <= 31) or [E, n], channel
        numbers -> dict of `better` / `equal` (int64: joint actions with a strictly larger / an exactly equal reward, the
        action itself included in `equal`), `reward` (rewards_of(actions)), each [E, A] or [E]; `total` (rb^n) and
        `mean_reward` (float64 [E]: the mean over all joint actions).  better == 0: an optimum; better / total: the share
        of joint actions strictly better than the given one.
        backend='landscape' (the default; rb^n <= 2^36): one rewards_of and one landscape call.
        backend='bound' (1..32 links, no cap on rb^n; weights >= 0): one rewards_of call and one count_better call with
        those rewards as thresholds and `max_nodes` as its budget.  The dict then also holds `exact` (bool), `better_max` /
        `equal_max` (object arrays of Python ints: count + open).  Where `exact`, better / equal are the landscape's numbers;
        elsewhere the budget ran out and the true counts lie in [better, better_max] and [equal, equal_max].  `mean_reward`
        is None with 'bound': nothing enumerates the landscape."""
        if backend not in RANK_BACKENDS:
            raise ValueError("backend must be one of %s, got %r" % (RANK_BACKENDS, backend))
        n, rb = _sizes(env)
        if backend == 'bound':
            self.check_count(n, rb, v2v_weight, v2i_weight, max_nodes)
        else:
            self.check_size(n, rb)
        E = env.E if hasattr(env, 'E') else 1
        host, had_k = self._check_actions(actions, E, n, rb)
        if host.shape[1] > MAX_RANKED:
            raise ValueError("1..%d joint actions per state can be ranked in one call, got %d" % (MAX_RANKED, host.shape[1]))
        reward = self.rewards_of(env, v2v_weight, v2i_weight, host)
        total = rb ** n
        if backend == 'bound':
            got = self.count_better(env, v2v_weight, v2i_weight, reward, max_nodes)
            out = dict(better=got['better'], equal=got['equal'], reward=reward, exact=got['exact'],
                       better_max=got['better'].astype(object) + got['open'], equal_max=got['equal'].astype(object) + got['open'])
            if not had_k:
                out = {k: v[:, 0] for k, v in out.items()}
            out.update(total=total, mean_reward=None, nodes_visited=got['nodes_visited'])
            return out
        edges = rank_edges(reward)
        counts, sums = self.landscape(env, v2v_weight, v2i_weight, edges)
        better, equal = rank_from_counts(counts, edges, reward)
        if not had_k:
            better, equal, reward = better[:, 0], equal[:, 0], reward[:, 0]
        return dict(better=better, equal=equal, total=total, mean_reward=sums / float(total), reward=reward)

    @staticmethod
    def decode(index, n, rb):
        return decode(index, n, rb)

    @staticmethod
    def encode(actions, rb):
        return encode(actions, rb)
