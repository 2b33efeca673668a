"""Mixed-size DQN: ONE shared-weight Q-network trained on scenarios with different numbers of V2V links at once.

A shared-weight GNN does not care how many links a graph has (GnnSpec(share_weights=True, variable_graphs=True)); the engine's
ragged path scores and fits batches whose graphs differ in size.  This module is the DQN glue around it:

  MixedReplay   one unmodified DeviceReplay per link count; a minibatch that draws from several of them is assembled into one
                ragged batch by ONE launch (v2x_replay_gather_mixed): xe / xe' rows, actions, rewards, graph_off, row_ptr and
                the graph-local CSR sources, pool after pool in ascending size.
  MixedAgent    one BatchedEnviron per link count; a rollout iteration steps every simulator of every environment once, all
                observations scored by ONE forward; replay() draws B E_k / sum E graphs from pool k and runs one
                v2x_dqn_step in its ragged form (one reward per graph, one action per node row, a single Huber mean).
                rollout='trajectory': every environment is a DeviceBatchedEnviron with streams='device' and the ceil(50 / sum E)
                iterations of a train step are ONE library call (v2x_rollout_steps_mixed: one walk launch, one assembly launch,
                one ragged forward, one finish launch for all link counts); the epsilon-greedy draws are taken ahead in the
                order the host rollout takes them, the transitions land in the pools' slots on the device, and the rewards
                come back with the losses at the end of the episode.  The default stays 'host'.
                trajectory_walk='wide': that call and test_run's device episodes spread every pool's steps over the chip
                (v2x_rollout_steps_mixed_wide / v2x_eval_steps_mixed_wide: six launches in the walk's place, the same bits);
                with rollout='host' it applies to evaluation alone.  The default stays 'serial'.
                test_run() evaluates the network on ANY set of link counts (the training sizes or others) against the
                random baseline and, on request, the optimum; eval_backend='device' runs an episode of all link counts as ONE
                library call (v2x_eval_steps_mixed) and one stacked optimum search per link count.  save_weights() /
                load_weights() keep the online and the target network in the files of rl.run.weight_file_names;
                train(save_interval=k) saves them every k episodes, and evaluate_training() scores those checkpoints -- K
                networks on ONE re-seeded episode per trial (the walk, the baseline and the optimum do not depend on the
                network: with eval_backend='device' one v2x_eval_sweep_mixed call and one stacked search per link count
                serve all K).

Only regular graphs (in-degree n - 2 everywhere) are stored: a transition whose graph has a link that is its own receiver (two
vehicles on one spot, rare) is counted in MixedReplay.dropped_irregular and left out -- the assembly is closed-form because
every stored graph of a pool has the same shape.
"""
import ctypes as C
import os

import numpy as np

from .. import lib as _lib
from ..engine import DeviceBatch, GnnEngine, current_stream_ptr
from ..packing import PackedBatch
from ..spec import GnnSpec
from .agent import Memory, MEMORY_CAPACITY, UPDATE_TARGET_FREQUENCY, MAX_EPSILON, MIN_EPSILON, _random_channels
from .replay import DeviceReplay

MIN_LINKS, MAX_LINKS = 3, DeviceReplay.MAX_LINKS
ROLLOUTS = ('host', 'trajectory')                     # how MixedAgent makes the iterations of a train step
EVAL_BACKENDS = ('host', 'device')                    # how MixedAgent.test_run makes the steps of an episode
EVAL_OPT_BACKENDS = ('device', 'bound', 'local')      # where MixedAgent.test_run searches the optimum (rl/optimum.py)
SCHEMES = ('gnn', 'random', 'optimal')                # the books of MixedAgent.test_run


def _check_sizes(sizes, what):
    sizes = [int(n) for n in sizes]
    if not sizes or len(sizes) > _lib.MIXED_MAX_POOLS:
        raise ValueError("%s: 1..%d link counts, got %d" % (what, _lib.MIXED_MAX_POOLS, len(sizes)))
    if len(set(sizes)) != len(sizes):
        raise ValueError("%s: the link counts must be distinct, got %s" % (what, sizes))
    for n in sizes:
        if not MIN_LINKS <= n <= MAX_LINKS:
            raise ValueError("%s: %d links -- a pool holds %d..%d links" % (what, n, MIN_LINKS, MAX_LINKS))
    return sorted(sizes)


def mixed_quotas(batch, weights):
    """`batch` graphs split in proportion to `weights` (simulators per size) by largest remainder: floor(B w_k / sum w) each,
    the graphs left over one by one to the largest fractional parts (ties: the earlier entry).  A zero quota is allowed."""
    w = [int(v) for v in weights]
    batch = int(batch)
    if batch < 0 or not w or min(w) < 0 or sum(w) == 0:
        raise ValueError("mixed_quotas: a non-negative batch and non-negative weights that do not all vanish")
    total = sum(w)
    quota = [batch * v // total for v in w]
    by_remainder = sorted(range(len(w)), key=lambda k: (-(batch * w[k] % total), k))
    for k in by_remainder[:batch - sum(quota)]:
        quota[k] += 1
    return quota


def draw_eval_step(envs, n_channels, fixed_epsilon):
    """the host draws of ONE step of MixedAgent.test_run, on the process-wide numpy stream: environment after environment
    (the caller's order: ascending size), simulator after simulator -- the random scheme's action, then np.random.random(),
    and _random_channels right after it when that draw is below fixed_epsilon (the simulator explores)
    -> ([baseline [E, n] int], [explore [E] uint8], [policy_random [E, n] int, zeros where greedy]) per environment"""
    baseline, explore, rand = [], [], []
    for env in envs:
        E, n = env.E, env.n_Veh
        b, x, r = np.zeros((E, n), int), np.zeros(E, np.uint8), np.zeros((E, n), int)
        for e in range(E):
            b[e] = _random_channels(n, 1, n_channels).reshape(n)
            if np.random.random() < fixed_epsilon:
                x[e] = 1
                r[e] = _random_channels(n, 1, n_channels).reshape(n)
        baseline.append(b)
        explore.append(x)
        rand.append(r)
    return baseline, explore, rand


def draw_eval_episode_ahead(envs, n_channels, fixed_epsilon, T):
    """the draws of the T steps of an episode, taken before its first step runs: step after step draw_eval_step -- nothing else
    draws inside an episode, so the numpy stream is the host loop's
    -> ([baseline [T, E, n]], [explore [T, E] uint8], [policy_random [T, E, n]]) per environment"""
    steps = [draw_eval_step(envs, n_channels, fixed_epsilon) for _ in range(T)]
    return tuple([np.stack([step[part][k] for step in steps]) for k in range(len(envs))] for part in range(3))


class MixedReplay(object):
    def __init__(self, capacity, sizes, device=0):
        """capacity: transitions PER link count; sizes: the distinct link counts (3..31, at most 8)"""
        self.sizes = _check_sizes(sizes, "MixedReplay")
        self.pools = {n: DeviceReplay(capacity, n, device=device) for n in self.sizes}
        first = self.pools[self.sizes[0]]
        self.torch, self.device, self._lib = first.torch, first.device, first._lib
        self.dropped_irregular = {n: 0 for n in self.sizes}
        self._out = {}

    def __len__(self):
        return sum(len(p) for p in self.pools.values())

    def stored(self, n):
        return len(self.pools[n])

    def add_many_packed(self, n, xe, xe_next, col, mask, regular, action, reward):
        """DeviceReplay.add_many_packed of the pool of n links for the REGULAR transitions of the block; the others are counted
        in dropped_irregular[n].  -> transitions stored"""
        if n not in self.pools:
            raise ValueError("MixedReplay: no pool of %d links (pools: %s)" % (n, self.sizes))
        pool = self.pools[n]
        regular = np.asarray(regular, bool)
        action = np.asarray(action, np.int32).reshape(len(regular), -1)
        reward = np.asarray(reward, np.float64).reshape(-1)
        if not regular.all():
            self.dropped_irregular[n] += int((~regular).sum())
            if not regular.any():
                return 0
            xe, xe_next, col, mask = (np.ascontiguousarray(a[regular]) for a in (xe, xe_next, col, mask))
            action, reward, regular = action[regular], reward[regular], regular[regular]
        pool.add_many_packed(xe, xe_next, col, mask, regular, action, reward)
        return int(len(regular))

    # ------------------------------------------------------------------ transitions written by the device (v2x_rollout_steps_mixed)
    def _pool(self, n, who):
        if n not in self.pools:
            raise ValueError("MixedReplay.%s: no pool of %d links (pools: %s)" % (who, n, self.sizes))
        return self.pools[n]

    def storage(self, n):
        """DeviceReplay.storage() of the pool of n links"""
        return self._pool(n, "storage").storage()

    def reserve(self, n, K):
        """DeviceReplay.reserve(K) of the pool of n links -> the first slot of the block the device is about to write"""
        return self._pool(n, "reserve").reserve(K)

    def commit(self, n, K, result):
        """DeviceReplay.commit(K, result) of the pool of n links: its head and size advance at once, the flags of the block are
        read from `result` when they are first needed"""
        self._pool(n, "commit").commit(K, result)

    def _buffers(self, counts):
        """output tensors and batch descriptors of a minibatch of counts[k] graphs from pool k: cached, so that the pointers
        are stable and a captured replay step is replayed"""
        out = self._out.get(counts)
        if out is None:
            torch, dev = self.torch, self.device
            B = sum(counts)
            R = sum(c * n for c, n in zip(counts, self.sizes))
            E = sum(c * n * (n - 2) for c, n in zip(counts, self.sizes))
            live = [n for c, n in zip(counts, self.sizes) if c > 0]
            t = dict(xe=torch.empty((R, 16), dtype=torch.float32, device=dev), xe_next=torch.empty((R, 16), dtype=torch.float32, device=dev),
                     action=torch.empty(R, dtype=torch.int32, device=dev), reward=torch.empty(B, dtype=torch.float64, device=dev),
                     graph_off=torch.empty(B + 1, dtype=torch.int32, device=dev), row_ptr=torch.empty(R + 1, dtype=torch.int32, device=dev),
                     col_idx=torch.empty(max(E, 1), dtype=torch.int32, device=dev))
            n_max = max(live)
            mk = lambda x: DeviceBatch.from_tensors(B, 0, x, t['row_ptr'], t['col_idx'], n_max * (n_max - 2), graph_off=t['graph_off'],
                                                    max_nodes=n_max)
            desc = _lib.MixedBatch(**{k: v.data_ptr() for k, v in t.items()})
            out = self._out[counts] = (t, mk(t['xe']), mk(t['xe_next']), desc)
        return out

    def sample(self, indices):
        """indices: {link count: logical indices into that pool's FIFO order (0 = oldest)}; sizes that are left out contribute
        nothing.  -> (batch of s, batch of s', action [R] int32, reward [B] float64), all in HBM: the graphs of the smallest
        size first, in the order of their indices.  s and s' share graph_off, row_ptr and col_idx."""
        for n in indices:
            if n not in self.pools:
                raise ValueError("MixedReplay.sample: no pool of %d links (pools: %s)" % (n, self.sizes))
        idx = [np.asarray(indices.get(n, ()), np.int64).reshape(-1) for n in self.sizes]
        counts = tuple(len(i) for i in idx)
        if sum(counts) == 0:
            raise ValueError("MixedReplay.sample: an empty minibatch")
        table = (_lib.ReplayPool * len(self.sizes))()
        used = []
        for k, n in enumerate(self.sizes):
            pool = self.pools[n]
            pool.flush()
            table[k].n_nodes, table[k].count = n, counts[k]
            if counts[k] == 0:
                continue
            if idx[k].min() < 0 or idx[k].max() >= pool.size:
                raise IndexError("MixedReplay.sample: pool of %d links holds %d transitions, index %d asked for"
                                 % (n, pool.size, int(idx[k].max() if idx[k].min() >= 0 else idx[k].min())))
            slots = pool.upload_slots(pool.logical_to_slot(idx[k]))
            used.append(pool)
            for name in ("xe", "xe_next", "col", "action", "reward"):
                setattr(table[k], name, getattr(pool, name).data_ptr())
            table[k].idx = slots.data_ptr()
        t, sb, sn, desc = self._buffers(counts)
        rc = self._lib.v2x_replay_gather_mixed(len(self.sizes), table, C.byref(desc), current_stream_ptr(self.device.index))
        _lib.check(self._lib, rc, None)
        for pool in used:
            pool.slots_consumed()
        return sb, sn, t['action'], t['reward']


class MixedAgent(object):
    """DQN on several scenario sizes with one shared-weight network (module docstring).  The epsilon schedule, the reward
    rule, the 50 transitions per train step and the 500-transition target sync are rl.agent.Agent's, counted over the
    simulators of all environments (stored and dropped transitions alike)."""

    def __init__(self, envs, cfg, feat_dim, n_mp_layers=2, use_graph=False, device=0, seed=None, capacity=MEMORY_CAPACITY,
                 rollout='host', trajectory_walk='serial'):
        from .device_sim import check_walk
        envs = list(envs)
        if rollout not in ROLLOUTS:
            raise ValueError("MixedAgent: rollout must be one of %s, got %r" % (list(ROLLOUTS), rollout))
        check_walk("MixedAgent: trajectory_walk", trajectory_walk)
        sizes = _check_sizes([getattr(e, 'n_Veh', 0) for e in envs], "MixedAgent")
        for e in envs:
            if not hasattr(e, 'observe_packed') or not hasattr(e, 'E'):
                raise ValueError("MixedAgent steps BatchedEnviron simulators, got %s" % type(e).__name__)
            if e.n_RB != 4 or not e.packed_ok(4):
                raise ValueError("MixedAgent: the environment of %d links must have n_RB = 4 and packed observations "
                                 "(libv2xsim.so), n_RB is %d" % (e.n_Veh, e.n_RB))
        if rollout == 'trajectory':
            from .device_sim import DeviceBatchedEnviron
            for e in envs:
                if not isinstance(e, DeviceBatchedEnviron) or e.stream_backend != 'device':
                    raise ValueError("MixedAgent: rollout='trajectory' steps every environment on the device: the environment of "
                                     "%d links must be a DeviceBatchedEnviron with streams='device', got %s%s"
                                     % (e.n_Veh, type(e).__name__,
                                        " with streams=%r" % e.stream_backend if isinstance(e, DeviceBatchedEnviron) else ""))
        self.rollout = rollout
        self.trajectory_walk = trajectory_walk                    # the walk of the mixed trajectory calls (rollout and evaluation)
        self.rollout_stats = {'trajectory': 0, 'host': 0}         # rollouts (one per train step) by the path that made them
        self.eval_stats = {'device_episodes': 0, 'host_episodes': 0}      # which path the evaluation episodes took
        self._eval_opt = None
        self._regular_look = None                                 # (the receivers last looked at, were all their graphs regular)
        self.envs = sorted(envs, key=lambda e: e.n_Veh)           # ascending size everywhere
        self.sizes = sizes
        self.num_CH = 4
        self.n_sims = sum(e.E for e in self.envs)
        self.batch_size, self.gamma = int(cfg.Batch_Size), cfg.Gamma
        self.v2v_weight, self.v2i_weight = cfg.v2v_weight, cfg.v2i_weight
        self.spec = GnnSpec(n_nodes=1, n_channels=self.num_CH, feat_dim=int(feat_dim), n_mp_layers=int(n_mp_layers),
                            share_weights=True, variable_graphs=True)
        self.online = GnnEngine(self.spec, device=device, use_graph=use_graph)
        self.target = GnnEngine(self.spec, device=device, use_graph=use_graph)
        from ..bs_brain import _glorot_list
        rng = np.random.default_rng(seed)
        self.online.set_weights(_glorot_list(self.spec, rng))
        self.target.set_weights(_glorot_list(self.spec, rng))
        self.memory = MixedReplay(capacity, sizes, device=device)
        self._draws = Memory(0)                        # (its sample_indices is the drawing rule; it stores nothing)
        self.epsilon, self.num_step, self._sync_mark = MAX_EPSILON, 0, 0
        self.num_Episodes, self.num_Train_Step = 1, 1
        self.n_iter = -(-50 // self.n_sims)            # rollout iterations per train step
        self.num_transition = self.n_iter * self.n_sims
        self.last_minibatch = None
        self._y, self._stats = {}, None

    def close(self):
        self.online.close()
        self.target.close()

    # ------------------------------------------------------------------ acting
    def observe(self):
        """[(xe [E, n, 16], mask [E, n], col [E, n (n - 2)], regular [E])] per environment, ascending size"""
        return [e.observe_packed(self.num_CH) for e in self.envs]

    def score(self, obs, envs=None, engine=None):
        """Q-values of all environments' observations by ONE forward of one ragged batch -> [q [E, n, C]] per environment.
        envs: the environments the observations are of (default: the agent's own); engine: the network that scores (default:
        the online network)"""
        envs = self.envs if envs is None else envs
        xe, rp, ci, sizes, edges = [], [np.zeros(1, np.int64)], [], [], 0
        for env, (x, mask, col, regular) in zip(envs, obs):
            E, n = mask.shape
            xe.append(x.reshape(E * n, 16))
            sizes += [n] * E
            if regular.all():                          # in-degree n - 2 everywhere: the CSR sources as observed
                deg = np.full(E * n, n - 2, np.int64)
                ci.append(col.reshape(-1))
            else:                                      # a link that is its own receiver (rare): expand the source masks
                bits = (mask[:, :, None] >> np.arange(n, dtype=np.int32)) & 1          # [E, q, p]
                deg = bits.sum(axis=2).reshape(-1).astype(np.int64)
                ci.append(np.nonzero(bits)[2].astype(np.int32))
            rp.append(edges + np.cumsum(deg))
            edges += int(deg.sum())
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        pb = PackedBatch(len(sizes), 0, np.ascontiguousarray(np.concatenate(xe)), np.concatenate(rp).astype(np.int32),
                         np.concatenate(ci).astype(np.int32), graph_off=offs)
        q = (self.online if engine is None else engine).forward(pb)
        out, r = [], 0
        for env in envs:
            rows = env.E * env.n_Veh
            out.append(q[r:r + rows].reshape(env.E, env.n_Veh, -1))
            r += rows
        return out

    def _policy_draws(self, step_no):
        """the epsilon-greedy draws of one iteration that starts at step `step_no`: environment after environment in ascending
        size, per simulator one uniform draw and, if it explores, its randint right after; epsilon advances per simulator
        -> ([actions [E, n, 1] int] per environment, [greedy simulators] per environment)"""
        C_ = self.num_CH
        steps = self.num_Episodes * 0.8 * self.num_Train_Step * self.num_transition
        per_step = (MAX_EPSILON - MIN_EPSILON) / steps
        actions, greedy = [], []
        for env in self.envs:                          # the draws of rl.agent.Agent._packed_iteration, environment after environment
            E, n = env.E, env.n_Veh
            a, g = np.zeros((E, n, 1), int), []
            for e in range(E):
                self.epsilon = MAX_EPSILON - per_step * step_no if step_no < steps else MIN_EPSILON
                step_no += 1
                if np.random.random() < self.epsilon:
                    a[e] = np.random.randint(0, C_, size=(n, 1))
                else:
                    g.append(e)
            actions.append(a)
            greedy.append(g)
        return actions, greedy

    def _draw_rollout_ahead(self, n_iter):
        """the draws of n_iter iterations, taken before the first of them runs: iteration, then environment in ascending size,
        then simulator -- the order _iteration consumes them in; nothing else draws inside a rollout, so the process-wide numpy
        stream and the final epsilon are those of the per-iteration path -> [_policy_draws] per iteration"""
        return [self._policy_draws(self.num_step + it * self.n_sims) for it in range(n_iter)]

    def _iteration(self, drawn=None):
        """every simulator of every environment steps once -> the rewards [E] per environment.  drawn: the iteration's
        _policy_draws when they were taken ahead (a device rollout that had to fall back)"""
        C_ = self.num_CH
        obs = self.observe()
        actions, greedy = self._policy_draws(self.num_step) if drawn is None else drawn
        if any(greedy):
            for a, g, q in zip(actions, greedy, self.score(obs)):
                if g:
                    a[g] = np.argmax(q[g], axis=2)[:, :, None]
        rewards = []
        for env, a, (xe, mask, col, regular) in zip(self.envs, actions, obs):
            v2v, v2i, _ = env.act(a)
            reward = self.v2v_weight * v2v.sum(axis=(1, 2)) + self.v2i_weight * v2i.sum(axis=1)
            xe_next = env.observe_packed(C_)[0]
            self.memory.add_many_packed(env.n_Veh, xe, xe_next, col, mask, regular, a.reshape(env.E, env.n_Veh), reward)
            rewards.append(reward)
        self.num_step += self.n_sims
        return rewards

    def _all_regular(self, envs=None):
        """every environment's resident graph is regular (envs: default the agent's own).  Receivers are fixed within an
        episode, so one look per set of receivers suffices (after a reset: one small download per environment); no wait for a
        result row in between."""
        envs = self.envs if envs is None else envs
        key = tuple(np.asarray(e.dest).tobytes() for e in envs)
        if self._regular_look is None or self._regular_look[0] != key:
            self._regular_look = (key, all(bool(np.all(e.resident_regular(self.num_CH))) for e in envs))
        return self._regular_look[1]

    def _trajectory_rollout(self, drawn):
        """The iterations `drawn` (_draw_rollout_ahead) as ONE library call on the resident states of all environments: per pool
        one reserve and one commit of T E_k slots, the model passed only when somebody is greedy.  -> [RolloutResult] per
        environment (the rewards [T, E_k] once they have arrived), or None when the host path has to run with these draws: an
        environment's resident graph is not regular (it cannot be scored from the fixed-degree CSR, and the host path leaves
        such transitions out), or a block does not fit a pool's ring."""
        from .device_sim import resident_rollout_steps_mixed
        T, mem = len(drawn), self.memory
        if any(T * e.E > mem.pools[e.n_Veh].capacity for e in self.envs) or not self._all_regular():
            return None
        explore, actions = [], []
        for k, env in enumerate(self.envs):
            ex = np.ones((T, env.E), np.uint8)
            for t, (_, greedy) in enumerate(drawn):
                ex[t, greedy[k]] = 0
            explore.append(ex)
            actions.append(np.stack([a[k] for a, _ in drawn]).reshape(T, env.E, env.n_Veh))
        anybody = any(g for _, greedy in drawn for g in greedy)
        sizes = [e.n_Veh for e in self.envs]
        heads = [mem.reserve(e.n_Veh, T * e.E) for e in self.envs]
        results = resident_rollout_steps_mixed(self.envs, explore, actions, [mem.storage(n) for n in sizes], heads,
                                               [mem.pools[n].capacity for n in sizes], self.v2v_weight, self.v2i_weight,
                                               engine=self.online if anybody else None, walk=self.trajectory_walk)
        for env, result in zip(self.envs, results):
            mem.commit(env.n_Veh, T * env.E, result)
        self.num_step += T * self.n_sims
        return results

    def generate_transitions(self, defer=False):
        """the ceil(50 / sum E) rollout iterations of one train step -> {link count: rewards [iterations x E]}.
        rollout='trajectory': all of them in one call on the device (rollout_stats counts the rollouts by the path they took);
        with defer the values are the RolloutResults whose downloads are in flight (.resolve().reward.reshape(-1): the same
        array) -- nothing waits for the device."""
        out = {e.n_Veh: [] for e in self.envs}
        drawn = [None] * self.n_iter
        if self.rollout == 'trajectory':
            drawn = self._draw_rollout_ahead(self.n_iter)
            results = self._trajectory_rollout(drawn)
            if results is not None:
                self.rollout_stats['trajectory'] += 1
                return {e.n_Veh: (r if defer else r.resolve().reward.reshape(-1)) for e, r in zip(self.envs, results)}
        self.rollout_stats['host'] += 1
        for d in drawn:
            for env, r in zip(self.envs, self._iteration(drawn=d)):
                out[env.n_Veh].append(r)
        return {n: np.concatenate(v) for n, v in out.items()}

    # ------------------------------------------------------------------ learning
    def quotas(self):
        """graphs of a minibatch per pool: B E_k / sum E by largest remainder over the pools that hold transitions"""
        w = [e.E if self.memory.stored(e.n_Veh) > 0 else 0 for e in self.envs]
        return mixed_quotas(self.batch_size, w)

    def replay(self, defer=False):
        """One DQN update on a mixed minibatch -> (loss, Q mean, Q max mean) as floats, or with defer (loss [1], sums [2, 1]) as
        device tensors (the sums of v2x_q_stats: all entries, per-row maxima)."""
        torch = self.memory.torch
        drawn = {}
        for env, quota in zip(self.envs, self.quotas()):                  # Memory.sample_indices' rule, ascending size
            if quota > 0:
                drawn[env.n_Veh] = np.asarray(self._draws.sample_indices(quota, self.memory.stored(env.n_Veh)), np.int64)
        self.last_minibatch = drawn
        sb, sn, action, reward = self.memory.sample(drawn)
        R, C_ = sb.n_rows, self.num_CH
        y = self._y.get(R)
        if y is None:
            y = self._y[R] = torch.empty((R, C_), dtype=torch.float32, device=sb.device)
        loss = self.online.dqn_step(self.target, sb, sn, action, reward, self.gamma, y_out=y)
        if self._stats is None or self._stats[1] == self._stats[0].shape[0]:   # a row per call: a deferred caller reads them later
            self._stats = [torch.empty((64, 2, 1), dtype=torch.float64, device=sb.device), 0]
        st = self._stats[0][self._stats[1]]
        self._stats[1] += 1
        rc = self.online._lib.v2x_q_stats(y.data_ptr(), R, 1, C_, st.data_ptr(), current_stream_ptr(self.online.device))
        _lib.check(self.online._lib, rc, None)
        if defer:
            return loss, st, R
        s = st.cpu().numpy()
        return float(loss.cpu().numpy()[0]), float(s[0, 0] / (R * C_)), float(s[1, 0] / R)

    def train(self, num_episodes, num_train_steps, verbose=False, save_dir=None, save_interval=None):
        """episodes x train steps x (ceil(50 / sum E) rollout iterations + 1 replay); target sync whenever another 500
        transitions have been collected.  save_dir: save_weights(save_dir, num_episodes, num_train_steps) at the end; with an
        integer save_interval also save_weights(save_dir, episode, num_train_steps) after every save_interval-th episode (the
        reference saves every 5: the checkpoints evaluate_training loads).
        -> (loss [1, episodes, steps], {link count: rewards [episodes, steps, iterations x E]},
        Q mean [episodes, steps], Q max mean [episodes, steps])"""
        if save_interval is not None and (int(save_interval) != save_interval or save_interval < 1):
            raise ValueError("MixedAgent.train: save_interval must be a positive integer or None, got %r" % (save_interval,))
        self.num_Episodes, self.num_Train_Step = int(num_episodes), int(num_train_steps)
        self.num_step, self._sync_mark = 0, 0
        loss = np.ones((1, num_episodes, num_train_steps))
        q_mean, q_max = np.zeros((num_episodes, num_train_steps)), np.zeros((num_episodes, num_train_steps))
        rewards = {e.n_Veh: np.zeros((num_episodes, num_train_steps, self.n_iter * e.E)) for e in self.envs}
        torch = self.memory.torch
        for ep in range(num_episodes):
            for env in self.envs:
                env.new_random_game(env.n_Veh)
            pending, rows = [], []
            for it in range(num_train_steps):
                for n, r in self.generate_transitions(defer=True).items():
                    if isinstance(r, np.ndarray):
                        rewards[n][ep, it] = r
                    else:                              # a device rollout's result row: read with the losses, below
                        rows.append((n, it, r))
                pending.append(self.replay(defer=True))
                mark = self.num_step // UPDATE_TARGET_FREQUENCY
                if mark > self._sync_mark:
                    self._sync_mark = mark
                    self.target.copy_weights_from(self.online)
            lo = torch.stack([p[0].double() for p in pending]).cpu().numpy()              # one read-back per episode
            st = torch.stack([p[1] for p in pending]).cpu().numpy()
            for n, it, r in rows:
                rewards[n][ep, it] = r.resolve().reward.reshape(-1)
            for pool in self.memory.pools.values():    # (the flags of the device blocks: their rows have arrived)
                pool.regular_flags()
            rows = np.array([p[2] for p in pending], np.float64)
            loss[0, ep] = lo[:, 0]
            q_mean[ep], q_max[ep] = st[:, 0, 0] / (rows * self.num_CH), st[:, 1, 0] / rows
            if verbose:
                print('episode', ep + 1, 'loss %.4f' % loss[0, ep].mean(),
                      'reward', {n: round(float(v[ep].sum()), 3) for n, v in rewards.items()})
            if save_dir is not None and save_interval is not None and (ep + 1) % save_interval == 0:
                self.save_weights(save_dir, ep + 1, num_train_steps)
        if save_dir is not None:
            self.save_weights(save_dir, num_episodes, num_train_steps)
        return loss, rewards, q_mean, q_max

    # ------------------------------------------------------------------ weights
    def _weight_paths(self, save_dir, num_episodes, num_train_steps):
        from .run import weight_file_names
        return [os.path.join(save_dir, name) for name in weight_file_names(int(num_episodes), int(num_train_steps), self.batch_size)]

    def save_weights(self, save_dir, num_episodes, num_train_steps):
        """the online and the target network into save_dir under the names of rl.run.weight_file_names(num_episodes,
        num_train_steps, batch size), in the container of GnnQModel.save_weights -> the two paths"""
        from ..bs_brain import keras_layer_table, save_weight_file
        os.makedirs(save_dir, exist_ok=True)
        paths = self._weight_paths(save_dir, num_episodes, num_train_steps)
        for index, (engine, path) in enumerate(zip((self.online, self.target), paths)):
            save_weight_file(path, engine.get_weights(), keras_layer_table(self.spec, index))
        return paths

    def load_weights(self, save_dir, num_episodes, num_train_steps):
        """the online and the target network from the two files save_weights wrote -> the two paths"""
        from ..bs_brain import load_weight_file
        paths = self._weight_paths(save_dir, num_episodes, num_train_steps)
        for engine, path in zip((self.online, self.target), paths):
            engine.set_weights(load_weight_file(path))
        return paths

    # ------------------------------------------------------------------ evaluation
    def _check_evaluate_training(self, eval_envs, checkpoints, engines, save_dir, num_trials, opt_backend, eval_backend, T):
        """ValueError for anything evaluate_training cannot take, before any draw, reset or load -> (the environments in
        ascending size, K)"""
        try:
            envs = MixedAgent._check_test_run(self, eval_envs, opt_backend, eval_backend, T)
        except ValueError as err:
            raise ValueError(str(err).replace("MixedAgent.test_run", "MixedAgent.evaluate_training"))
        if (engines is None) == (checkpoints is None):
            raise ValueError("MixedAgent.evaluate_training: give the checkpoints' episode tags (with save_dir) or their loaded "
                             "engines, one of the two")
        if engines is None and save_dir is None:
            raise ValueError("MixedAgent.evaluate_training: checkpoints are loaded from save_dir")
        K = len(list(checkpoints if engines is None else engines))
        if not 1 <= K <= _lib.SWEEP_MAX_MODELS:
            raise ValueError("MixedAgent.evaluate_training: 1..%d checkpoints, got %d" % (_lib.SWEEP_MAX_MODELS, K))
        if T < 1 or int(num_trials) < 1:
            raise ValueError("MixedAgent.evaluate_training: at least one step and one trial, got %d and %d" % (T, num_trials))
        return envs, K

    def _check_test_run(self, eval_envs, opt_backend, eval_backend, num_test_step):
        """ValueError for anything test_run cannot take, before any draw or reset -> the environments in ascending size"""
        if eval_backend not in EVAL_BACKENDS:
            raise ValueError("MixedAgent.test_run: eval_backend must be one of %s, got %r" % (list(EVAL_BACKENDS), eval_backend))
        if opt_backend not in EVAL_OPT_BACKENDS:
            raise ValueError("MixedAgent.test_run: opt_backend must be one of %s (the searches of rl/optimum.py on the GPU), got %r"
                             % (list(EVAL_OPT_BACKENDS), opt_backend))
        envs = list(eval_envs)
        _check_sizes([getattr(e, 'n_Veh', 0) for e in envs], "MixedAgent.test_run")
        for e in envs:
            if not hasattr(e, 'observe_packed') or not hasattr(e, 'E'):
                raise ValueError("MixedAgent.test_run steps BatchedEnviron simulators, got %s" % type(e).__name__)
            if e.n_RB != self.num_CH or not e.packed_ok(self.num_CH):
                raise ValueError("MixedAgent.test_run: the environment of %d links must have n_RB = %d and packed observations "
                                 "(libv2xsim.so), n_RB is %d" % (e.n_Veh, self.num_CH, e.n_RB))
        if eval_backend == 'device':
            from .device_sim import MAX_STATES, DeviceBatchedEnviron
            for e in envs:
                if not isinstance(e, DeviceBatchedEnviron) or e.stream_backend != 'device':
                    raise ValueError("MixedAgent.test_run: eval_backend='device' steps every environment on the device: the "
                                     "environment of %d links must be a DeviceBatchedEnviron with streams='device', got %s%s"
                                     % (e.n_Veh, type(e).__name__,
                                        " with streams=%r" % e.stream_backend if isinstance(e, DeviceBatchedEnviron) else ""))
                if num_test_step * e.E > MAX_STATES:
                    raise ValueError("MixedAgent.test_run: eval_backend='device' needs T E <= %d (the snapshots of an episode are "
                                     "one stacked search problem), got T = %d, E = %d at %d links"
                                     % (MAX_STATES, num_test_step, e.E, e.n_Veh))
        return sorted(envs, key=lambda e: e.n_Veh)

    def _optimum_actions(self, states, n_states, n, opt_backend, opt_restarts, calls):
        """the joint actions [n_states, n] one search of rl/optimum.py finds for the stacked states (an environment's E
        simulators, or the T E snapshots of an episode); calls: the single-state calls the search stands for -- 'bound' gets
        their node budget"""
        from .optimum import DEFAULT_LOCAL_RESTARTS, DEFAULT_MAX_NODES, OptimalAllocation, decode
        if self._eval_opt is None:
            self._eval_opt = OptimalAllocation(self.online.device)
        opt, w_v2v, w_v2i = self._eval_opt, self.v2v_weight, self.v2i_weight
        if opt_backend == 'local':
            restarts = DEFAULT_LOCAL_RESTARTS if opt_restarts is None else opt_restarts
            return np.asarray(opt.search_local(states, w_v2v, w_v2i, restarts=restarts)[0]).reshape(n_states, n)
        if opt_backend == 'bound':
            index, _ = opt.search_bound(states, w_v2v, w_v2i, max_nodes=calls * DEFAULT_MAX_NODES)
        else:
            index, _ = opt.search(states, w_v2v, w_v2i)
        return decode(index, n, self.num_CH).reshape(n_states, n)

    def test_run(self, eval_envs, num_episodes, num_test_step, opt_flag=False, opt_backend='device', opt_restarts=None,
                 fixed_epsilon=0.0, eval_backend='host'):
        """Agent.test_run for the shared-weight network on several link counts at once: the policy (greedy, or random with
        probability fixed_epsilon per simulator and step) next to the random-action baseline and, with opt_flag, the optimum.
        eval_envs: BatchedEnvirons of 1..8 distinct link counts -- not necessarily the training sizes; the E_k simulators of an
        environment are parallel episodes.  -> {link count: {'gnn': books, 'random': books[, 'optimal': books]}}, books the five
        arrays of Agent.test_run -- return [episodes, E_k], reward [episodes, E_k, steps], V2V rates [episodes, E_k, steps, n],
        V2I rates and base-station interference [episodes, E_k, steps, C] -- filled with its numpy expressions.
        A step of the 'host' loop: draw_eval_step (every environment in ascending size, every simulator: the random scheme's
        action, np.random.random(), _random_channels if it is below fixed_epsilon); the baseline's rates
        (compute_reward_with_channel_selection); with opt_flag one search of rl/optimum.py per environment over its E_k states
        (opt_backend 'device': exhaustive, 'bound': branch and bound, 'local' with opt_restarts restarts: a lower bound on the
        optimum, not the optimum; the host's brute force is refused) and the rates of what it found; ONE score() of all
        observations when somebody is greedy; env.act under the policy's actions.
        eval_backend='device' (every environment a DeviceBatchedEnviron with streams='device', T E_k <= 65535; anything else is
        a ValueError before any draw or reset): the draws of an episode are taken ahead in the host loop's order
        (draw_eval_episode_ahead), ONE resident_evaluate_steps_mixed call walks, scores and pays all link counts, and with
        opt_flag one stacked search and one rates() call per link count run on trajectory_states(T) ('bound' with the node
        budget of T E_k single calls).  Same books, numpy stream, num_step and simulator state as 'host'.  An episode in which
        some environment's graph is not regular after the reset runs through the host loop; eval_stats counts both kinds."""
        T, C_ = int(num_test_step), self.num_CH
        envs = self._check_test_run(eval_envs, opt_backend, eval_backend, T)
        n_sims = sum(e.E for e in envs)
        w_v2v, w_v2i = self.v2v_weight, self.v2i_weight
        schemes = SCHEMES if opt_flag else SCHEMES[:2]

        def book(E, n):
            return [np.zeros((num_episodes, E)), np.zeros((num_episodes, E, T)), np.zeros((num_episodes, E, T, n)),
                    np.zeros((num_episodes, E, T, C_)), np.zeros((num_episodes, E, T, C_))]

        def record(b, ep, e, st, v2v, v2i, interference):
            b[1][ep, e, st] = w_v2v * np.sum(v2v) + w_v2i * np.sum(v2i)
            b[0][ep, e] += b[1][ep, e, st]
            b[2][ep, e, st, :] = np.sum(v2v, axis=1)
            b[3][ep, e, st, :] = v2i
            b[4][ep, e, st, :] = interference

        def record_optimum(b, ep, e, st, v2v, v2i, interference):
            if w_v2v * np.sum(v2v) + w_v2i * np.sum(v2i) > 0:             # at least one feasible solution
                record(b, ep, e, st, v2v, v2i, interference)

        books = {env.n_Veh: {s: book(env.E, env.n_Veh) for s in schemes} for env in envs}
        for ep in range(num_episodes):
            for env in envs:
                env.new_random_game(env.n_Veh)
            if eval_backend == 'device' and T > 0 and self._all_regular(envs):
                from .device_sim import resident_evaluate_steps_mixed
                baseline, explore, rand = draw_eval_episode_ahead(envs, C_, fixed_epsilon, T)
                anybody = not all(x.all() for x in explore)
                results = resident_evaluate_steps_mixed(envs, explore, rand, baseline, w_v2v, w_v2i,
                                                        engine=self.online if anybody else None, walk=self.trajectory_walk)
                for env, res in zip(envs, results):
                    E, n, b = env.E, env.n_Veh, books[env.n_Veh]
                    r = res.resolve()
                    if opt_flag:
                        states = env.trajectory_states(T)
                        found = self._optimum_actions(states, T * E, n, opt_backend, opt_restarts, T * E)
                        o_v2v, o_v2i, o_intf = (a.reshape((T, E) + a.shape[1:]) for a in states.rates(found))
                    for st in range(T):
                        for e in range(E):
                            record(b['random'], ep, e, st, r.v2v_rate[1, st, e][:, None], r.v2i_rate[1, st, e], r.interference[1, st, e])
                            if opt_flag:
                                record_optimum(b['optimal'], ep, e, st, o_v2v[st, e][:, None], o_v2i[st, e], o_intf[st, e])
                            record(b['gnn'], ep, e, st, r.v2v_rate[0, st, e][:, None], r.v2i_rate[0, st, e], r.interference[0, st, e])
                self.num_step += T * n_sims
                self.eval_stats['device_episodes'] += 1
                continue
            self.eval_stats['host_episodes'] += 1
            for st in range(T):
                baseline, explore, rand = draw_eval_step(envs, C_, fixed_epsilon)
                for env, a in zip(envs, baseline):
                    v2v, v2i, intf = env.compute_reward_with_channel_selection(a[:, :, None])
                    for e in range(env.E):
                        record(books[env.n_Veh]['random'], ep, e, st, v2v[e], v2i[e], intf[e])
                if opt_flag:
                    for env in envs:
                        found = self._optimum_actions(env, env.E, env.n_Veh, opt_backend, opt_restarts, env.E)
                        v2v, v2i, intf = env.compute_reward_with_channel_selection(found[:, :, None])
                        for e in range(env.E):
                            record_optimum(books[env.n_Veh]['optimal'], ep, e, st, v2v[e], v2i[e], intf[e])
                actions = [r[:, :, None].copy() for r in rand]
                if not all(x.all() for x in explore):
                    obs = [env.observe_packed(C_) for env in envs]
                    for a, x, q in zip(actions, explore, self.score(obs, envs)):
                        g = np.nonzero(x == 0)[0]
                        if len(g):
                            a[g] = np.argmax(q[g], axis=2)[:, :, None]
                for env, a in zip(envs, actions):
                    v2v, v2i, intf = env.act(a)
                    for e in range(env.E):
                        record(books[env.n_Veh]['gnn'], ep, e, st, v2v[e], v2i[e], intf[e])
                self.num_step += n_sims
        return books

    def evaluate_training(self, eval_envs, checkpoints, num_test_step, num_trials, fixed_epsilon, opt_flag=False,
                          opt_backend='device', opt_restarts=None, eval_backend='host', save_dir=None, engines=None,
                          num_train_steps=None):
        """Evaluation of the TRAINING PROCESS for the shared-weight network (Agent.evaluate_training_diff_trials; the reference's
        RL_Evaluated_main_Epsilon_DiffTrails.py): K saved networks under a FIXED epsilon-greedy policy over re-seeded trials,
        next to the random scheme and, with opt_flag, the optimum -- on any link counts (eval_envs as for test_run).
        checkpoints: the episode tags train(save_interval=...) saved under (save_weights(save_dir, tag, num_train_steps);
        num_train_steps defaults to the agent's last train()); or engines: K loaded GnnEngines of the agent's spec.
        The reference re-seeds before every (trial, checkpoint), so all checkpoints of a trial face the same episode and the
        same epsilon draws and differ in the network alone.  Here that holds by construction -- trial t:
        random.seed(t + 1), np.random.seed(t + 1); every environment is reset once; the episode's draws are taken once
        (draw_eval_episode_ahead: ascending size, simulator); all K checkpoints are scored on that ONE walked episode, and the
        simulators step under the LAST checkpoint's actions.
        -> {link count: {'gnn': books, 'random': books[, 'optimal': books]}}, books the five arrays of test_run -- return,
        reward, V2V rates, V2I rates, base-station interference -- filled with its numpy expressions, with the leading axes
        [trials, K, E_k] for 'gnn' (reward [trials, K, E_k, steps]) and [trials, E_k] for the two others.
        eval_backend='host' is the definition.  Per step: the baseline's rates; with opt_flag one search per environment;
        for k = 0 .. K - 1 one score() by network k (when somebody is greedy) and the rates of its actions, computed without
        stepping (compute_reward_with_channel_selection); then one env.act under network K - 1's actions.
        eval_backend='device' (what test_run(eval_backend='device') needs of the environments, refused before any draw or
        reset): ONE resident_evaluate_sweep_mixed call per trial (trajectory_walk='wide': on the pools' wide workspaces) and,
        with opt_flag, one stacked search and one rates() call per link count on trajectory_states(T).  Same books, generator
        states, num_step and simulator state as 'host'.  A trial in which some environment's graph is not regular after the
        reset runs the host loop; eval_stats counts both kinds."""
        import random
        T, C_ = int(num_test_step), self.num_CH
        envs, K = self._check_evaluate_training(eval_envs, checkpoints, engines, save_dir, num_trials, opt_backend, eval_backend, T)
        num_trials = int(num_trials)
        n_sims = sum(e.E for e in envs)
        w_v2v, w_v2i = self.v2v_weight, self.v2i_weight

        def book(lead, n):
            return [np.zeros(lead), np.zeros(lead + (T,)), np.zeros(lead + (T, n)), np.zeros(lead + (T, C_)), np.zeros(lead + (T, C_))]

        def record(b, at, st, v2v, v2i, interference):                  # (test_run's record, `at` = the book's leading index)
            b[1][at + (st,)] = w_v2v * np.sum(v2v) + w_v2i * np.sum(v2i)
            b[0][at] += b[1][at + (st,)]
            b[2][at + (st,)] = np.sum(v2v, axis=1)
            b[3][at + (st,)] = v2i
            b[4][at + (st,)] = interference

        def record_optimum(b, at, st, v2v, v2i, interference):
            if w_v2v * np.sum(v2v) + w_v2i * np.sum(v2i) > 0:             # at least one feasible solution
                record(b, at, st, v2v, v2i, interference)

        books = {}
        for env in envs:
            b = books[env.n_Veh] = {'gnn': book((num_trials, K, env.E), env.n_Veh), 'random': book((num_trials, env.E), env.n_Veh)}
            if opt_flag:
                b['optimal'] = book((num_trials, env.E), env.n_Veh)
        loaded = []
        if engines is None:
            from ..bs_brain import load_weight_file
            steps = self.num_Train_Step if num_train_steps is None else num_train_steps
            for tag in checkpoints:
                path = self._weight_paths(save_dir, tag, steps)[0]
                if not os.path.exists(path):
                    raise ValueError("MixedAgent.evaluate_training: no checkpoint %s" % path)
            for tag in checkpoints:
                engine = GnnEngine(self.spec, device=self.online.device)
                loaded.append(engine)
                engine.set_weights(load_weight_file(self._weight_paths(save_dir, tag, steps)[0]))
            engines = loaded
        engines = list(engines)
        try:
            for tr in range(num_trials):
                random.seed(tr + 1)
                np.random.seed(tr + 1)
                for env in envs:
                    env.new_random_game(env.n_Veh)
                baseline, explore, rand = draw_eval_episode_ahead(envs, C_, fixed_epsilon, T)
                if eval_backend == 'device' and self._all_regular(envs):
                    from .device_sim import resident_evaluate_sweep_mixed
                    anybody = not all(x.all() for x in explore)
                    results = resident_evaluate_sweep_mixed(envs, explore, rand, baseline, w_v2v, w_v2i,
                                                            engines=engines if anybody else None, K=K, walk=self.trajectory_walk)
                    for env, res in zip(envs, results):
                        E, n, b = env.E, env.n_Veh, books[env.n_Veh]
                        r = res.resolve()
                        if opt_flag:
                            states = env.trajectory_states(T)
                            found = self._optimum_actions(states, T * E, n, opt_backend, opt_restarts, T * E)
                            o_v2v, o_v2i, o_intf = (a.reshape((T, E) + a.shape[1:]) for a in states.rates(found))
                        for st in range(T):
                            for e in range(E):
                                record(b['random'], (tr, e), st, r.v2v_rate[K, st, e][:, None], r.v2i_rate[K, st, e],
                                       r.interference[K, st, e])
                                if opt_flag:
                                    record_optimum(b['optimal'], (tr, e), st, o_v2v[st, e][:, None], o_v2i[st, e], o_intf[st, e])
                                for k in range(K):
                                    record(b['gnn'], (tr, k, e), st, r.v2v_rate[k, st, e][:, None], r.v2i_rate[k, st, e],
                                           r.interference[k, st, e])
                    self.num_step += T * n_sims
                    self.eval_stats['device_episodes'] += 1
                    continue
                self.eval_stats['host_episodes'] += 1
                for st in range(T):
                    for env, a in zip(envs, baseline):
                        v2v, v2i, intf = env.compute_reward_with_channel_selection(a[st][:, :, None])
                        for e in range(env.E):
                            record(books[env.n_Veh]['random'], (tr, e), st, v2v[e], v2i[e], intf[e])
                    if opt_flag:
                        for env in envs:
                            found = self._optimum_actions(env, env.E, env.n_Veh, opt_backend, opt_restarts, env.E)
                            v2v, v2i, intf = env.compute_reward_with_channel_selection(found[:, :, None])
                            for e in range(env.E):
                                record_optimum(books[env.n_Veh]['optimal'], (tr, e), st, v2v[e], v2i[e], intf[e])
                    greedy = not all(x[st].all() for x in explore)
                    obs = [env.observe_packed(C_) for env in envs] if greedy else None
                    for k, engine in enumerate(engines):
                        actions = [r[st][:, :, None].copy() for r in rand]
                        if greedy:
                            for a, x, q in zip(actions, explore, self.score(obs, envs, engine=engine)):
                                g = np.nonzero(x[st] == 0)[0]
                                if len(g):
                                    a[g] = np.argmax(q[g], axis=2)[:, :, None]
                        for env, a in zip(envs, actions):
                            v2v, v2i, intf = env.compute_reward_with_channel_selection(a)
                            for e in range(env.E):
                                record(books[env.n_Veh]['gnn'], (tr, k, e), st, v2v[e], v2i[e], intf[e])
                    for env, a in zip(envs, actions):                     # the simulators step under the last checkpoint's actions
                        env.act(a)
                    self.num_step += n_sims
        finally:
            for engine in loaded:
                engine.close()
        return books
