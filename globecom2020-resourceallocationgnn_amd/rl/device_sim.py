"""The simulator's channel step, observation and rates on the GPU (csrc/v2xsimdev.hip, the v2x_sim_* entry points of
include/v2xgnn.h): the device counterpart of rl/native_sim.py's channels / interference_db / observe_packed / reward.

`DeviceChannels` owns the arrays of E simulator states of n links and rb resource blocks as torch tensors in HBM --
shadowing, path loss + shadowing, fast fading, observation, rates -- and issues the three launches on torch's current
stream.  Only small things cross the bus: the uniforms of a step go up (one pinned staging buffer), the packed
observation (xe / mask / col / regular) and the rates come down.

    dc = DeviceChannels(E, n, rb)
    dc.upload('v2i_shadow', s_i); dc.upload('v2v_shadow', s_v)
    dc.step(u, vel, pos)                        # u [E, n_u] uniforms of the step: v2x_sim_channels
    dc.observe(dest)                            # v2x_sim_observe
    xe, mask, col, regular = dc.fetch_observation()
    dc.rates(actions)                           # v2x_sim_rates
    r = dc.fetch_rates()                        # dict: v2v_rate, v2i_rate, interference, v2i_interf, v2v_interf
    index, reward = OptimalAllocation().search(dc, 1.0, 0.1)        # on the device arrays, no upload

Mobility and the MT19937 streams have a device form too (v2x_sim_stream), and a whole step is one call that needs nothing
from the host but the actions (v2x_sim_advance: rates, stream, channels, observation -- four launches, capturable):

    dc.set_grid((up, down, left, right), width, height, timestep)
    dc.upload('keys', keys); dc.upload('mtpos', mtpos); dc.upload('pos', xy); dc.upload('dirs', dirs); dc.upload('vel', vel)
    dc.stream(mobility=True)                    # moves the vehicles, then the step's uniforms into tensor('u')
    dc.advance(actions)                         # or all of a step at once
    dc.traffic                                  # {'bytes_up': ..., 'bytes_down': ...}: every byte this object sent over the bus

The episode reset (new_random_game) runs on the resident state too (v2x_sim_reset: the draws, the channel update and the
observation in three launches; reset_draw() is the first launch alone):

    dc.reset()                                  # new vehicles, initial shadowing, channels, receivers, observation
    vel, dest, regular, status = dc.fetch_reset()      # one small download; status bit 0: reset_tie_flags(pos, dest)

A DQN rollout runs on the resident state as well, one iteration per call (v2x_rollout_step) or T of them in one call
(v2x_rollout_steps).  The two calls are ONE host path -- one argument check, one set of buffers per T (T = None: the single
iteration), one policy upload through a ring of page-locked copies, one struct builder, one result download -- that ends in
the entry point of its name; both hand out a RolloutResult:

    res = dc.rollout_step(explore, random_actions, storage, head, capacity, w_v2v, w_v2i, engine, row_ptr)      # [E], [E, n]
    res = dc.rollout_steps(explore, random_actions, storage, head, capacity, w_v2v, w_v2i, engine, row_ptr)     # [T, E], [T, E, n]
    res.resolve().reward, res.regular           # [E], [2, E] / [T, E], [T, 2, E]
    res.stored_regular, res.resident_regular    # the flags of the stored slots [T E]; of the observation left resident [E]

An evaluation episode runs the same way (v2x_eval_steps: no replay memory, the policy and a baseline scheme paid per state,
rates instead of a reward alone), and the T snapshots it leaves are one stacked problem for OptimalAllocation:

    res = dc.eval_steps(explore, policy_random, baseline_actions, w_v2v, w_v2i, engine)       # [T, E], [T, E, n], [T, E, n] or None
    res.resolve().v2v_rate, res.v2i_rate, res.interference, res.reward, res.actions, res.regular     # [S, T, E, ...], [T + 1, E]
    states = dc.trajectory_states(T)            # E' = T E states; valid until the next trajectory call of that T
    index, reward = OptimalAllocation().search(states, 1.0, 0.1); states.rates(actions)

Both trajectory calls take walk='serial' (the default: one workgroup per simulator walks its T steps) or walk='wide'
(v2x_rollout_steps_wide / v2x_eval_steps_wide: the steps spread over the chip, the same bits); dc.walk_calls counts them.
With walk='wide' they also take stream_phase='chain' (the default: one launch draws the streams of all T steps) or
stream_phase='split' (v2x_rollout_steps_split / v2x_eval_steps_split: raw words, offset walk and conversion in three launches,
the same bits); dc.stream_phase_calls counts the wide calls by the form that ran.  At one simulator of 20 links and T = 50
the split form takes the rollout from 1.54 to 0.88 ms (the host library's native rollout: 1.06 ms); at 50 simulators and T = 1
the forms are level (profiles/trajectory_split_timing.json).

Several DeviceChannels of DIFFERENT link counts make their rollouts in one library call (v2x_rollout_steps_mixed: one walk
launch, one assembly launch, one forward of a variable_graphs engine over all pools' observations, one finish launch), every
pool with its own policy upload, replay storage and result download; resident_rollout_steps_mixed does the same for one
DeviceBatchedEnviron per link count (rl/mixed.py, MixedAgent(rollout='trajectory')).  walk='wide' spreads every pool's steps
over the chip (v2x_rollout_steps_mixed_wide: six launches in the walk's place, the wide walk with the split stream phase on
every pool's own cached workspaces, the same bits; each pool's walk_calls['wide'] and stream_phase_calls['split'] count it):

    rows = rollout_steps_mixed([dc8, dc12], [explore8, explore12], [random8, random12], [storage8, storage12], heads, capacities,
                               w_v2v, w_v2i, engine)                                          # -> [RolloutResult] per pool

... and their evaluation episodes (v2x_eval_steps_mixed: the same walk, assembly and forward, one finish launch that pays both
schemes of every pool), every pool with its own policy upload and result download; resident_evaluate_steps_mixed for one
DeviceBatchedEnviron per link count (MixedAgent.test_run(eval_backend='device')), walk='wide' as above
(v2x_eval_steps_mixed_wide); afterwards every pool's trajectory_states(T) holds its T snapshots:

    rows = eval_steps_mixed([dc8, dc12], [explore8, explore12], [random8, random12], [baseline8, baseline12], w_v2v, w_v2i,
                            engine)                                                           # -> [EvalResult] per pool

... and K networks on those same steps (v2x_eval_sweep_mixed: ONE walk, one assembly, K forwards of the one batch, one finish
launch that pays every network's policy on the shared draws and the baseline); resident_evaluate_sweep_mixed for one
DeviceBatchedEnviron per link count (MixedAgent.evaluate_training(eval_backend='device')):

    rows = eval_sweep_mixed([dc8, dc12], [explore8, explore12], [random8, random12], [baseline8, baseline12], w_v2v, w_v2i,
                            [engine_a, engine_b, engine_c])                    # -> [EvalResult] per pool, 3 + 1 schemes

`DeviceBatchedEnviron` is a `BatchedEnviron` whose heavy arrays never leave HBM: the channel update, the observable
interference, the observation and the rates run on the device; mobility and the MT19937 streams stay on the host
(libv2xsim.so) by default and move to the device with streams='device'.
The host simulator stays the default and the definition; the two agree to the rounding of the two math libraries
(tests/test_gpu_device_sim.py).  There is no CPU fallback: without a GPU every device call raises.

Beyond the 31 links of the packed observation (one 32-bit source mask per link) the resident observation is kept in RECEIVER
form -- `observe_recv`: xe as before, the links' receivers and one flag byte per state in place of mask / col / regular -- and
`rollout_steps_recv` is the whole rollout of 3..128-link simulators in one call (v2x_rollout_steps_recv), stored in
rl/replay.py ReceiverReplay's layout; `DeviceBatchedEnviron(streams='device')` serves 32..128 links on it.  It takes
stream_phase='chain' (the default) or 'split' too (v2x_rollout_steps_recv_split: raw words, an offset walk with two vehicles
per lane and the conversion in three launches on a second workspace made once per T; the same bits, 2.5-2.7x faster at
32..128 links, profiles/rollout_recv_split_timing.json), and with 'split' stream_words='serial' (the default) or 'jump'
(v2x_rollout_steps_recv_jump: the raw words beyond a prefix drawn in chunks that jump-ahead polynomials of MT19937 enter --
`jump_plan`, a table and a scratch made once; the same word array, the call 2-10.7x faster again at 32..128 links,
profiles/rollout_recv_jump_timing.json; the evaluation and sweep calls below take it too).  `eval_steps_recv` is the evaluation episode of that form
(v2x_eval_steps_recv / _split: the same front, then k_eval_finish_recv paying the policy and the baseline on every step's
snapshot; -> RecvEvalResult), on the same buffers; `DeviceBatchedEnviron.evaluate_steps` goes through it beyond 31 links, and
trajectory_states(T) serves the snapshots of whichever form ran last (profiles/eval_recv_timing.json).  `eval_sweep_recv`
scores K fixed-size networks on those same steps in one call (v2x_eval_sweep_recv / _split: that front once, K - 1 further
forwards of the one batch, k_eval_finish_sweep_recv; -> RecvEvalResult of K (+ 1) schemes); `DeviceBatchedEnviron.evaluate_sweep`
is its resident form, Agent.evaluate_training_sweep its caller (profiles/eval_sweep_recv_timing.json).
"""
import ctypes as C

import numpy as np

from . import native_sim
from ..lib import (Eval, EvalMixed, EvalRecv, EvalSweep, EvalSweepRecv, MIXED_MAX_POOLS, SWEEP_MAX_MODELS, OptProblem, Rollout,
                   MtJump, RolloutMixed, RolloutRecv, RolloutTraj, SimReset, SimStep, TrajWs, check, load_library)
from .batched_env import BatchedEnviron

MAX_LINKS, MAX_RB, MAX_STATES = 128, 16, 65535          # v2x_sim_channels / v2x_sim_rates
OBSERVE_MIN_LINKS, OBSERVE_MAX_LINKS, XE_WIDTH = 3, 31, 16
RECV_MAX_LINKS = 128                                     # v2x_sim_observe_recv / v2x_rollout_steps_recv: receivers, no source masks
FLAG_OWN, FLAG_BAD = 1, 2                                # the bits of their flag bytes
MT_WORDS, MAX_LANES = 624, 64                            # v2x_sim_stream

# the radio constants of BatchedEnviron (Environment.py:183-212)
DEFAULT_CONSTANTS = dict(p_v2v=10.0, p_v2i=23.0, veh_gain=3.0, bs_gain=8.0, bs_nf=5.0, veh_nf=9.0, sig2=10 ** (-114 / 10))

_CHANNEL_TENSORS = ('v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff')


def uniforms_per_step(n, rb):
    """uniforms one channel update of a state consumes: n + n^2 shadowing draws, 2 n rb + 2 n^2 rb Rayleigh draws (even)"""
    return n + n * n + 2 * n * rb + 2 * n * n * rb


RESET_MAX_LINKS = 28                                     # v2x_sim_reset: groups of four vehicles, one thread per link in a wave
RESET_TIE, RESET_NO_DRAW = 1, 2                          # the bits of its status flags
RESETS = ('host', 'device')                              # who runs new_random_game of a DeviceBatchedEnviron


def check_reset_grid(who, lanes, width, height):
    """ValueError unless the squared distances of a device reset are exact: every lane coordinate a multiple of 2^-10 in
    [0, 2^15), width and height integers there (vehicles stand on a lane and on an integer along it), so dx dx + dy dy is a sum
    of two 50-bit integers over 2^20 and the ranking by it is the ranking by the host's np.abs"""
    tab = np.asarray(lanes, np.float64)
    if not (np.all(tab >= 0) and np.all(tab < 32768.0) and np.all(tab * 1024.0 == np.floor(tab * 1024.0))):
        raise ValueError("%s: the device reset ranks neighbours by exact squared distances: lane coordinates must be multiples of "
                         "2^-10 in [0, 2^15)" % who)
    for name, v in (('width', width), ('height', height)):
        if not (0 <= v < 32768.0 and v == np.floor(v)):
            raise ValueError("%s: the device reset draws positions as integers in [0, %s]: an integer in [0, 2^15) needed, got %r"
                             % (who, name, v))


def reset_tie_flags(pos, dest):
    """Bit 0 of v2x_sim_reset's status from host arrays: pos [E, n, 2], dest [E, n] -> [E] uint8, 1 where for some link another
    vehicle (the link itself included) has exactly the squared distance dx dx + dy dy of the link's receiver.  These are the
    resets whose receivers depend on the order a sort leaves among equal keys: numpy's argsort leaves whatever its build and
    the CPU give, the device ranks by (squared distance, index)."""
    pos, dest = np.asarray(pos, np.float64), np.asarray(dest, np.int64)
    dx = pos[:, :, None, 0] - pos[:, None, :, 0]
    dy = pos[:, :, None, 1] - pos[:, None, :, 1]
    d2 = dx * dx + dy * dy                                                   # [e, link, vehicle]
    same = d2 == np.take_along_axis(d2, dest[:, :, None], axis=2)
    np.put_along_axis(same, dest[:, :, None], False, axis=2)                 # (the receiver itself)
    return same.any(axis=(1, 2)).astype(np.uint8)


def _align(x, a=64):
    return (x + a - 1) // a * a


def trajectory_workspace_layout(E, n, rb, T):
    """-> (the byte offsets of traj_xe, traj_col, traj_mask, traj_regular, traj_v2v_ff, traj_v2i_ff, traj_v2i_abs in the one
    workspace of v2x_rollout_steps, its size): the formula of include/v2xgnn.h, every array rounded up to 256 bytes"""
    parts = (4 * (T + 1) * E * n * XE_WIDTH, 4 * (T + 1) * E * n * (n - 2), 4 * (T + 1) * E * n, (T + 1) * E,
             8 * T * E * n * n * rb, 8 * T * E * n * rb, 8 * T * E * n)
    offs, o = [], 0
    for b in parts:
        offs.append(o)
        o += _align(b, 256)
    return dict(zip(('traj_xe', 'traj_col', 'traj_mask', 'traj_regular', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs'), offs)), o


def wide_workspace_layout(E, n, rb, T):
    """-> (the byte offsets of u_all, xy_all, pl, gs, ob_state, ob_interf in the workspace of the wide walk, its size): the
    formula of include/v2xgnn.h (v2x_traj_wide_workspace_bytes), every array rounded up to 256 bytes"""
    n_u, n_el = uniforms_per_step(n, rb), n + n * n
    parts = (8 * T * E * n_u, 16 * T * E * n, 8 * T * E * n_el, 8 * T * E * n_el, 8 * (T - 1) * E * n * (3 * rb + 1),
             8 * (T - 1) * E * n * rb)
    offs, o = [], 0
    for b in parts:
        offs.append(o)
        o += _align(b, 256)
    return dict(zip(('u_all', 'xy_all', 'pl', 'gs', 'ob_state', 'ob_interf'), offs)), o


RECV_SECTIONS = ('traj_xe', 'traj_recv', 'traj_flags', 'traj_v2v_ff', 'traj_v2i_ff', 'traj_v2i_abs', 'row_ptr', 'col_idx')


def recv_workspace_layout(E, n, rb, T):
    """-> (the byte offsets of RECV_SECTIONS and, under 'wide', of the wide walk's own part in the ONE workspace of
    v2x_rollout_steps_recv, its size): the formula of include/v2xgnn.h, every array rounded up to 256 bytes"""
    parts = (4 * (T + 1) * E * n * XE_WIDTH, 4 * (T + 1) * E * n, (T + 1) * E, 8 * T * E * n * n * rb, 8 * T * E * n * rb,
             8 * T * E * n, 4 * (T * E * n + 1), 4 * T * E * n * (n - 1))
    offs, o = [], 0
    for b in parts:
        offs.append(o)
        o += _align(b, 256)
    d = dict(zip(RECV_SECTIONS, offs))
    d['wide'] = o
    return d, o + wide_workspace_layout(E, n, rb, T)[1]


def own_receiver_counts(dest):
    """dest [E, n] host integers -> (own [E] int32: links of the state that are their own receiver, bad [E] bool: some receiver
    outside [0, n)): what the host knows about the receivers before they go up (the rule of ReceiverReplay.sample: the
    own-receiver counts decide whether a batch needs edge_base)"""
    d = np.asarray(dest)
    n = d.shape[-1]
    return (d == np.arange(n)).sum(axis=-1).astype(np.int32), ((d < 0) | (d >= n)).any(axis=-1)


WALKS = ('serial', 'wide')                               # how a trajectory call walks a state's T steps (v2x_*_steps / v2x_*_steps_wide)


def check_walk(who, walk):
    """ValueError unless walk names a form of the trajectory"""
    if walk not in WALKS:
        raise ValueError("%s: walk must be one of %s, got %r" % (who, ", ".join(repr(w) for w in WALKS), walk))
    return walk


STREAM_PHASES = ('chain', 'split')                       # the stream phase of a wide walk: k_traj_stream, or words / walk / uniforms


def check_stream_phase(who, stream_phase, walk='wide'):
    """ValueError unless stream_phase names a form of the wide walk's stream phase, and 'split' comes with walk='wide'"""
    if stream_phase not in STREAM_PHASES:
        raise ValueError("%s: stream_phase must be one of %s, got %r" % (who, ", ".join(repr(w) for w in STREAM_PHASES), stream_phase))
    if stream_phase == 'split' and walk != 'wide':
        raise ValueError("%s: stream_phase='split' needs walk='wide' (it is a form of the wide walk's stream phase), got walk=%r"
                         % (who, walk))
    return stream_phase


STREAM_WORDS = ('serial', 'jump')                         # the words launch of a receiver-form split stream phase: one chain, or chunks
JUMP_FIRST = MT_WORDS + 88 * 227                         # 20600 >= 20561: the prefix every chunk's seeds are made from, in whole rounds
JUMP_STRIDE = 227 * 256                                  # words per chunk (the measured strides)
JUMP_SLICES = 8                                          # the slices of a polynomial in the scratch of v2x_mt_jump_scratch_bytes


def check_stream_words(who, stream_words, stream_phase):
    """ValueError unless stream_words names a form of the words launch, and 'jump' comes with stream_phase='split'"""
    if stream_words not in STREAM_WORDS:
        raise ValueError("%s: stream_words must be one of %s, got %r" % (who, ", ".join(repr(w) for w in STREAM_WORDS), stream_words))
    if stream_words == 'jump' and stream_phase != 'split':
        raise ValueError("%s: stream_words='jump' needs stream_phase='split' (it draws the split stream phase's words in chunks), got "
                         "stream_phase=%r" % (who, stream_phase))
    return stream_words


def jump_plan(nbw):
    """-> (first, stride, count) of v2x_mt_jump for a word array of nbw words per state: the prefix [0, first) is drawn serially,
    chunk p = 1 .. count begins at first + (p - 1) stride and the last one ends at nbw; count = 0 (the serial words launch) when
    the prefix covers the array"""
    nbw = int(nbw)
    count = -(-(nbw - JUMP_FIRST) // JUMP_STRIDE) if nbw > JUMP_FIRST else 0
    return JUMP_FIRST, JUMP_STRIDE, count


def split_stream_blocks(n, rb, T, n_lanes):
    """NB of include/v2xgnn.h: the blocks of 624 words that bound what T steps of a state consume -- a step draws 2 n_u words
    and at most one double per pair of a vehicle and a lane of its two tables, the entry position is at most 624"""
    return 1 + -(-T * (2 * uniforms_per_step(n, rb) + 4 * n * n_lanes) // MT_WORDS)


def split_workspace_layout(E, n, rb, T, n_lanes):
    """-> (the byte offsets of words [E][NB][624] uint32 and off [T + 1][E] int64 in the workspace of the split stream phase, its
    size): the formula of include/v2xgnn.h (v2x_traj_split_workspace_bytes), both arrays rounded up to 256 bytes"""
    parts = (4 * E * split_stream_blocks(n, rb, T, n_lanes) * MT_WORDS, 8 * (T + 1) * E)
    offs, o = [], 0
    for b in parts:
        offs.append(o)
        o += _align(b, 256)
    return dict(zip(('words', 'off'), offs)), o


def eval_result_layout(E, n, rb, T, schemes):
    """-> (the byte offsets of v2v_rate, v2i_rate, interference, reward, actions, regular in the result block of v2x_eval_steps,
    its size): the layout of include/v2xgnn.h -- the doubles first, then the int32 actions, then the flags, back to back"""
    K, m = schemes * T * E, min(rb, n)
    parts = (('v2v_rate', 8 * K * n), ('v2i_rate', 8 * K * m), ('interference', 8 * K * rb), ('reward', 8 * K), ('actions', 4 * K * n),
             ('regular', (T + 1) * E))
    offs, o = {}, 0
    for k, b in parts:
        offs[k] = o
        o += b
    return offs, _align(o, 8)


class EvalResult(object):
    """What DeviceChannels.eval_steps brings back, scheme major (scheme 0 the policy, scheme 1 the baseline when one was given):
    actions [S, T, E, n] int32, v2v_rate [S, T, E, n], v2i_rate [S, T, E, min(rb, n)], interference [S, T, E, rb], reward
    [S, T, E] and regular [T + 1, E] (the flags of the observation at entry and after every step).  As with RolloutResult the
    bytes are on their way when this object is handed out; resolve() waits (once) and keeps plain copies."""

    FIELDS = ('v2v_rate', 'v2i_rate', 'interference', 'reward', 'actions', 'regular')

    def __init__(self, free, event, pin, E, n, rb, T, schemes):
        self._free, self._event, self._pin = free, event, pin
        self.E, self.n, self.rb, self.T, self.schemes = E, n, rb, T, schemes
        for k in self.FIELDS:
            setattr(self, k, None)

    def resolve(self):
        if self._pin is not None:
            self._event.synchronize()
            E, n, rb, T, S = self.E, self.n, self.rb, self.T, self.schemes
            offs, _ = eval_result_layout(E, n, rb, T, S)
            raw, K = self._pin.numpy(), S * T * E
            f64 = lambda k, w: raw[offs[k]:offs[k] + 8 * K * w].view(np.float64).copy()          # noqa: E731
            self.v2v_rate = f64('v2v_rate', n).reshape(S, T, E, n)
            self.v2i_rate = f64('v2i_rate', min(rb, n)).reshape(S, T, E, min(rb, n))
            self.interference = f64('interference', rb).reshape(S, T, E, rb)
            self.reward = f64('reward', 1).reshape(S, T, E)
            self.actions = raw[offs['actions']:offs['actions'] + 4 * K * n].view(np.int32).reshape(S, T, E, n).copy()
            self.regular = raw[offs['regular']:offs['regular'] + (T + 1) * E].reshape(T + 1, E).astype(bool)
            self._free.append(self._pin)
            self._pin = self._event = None
        return self

    @property
    def resident_regular(self):
        """the flags [E] of the observation the call left resident"""
        return self.resolve().regular[-1]


class RecvEvalResult(EvalResult):
    """EvalResult of eval_steps_recv: the same block, its last section read as flag bytes (.flags [T + 1, E] uint8: FLAG_OWN,
    FLAG_BAD, of the observation at entry and after every step); .regular is flags == 0"""

    def resolve(self):
        if self._pin is not None:
            self._event.synchronize()
            o = eval_result_layout(self.E, self.n, self.rb, self.T, self.schemes)[0]['regular']
            self.flags = self._pin.numpy()[o:o + (self.T + 1) * self.E].reshape(self.T + 1, self.E).copy()
            EvalResult.resolve(self)
            self.regular = self.flags == 0
        return self


class TrajectoryStates(object):
    """The T snapshots a trajectory call (rollout_steps / eval_steps) of block length T left in its workspace, as ONE stacked
    problem of T E states for OptimalAllocation (state t E + e: simulator e before its step t).  The channel arrays are views
    over the workspace, no copy; valid until the next trajectory call of that T on the same DeviceChannels."""

    n_Neighbor = 1

    def __init__(self, dc, T, io):
        t, E, n, rb = dc.torch, dc.E, dc.n, dc.rb
        K, ws, offs = T * E, io['workspace'], io['offsets']
        self._dc, self.T = dc, T
        self.E, self.n_Veh, self.n_RB = K, n, rb
        view = lambda k, count, shape: ws[offs[k]:offs[k] + 8 * count].view(t.float64).view(shape)   # noqa: E731
        self._tensors = [view('traj_v2v_ff', K * n * n * rb, (K, n, n, rb)), view('traj_v2i_ff', K * n * rb, (K, n, rb)),
                         view('traj_v2i_abs', K * n, (K, n)), dc.tensor('dest').repeat(T, 1)]

    def problem_tensors(self, device=None):
        """-> ([v2v_ff [T E, n, n, rb], v2i_ff, v2i_abs, dest [T E, n]] device tensors, constants)"""
        if device is not None and device != self._dc.device:
            raise ValueError("the simulator state lives on %s, the search runs on %s" % (self._dc.device, device))
        return list(self._tensors), dict(self._dc.constants)

    def rates(self, actions):
        """v2x_sim_rates of one joint action per snapshot: actions [T E, n] host integers -> (v2v_rate [T E, n], v2i_rate
        [T E, min(rb, n)], interference [T E, rb]) host arrays; one upload, one launch, one download"""
        dc, K, n, rb = self._dc, self.E, self.n_Veh, self.n_RB
        m = min(rb, n)
        a = np.asarray(actions)
        if a.dtype.kind not in 'iu':
            raise ValueError("actions must be integers, got dtype %s" % a.dtype)
        if a.shape == (K, n, 1):
            a = a.reshape(K, n)
        if a.shape != (K, n):
            raise ValueError("actions: an array of shape %s expected, got %s" % ([K, n], list(a.shape)))
        t = dc.torch
        dev = t.empty((K, n), dtype=t.int32, device=dc.device)
        dc._up(dev, np.ascontiguousarray(a, np.int32))
        out = t.empty(K * (n + m + rb), dtype=t.float64, device=dc.device)
        v = self._tensors
        prob = OptProblem(E=K, n=n, rb=rb, pad_=0, v2v_ff=v[0].data_ptr(), v2i_ff=v[1].data_ptr(), v2i_abs=v[2].data_ptr(),
                          dest=v[3].data_ptr(), w_v2v=0.0, w_v2i=0.0, **dc.constants)
        base = out.data_ptr()
        check(dc._lib, dc._lib.v2x_sim_rates(C.byref(prob), dev.data_ptr(), base, base + 8 * K * n, base + 8 * K * (n + m), None, None,
                                             dc._stream()))
        host = out.cpu().numpy()
        dc.traffic['bytes_down'] += host.nbytes
        return (host[:K * n].reshape(K, n).copy(), host[K * n:K * (n + m)].reshape(K, m).copy(),
                host[K * (n + m):].reshape(K, rb).copy())


class RolloutResult(object):
    """What a resident rollout call brings back: from DeviceChannels.rollout_step (T None) the rewards [E] and the regularity
    flags [2, E] of the stored observation and of the next one; from rollout_steps the same per iteration, [T, E] and
    [T, 2, E].  The bytes are on their way to a page-locked buffer when this object is handed out; resolve() waits for the
    event recorded behind that copy (once), keeps plain copies in .reward / .regular and gives the buffer back to `free`."""

    def __init__(self, free, event, pin, E, T=None):
        self._free, self._event, self._pin, self.E, self.T = free, event, pin, E, T
        self.reward = self.regular = None

    def resolve(self):
        if self._pin is not None:
            self._event.synchronize()
            lead = () if self.T is None else (self.T,)
            raw, K = self._pin.numpy(), (self.T or 1) * self.E
            self.reward = raw[:8 * K].view(np.float64).reshape(lead + (self.E,)).copy()
            self.regular = raw[8 * K:10 * K].reshape(lead + (2, self.E)).astype(bool)
            self._free.append(self._pin)
            self._pin = self._event = None
        return self

    @property
    def stored_regular(self):
        """the flags of the stored observations in slot order (t major, e minor), flat [T E]"""
        return self.resolve().regular.reshape(-1, 2, self.E)[:, 0, :].reshape(-1)

    @property
    def resident_regular(self):
        """the flags [E] of the observation the call left resident"""
        return self.resolve().regular.reshape(-1, 2, self.E)[-1, 1]


class RecvRolloutResult(RolloutResult):
    """RolloutResult of rollout_steps_recv: the same bytes, read as flag bytes (.flags [T, 2, E] uint8: FLAG_OWN, FLAG_BAD);
    .regular is flags == 0"""

    def resolve(self):
        if self._pin is not None:
            K = self.T * self.E
            self._event.synchronize()
            self.flags = self._pin.numpy()[8 * K:10 * K].reshape(self.T, 2, self.E).copy()
            RolloutResult.resolve(self)
            self.regular = self.flags == 0
        return self


def _block_length(explore):
    """T of the explore flags [T, E] of a block (0: not a block, refused by the check)"""
    shape = np.shape(explore)
    return shape[0] if len(shape) == 2 else 0


class DeviceChannels(object):
    """The device arrays of E simulator states and the v2x_sim_* calls on them.  Argument checks (ValueError) come before any
    device work; the device is touched at the first call that needs it."""

    n_Neighbor = 1                                       # (what OptimalAllocation asks of a simulator)

    def __init__(self, E, n, rb, device=0, constants=None):
        E, n, rb = int(E), int(n), int(rb)
        if not 1 <= E <= MAX_STATES or not 1 <= n <= MAX_LINKS or not 1 <= rb <= MAX_RB:
            raise ValueError("DeviceChannels supports 1..%d states, 1..%d links and 1..%d resource blocks, got E = %d, n = %d, "
                             "rb = %d" % (MAX_STATES, MAX_LINKS, MAX_RB, E, n, rb))
        self.E, self.n, self.rb = E, n, rb
        self.n_Veh, self.n_RB = n, rb
        self.n_u = uniforms_per_step(n, rb)
        self.device_index = int(device)
        self.constants = dict(DEFAULT_CONSTANTS)
        if constants:
            unknown = set(constants) - set(DEFAULT_CONSTANTS)
            if unknown:
                raise ValueError("unknown constants %s" % sorted(unknown))
            self.constants.update({k: float(v) for k, v in constants.items()})
        self.torch = None
        self._t = {}                                     # name -> device tensor
        self._obs_ready = False
        self._own = None                                 # own_receiver_counts of the receivers the device holds, when the host sent them
        self._h2d_done = None
        self._grid = None                                # set_grid(): (lanes [4, n_lanes] float64, width, height, timestep)
        self._grid_sent = False
        self.traffic = {'bytes_up': 0, 'bytes_down': 0}  # every host <-> device copy this object issues
        self._roll = {}                                  # _rollout_io(): None (rollout_step) or T (rollout_steps) -> its buffers
        self._traj_form = {}                             # T -> 'recv' when the last trajectory call of that T ran in receiver form
        self._mixed = {}                                 # mixed_rollout_buffers(): ((E_k, n_k)..., T) of the pools this one leads
        self.walk_calls = {w: 0 for w in WALKS}          # trajectory calls made (rollout_steps / eval_steps), by the walk that ran
        self.stream_phase_calls = {p: 0 for p in STREAM_PHASES}     # the wide ones among them, by the form of the stream phase
        self.stream_words_calls = {w: 0 for w in STREAM_WORDS}      # the receiver-form split ones among those, by the words launch
        self._jump_tables = {}                                      # (first, stride, count) -> the uploaded polynomials

    # the packed observation (xe / mask / col / regular) is current; any assignment -- a step, another observation, a reset --
    # also says that the receiver form (observe_recv: xe / recv / flags) no longer is: observe_recv sets its own flag after it
    def _get_obs_ready(self):
        return self.__dict__.get('_packed_ready', False)

    def _set_obs_ready(self, value):
        self.__dict__['_packed_ready'] = bool(value)
        self._recv_ready = False

    _obs_ready = property(_get_obs_ready, _set_obs_ready)

    # ------------------------------------------------------------------ shapes and checks
    def shapes(self):
        E, n, rb, m = self.E, self.n, self.rb, min(self.rb, self.n)
        return {'u': (E, self.n_u), 'vel': (E, n), 'pos': (E, n, 2), 'v2i_shadow': (E, n), 'v2v_shadow': (E, n, n),
                'v2v_abs': (E, n, n), 'v2i_abs': (E, n), 'v2v_ff': (E, n, n, rb), 'v2i_ff': (E, n, rb), 'dest': (E, n),
                'actions': (E, n), 'interf_db': (E, n, rb), 'state': (E, n, 3 * rb + 1), 'xe': (E, n, XE_WIDTH), 'mask': (E, n),
                'col': (E, n * max(n - 2, 0)), 'regular': (E,), 'v2v_rate': (E, n), 'v2i_rate': (E, m), 'interference': (E, rb),
                'v2i_interf': (E, rb), 'v2v_interf': (E, n), 'keys': (E, MT_WORDS), 'mtpos': (E,), 'dirs': (E, n), 'status': (E,),
                'recv': (E, n), 'flags': (E,)}

    @staticmethod
    def check_observe(n, C, rb=None):
        """The limits of v2x_sim_observe (those of v2xsim_observe_packed)."""
        if not OBSERVE_MIN_LINKS <= n <= OBSERVE_MAX_LINKS:
            raise ValueError("the device observation supports %d..%d links, got %d" % (OBSERVE_MIN_LINKS, OBSERVE_MAX_LINKS, n))
        if rb is not None and C != rb:
            raise ValueError("the device observation is built for n_channels == n_RB (%d), got %d" % (rb, C))
        if C > n:
            raise ValueError("the device observation needs n_RB <= links (block r's V2I transmitter is vehicle r), got %d > %d"
                             % (C, n))
        if 3 * C + 1 > XE_WIDTH:
            raise ValueError("an observation row of 3 * %d + 1 values exceeds the packed width of %d" % (C, XE_WIDTH))

    def _check_input(self, name, a, dtype_kind='f'):
        """a host array or device tensor for slot `name` -> ('host', contiguous numpy array) or ('dev', tensor)"""
        shape = self.shapes()[name]
        if hasattr(a, 'data_ptr'):
            if tuple(a.shape) != shape:
                raise ValueError("%s: a tensor of shape %s expected, got %s" % (name, list(shape), list(a.shape)))
            want = {'f': 'torch.float64', 'i': 'torch.int64', 'a': 'torch.int32', 'k': 'torch.int32', 'b': 'torch.int8'}[dtype_kind]
            if str(a.dtype) != want or not a.is_contiguous():
                raise ValueError("%s: a contiguous %s tensor expected, got %s" % (name, want, a.dtype))
            return 'dev', a
        a = np.asarray(a)
        if dtype_kind in 'iakb' and a.dtype.kind not in 'iu':
            raise ValueError("%s must be integers, got dtype %s" % (name, a.dtype))
        if dtype_kind == 'k' and name == 'keys' and a.dtype.itemsize != 4:
            raise ValueError("keys must be 32-bit words (uint32, the layout of RandomState.get_state()), got dtype %s" % a.dtype)
        if dtype_kind == 'f' and a.dtype.kind not in 'fiu':
            raise ValueError("%s must be real numbers, got dtype %s" % (name, a.dtype))
        if name == 'actions' and a.shape == shape + (1,):
            a = a.reshape(shape)
        if a.shape != shape and not (name in ('v2v_ff', 'interf_db') and a.size == int(np.prod(shape))):
            raise ValueError("%s: an array of shape %s expected, got %s" % (name, list(shape), list(a.shape)))
        if dtype_kind == 'k' and name == 'keys':
            return 'host', np.ascontiguousarray(a.reshape(shape)).view(np.int32)       # (the bits: torch has no uint32 copies)
        return 'host', np.ascontiguousarray(a.reshape(shape), {'f': np.float64, 'i': np.int64, 'a': np.int32, 'k': np.int32,
                                                               'b': np.int8}[dtype_kind])

    # ------------------------------------------------------------------ device side
    def _init_device(self):
        if self.torch is not None:
            return
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceChannels needs a GPU (there is no CPU fallback; the host path is rl/native_sim.py)")
        self._lib = load_library()
        self.device = torch.device('cuda', self.device_index)
        self._pin = True
        self.torch = torch
        self._allocate()

    def _allocate(self):
        t, sh = self.torch, self.shapes()
        f64 = t.float64
        # the inputs of a step: ONE staging buffer (page-locked) and one device buffer, u | vel | pos
        sizes = [int(np.prod(sh[k])) for k in ('u', 'vel', 'pos')]
        self._in_host = t.empty(sum(sizes), dtype=f64, pin_memory=self._pin)
        self._in_dev = t.empty(sum(sizes), dtype=f64, device=self.device)
        o = 0
        self._in_np = {}
        for k, s in zip(('u', 'vel', 'pos'), sizes):
            self._t[k] = self._in_dev[o:o + s].view(sh[k])
            self._in_np[k] = self._in_host[o:o + s].view(sh[k]).numpy()
            o += s
        for k in _CHANNEL_TENSORS + ('interf_db', 'state'):
            self._t[k] = t.zeros(sh[k], dtype=f64, device=self.device)
        self._t['dest'] = t.zeros(sh['dest'], dtype=t.int64, device=self.device)
        self._t['actions'] = t.zeros(sh['actions'], dtype=t.int32, device=self.device)
        # the stream state of v2x_sim_stream: key words as int32 bits, positions (624: "block used up", nothing to read yet)
        self._t['keys'] = t.zeros(sh['keys'], dtype=t.int32, device=self.device)
        self._t['mtpos'] = t.full(sh['mtpos'], MT_WORDS, dtype=t.int32, device=self.device)
        self._t['dirs'] = t.zeros(sh['dirs'], dtype=t.int8, device=self.device)
        self._t['status'] = t.zeros(sh['status'], dtype=t.uint8, device=self.device)
        self._reset_io = None                            # fetch_reset(): the packed copy of vel | dest | regular | status
        if self._grid is not None:
            self._send_grid()
        # the small results, each group one device buffer and one page-locked copy (one download per group)
        self._obs_dev, self._obs_host, self._obs_np = self._group((('xe', t.float32), ('mask', t.int32), ('col', t.int32),
                                                                   ('regular', t.uint8)))
        self._rates_dev, self._rates_host, self._rates_np = self._group(tuple(
            (k, f64) for k in ('v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf')))
        # the receiver form's own small outputs (observe_recv; xe is shared with the packed form)
        self._recv_dev, self._recv_host, self._recv_np = self._group((('recv', t.int32), ('flags', t.uint8)))

    def _group(self, fields):
        t, sh = self.torch, self.shapes()
        offs, o = [], 0
        for k, dt in fields:
            nbytes = int(np.prod(sh[k])) * t.empty(0, dtype=dt).element_size()
            offs.append((k, dt, o, nbytes))
            o = _align(o + nbytes)
        dev = t.zeros(max(o, 64), dtype=t.uint8, device=self.device)
        host = t.zeros(max(o, 64), dtype=t.uint8, pin_memory=self._pin)
        views = {}
        for k, dt, o, nbytes in offs:
            self._t[k] = dev[o:o + nbytes].view(dt).view(sh[k])
            views[k] = host[o:o + nbytes].view(dt).view(sh[k]).numpy()
        return dev, host, views

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _sync(self):
        self.torch.cuda.current_stream(self.device).synchronize()

    def _staging_free(self):
        """the last upload out of the staging buffer has left it"""
        if self._h2d_done is not None:
            self._h2d_done.synchronize()

    def _staging_sent(self):
        if self._pin:
            if self._h2d_done is None:
                self._h2d_done = self.torch.cuda.Event()
            self._h2d_done.record(self.torch.cuda.current_stream(self.device))

    def tensor(self, name):
        """the device tensor behind `name` (see shapes()); valid for the life of this object"""
        self._init_device()
        return self._t[name]

    _KINDS = {'dest': 'i', 'actions': 'a', 'keys': 'k', 'mtpos': 'k', 'dirs': 'b'}

    def _up(self, tensor, host_array):
        """one host -> device copy, counted"""
        src = self.torch.from_numpy(host_array)
        tensor.copy_(src)
        self.traffic['bytes_up'] += src.numel() * src.element_size()

    def upload(self, name, array):
        """host array -> the device tensor `name` (shadowing states, channel arrays, dest, keys, mtpos, dirs, ...)"""
        where, a = self._check_input(name, array, self._KINDS.get(name, 'f'))
        self._init_device()
        if name == 'dest':
            self._own = own_receiver_counts(a) if where == 'host' else None
        if where == 'dev':
            self._t[name].copy_(a)
        else:
            self._up(self._t[name], a)
        return self._t[name]

    def download(self, *names):
        """host copies (numpy) of the named device tensors, in order; no names: the six channel arrays.  keys come back as
        uint32 (the layout of RandomState.get_state())."""
        self._init_device()
        names = names or _CHANNEL_TENSORS
        out = []
        for k in names:
            a = self._t[k].cpu().numpy()
            self.traffic['bytes_down'] += a.nbytes
            out.append(a.view(np.uint32) if k == 'keys' else a)
        return out[0] if len(out) == 1 else tuple(out)

    # ------------------------------------------------------------------ the three calls
    def step(self, u, vel=None, pos=None):
        """One channel update of every state (v2x_sim_channels) from the step's uniforms u [E, n_u]; vel [E, n] and pos
        [E, n, 2] (None: what the device holds).  Host arrays travel through the page-locked staging buffer in one copy;
        device tensors (float64, contiguous) are read where they are.  Shadowing is updated in place."""
        given = {'u': u, 'vel': vel, 'pos': pos}
        checked = {k: self._check_input(k, v) for k, v in given.items() if v is not None}
        self._init_device()
        host = [k for k in ('u', 'vel', 'pos') if k in checked and checked[k][0] == 'host']
        if host:
            self._staging_free()
            for k in host:
                self._in_np[k][...] = checked[k][1]
            self.traffic['bytes_up'] += 8 * sum(self._t[k].numel() for k in host)
            if len(host) == 3:
                self._in_dev.copy_(self._in_host, non_blocking=True)
            else:
                o = 0
                for k in ('u', 'vel', 'pos'):
                    s = self._t[k].numel()
                    if k in host:
                        self._in_dev[o:o + s].copy_(self._in_host[o:o + s], non_blocking=True)
                    o += s
            self._staging_sent()
        src = {k: (checked[k][1] if k in checked and checked[k][0] == 'dev' else self._t[k]) for k in ('u', 'vel', 'pos')}
        self._keep = src                                 # the launch is asynchronous: its inputs stay alive
        T = self._t
        check(self._lib, self._lib.v2x_sim_channels(
            self.E, self.n, self.rb, src['u'].data_ptr(), self.n_u, src['vel'].data_ptr(), src['pos'].data_ptr(),
            T['v2i_shadow'].data_ptr(), T['v2v_shadow'].data_ptr(), T['v2v_abs'].data_ptr(), T['v2i_abs'].data_ptr(),
            T['v2v_ff'].data_ptr(), T['v2i_ff'].data_ptr(), self._stream()))
        self._obs_ready = False

    def observe(self, dest=None, power=None):
        """Observable interference + packed observation of the current channels (v2x_sim_observe) for n_channels = rb.
        dest [E, n]: the receivers (host integers or an int64 device tensor; None: what the device holds); power: the V2V
        power entry of the observation (default: the constants' p_v2v).  Results stay on the device (tensor('interf_db'),
        'state', 'xe', 'mask', 'col', 'regular'); fetch_observation() brings the packed part to the host."""
        self.check_observe(self.n, self.rb)
        where = None
        if dest is not None:
            where, d = self._check_input('dest', dest, 'i')
        self._init_device()
        if where == 'dev':
            self._t['dest'].copy_(d)
            self._own = None
        elif where is not None:
            self._up(self._t['dest'], d)
            self._own = own_receiver_counts(d)
        T, c = self._t, self.constants
        check(self._lib, self._lib.v2x_sim_observe(
            self.E, self.n, self.rb, T['dest'].data_ptr(), T['v2v_ff'].data_ptr(), T['v2i_ff'].data_ptr(), c['p_v2i'],
            c['veh_gain'], c['veh_nf'], c['sig2'], float(c['p_v2v'] if power is None else power), T['interf_db'].data_ptr(),
            T['state'].data_ptr(), T['xe'].data_ptr(), T['mask'].data_ptr(), T['col'].data_ptr(), T['regular'].data_ptr(),
            self._stream()))
        self._obs_ready = True

    def fetch_observation(self):
        """-> (xe [E, n, 16] float32, mask [E, n] int32, col [E, n (n-2)] int32, regular [E] bool) of the last observe():
        one download, fresh host arrays."""
        self._init_device()
        if not self._obs_ready:
            raise RuntimeError("fetch_observation: no observe() since the last step()")
        self._obs_host.copy_(self._obs_dev, non_blocking=True)
        self.traffic['bytes_down'] += self._obs_host.numel()
        self._sync()
        v = self._obs_np
        return v['xe'].copy(), v['mask'].copy(), v['col'].copy(), v['regular'].astype(bool)

    def rates(self, actions, dest=None):
        """The rates of one joint action per state (v2x_sim_rates): actions [E, n] (or [E, n, 1]) channel numbers, host
        integers or an int32 device tensor.  A channel outside [0, rb) gives that state NaN rates.  Results stay on the
        device (tensor('v2v_rate'), ...); fetch_rates() brings them to the host."""
        where, a = self._check_input('actions', actions, 'a')
        dwhere = None
        if dest is not None:
            dwhere, d = self._check_input('dest', dest, 'i')
        self._init_device()
        if dwhere == 'dev':
            self._t['dest'].copy_(d)
            self._own = None
        elif dwhere is not None:
            self._up(self._t['dest'], d)
            self._own = own_receiver_counts(d)
        if where == 'host':
            self._up(self._t['actions'], a)
            a = self._t['actions']
        self._keep_actions = a
        T = self._t
        prob = self.problem()
        check(self._lib, self._lib.v2x_sim_rates(
            C.byref(prob), a.data_ptr(), T['v2v_rate'].data_ptr(), T['v2i_rate'].data_ptr(), T['interference'].data_ptr(),
            T['v2i_interf'].data_ptr(), T['v2v_interf'].data_ptr(), self._stream()))

    def fetch_rates(self):
        """-> dict of host arrays of the last rates(): v2v_rate [E, n], v2i_rate [E, min(rb, n)], interference [E, rb] (without
        noise), v2i_interf [E, rb] and v2v_interf [E, n] (with noise); one download."""
        self._init_device()
        self._rates_host.copy_(self._rates_dev, non_blocking=True)
        self.traffic['bytes_down'] += self._rates_host.numel()
        self._sync()
        return {k: v.copy() for k, v in self._rates_np.items()}

    # ------------------------------------------------------------------ mobility, streams and the one-call step
    def set_grid(self, lanes, width, height, timestep):
        """The lane grid of the mobility rule: lanes = the (up, down, left, right) tables, [4, n_lanes] coordinates (the order
        of native_sim.positions); the map is [0, width] x [0, height]; timestep: seconds per step.  Goes up once: now, or when
        the device is first touched."""
        try:
            tab = np.ascontiguousarray(np.asarray(lanes, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError("set_grid: lanes must be four tables of equal length (up, down, left, right)")
        if tab.ndim != 2 or tab.shape[0] != 4 or not 1 <= tab.shape[1] <= MAX_LANES:
            raise ValueError("set_grid: lanes of shape [4, 1..%d] expected (up, down, left, right), got %s"
                             % (MAX_LANES, list(tab.shape)))
        vals = (float(width), float(height), float(timestep))
        if not np.all(np.isfinite(tab)) or not all(np.isfinite(v) for v in vals):
            raise ValueError("set_grid: lanes, width, height and timestep must be finite")
        self._grid = (tab,) + vals
        self._grid_sent = False
        if self.torch is not None:                       # (not inside the next call, which may be under stream capture)
            self._send_grid()

    def _send_grid(self):
        if not self._grid_sent:
            tab = self._grid[0]
            if 'lanes' not in self._t or tuple(self._t['lanes'].shape) != tab.shape:
                self._t['lanes'] = self.torch.zeros(tab.shape, dtype=self.torch.float64, device=self.device)
            self._up(self._t['lanes'], tab)
            self._grid_sent = True

    def _check_mobility(self, who, mobility):
        if not isinstance(mobility, (bool, np.bool_)):
            raise ValueError("%s: mobility must be True or False, got %r" % (who, mobility))
        if mobility and self._grid is None:
            raise ValueError("%s: mobility needs the lane grid (set_grid) first" % who)

    def stream(self, mobility=True):
        """v2x_sim_stream on the resident state: one renew_positions step of every vehicle (mobility=True; needs set_grid and
        the resident keys / mtpos / pos / dirs / vel), then the next n_u uniforms of every stream into tensor('u') -- what
        step(dc.tensor('u')) consumes.  Bit for bit native_sim.positions followed by native_sim.mt_uniforms."""
        self._check_mobility("stream", mobility)
        self._init_device()
        T = self._t
        tab, width, height, timestep = self._grid if mobility else (None, 0.0, 0.0, 0.0)
        if mobility:
            self._send_grid()
        check(self._lib, self._lib.v2x_sim_stream(
            self.E, self.n, T['keys'].data_ptr(), T['mtpos'].data_ptr(), T['pos'].data_ptr() if mobility else None,
            T['dirs'].data_ptr(), T['vel'].data_ptr(), timestep, tab.shape[1] if mobility else 0,
            T['lanes'].data_ptr() if mobility else None, width, height, T['u'].data_ptr(), self.n_u, self._stream()))

    def advance(self, actions=None, power=None):
        """One whole simulator step in one call (v2x_sim_advance): the rates of `actions` on the current channels (None: no
        rates), mobility and the step's uniforms, the channel update, the observation -- all on the resident state, so the
        actions ([E, n] or [E, n, 1] host integers, or an int32 device tensor) are the only thing that goes up.  Results as
        after rates() / step() / observe(): fetch_rates(), fetch_observation()."""
        where = None
        if actions is not None:
            where, a = self._check_input('actions', actions, 'a')
        self.check_observe(self.n, self.rb)
        self._check_mobility("advance", True)
        self._init_device()
        self._send_grid()
        T = self._t
        if where == 'host':
            self._up(T['actions'], a)
            a = T['actions']
        self._keep_actions = a if actions is not None else None
        s = self._sim_step(a.data_ptr() if actions is not None else None, power)
        check(self._lib, self._lib.v2x_sim_advance(C.byref(s), self._stream()))
        self._obs_ready = True

    def _sim_step(self, actions_ptr, power=None):
        T, c = self._t, self.constants
        tab, width, height, timestep = self._grid
        return SimStep(problem=self.problem(), n_lanes=tab.shape[1], n_u=self.n_u, timestep=timestep, width=width, height=height,
                       power=float(c['p_v2v'] if power is None else power), xy=T['pos'].data_ptr(), actions=actions_ptr,
                       **{k: T[k].data_ptr() for k in ('keys', 'mtpos', 'dirs', 'vel', 'lanes', 'u') + _CHANNEL_TENSORS + (
                           'interf_db', 'state', 'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate', 'interference',
                           'v2i_interf', 'v2v_interf')})

    # ------------------------------------------------------------------ the episode reset on the resident state
    def check_reset(self, who="reset"):
        """ValueError unless an episode reset can run on this object: the limits of v2x_sim_reset and the lane grid"""
        if self.n % 4 or not 4 <= self.n <= RESET_MAX_LINKS:
            raise ValueError("%s: a reset places groups of four vehicles: a multiple of 4 in 4..%d links supported, got %d"
                             % (who, RESET_MAX_LINKS, self.n))
        self.check_observe(self.n, self.rb)
        self._check_mobility(who, True)
        check_reset_grid(who, self._grid[0], self._grid[1], self._grid[2])

    def _sim_reset(self, power=None):
        T = self._t
        return SimReset(step=self._sim_step(None, power), vel=T['vel'].data_ptr(), dest=T['dest'].data_ptr(),
                        status=T['status'].data_ptr())

    def _reset_call(self, who, power):
        """v2x_sim_<who> on the resident state, after the checks"""
        self.check_reset(who)
        self._init_device()
        self._send_grid()
        r = self._sim_reset(power)
        check(self._lib, getattr(self._lib, "v2x_sim_" + who)(C.byref(r), self._stream()))

    def reset_draw(self):
        """The draws of an episode reset on the resident streams (v2x_sim_reset_draw, one launch): new vehicles into pos / dirs /
        vel, the initial shadowing, the channel update's uniforms into tensor('u'), the receivers into tensor('dest'), the flags
        into tensor('status') (bit 0: a receiver tied in distance, reset_tie_flags; bit 1: a draw found no value).  Bit for bit
        native_sim.reset_vehicles, two native_sim.mt_uniforms calls and native_sim.sample_dest on the ranked neighbours, except
        the receivers of flagged states."""
        self._reset_call("reset_draw", None)
        self._obs_ready = False

    def reset(self, power=None):
        """new_random_game of every resident state in one call (v2x_sim_reset: reset_draw, the channel update on the new
        vehicles, the observation of the new receivers -- three launches).  fetch_reset() brings the small results down."""
        self._reset_call("reset", power)
        self._obs_ready = True

    def fetch_reset(self):
        """-> (vel [E, n] float64, dest [E, n] int64, regular [E] bool, status [E] uint8) as the last reset() left them: packed on
        the device, one download, fresh host arrays"""
        self._init_device()
        t, E, n = self.torch, self.E, self.n
        if self._reset_io is None:
            nbytes = _align(16 * E * n + 2 * E)
            self._reset_io = (t.zeros(nbytes, dtype=t.uint8, device=self.device), t.zeros(nbytes, dtype=t.uint8, pin_memory=self._pin))
        dev, host = self._reset_io
        o = 0
        for k, width in (('vel', 8), ('dest', 8), ('regular', 1), ('status', 1)):
            src = self._t[k]
            dev[o:o + width * src.numel()].view(src.dtype).view(src.shape).copy_(src)
            o += width * src.numel()
        host.copy_(dev, non_blocking=True)
        self.traffic['bytes_down'] += host.numel()
        self._sync()
        raw = host.numpy()
        vel = raw[:8 * E * n].view(np.float64).reshape(E, n).copy()
        dest = raw[8 * E * n:16 * E * n].view(np.int64).reshape(E, n).copy()
        return vel, dest, raw[16 * E * n:16 * E * n + E].astype(bool), raw[16 * E * n + E:16 * E * n + 2 * E].copy()

    # ------------------------------------------------------------------ DQN rollouts on the resident state
    # One host path with two entry points: rollout_step() makes one iteration (v2x_rollout_step), rollout_steps() T of them
    # (v2x_rollout_steps).  Everything around the library call is shared and takes T = None for the one iteration (no leading
    # axis, the resident observation is the batch) or the T of a block (a leading axis of T, the trajectory workspace).
    def rollout_steps_policy_bytes(self, T):
        """bytes of the one buffer rollout_steps() uploads: random_actions [T, E, n] int32, then explore [T, E] bytes"""
        return _align(4 * T * self.E * self.n + T * self.E, 4)

    def rollout_steps_result_bytes(self, T):
        """bytes of the result block rollout_steps() downloads: reward [T, E] float64, then regular [T, 2, E] bytes"""
        return _align(10 * T * self.E, 8)

    @property
    def rollout_policy_bytes(self):
        """bytes of the one buffer rollout_step() uploads: random_actions [E, n] int32, then explore [E] bytes"""
        return self.rollout_steps_policy_bytes(1)

    @property
    def rollout_result_bytes(self):
        """bytes of the result row rollout_step() downloads: reward [E] float64, then regular [2, E] bytes"""
        return self.rollout_steps_result_bytes(1)

    def _check_rollout(self, who, T, explore, random_actions, storage, head, capacity):
        """ValueError unless the arguments of rollout_step() (T None) / rollout_steps() fit this object; -> (explore uint8,
        random_actions int32) of shapes [E] and [E, n], under a leading axis of T for a block"""
        E, n = self.E, self.n
        lead, K = (() if T is None else (T,)), (E if T is None else T * E)
        self.check_observe(n, self.rb)
        self._check_mobility(who, True)
        ex = np.asarray(explore)
        if K < 1 or ex.shape != lead + (E,) or ex.dtype.kind not in 'biu':
            raise ValueError("explore: %s flags expected, got shape %s of dtype %s"
                             % (E if T is None else "[T, %d] with T >= 1" % E, list(ex.shape), ex.dtype))
        ra = np.asarray(random_actions)
        if ra.dtype.kind not in 'iu':
            raise ValueError("random_actions must be integers, got dtype %s" % ra.dtype)
        if ra.shape == lead + (E, n, 1):
            ra = ra.reshape(lead + (E, n))
        if ra.shape != lead + (E, n):
            raise ValueError("random_actions: an array of shape %s expected, got %s" % (list(lead + (E, n)), list(ra.shape)))
        head, capacity = int(head), int(capacity)
        if not K <= capacity or not 0 <= head < capacity:
            raise ValueError("%s: %sE <= capacity and 0 <= head < capacity needed, got %sE = %d, head = %d, capacity = %d"
                             % (who, "" if T is None else "T ", "" if T is None else "T = %d, " % T, E, head, capacity))
        want = {'xe': (n, XE_WIDTH), 'xe_next': (n, XE_WIDTH), 'col': (n * (n - 2),), 'mask': (n,), 'action': (n,), 'reward': ()}
        for k, tail in want.items():
            t = storage.get(k)
            if t is None or tuple(t.shape[1:]) != tail or not t.is_contiguous():
                raise ValueError("%s: replay storage %r of shape [slots] + %s expected" % (who, k, list(tail)))
            if t.shape[0] < (capacity if head + K > capacity else head + K):      # (a block that wraps touches the last slot)
                raise ValueError("%s: replay storage %r has %d slots, the block at %d needs more" % (who, k, t.shape[0], head))
        return ex.astype(np.uint8), np.ascontiguousarray(ra, np.int32)

    def check_rollout(self, explore, random_actions, storage, head, capacity):
        """ValueError unless the arguments of rollout_step() fit this object; -> (explore [E] uint8, random_actions [E, n] int32)"""
        return self._check_rollout("rollout_step", None, explore, random_actions, storage, head, capacity)

    def check_rollout_steps(self, explore, random_actions, storage, head, capacity):
        """ValueError unless the arguments of rollout_steps() fit this object; -> (T, explore [T, E] uint8, random_actions
        [T, E, n] int32)"""
        T = _block_length(explore)
        return (T,) + self._check_rollout("rollout_steps", T, explore, random_actions, storage, head, capacity)

    def _rollout_io(self, T):
        """the buffers of rollout_step() (T None) or of rollout_steps() for blocks of T iterations, made once per T: policy_dev
        (random_actions int32 | explore bytes) behind a ring of four page-locked copies with their events, result_dev (reward
        float64 | regular bytes) with the free list of its page-locked copies, q [graphs n, rb] float32, the observations a
        model scores (xe, col of `graphs` graphs) with the cached DeviceBatch, and for a block the trajectory workspace"""
        self._init_device()
        io = self._roll.get(T)
        if io is None:
            t, E, n, rb = self.torch, self.E, self.n, self.rb
            K = (T or 1) * E
            nb = self.rollout_steps_policy_bytes(T or 1)
            io = self._roll[T] = {
                'policy_dev': t.zeros(nb, dtype=t.uint8, device=self.device),
                'policy_pin': [t.zeros(nb, dtype=t.uint8, pin_memory=self._pin) for _ in range(4)], 'policy_ev': [None] * 4, 'next': 0,
                'result_dev': t.zeros(self.rollout_steps_result_bytes(T or 1), dtype=t.uint8, device=self.device), 'free': [],
                'q': t.zeros((K * n, rb), dtype=t.float32, device=self.device), 'graphs': K, 'batch': {}}
            if T is None:
                io['xe'], io['col'] = self._t['xe'].view(E * n, XE_WIDTH), self._t['col'].view(-1)
            else:
                offs, size = trajectory_workspace_layout(E, n, rb, T)
                ws = io['workspace'] = self._sized_workspace("trajectory workspace", T, self._lib.v2x_rollout_steps_workspace_bytes(E, n, rb, T),
                                                             size, who="rollout_steps")
                io['offsets'] = offs
                # entries 0..T-1 of the trajectory, where k_sim_trajectory writes them
                io['xe'] = ws[offs['traj_xe']:offs['traj_xe'] + 4 * K * n * XE_WIDTH].view(t.float32).view(K * n, XE_WIDTH)
                io['col'] = ws[offs['traj_col']:offs['traj_col'] + 4 * K * n * (n - 2)].view(t.int32)
        return io

    def _sized_workspace(self, name, T, need, size, who=None, n_lanes=None, aligned=False, least=0):
        """a zeroed device workspace `name` for blocks of T, of the `size` bytes its documented layout gives (`least` at least):
        ValueError unless the library's size `need` is the same; aligned: RuntimeError unless the allocator returned it 256-byte
        aligned.  who: the call both refusals name"""
        if need != size:
            dims = "E = %d, n = %d, rb = %d, T = %d" % (self.E, self.n, self.rb, T) + ("" if n_lanes is None else ", n_lanes = %d" % n_lanes)
            raise ValueError("%sthe library sizes the %s of %s at %d bytes, the documented layout at %d"
                             % (who + ": " if who else "", name, dims, need, size))
        ws = self.torch.zeros(max(size, least), dtype=self.torch.uint8, device=self.device)
        if aligned and ws.data_ptr() % 256:
            raise RuntimeError("%s: the allocator returned a %s that is not 256-byte aligned" % (who, name))
        return ws

    def _wide_workspace(self, T):
        """the workspace of the wide walk for blocks of T, made at the first wide call of that T and kept in _rollout_io(T) next
        to the trajectory workspace; the device never sends it anywhere: no traffic"""
        io = self._rollout_io(T)
        ws = io.get('wide_workspace')
        if ws is None:
            E, n, rb = self.E, self.n, self.rb
            ws = io['wide_workspace'] = self._sized_workspace("wide-walk workspace", T, self._lib.v2x_traj_wide_workspace_bytes(E, n, rb, T),
                                                              wide_workspace_layout(E, n, rb, T)[1], least=256)
        return ws

    def _split_workspace(self, T):
        """the second workspace of a wide walk whose stream phase is split, for blocks of T on the current lane grid: made at the
        first split call of that T (again when set_grid() changes the number of lanes) and kept in _rollout_io(T) under its own
        key; like the wide workspace it never crosses the bus"""
        io = self._rollout_io(T)
        E, n, rb, n_lanes = self.E, self.n, self.rb, self._grid[0].shape[1]
        ws = io.get('split_workspace')
        if ws is None or io.get('split_lanes') != n_lanes:
            ws = io['split_workspace'] = self._sized_workspace(
                "split-stream workspace", T, self._lib.v2x_traj_split_workspace_bytes(E, n, rb, T, n_lanes),
                split_workspace_layout(E, n, rb, T, n_lanes)[1], n_lanes=n_lanes)
            io['split_lanes'] = n_lanes
        return ws

    def rollout_buffers(self):
        """the device buffers of rollout_step(): policy_dev (random_actions [E, n] int32 | explore [E] bytes), result_dev (reward [E]
        float64 | regular [2, E] bytes), q [E n, rb] float32"""
        return self._rollout_io(None)

    def rollout_steps_buffers(self, T):
        """the device buffers of rollout_steps() for blocks of T iterations: workspace (the trajectory, carved by
        trajectory_workspace_layout), policy_dev (random_actions [T, E, n] int32 | explore [T, E] bytes), result_dev (reward
        [T, E] float64 | regular [T, 2, E] bytes), q [T E n, rb] float32"""
        return self._rollout_io(T)

    def _rollout_batch(self, io, graphs, xe, col, row_ptr):
        """`graphs` observations of n rows as the engine's batch, xe and the CSR sources where the kernels write them (every
        state regular: n - 2 sources per row, row_ptr the constant pointer of graphs n rows); kept in io for the next call"""
        from ..engine import DeviceBatch
        db = io['batch'].get(row_ptr.data_ptr())
        if db is None:
            db = DeviceBatch.from_tensors(graphs, self.n, xe, row_ptr, col, self.n * (self.n - 2))
            io['batch'] = {row_ptr.data_ptr(): db}
            io['row_ptr'] = row_ptr
        return db

    def rollout_batch(self, row_ptr):
        """the resident observation as the engine's batch: E graphs of n rows, where v2x_sim_observe writes them"""
        io = self._rollout_io(None)
        return self._rollout_batch(io, io['graphs'], io['xe'], io['col'], row_ptr)

    def _rollout_struct(self, T, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr, power):
        """what the library takes: the v2x_rollout of the resident tensors and the buffers of _rollout_io(T) -- the policy comes
        from policy_dev, the result goes to result_dev, the actions to tensor('actions') -- and around it, for a block, the
        v2x_rollout_traj with the workspace"""
        io = self._rollout_io(T)
        self._send_grid()
        t, K = self._t, io['graphs']
        base, res = io['policy_dev'].data_ptr(), io['result_dev'].data_ptr()
        r = Rollout(model=None, q=io['q'].data_ptr(), explore=base + 4 * K * self.n, random_actions=base, actions=t['actions'].data_ptr(),
                    step=self._sim_step(t['actions'].data_ptr(), power), w_v2v=float(v2v_weight), w_v2i=float(v2i_weight),
                    rep_xe=storage['xe'].data_ptr(), rep_xe_next=storage['xe_next'].data_ptr(), rep_col=storage['col'].data_ptr(),
                    rep_mask=storage['mask'].data_ptr(), rep_action=storage['action'].data_ptr(),
                    rep_reward=storage['reward'].data_ptr(), head=int(head), capacity=int(capacity),
                    result_reward=res, result_regular=res + 8 * K)
        if engine is not None:
            from ..engine import _batch_struct
            r.model = engine._h
            r.batch = _batch_struct(self._rollout_batch(io, K, io['xe'], io['col'], row_ptr))
        if T is None:
            return r
        ws = io['workspace'].data_ptr()
        return RolloutTraj(r=r, T=T, pad_=0, **{k: ws + o for k, o in io['offsets'].items()})

    def rollout_struct(self, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None, power=None):
        """the v2x_rollout of the resident tensors and rollout_buffers() (what rollout_step() passes to the library)"""
        return self._rollout_struct(None, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr, power)

    def rollout_steps_struct(self, T, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None, power=None):
        """the v2x_rollout_traj of the resident tensors and rollout_steps_buffers(T) (what rollout_steps() passes to the library)"""
        return self._rollout_struct(T, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr, power)

    def _upload_policy(self, io, random_actions, explore):
        """the host's draws -> io['policy_dev'] through the next of the four page-locked copies (its event guards the reuse)"""
        pin, nb = self._ring_next(io, 'policy_', 'next'), 4 * random_actions.size
        pin[:nb].view(np.int32)[:] = random_actions.reshape(-1)
        pin[nb:nb + explore.size] = explore.reshape(-1)
        self._ring_send(io, 'policy_', 'next')

    def _ring_next(self, io, ring, next_key):
        """-> the numpy view of the next of the four page-locked copies io[ring + 'pin'], once the upload that last read it is
        through (its event guards the reuse); the caller fills it and hands it to _ring_send"""
        i = io[next_key]
        if io[ring + 'ev'][i] is not None:
            io[ring + 'ev'][i].synchronize()
        return io[ring + 'pin'][i].numpy()

    def _ring_send(self, io, ring, next_key, size=None):
        """the copy _ring_next gave out -> io[ring + 'dev'] (their first `size` elements; None: all), counted in traffic"""
        t, i = self.torch, io[next_key]
        io[next_key] = (i + 1) % 4
        pin, dev, ev = io[ring + 'pin'][i], io[ring + 'dev'], io[ring + 'ev']
        if size is None:
            dev.copy_(pin, non_blocking=True)
        else:
            dev[:size].copy_(pin[:size], non_blocking=True)
        self.traffic['bytes_up'] += (dev.numel() if size is None else size) * dev.element_size()
        if ev[i] is None:
            ev[i] = t.cuda.Event()
        ev[i].record(t.cuda.current_stream(self.device))

    def _download(self, dev, free, size=None):
        """the block `dev` (its first `size` bytes; None: all of it) -> a page-locked copy (a returned one of `free`, or a new
        one), counted in traffic; -> (free, event, copy): what every result class takes first, the download in flight"""
        t = self.torch
        pinned = free.pop() if free else t.zeros(dev.numel(), dtype=t.uint8, pin_memory=self._pin)
        if size is None:
            pinned.copy_(dev, non_blocking=True)
        else:
            pinned[:size].copy_(dev[:size], non_blocking=True)
        self.traffic['bytes_down'] += dev.numel() if size is None else size
        ev = t.cuda.Event()
        ev.record(t.cuda.current_stream(self.device))
        return free, ev, pinned

    def _download_result(self, io, T, cls=RolloutResult):
        """io['result_dev'] -> the RolloutResult (cls), its download in flight"""
        return cls(*self._download(io['result_dev'], io['free']), self.E, T)

    def _rollout(self, who, T, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr, power,
                 walk='serial', stream_phase='chain'):
        """rollout_step() (T None) / rollout_steps(): check, upload the policy, the one library call, start the download"""
        check_walk(who, walk)
        check_stream_phase(who, stream_phase, walk)
        ex, ra = self._check_rollout(who, T, explore, random_actions, storage, head, capacity)
        if engine is not None and row_ptr is None:
            raise ValueError("%s: scoring needs the CSR row pointer of the %s batch" % (who, "resident" if T is None else "trajectory's"))
        self._init_device()
        if not self._obs_ready:
            raise RuntimeError("%s: no observe() since the last step()" % who)
        io = self._rollout_io(T)
        self._upload_policy(io, ra, ex)
        r = self._rollout_struct(T, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr, power)
        self._keep_actions = self._t['actions']
        if T is None:
            check(self._lib, self._lib.v2x_rollout_step(C.byref(r), self._stream()))
        else:
            self._trajectory_call(self._lib.v2x_rollout_steps, self._lib.v2x_rollout_steps_wide, self._lib.v2x_rollout_steps_split, r,
                                  T, walk, stream_phase)
        self._obs_ready = True
        return self._download_result(io, T)

    def _trajectory_call(self, serial, wide, split, r, T, walk, stream_phase):
        """the library call of a trajectory struct r in the form `walk` and `stream_phase` name, counted in walk_calls (a split
        call is a wide one there) and, the wide ones, in stream_phase_calls"""
        if walk == 'wide':
            ws = self._wide_workspace(T)
            if stream_phase == 'split':
                ss = self._split_workspace(T)
                check(self._lib, split(C.byref(r), ws.data_ptr(), ws.numel(), ss.data_ptr(), ss.numel(), self._stream()))
            else:
                check(self._lib, wide(C.byref(r), ws.data_ptr(), ws.numel(), self._stream()))
            self.stream_phase_calls[stream_phase] += 1
        else:
            check(self._lib, serial(C.byref(r), self._stream()))
        self.walk_calls[walk] += 1
        self._traj_form.pop(T, None)

    def rollout_step(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None,
                     power=None):
        """One DQN rollout iteration in one call (v2x_rollout_step) on the resident state: the Q-values of the resident
        observation (engine: a GnnEngine, with row_ptr the constant CSR pointer of E n rows; None: nobody is greedy, no
        forward), the actions (explore [E] flags, random_actions [E, n]: the host's epsilon-greedy draws, uploaded as one small
        buffer), the simulator step, the reward v2v_weight * sum(V2V rates) + v2i_weight * sum(V2I rates) in numpy's order, and
        the transitions into slots (head + e) % capacity of `storage` (the replay's device tensors xe, xe_next, col, mask,
        action, reward).  The current observation must be on the device (observe() / advance() / a previous rollout_step).
        -> a RolloutResult whose download is in flight.  Afterwards as after advance(): fetch_rates(), fetch_observation()."""
        return self._rollout("rollout_step", None, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine,
                             row_ptr, power)

    def rollout_steps(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None,
                      power=None, walk='serial', stream_phase='chain'):
        """T DQN rollout iterations in ONE call (v2x_rollout_steps) on the resident state: every simulator walks its T steps in
        one kernel, one forward scores all T E observations (engine: a GnnEngine, with row_ptr the constant CSR pointer of
        T E n rows; None: nobody is greedy anywhere in the block, no forward), and one kernel picks (explore [T, E] flags,
        random_actions [T, E, n]: the host's draws, one upload), pays and stores the T E transitions into slots
        (head + t E + e) % capacity of `storage`.  Bit for bit T calls of rollout_step().  -> a RolloutResult whose download
        (one) is in flight.  Afterwards as after the last rollout_step: fetch_rates(), fetch_observation().
        walk: 'serial' (one workgroup per simulator walks its T steps) or 'wide' (v2x_rollout_steps_wide: the steps spread over
        the chip, four launches, the same bits); walk_calls counts which ran.
        stream_phase (walk='wide' only): 'chain' (the first of the four launches draws the streams of all T steps) or 'split'
        (v2x_rollout_steps_split: raw words, offset walk and conversion as three launches, the same bits); stream_phase_calls
        counts the wide calls by it."""
        return self._rollout("rollout_steps", _block_length(explore), explore, random_actions, storage, head, capacity, v2v_weight,
                             v2i_weight, engine, row_ptr, power, walk, stream_phase)

    # ------------------------------------------------------------------ 3..128 links: the receiver form (ReceiverReplay's layout)
    @staticmethod
    def check_observe_recv(n, C, rb=None):
        """The limits of v2x_sim_observe_recv / v2x_rollout_steps_recv: check_observe's with 128 links in place of 31."""
        if not OBSERVE_MIN_LINKS <= n <= RECV_MAX_LINKS:
            raise ValueError("the device observation in receiver form supports %d..%d links, got %d"
                             % (OBSERVE_MIN_LINKS, RECV_MAX_LINKS, n))
        DeviceChannels.check_observe(min(n, OBSERVE_MAX_LINKS), C, rb)

    def observe_recv(self, dest=None, power=None):
        """observe() for 3..128 links (v2x_sim_observe_recv): interf_db, state and xe as observe() leaves them, and in place of
        mask / col / regular the receivers (tensor('recv') [E, n] int32, recv[q] == q: link q is its own receiver) and one flag
        byte per state (tensor('flags'): FLAG_OWN some link is its own receiver, FLAG_BAD some receiver outside [0, n): NaN
        rows, recv[q] = q throughout).  Host receivers are looked at before they go up (own_receiver_counts): that is where
        rollout_steps_recv learns whether its batch needs edge_base."""
        self.check_observe_recv(self.n, self.rb)
        where = None
        if dest is not None:
            where, d = self._check_input('dest', dest, 'i')
        self._init_device()
        if where == 'dev':
            self._t['dest'].copy_(d)
            self._own = None
        elif where is not None:
            self._up(self._t['dest'], d)
            self._own = own_receiver_counts(d)
        T, c = self._t, self.constants
        check(self._lib, self._lib.v2x_sim_observe_recv(
            self.E, self.n, self.rb, T['dest'].data_ptr(), T['v2v_ff'].data_ptr(), T['v2i_ff'].data_ptr(), c['p_v2i'],
            c['veh_gain'], c['veh_nf'], c['sig2'], float(c['p_v2v'] if power is None else power), T['interf_db'].data_ptr(),
            T['state'].data_ptr(), T['xe'].data_ptr(), T['recv'].data_ptr(), T['flags'].data_ptr(), self._stream()))
        self._obs_ready = False                          # (xe is shared: the packed form's mask / col / regular are not of it)
        self._recv_ready = True

    def fetch_observation_recv(self):
        """-> (xe [E, n, 16] float32, recv [E, n] int32, flags [E] uint8) of the last observe_recv(): fresh host arrays"""
        self._init_device()
        if not self._recv_ready:
            raise RuntimeError("fetch_observation_recv: no observe_recv() since the last step()")
        xe = self._t['xe'].cpu().numpy()
        self._recv_host.copy_(self._recv_dev, non_blocking=True)
        self.traffic['bytes_down'] += xe.nbytes + self._recv_host.numel()
        self._sync()
        return xe, self._recv_np['recv'].copy(), self._recv_np['flags'].copy()

    def csr_from_recv(self, G, row_ptr, col_idx, edge_base=None):
        """row_ptr [G n + 1] / col_idx (int32 device tensors) of G graphs on the resident receivers of the last observe_recv(),
        graph g on state g % E (v2x_csr_from_recv); edge_base: an int32 tensor [G + 1] the device can read, or None (every
        graph regular)"""
        self._init_device()
        if not self._recv_ready:
            raise RuntimeError("csr_from_recv: no observe_recv() since the last step()")
        n, G = self.n, int(G)
        need = n * (n - 2) * G if edge_base is None else None
        if row_ptr.numel() < G * n + 1 or (need is not None and col_idx.numel() < need):
            raise ValueError("csr_from_recv: row_ptr of %d and col_idx of %d entries needed" % (G * n + 1, need))
        check(self._lib, self._lib.v2x_csr_from_recv(G, self.E, n, self._t['recv'].data_ptr(),
                                                     None if edge_base is None else edge_base.data_ptr(), row_ptr.data_ptr(),
                                                     col_idx.data_ptr(), self._stream()))

    def check_rollout_steps_recv(self, explore, random_actions, storage, head, capacity, own=None, stream_phase='chain',
                                 stream_words='serial'):
        """ValueError unless the arguments of rollout_steps_recv() fit this object; -> (T, explore [T, E] uint8, random_actions
        [T, E, n] int32, own [E] int32)"""
        who, E, n = "rollout_steps_recv", self.E, self.n
        check_stream_phase(who, stream_phase)
        check_stream_words(who, stream_words, stream_phase)
        T = _block_length(explore)
        self.check_observe_recv(n, self.rb)
        self._check_mobility(who, True)
        ex = np.asarray(explore)
        if T < 1 or ex.shape != (T, E) or ex.dtype.kind not in 'biu':
            raise ValueError("explore: [T, %d] flags with T >= 1 expected, got shape %s of dtype %s" % (E, list(ex.shape), ex.dtype))
        ra = np.asarray(random_actions)
        if ra.dtype.kind not in 'iu':
            raise ValueError("random_actions must be integers, got dtype %s" % ra.dtype)
        if ra.shape == (T, E, n, 1):
            ra = ra.reshape(T, E, n)
        if ra.shape != (T, E, n):
            raise ValueError("random_actions: an array of shape %s expected, got %s" % ([T, E, n], list(ra.shape)))
        head, capacity, K = int(head), int(capacity), T * E
        if not K <= capacity or not 0 <= head < capacity:
            raise ValueError("%s: T E <= capacity and 0 <= head < capacity needed, got T = %d, E = %d, head = %d, capacity = %d"
                             % (who, T, E, head, capacity))
        if K * n * (n - 1) > 2 ** 31 - 1:
            raise ValueError("%s: T E = %d graphs of %d links exceed the 32-bit sizes of a batch" % (who, K, n))
        want = {'xe': (n, XE_WIDTH), 'xe_next': (n, XE_WIDTH), 'recv': (n,), 'action': (n,), 'reward': ()}
        for k, tail in want.items():
            t = storage.get(k)
            if t is None or tuple(t.shape[1:]) != tail or not t.is_contiguous():
                raise ValueError("%s: replay storage %r of shape [slots] + %s expected" % (who, k, list(tail)))
            if t.shape[0] < (capacity if head + K > capacity else head + K):      # (a block that wraps touches the last slot)
                raise ValueError("%s: replay storage %r has %d slots, the block at %d needs more" % (who, k, t.shape[0], head))
        if own is not None:
            own = np.asarray(own, np.int32)                  # (the rollout casts what it is given; the evaluation refuses floats)
        return T, ex.astype(np.uint8), np.ascontiguousarray(ra, np.int32), self._own_counts(who, own, "")

    def _own_counts(self, who, own, word):
        """own, the states' own-receiver counts of a receiver-form call -- None: those of the receivers this object last sent up
        from the host -> [E] int32; ValueError unless they are E integers in [0, n] (word: how the refusal qualifies them)"""
        E, n = self.E, self.n
        if own is None:
            if self._own is None:
                raise ValueError("%s: the receivers went up as a device tensor: pass own, the states' own-receiver counts [E] (the "
                                 "host decides whether the batch needs edge_base)" % who)
            own, bad = self._own
            if bad.any():
                raise ValueError("%s: state(s) %s hold a receiver outside [0, %d)" % (who, np.nonzero(bad)[0].tolist(), n))
        own = np.asarray(own)
        if own.dtype.kind not in 'iu' or own.reshape(-1).shape != (E,) or (own < 0).any() or (own > n).any():
            raise ValueError("%s: own: %d %sown-receiver counts in [0, %d] expected" % (who, E, word, n))
        return own.reshape(-1).astype(np.int32)

    def _recv_io(self, T):
        """the buffers of rollout_steps_recv() for blocks of T, made once per T: the policy ring and the result block of
        _rollout_io, q, the ONE workspace (recv_workspace_layout) and a ring of four page-locked edge_base [T E + 1]"""
        self._init_device()
        io = self._roll.get(('recv', T))
        if io is None:
            t, E, n, rb = self.torch, self.E, self.n, self.rb
            K = T * E
            nb = self.rollout_steps_policy_bytes(T)
            offs, size = recv_workspace_layout(E, n, rb, T)
            ws = self._sized_workspace("workspace", T, self._lib.v2x_rollout_recv_workspace_bytes(E, n, rb, T), size,
                                       who="rollout_steps_recv", aligned=True)
            io = self._roll[('recv', T)] = {
                'policy_dev': t.zeros(nb, dtype=t.uint8, device=self.device),
                'policy_pin': [t.zeros(nb, dtype=t.uint8, pin_memory=self._pin) for _ in range(4)], 'policy_ev': [None] * 4, 'next': 0,
                'result_dev': t.zeros(self.rollout_steps_result_bytes(T), dtype=t.uint8, device=self.device), 'free': [],
                'q': t.zeros((K * n, rb), dtype=t.float32, device=self.device), 'graphs': K, 'workspace': ws, 'offsets': offs,
                'eb_pin': [t.zeros(K + 1, dtype=t.int32, pin_memory=self._pin) for _ in range(4)], 'eb_ev': [None] * 4, 'eb_next': 0,
                'eb_dev': t.zeros(K + 1, dtype=t.int32, device=self.device)}
            view = lambda k, count, dt: ws[offs[k]:offs[k] + count * t.empty(0, dtype=dt).element_size()].view(dt)   # noqa: E731
            io['xe'] = view('traj_xe', K * n * XE_WIDTH, t.float32).view(K * n, XE_WIDTH)
            io['row_ptr'] = view('row_ptr', K * n + 1, t.int32)
            io['col_any'] = view('col_idx', K * n * (n - 1), t.int32)
        return io

    def _recv_split_workspace(self, T):
        """the second workspace of a rollout_steps_recv() whose stream phase is split, for blocks of T on the current lane grid:
        made at the first split call of that T (again when set_grid() changes the number of lanes) and kept next to
        _recv_io(T)'s buffers; it never crosses the bus"""
        io = self._recv_io(T)
        E, n, rb, n_lanes = self.E, self.n, self.rb, self._grid[0].shape[1]
        ws = io.get('split_workspace')
        if ws is None or io.get('split_lanes') != n_lanes:
            ws = self._sized_workspace("split-stream workspace", T, self._lib.v2x_rollout_recv_split_workspace_bytes(E, n, rb, T, n_lanes),
                                       split_workspace_layout(E, n, rb, T, n_lanes)[1], who="rollout_steps_recv", n_lanes=n_lanes,
                                       aligned=True)
            io['split_workspace'], io['split_lanes'] = ws, n_lanes
        return ws

    jump_plan = staticmethod(jump_plan)

    def _recv_jump_table(self, T):
        """the v2x_mt_jump of a receiver-form split call whose words are drawn in chunks (stream_words='jump'), for blocks of T
        on the current lane grid: jump_plan() of the word array's length, the polynomials of v2x_mt_jump_polys uploaded once per
        (first, stride, count) of this object -- they depend on the chunk positions alone, not on T, the states or the seeds --
        and the scratch of v2x_mt_jump_scratch_bytes kept next to _recv_io(T)'s buffers; built once, never per call"""
        io = self._recv_io(T)
        E, n, rb, n_lanes = self.E, self.n, self.rb, self._grid[0].shape[1]
        jump = io.get('jump')
        if jump is None or io.get('jump_lanes') != n_lanes:
            t = self.torch
            plan = first, stride, count = self.jump_plan(split_stream_blocks(n, rb, T, n_lanes) * MT_WORDS)
            polys = scratch = None
            if count:
                polys = self._jump_tables.get(plan)
                if polys is None:
                    host = np.zeros((count, MT_WORDS), np.uint32)
                    check(self._lib, self._lib.v2x_mt_jump_polys(first, stride, count, host.ctypes.data))
                    polys = self._jump_tables[plan] = t.from_numpy(host.view(np.int32)).to(self.device)
                    self.traffic['bytes_up'] += host.nbytes
                need = self._lib.v2x_mt_jump_scratch_bytes(E, count)
                if need != _align(4 * E * count * JUMP_SLICES * MT_WORDS, 256):
                    raise ValueError("rollout_steps_recv: the library sizes the jump scratch of E = %d, count = %d at %d bytes, the "
                                     "documented formula at %d" % (E, count, need, _align(4 * E * count * JUMP_SLICES * MT_WORDS, 256)))
                scratch = t.zeros(need, dtype=t.uint8, device=self.device)
                if polys.data_ptr() % 256 or scratch.data_ptr() % 256:
                    raise RuntimeError("rollout_steps_recv: the allocator returned a jump table or scratch that is not 256-byte aligned")
            jump = MtJump(first=first, stride=stride, count=count, pad_=0, polys=None if polys is None else polys.data_ptr(),
                          scratch=None if scratch is None else scratch.data_ptr(), scratch_bytes=0 if scratch is None else scratch.numel())
            jump._keep = (polys, scratch)                    # (kept alive with the struct)
            io['jump'], io['jump_lanes'] = jump, n_lanes
        return jump

    def _recv_call(self, family, r, io, T, stream_phase, stream_words):
        """the one library call of the receiver-form struct r on io's workspace: v2x_<family>_recv ('rollout_steps', 'eval_steps'
        or 'eval_sweep'), with stream_phase='split' its _split form on _recv_split_workspace(T) or, stream_words='jump', its _jump
        form on the cached table of _recv_jump_table(T) as well; counted in walk_calls (a wide walk), stream_phase_calls and, the
        split ones, stream_words_calls.  Afterwards the resident observation and trajectory T are in receiver form."""
        lib, ws, name = self._lib, io['workspace'], 'v2x_%s_recv' % family
        self._keep_actions = self._t['actions']
        if stream_phase != 'split':
            check(lib, getattr(lib, name)(C.byref(r), ws.data_ptr(), ws.numel(), self._stream()))
        else:
            sws = self._recv_split_workspace(T)
            if stream_words == 'jump':
                check(lib, getattr(lib, name + '_jump')(C.byref(r), ws.data_ptr(), ws.numel(), sws.data_ptr(), sws.numel(),
                                                        C.byref(self._recv_jump_table(T)), self._stream()))
            else:
                check(lib, getattr(lib, name + '_split')(C.byref(r), ws.data_ptr(), ws.numel(), sws.data_ptr(), sws.numel(), self._stream()))
            self.stream_words_calls[stream_words] += 1
        self.walk_calls['wide'] += 1
        self.stream_phase_calls[stream_phase] += 1
        self._traj_form[T] = 'recv'
        self._obs_ready = False
        self._recv_ready = True

    def rollout_steps_recv_buffers(self, T):
        """the device buffers of rollout_steps_recv() for blocks of T: workspace (carved by recv_workspace_layout: offsets),
        policy_dev, result_dev (reward [T, E] float64 | flags [T, 2, E] bytes), q [T E n, rb] float32"""
        return self._recv_io(T)

    def _edge_base(self, io, own, T):
        """own [E] -> (edge_base pointer or None, n_edges, max_edges) of the T E graphs of a trajectory: every state regular
        needs none; otherwise the cumulative sum of n (n - 2) + own[g % E] goes up through the next of four page-locked copies"""
        n, K = self.n, io['graphs']
        if not own.any():
            return None, K * n * (n - 2), n * (n - 2)
        eb = np.zeros(K + 1, np.int64)
        np.cumsum(n * (n - 2) + np.tile(own.astype(np.int64), T), out=eb[1:])
        self._ring_next(io, 'eb_', 'eb_next')[:] = eb
        self._ring_send(io, 'eb_', 'eb_next')
        return io['eb_dev'].data_ptr(), int(eb[-1]), n * (n - 1)

    def rollout_steps_recv_struct(self, T, storage, head, capacity, v2v_weight, v2i_weight, engine=None, edge_base=None,
                                  n_edges=None, max_edges=None, power=None):
        """the v2x_rollout_recv of the resident tensors and rollout_steps_recv_buffers(T) (what rollout_steps_recv() passes to
        the library); edge_base: a device-readable pointer or None, with the batch's n_edges / max_edges it implies (None:
        every graph regular)"""
        io = self._recv_io(T)
        self._send_grid()
        t, K, n = self._t, io['graphs'], self.n
        base, res, ws = io['policy_dev'].data_ptr(), io['result_dev'].data_ptr(), io['workspace'].data_ptr()
        step = self._recv_step(power)
        r = RolloutRecv(model=None, q=io['q'].data_ptr(), explore=base + 4 * K * n, random_actions=base, actions=t['actions'].data_ptr(),
                        step=step, recv=t['recv'].data_ptr(), flags=t['flags'].data_ptr(), w_v2v=float(v2v_weight),
                        w_v2i=float(v2i_weight), T=T, pad_=0, edge_base=edge_base, rep_xe=storage['xe'].data_ptr(),
                        rep_xe_next=storage['xe_next'].data_ptr(), rep_recv=storage['recv'].data_ptr(),
                        rep_action=storage['action'].data_ptr(), rep_reward=storage['reward'].data_ptr(), head=int(head),
                        capacity=int(capacity), result_reward=res, result_flags=res + 8 * K,
                        **{k: ws + io['offsets'][k] for k in RECV_SECTIONS})
        return self._recv_scored(r, io, engine, edge_base, n_edges, max_edges)

    def _recv_step(self, power):
        """the v2x_sim_step of a receiver-form struct: _sim_step with the action buffer in it and the packed form's fields empty"""
        step = self._sim_step(self._t['actions'].data_ptr(), power)
        step.mask = step.col = step.regular = None           # (not read: the receiver form has recv / flags)
        return step

    def _recv_scored(self, r, io, engine, edge_base, n_edges, max_edges):
        """-> the receiver-form struct r, with `engine` (when given) and the cached batch of io's T E graphs attached: n_edges /
        max_edges as edge_base implies them, or those of regular graphs without one"""
        if engine is not None:
            from ..engine import _batch_struct
            if edge_base is None:
                n_edges, max_edges = io['graphs'] * self.n * (self.n - 2), self.n * (self.n - 2)
            r.model = engine._h
            r.batch = _batch_struct(self._recv_batch(io, n_edges, max_edges))
        return r

    def rollout_steps_recv(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None, own=None,
                           power=None, stream_phase='chain', stream_words='serial'):
        """rollout_steps(walk='wide') for 3..128 links into ReceiverReplay's layout, ONE call (v2x_rollout_steps_recv): the wide
        walk, the observations of entries 1..T in receiver form, the closed-form CSR of the T E graphs, one forward (engine
        given), and the finish that picks, pays and stores xe / xe_next / recv / action / reward into slots
        (head + t E + e) % capacity of `storage` (the tensors of ReceiverReplay.storage()).  States with an own-receiver link
        are scored and stored like the others.  own: the states' own-receiver counts [E]; None: those of the receivers this
        object last sent up from the host.  The current observation must be resident in receiver form (observe_recv() or a
        previous rollout_steps_recv()).  stream_phase: 'chain' (the first launch draws the streams of all T steps) or 'split'
        (v2x_rollout_steps_recv_split: raw words, offset walk and conversion as three launches on a second workspace made once
        per T, the same bits); stream_phase_calls counts the calls by it.  stream_words (stream_phase='split' only): 'serial'
        (one workgroup per state draws all its words) or 'jump' (v2x_rollout_steps_recv_jump: the words beyond a prefix drawn in
        chunks entered by jump-ahead polynomials, the same bits; the table and a scratch are made once per T);
        stream_words_calls counts the split calls by it.  -> a RecvRolloutResult whose download is in flight."""
        who = "rollout_steps_recv"
        T, ex, ra, own = self.check_rollout_steps_recv(explore, random_actions, storage, head, capacity, own, stream_phase,
                                                       stream_words)
        self._init_device()
        if not self._recv_ready:
            raise RuntimeError("%s: no observe_recv() since the last step()" % who)
        io = self._recv_io(T)
        self._upload_policy(io, ra, ex)
        eb, n_edges, max_edges = self._edge_base(io, own, T) if engine is not None else (None, None, None)
        r = self.rollout_steps_recv_struct(T, storage, head, capacity, v2v_weight, v2i_weight, engine, eb, n_edges, max_edges, power)
        self._recv_call('rollout_steps', r, io, T, stream_phase, stream_words)
        return self._download_result(io, T, RecvRolloutResult)

    # ------------------------------------------------------------------ an evaluation episode on the resident state
    def eval_steps_policy_bytes(self, T, baseline=True):
        """bytes of the one buffer eval_steps() uploads: policy_random [T, E, n] int32, explore [T, E] bytes (rounded up to 4),
        then, with a baseline scheme, baseline_actions [T, E, n] int32"""
        K = T * self.E
        return _align(4 * K * self.n + K, 4) + (4 * K * self.n if baseline else 0)

    def eval_steps_result_bytes(self, T, schemes=2):
        """bytes of the result block eval_steps() downloads (eval_result_layout)"""
        return eval_result_layout(self.E, self.n, self.rb, T, schemes)[1]

    def check_eval_steps(self, explore, policy_random, baseline_actions):
        """ValueError unless the arguments of eval_steps() fit this object; -> (T, explore [T, E] uint8, policy_random [T, E, n]
        int32, baseline_actions [T, E, n] int32 or None)"""
        self.check_observe(self.n, self.rb)
        # (called unbound by _PoolShape, the shape-only stand-in of the mixed calls: it has E, n and _check_mobility)
        return DeviceChannels._check_eval_arrays(self, "eval_steps", explore, policy_random, baseline_actions)

    def _check_eval_arrays(self, who, explore, policy_random, baseline_actions):
        """what check_eval_steps and check_eval_steps_recv ask of the draws of an evaluation block"""
        E, n = self.E, self.n
        self._check_mobility(who, True)
        T = _block_length(explore)
        ex = np.asarray(explore)
        if T < 1 or ex.shape != (T, E) or ex.dtype.kind not in 'biu':
            raise ValueError("explore: [T, %d] flags with T >= 1 expected, got shape %s of dtype %s" % (E, list(ex.shape), ex.dtype))
        if T * E > MAX_STATES:
            raise ValueError("%s: T E <= %d needed (the snapshots are one stacked search problem), got T = %d, E = %d"
                             % (who, MAX_STATES, T, E))
        out = []
        for name, a in (('policy_random', policy_random), ('baseline_actions', baseline_actions)):
            if a is None and name == 'baseline_actions':
                out.append(None)
                continue
            a = np.asarray(a)
            if a.dtype.kind not in 'iu':
                raise ValueError("%s must be integers, got dtype %s" % (name, a.dtype))
            if a.shape == (T, E, n, 1):
                a = a.reshape(T, E, n)
            if a.shape != (T, E, n):
                raise ValueError("%s: an array of shape %s expected, got %s" % (name, [T, E, n], list(a.shape)))
            out.append(np.ascontiguousarray(a, np.int32))
        return T, ex.astype(np.uint8), out[0], out[1]

    def _eval_io(self, T):
        """_rollout_io(T) -- the trajectory workspace, q and the cached T E-graph batch are shared with rollout_steps() -- with
        the evaluation's own policy buffer (ring of four page-locked copies) and result block added at the first use"""
        return self._add_eval_buffers(self._rollout_io(T), T)

    def _add_eval_buffers(self, io, T):
        """the evaluation's own policy ring and result block in the buffers `io` of blocks of T, made at the first use"""
        if 'eval_policy_dev' not in io:
            t, nb = self.torch, self.eval_steps_policy_bytes(T)
            io['eval_policy_dev'] = t.zeros(nb, dtype=t.uint8, device=self.device)
            io['eval_policy_pin'] = [t.zeros(nb, dtype=t.uint8, pin_memory=self._pin) for _ in range(4)]
            io['eval_policy_ev'], io['eval_next'] = [None] * 4, 0
            io['eval_result_dev'] = t.zeros(self.eval_steps_result_bytes(T, 2), dtype=t.uint8, device=self.device)
            io['eval_free'] = []
        return io

    def _eval_upload(self, io, T, ex, ra, ba):
        """the host's draws of an evaluation block -> io['eval_policy_dev'] through the next of the four page-locked copies (its
        event guards the reuse)"""
        pin, K, n = self._ring_next(io, 'eval_policy_', 'eval_next'), T * self.E, self.n
        nb = self.eval_steps_policy_bytes(T, ba is not None)
        pin[:4 * K * n].view(np.int32)[:] = ra.reshape(-1)
        pin[4 * K * n:4 * K * n + K] = ex.reshape(-1)
        if ba is not None:
            pin[nb - 4 * K * n:nb].view(np.int32)[:] = ba.reshape(-1)
        self._ring_send(io, 'eval_policy_', 'eval_next', nb)

    def _eval_download(self, io, T, S, cls=EvalResult):
        """the result block of S schemes in io['eval_result_dev'] (a block of two schemes: only the S there are come down) ->
        the EvalResult (cls), its download in flight"""
        return cls(*self._download(io['eval_result_dev'], io['eval_free'], self.eval_steps_result_bytes(T, S)), self.E, self.n, self.rb, T, S)

    def _sweep_io(self, T, S):
        """-> (_eval_io(T), the result block of a sweep of S schemes (eval_sweep_mixed): its device block 'dev' and the
        page-locked copies that came back 'free', made at the first use of (T, S))"""
        io = self._eval_io(T)
        sw = io.setdefault('sweep', {}).get(S)
        if sw is None:
            t = self.torch
            sw = io['sweep'][S] = {'dev': t.zeros(self.eval_steps_result_bytes(T, S), dtype=t.uint8, device=self.device), 'free': []}
        return io, sw

    def _sweep_download(self, sw, T, S, cls=EvalResult):
        """_eval_download for the result block of a sweep"""
        return cls(*self._download(sw['dev'], sw['free']), self.E, self.n, self.rb, T, S)

    def eval_steps_struct(self, T, v2v_weight, v2i_weight, engine=None, row_ptr=None, power=None, baseline=True):
        """the v2x_eval of the resident tensors and the buffers of _eval_io(T) (what eval_steps() passes to the library)"""
        io = self._eval_io(T)
        self._send_grid()
        t, K, n = self._t, T * self.E, self.n
        base, res = io['eval_policy_dev'].data_ptr(), io['eval_result_dev'].data_ptr()
        offs, _ = eval_result_layout(self.E, n, self.rb, T, 2 if baseline else 1)
        ws = io['workspace'].data_ptr()
        r = Eval(model=None, q=io['q'].data_ptr(), explore=base + 4 * K * n, random_actions=base,
                 baseline_actions=base + _align(4 * K * n + K, 4) if baseline else None, actions=t['actions'].data_ptr(),
                 step=self._sim_step(t['actions'].data_ptr(), power), w_v2v=float(v2v_weight), w_v2i=float(v2i_weight), T=T, pad_=0,
                 **{k: ws + o for k, o in io['offsets'].items()}, **{'result_' + k: res + o for k, o in offs.items()})
        if engine is not None:
            from ..engine import _batch_struct
            if row_ptr is None:                          # the constant CSR pointer of T E n rows of n - 2 sources, made once per T
                row_ptr = io.get('eval_row_ptr')
                if row_ptr is None:
                    row_ptr = io['eval_row_ptr'] = self.torch.arange(K * n + 1, dtype=self.torch.int32, device=self.device) * (n - 2)
            r.model = engine._h
            r.batch = _batch_struct(self._rollout_batch(io, K, io['xe'], io['col'], row_ptr))
        return r

    def eval_steps(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=None, row_ptr=None, power=None,
                   walk='serial', stream_phase='chain'):
        """The T steps of an evaluation episode in ONE call (v2x_eval_steps) on the resident state: every simulator walks its T
        steps in one kernel, one forward scores all T E observations (engine: a GnnEngine; row_ptr: the constant CSR pointer of
        T E n rows, made here when None; engine None: nobody is greedy, no forward), and one kernel pays two schemes per state --
        the policy (explore [T, E] flags, policy_random [T, E, n]) and the baseline (baseline_actions [T, E, n]; None: no
        baseline scheme) -- on the step's snapshot.  No replay memory is touched.  One upload (the draws), one download (the
        result block) -> an EvalResult whose download is in flight.  Afterwards the resident state is what T advance() calls
        under the policy's actions leave, and trajectory_states(T) holds the T snapshots.  walk, stream_phase: as for
        rollout_steps() (v2x_eval_steps_wide, v2x_eval_steps_split)."""
        check_walk("eval_steps", walk)
        check_stream_phase("eval_steps", stream_phase, walk)
        T, ex, ra, ba = self.check_eval_steps(explore, policy_random, baseline_actions)
        self._init_device()
        if not self._obs_ready:
            raise RuntimeError("eval_steps: no observe() since the last step()")
        io = self._eval_io(T)
        self._eval_upload(io, T, ex, ra, ba)
        r = self.eval_steps_struct(T, v2v_weight, v2i_weight, engine, row_ptr, power, ba is not None)
        self._keep_actions = self._t['actions']
        self._trajectory_call(self._lib.v2x_eval_steps, self._lib.v2x_eval_steps_wide, self._lib.v2x_eval_steps_split, r, T, walk,
                              stream_phase)
        self._obs_ready = True
        return self._eval_download(io, T, 2 if ba is not None else 1)

    # ------------------------------------------------------------------ an evaluation episode of 3..128 links (receiver form)
    def check_eval_steps_recv(self, explore, policy_random, baseline_actions, own=None, stream_phase='chain', stream_words='serial'):
        """ValueError unless the arguments of eval_steps_recv() fit this object; -> (T, explore [T, E] uint8, policy_random
        [T, E, n] int32, baseline_actions [T, E, n] int32 or None, own [E] int32)"""
        who, E, n = "eval_steps_recv", self.E, self.n
        check_stream_phase(who, stream_phase)
        check_stream_words(who, stream_words, stream_phase)
        self.check_observe_recv(n, self.rb)
        T, ex, ra, ba = self._check_eval_arrays(who, explore, policy_random, baseline_actions)
        if T * E * n * (n - 1) > 2 ** 31 - 1:
            raise ValueError("%s: T E = %d graphs of %d links exceed the 32-bit sizes of a batch" % (who, T * E, n))
        return T, ex, ra, ba, self._own_counts(who, own, "integer ")

    def _recv_eval_io(self, T):
        """_recv_io(T) -- the ONE workspace, q, the cached batches and the edge_base ring are shared with rollout_steps_recv() --
        with the evaluation's own policy ring and result block added at the first use"""
        io = self._recv_io(T)
        if 'eval_policy_dev' not in io:
            need = self._lib.v2x_eval_recv_result_bytes(self.E, self.n, self.rb, T, 2)
            if need != self.eval_steps_result_bytes(T, 2):
                raise ValueError("eval_steps_recv: the library sizes the result block of E = %d, n = %d, rb = %d, T = %d at %d bytes, "
                                 "the documented layout at %d" % (self.E, self.n, self.rb, T, need, self.eval_steps_result_bytes(T, 2)))
        return self._add_eval_buffers(io, T)

    def eval_steps_recv_buffers(self, T):
        """the device buffers of eval_steps_recv() for blocks of T: those of rollout_steps_recv_buffers(T) (workspace, q) with
        eval_policy_dev and eval_result_dev (the result block of two schemes, carved by eval_result_layout)"""
        return self._recv_eval_io(T)

    def _recv_batch(self, io, n_edges, max_edges):
        """the cached DeviceBatch of the T E graphs of io's workspace with that many edges"""
        from ..engine import DeviceBatch
        key = (n_edges, max_edges)
        db = io.get('batch', {}).get(key)
        if db is None:
            db = DeviceBatch.from_tensors(io['graphs'], self.n, io['xe'], io['row_ptr'], io['col_any'][:n_edges], max_edges)
            io['batch'] = {key: db}
        return db

    def eval_steps_recv_struct(self, T, v2v_weight, v2i_weight, engine=None, edge_base=None, n_edges=None, max_edges=None, power=None,
                               baseline=True):
        """the v2x_eval_recv of the resident tensors and the buffers of _recv_eval_io(T) (what eval_steps_recv() passes to the
        library); edge_base, n_edges, max_edges: as for rollout_steps_recv_struct"""
        io = self._recv_eval_io(T)
        self._send_grid()
        t, K, n = self._t, io['graphs'], self.n
        base, res, ws = io['eval_policy_dev'].data_ptr(), io['eval_result_dev'].data_ptr(), io['workspace'].data_ptr()
        offs, _ = eval_result_layout(self.E, n, self.rb, T, 2 if baseline else 1)
        step = self._recv_step(power)
        r = EvalRecv(model=None, q=io['q'].data_ptr(), explore=base + 4 * K * n, random_actions=base,
                     baseline_actions=base + _align(4 * K * n + K, 4) if baseline else None, actions=t['actions'].data_ptr(),
                     step=step, recv=t['recv'].data_ptr(), flags=t['flags'].data_ptr(), w_v2v=float(v2v_weight),
                     w_v2i=float(v2i_weight), T=T, pad_=0, edge_base=edge_base,
                     **{k: ws + io['offsets'][k] for k in RECV_SECTIONS},
                     **{'result_' + ('flags' if k == 'regular' else k): res + o for k, o in offs.items()})
        return self._recv_scored(r, io, engine, edge_base, n_edges, max_edges)

    def eval_steps_recv(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=None, own=None, power=None,
                        stream_phase='chain', stream_words='serial'):
        """eval_steps(walk='wide') for 3..128 links on the receiver-form resident state, ONE call (v2x_eval_steps_recv): the wide
        walk, the observations of entries 1..T in receiver form, the closed-form CSR of the T E graphs, one forward (engine
        given; None: nobody is greedy, no forward) and the finish that pays the policy and, when given, the baseline on every
        step's snapshot.  It runs on the buffers of rollout_steps_recv() of that T (workspace, q, cached batches, edge_base
        ring) with a policy ring and a result block of its own; no replay memory is touched.  States with an own-receiver link
        are scored like the others.  own, stream_phase, stream_words: as for rollout_steps_recv() (v2x_eval_steps_recv_split /
        _jump).  The current observation must be resident
        in receiver form.  -> a RecvEvalResult whose download is in flight; afterwards the resident state is what T advance()
        calls under the policy's actions leave, and trajectory_states(T) holds the T snapshots."""
        who = "eval_steps_recv"
        T, ex, ra, ba, own = self.check_eval_steps_recv(explore, policy_random, baseline_actions, own, stream_phase, stream_words)
        self._init_device()
        if not self._recv_ready:
            raise RuntimeError("%s: no observe_recv() since the last step()" % who)
        io = self._recv_eval_io(T)
        self._eval_upload(io, T, ex, ra, ba)
        eb, n_edges, max_edges = self._edge_base(io, own, T) if engine is not None else (None, None, None)
        r = self.eval_steps_recv_struct(T, v2v_weight, v2i_weight, engine, eb, n_edges, max_edges, power, ba is not None)
        self._recv_call('eval_steps', r, io, T, stream_phase, stream_words)
        return self._eval_download(io, T, 2 if ba is not None else 1, RecvEvalResult)

    # ------------------------------------------------------------------ K networks on one walked episode (receiver form)
    def check_eval_sweep_recv(self, explore, policy_random, baseline_actions, engines=None, K=None, own=None, stream_phase='chain',
                              stream_words='serial'):
        """ValueError unless the arguments of eval_sweep_recv() fit this object; -> (T, explore, policy_random, baseline_actions,
        own) as check_eval_steps_recv returns them, and K"""
        who = "eval_sweep_recv"
        try:
            checked = self.check_eval_steps_recv(explore, policy_random, baseline_actions, own, stream_phase, stream_words)
        except ValueError as err:
            raise ValueError(str(err).replace("eval_steps_recv", who))
        return checked + (_check_sweep_engines(who, engines, K, self.rb, self.n),)

    def _recv_sweep_io(self, T, S, K):
        """-> (_recv_eval_io(T), the sweep's own buffers: the result block of S schemes 'dev' with the page-locked copies that
        came back 'free', made at the first use of (T, S), and the Q workspace [K, T E n, rb] of (T, K))"""
        io = self._recv_eval_io(T)
        t = self.torch
        sw = io.setdefault('sweep', {}).get(S)
        if sw is None:
            size = self.eval_steps_result_bytes(T, S)
            need = self._lib.v2x_eval_sweep_recv_result_bytes(self.E, self.n, self.rb, T, S)
            if need != size:
                raise ValueError("eval_sweep_recv: the library sizes the result block of E = %d, n = %d, rb = %d, T = %d, %d schemes at "
                                 "%d bytes, the documented layout at %d" % (self.E, self.n, self.rb, T, S, need, size))
            sw = io['sweep'][S] = {'dev': t.zeros(size, dtype=t.uint8, device=self.device), 'free': []}
        q = io.setdefault('sweep_q', {}).get(K)
        if q is None:
            q = io['sweep_q'][K] = t.zeros((K, io['graphs'] * self.n, self.rb), dtype=t.float32, device=self.device)
        return io, sw, q

    def eval_sweep_recv_struct(self, T, K, v2v_weight, v2i_weight, engines=None, edge_base=None, n_edges=None, max_edges=None,
                               power=None, baseline=True):
        """the v2x_eval_sweep_recv of the resident tensors and the buffers of _recv_sweep_io (what eval_sweep_recv() passes to
        the library): eval_steps_recv_struct with engine 0's batch, the result pointers in the sweep's own block of S schemes"""
        S = K + (1 if baseline else 0)
        io, sw, q = self._recv_sweep_io(T, S, K)
        base = self.eval_steps_recv_struct(T, v2v_weight, v2i_weight, engines[0] if engines else None, edge_base, n_edges, max_edges,
                                           power, baseline)
        base.model = base.q = None
        offs, _ = eval_result_layout(self.E, self.n, self.rb, T, S)
        for name, o in offs.items():
            setattr(base, 'result_' + ('flags' if name == 'regular' else name), sw['dev'].data_ptr() + o)
        s = EvalSweepRecv(base=base, K=K, pad_=0, models=None, q=None)
        if engines:
            s._handles = (C.c_void_p * K)(*[engine._h for engine in engines])     # (kept alive with the struct)
            s.models = s._handles
            s.q = q.data_ptr()
        return s

    def eval_sweep_recv(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=None, K=None, own=None,
                        power=None, stream_phase='chain', stream_words='serial'):
        """eval_steps_recv() for K networks on the SAME steps in ONE call (v2x_eval_sweep_recv / _split): its arguments with a
        list of K fixed-size `engines` of one spec in the engine's place (None: nobody is greedy anywhere, no CSR, no forward; K
        then says how many identical policy schemes the result holds, default 1).  One walk, one observation pass, one CSR, K
        forwards of the one batch, one finish: scheme k < K is engine k's policy on the shared explore flags and random actions,
        scheme K the baseline (when given).  It runs on the buffers of eval_steps_recv() of that T with a result block per
        (T, S) and a Q workspace per (T, K) of its own.  The resident state afterwards is the one engine K - 1's own
        eval_steps_recv() leaves, and trajectory_states(T) holds the T snapshots.  stream_phase, stream_words: as for
        rollout_steps_recv() (v2x_eval_sweep_recv_split / _jump).
        -> a RecvEvalResult of K (+ 1) schemes, its download in flight."""
        who = "eval_sweep_recv"
        T, ex, ra, ba, own, K = self.check_eval_sweep_recv(explore, policy_random, baseline_actions, engines, K, own, stream_phase,
                                                           stream_words)
        engines = None if engines is None else list(engines)
        self._init_device()
        if not self._recv_ready:
            raise RuntimeError("%s: no observe_recv() since the last step()" % who)
        S = K + (1 if ba is not None else 0)
        io, sw, _ = self._recv_sweep_io(T, S, K)
        self._eval_upload(io, T, ex, ra, ba)
        eb, n_edges, max_edges = self._edge_base(io, own, T) if engines is not None else (None, None, None)
        s = self.eval_sweep_recv_struct(T, K, v2v_weight, v2i_weight, engines, eb, n_edges, max_edges, power, ba is not None)
        self._recv_call('eval_sweep', s, io, T, stream_phase, stream_words)
        return self._sweep_download(sw, T, S, RecvEvalResult)

    def trajectory_states(self, T):
        """-> TrajectoryStates: the T snapshots the last rollout_steps() / eval_steps() of block length T (or their receiver
        forms, rollout_steps_recv() / eval_steps_recv(): whichever ran last at that T) left in its workspace,
        as one stacked problem of T E states (E = T self.E, n_Veh, n_RB, problem_tensors(), rates()) for OptimalAllocation.
        Views over the workspace, no copy: valid until the next trajectory call of that T."""
        T = int(T)
        if T < 1 or T * self.E > MAX_STATES:
            raise ValueError("trajectory_states: 1 <= T and T E <= %d needed, got T = %d, E = %d" % (MAX_STATES, T, self.E))
        key = ('recv', T) if self._traj_form.get(T) == 'recv' else T     # (the form of the last trajectory call of that T)
        if self.torch is None or key not in self._roll:
            raise RuntimeError("trajectory_states: no trajectory call of T = %d has run on this object" % T)
        return TrajectoryStates(self, T, self._roll[key])

    # ------------------------------------------------------------------ for OptimalAllocation
    def problem(self, v2v_weight=0.0, v2i_weight=0.0):
        """the v2x_opt_problem of the device arrays"""
        self._init_device()
        T = self._t
        return OptProblem(E=self.E, n=self.n, rb=self.rb, pad_=0, v2v_ff=T['v2v_ff'].data_ptr(), v2i_ff=T['v2i_ff'].data_ptr(),
                          v2i_abs=T['v2i_abs'].data_ptr(), dest=T['dest'].data_ptr(), w_v2v=float(v2v_weight),
                          w_v2i=float(v2i_weight), **self.constants)

    def problem_tensors(self, device=None):
        """-> ([v2v_ff, v2i_ff, v2i_abs, dest] device tensors, constants): what OptimalAllocation uploads for a host simulator"""
        self._init_device()
        if device is not None and device != self.device:
            raise ValueError("the simulator state lives on %s, the search runs on %s" % (self.device, device))
        return [self._t[k] for k in ('v2v_ff', 'v2i_ff', 'v2i_abs', 'dest')], dict(self.constants)


# ---------------------------------------------------------------------- rollouts of several link counts in one call
def mixed_rollout_bases(pools, T):
    """pools: [(E_k, n_k)] in ascending n; -> (gbase, rbase, ebase, (B, R, Ed)): the first graph / row / edge of every pool in the
    ragged batch of v2x_rollout_steps_mixed (pool-major: T E_j graphs of n_j rows and n_j (n_j - 2) edges for every pool j
    before k) and the batch's totals"""
    gbase, rbase, ebase, B, R, Ed = [], [], [], 0, 0, 0
    for E, n in pools:
        gbase.append(B)
        rbase.append(R)
        ebase.append(Ed)
        B, R, Ed = B + T * E, R + T * E * n, Ed + T * E * n * (n - 2)
    return gbase, rbase, ebase, (B, R, Ed)


def mixed_rollout_buffers(channels, T):
    """the ragged batch a mixed rollout of these DeviceChannels with blocks of T scores -- xe [R, 16], graph_off [B + 1],
    row_ptr [R + 1], col_idx [Ed], q [R, rb], written by the call -- made once per ((E_k, n_k)..., T) and owned by the FIRST
    pool's DeviceChannels: stable pointers, released with that object, and two sets of simulators never share a buffer
    (16 R and Ed are 32-bit sizes of a batch: ValueError beyond)"""
    dc0 = channels[0]
    dc0._init_device()
    key = (tuple((dc.E, dc.n) for dc in channels), int(T))
    buf = dc0._mixed.get(key)
    if buf is None:
        t = dc0.torch
        _, _, _, (B, R, Ed) = mixed_rollout_bases(key[0], T)
        if R * XE_WIDTH >= 2 ** 31 or Ed >= 2 ** 31:
            raise ValueError("rollout_steps_mixed: %d rows and %d edges exceed the 32-bit sizes of a batch" % (R, Ed))
        i32 = lambda k: t.zeros(k, dtype=t.int32, device=dc0.device)       # noqa: E731
        buf = dc0._mixed[key] = {
            'xe': t.zeros((R, XE_WIDTH), dtype=t.float32, device=dc0.device), 'graph_off': i32(B + 1), 'row_ptr': i32(R + 1),
            'col_idx': i32(max(Ed, 1)), 'q': t.zeros((R, dc0.rb), dtype=t.float32, device=dc0.device), 'sizes': (B, R, Ed)}
    return buf


def _check_mixed_pools(who, channels, per_pool):
    channels = list(channels)
    if not 1 <= len(channels) <= MIXED_MAX_POOLS:
        raise ValueError("%s: 1..%d pools, got %d" % (who, MIXED_MAX_POOLS, len(channels)))
    for name, arg in per_pool.items():
        if len(arg) != len(channels):
            raise ValueError("%s: one %s per pool expected, got %d for %d pools" % (who, name, len(arg), len(channels)))
    sizes = [dc.n for dc in channels]
    if any(b <= a for a, b in zip(sizes, sizes[1:])):
        raise ValueError("%s: the pools' link counts must ascend strictly, got %s" % (who, sizes))
    if len(set(dc.rb for dc in channels)) != 1:
        raise ValueError("%s: one channel count for all pools, got %s" % (who, [dc.rb for dc in channels]))
    return channels


def _mixed_pools_ready(who, channels):
    """every pool of a mixed call initialised, all on one device, every observation resident"""
    for dc in channels:
        dc._init_device()
        if dc.device != channels[0].device:
            raise ValueError("%s: the pools live on %s and %s" % (who, channels[0].device, dc.device))
        if not dc._obs_ready:
            raise RuntimeError("%s: no observe() since the last step() (pool of %d links)" % (who, dc.n))


def _mixed_batch_pointers(m, channels, T, names=('xe', 'graph_off', 'row_ptr', 'col_idx', 'q')):
    """the ragged batch of mixed_rollout_buffers(channels, T) (and its Q rows) into the fields `names` of the mixed struct m"""
    buf = mixed_rollout_buffers(channels, T)
    for name in names:
        setattr(m, name, buf[name].data_ptr())


def _mixed_traj_ws(channels, T):
    """the v2x_traj_ws table of a mixed wide walk: every pool supplies the wide and split workspaces its own single-size calls
    use (cached in the pool's _rollout_io(T): they outlive the call)"""
    table = (TrajWs * len(channels))()
    for k, dc in enumerate(channels):
        ws, ss = dc._wide_workspace(T), dc._split_workspace(T)
        table[k] = TrajWs(ws.data_ptr(), ws.numel(), ss.data_ptr(), ss.numel())
    return table


def _mixed_trajectory_call(serial, wide, m, channels, T, walk):
    """the library call of a mixed trajectory struct m in the form `walk` names: serial(m, stream), or with 'wide'
    wide(m, _mixed_traj_ws, stream).  Counted per pool as _trajectory_call counts: the mixed wide walk is a wide call whose stream
    phase is split.  Afterwards every pool's observation is resident."""
    dc0 = channels[0]
    for dc in channels:
        dc._keep_actions = dc._t['actions']
    if walk == 'wide':
        check(dc0._lib, wide(C.byref(m), _mixed_traj_ws(channels, T), dc0._stream()))
    else:
        check(dc0._lib, serial(C.byref(m), dc0._stream()))
    for dc in channels:
        dc.walk_calls[walk] += 1
        dc._traj_form.pop(T, None)
        if walk == 'wide':
            dc.stream_phase_calls['split'] += 1
        dc._obs_ready = True


def _check_mixed_envs(who, envs, per_pool, streams_first=True):
    """what the resident_*_mixed wrappers refuse of their lists before anything else -> envs; streams_first: the evaluation
    wrappers ask streams='device' of every environment here, before their shape checks"""
    envs = list(envs)
    for name, arg in per_pool.items():
        if len(arg) != len(envs):
            raise ValueError("%s: one %s per environment expected, got %d for %d environments" % (who, name, len(arg), len(envs)))
    for env in envs if streams_first else ():
        if getattr(env, 'stream_backend', None) != 'device':
            raise ValueError("%s needs streams='device' in every environment (mobility and the MT19937 streams advance inside the "
                             "call)" % who)
    return envs


def rollout_steps_mixed(channels, explore, random_actions, storages, heads, capacities, v2v_weight, v2i_weight, engine=None,
                        power=None, walk='serial'):
    """DeviceChannels.rollout_steps for several link counts in ONE library call (v2x_rollout_steps_mixed): channels is one
    DeviceChannels per link count in ascending size, and explore [T, E_k], random_actions [T, E_k, n_k], storages, heads and
    capacities are lists with pool k's argument of rollout_steps in place k (the same T everywhere).  One launch walks every
    simulator of every pool, one forward of a variable_graphs `engine` scores all their observations as one ragged batch
    (None: nobody is greedy anywhere, no forward), one launch picks, pays and stores every transition into its own pool's
    slots.  Per pool the bits of its own rollout_steps, given the same Q-values.  Every pool keeps its own policy upload and
    result download.  walk='wide': six launches over all pools' steps in the walk launch's place (v2x_rollout_steps_mixed_wide,
    the same bits).  -> [RolloutResult] per pool, the downloads in flight."""
    who = "rollout_steps_mixed"
    check_walk(who, walk)
    per_pool = dict(explore=explore, random_actions=random_actions, storages=storages, heads=heads, capacities=capacities)
    channels = _check_mixed_pools(who, channels, per_pool)
    T = _block_length(explore[0])
    checked = []
    for k, dc in enumerate(channels):
        if _block_length(explore[k]) != T:
            raise ValueError("%s: pool %d (%d links) has a block of %d iterations, pool 0 of %d"
                             % (who, k, dc.n, _block_length(explore[k]), T))
        checked.append(dc._check_rollout(who, T, explore[k], random_actions[k], storages[k], heads[k], capacities[k]))
    if engine is not None and not (engine.spec.variable_graphs and engine.spec.n_channels == channels[0].rb):
        raise ValueError("%s: scoring needs a variable_graphs engine of %d channels" % (who, channels[0].rb))
    _mixed_pools_ready(who, channels)
    table = (RolloutTraj * len(channels))()
    ios = []
    for k, (dc, (ex, ra)) in enumerate(zip(channels, checked)):
        io = dc._rollout_io(T)
        dc._upload_policy(io, ra, ex)
        table[k] = dc.rollout_steps_struct(T, storages[k], heads[k], capacities[k], v2v_weight, v2i_weight, engine=None, power=power)
        ios.append(io)
    m = RolloutMixed(n_pools=len(channels), T=T, pools=table, model=None)
    if engine is not None:
        m.model = engine._h
        _mixed_batch_pointers(m, channels, T)
    lib = channels[0]._lib
    _mixed_trajectory_call(lib.v2x_rollout_steps_mixed, lib.v2x_rollout_steps_mixed_wide, m, channels, T, walk)
    return [dc._download_result(io, T) for dc, io in zip(channels, ios)]


def resident_rollout_steps_mixed(envs, explore, random_actions, storages, heads, capacities, v2v_weight, v2i_weight, engine=None,
                                 walk='serial'):
    """rollout_steps_mixed() on the resident states of one DeviceBatchedEnviron (streams='device') per link count, ascending
    size: the bookkeeping of DeviceBatchedEnviron.rollout_steps around every environment, the ONE library call in the middle.
    -> [RolloutResult] per environment, the downloads in flight."""
    who = "rollout_steps_mixed"
    check_walk(who, walk)
    per_pool = dict(explore=explore, random_actions=random_actions, storages=storages, heads=heads, capacities=capacities)
    envs = _check_mixed_envs(who, envs, per_pool, streams_first=False)     # (each environment's _resident_before asks it)
    channels = [env._resident_before(who, lambda dc, k=k: dc.check_rollout_steps(explore[k], random_actions[k], storages[k], heads[k],
                                                                                 capacities[k]))
                for k, env in enumerate(envs)]
    results = rollout_steps_mixed(channels, explore, random_actions, storages, heads, capacities, v2v_weight, v2i_weight, engine=engine,
                                  walk=walk)
    for env, result in zip(envs, results):
        env._resident_after(result)
    return results


def _check_eval_mixed(who, channels, explore, policy_random, baseline_actions):
    """what eval_steps_mixed refuses of its lists, before any device work -> (channels, T, [check_eval_steps] per pool)"""
    channels = _check_mixed_pools(who, channels, dict(explore=explore, policy_random=policy_random, baseline_actions=baseline_actions))
    T = _block_length(explore[0])
    checked = []
    for k, dc in enumerate(channels):
        if _block_length(explore[k]) != T:
            raise ValueError("%s: pool %d (%d links) has a block of %d steps, pool 0 of %d" % (who, k, dc.n, _block_length(explore[k]), T))
        if (baseline_actions[k] is None) != (baseline_actions[0] is None):
            raise ValueError("%s: pool %d (%d links) has %s baseline_actions, pool 0 has %s: one number of schemes for all pools"
                             % (who, k, dc.n, "no" if baseline_actions[k] is None else "", "none" if baseline_actions[0] is None else "them"))
        try:
            checked.append(dc.check_eval_steps(explore[k], policy_random[k], baseline_actions[k]))
        except ValueError as err:
            raise ValueError("%s: pool %d (%d links): %s" % (who, k, dc.n, err))
    return channels, T, checked


def eval_steps_mixed(channels, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=None, power=None,
                     walk='serial'):
    """DeviceChannels.eval_steps for several link counts in ONE library call (v2x_eval_steps_mixed): channels is one
    DeviceChannels per link count in ascending size, and explore [T, E_k], policy_random [T, E_k, n_k] and baseline_actions
    [T, E_k, n_k] (None in every place: no baseline scheme) are lists with pool k's argument of eval_steps in place k (the
    same T everywhere).  One launch walks every simulator of every pool, one forward of a variable_graphs `engine` scores all
    their observations as one ragged batch (None: nobody is greedy anywhere, no forward), one launch pays both schemes of
    every (pool, t, e).  Per pool the bits of its own eval_steps, given the same Q-values.  Every pool keeps its own policy
    upload and result download.  walk='wide': six launches over all pools' steps in the walk launch's place
    (v2x_eval_steps_mixed_wide, the same bits).  Afterwards every pool's trajectory_states(T) holds its T snapshots.
    -> [EvalResult] per pool, the downloads in flight."""
    who = "eval_steps_mixed"
    check_walk(who, walk)
    channels, T, checked = _check_eval_mixed(who, channels, explore, policy_random, baseline_actions)
    if engine is not None and not (engine.spec.variable_graphs and engine.spec.n_channels == channels[0].rb):
        raise ValueError("%s: scoring needs a variable_graphs engine of %d channels" % (who, channels[0].rb))
    _mixed_pools_ready(who, channels)
    baseline = checked[0][3] is not None
    table = (Eval * len(channels))()
    ios = []
    for k, (dc, (_, ex, ra, ba)) in enumerate(zip(channels, checked)):
        io = dc._eval_io(T)
        dc._eval_upload(io, T, ex, ra, ba)
        table[k] = dc.eval_steps_struct(T, v2v_weight, v2i_weight, engine=None, power=power, baseline=baseline)
        ios.append(io)
    m = EvalMixed(n_pools=len(channels), T=T, pools=table, model=None)
    if engine is not None:
        m.model = engine._h
        _mixed_batch_pointers(m, channels, T)
    lib = channels[0]._lib
    _mixed_trajectory_call(lib.v2x_eval_steps_mixed, lib.v2x_eval_steps_mixed_wide, m, channels, T, walk)
    return [dc._eval_download(io, T, 2 if baseline else 1) for dc, io in zip(channels, ios)]


def resident_evaluate_steps_mixed(envs, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=None,
                                  walk='serial'):
    """eval_steps_mixed() on the resident states of one DeviceBatchedEnviron (streams='device') per link count, ascending size:
    the bookkeeping of DeviceBatchedEnviron.evaluate_steps around every environment, the ONE library call in the middle.
    Afterwards env.trajectory_states(T) of every environment holds that pool's T snapshots.
    -> [EvalResult] per environment, the downloads in flight."""
    who = "eval_steps_mixed"
    check_walk(who, walk)
    envs = _check_mixed_envs(who, envs, dict(explore=explore, policy_random=policy_random, baseline_actions=baseline_actions))
    _check_eval_mixed(who, [_PoolShape(env) for env in envs], explore, policy_random, baseline_actions)   # before any device work
    channels = [env._resident_before(who, lambda dc, k=k: dc.check_eval_steps(explore[k], policy_random[k], baseline_actions[k]))
                for k, env in enumerate(envs)]
    results = eval_steps_mixed(channels, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=engine, walk=walk)
    for env, result in zip(envs, results):
        env._resident_after(result)
    return results


def mixed_sweep_q(channels, T, K):
    """the Q workspace [K, R, rb] of a sweep of K networks over the ragged batch of mixed_rollout_buffers(channels, T), made once
    per (K, T) and kept with that batch"""
    buf = mixed_rollout_buffers(channels, T)
    q = buf.setdefault('sweep_q', {}).get(K)
    if q is None:
        dc0 = channels[0]
        q = buf['sweep_q'][K] = dc0.torch.zeros((K, buf['sizes'][1], dc0.rb), dtype=dc0.torch.float32, device=dc0.device)
    return q


def _check_sweep_engines(who, engines, K, rb, n=None):
    """what a sweep refuses of its networks, before any device work -> K.  n None: variable_graphs engines of rb channels (the
    mixed sweep); n given: fixed-size engines of n links and rb channels (the receiver-form sweep)"""
    if engines is None:
        K = 1 if K is None else int(K)
    else:
        engines = list(engines)
        if K is not None and int(K) != len(engines):
            raise ValueError("%s: K = %d, but %d engines" % (who, K, len(engines)))
        K = len(engines)
    if not 1 <= K <= SWEEP_MAX_MODELS:
        raise ValueError("%s: 1..%d networks, got %d" % (who, SWEEP_MAX_MODELS, K))
    for k, engine in enumerate(engines or ()):
        spec = None if engine is None else engine.spec
        if n is None and (spec is None or not (spec.variable_graphs and spec.n_channels == rb)):
            raise ValueError("%s: scoring needs variable_graphs engines of %d channels (engine %d)" % (who, rb, k))
        if n is not None and (spec is None or spec.variable_graphs or spec.n_nodes != n or spec.n_channels != rb):
            raise ValueError("%s: scoring needs fixed-size engines of %d links and %d channels (engine %d)" % (who, n, rb, k))
        if engine.spec != engines[0].spec:
            raise ValueError("%s: engine %d has another spec than engine 0: the networks of a sweep are checkpoints of one network"
                             % (who, k))
    return K


def eval_sweep_mixed(channels, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=None, K=None, power=None,
                     walk='serial'):
    """eval_steps_mixed for K networks on the SAME steps in ONE library call (v2x_eval_sweep_mixed): the arguments of
    eval_steps_mixed with a list of K variable_graphs `engines` of one spec in the engine's place (None: nobody is greedy
    anywhere, no forward; K then says how many identical policy schemes the result holds, default 1).  One walk (walk='wide':
    the six launches of the mixed wide walk), one assembly, K forwards of the one ragged batch into the Q workspace of
    mixed_sweep_q, one finish launch: scheme k < K is engine k's policy on the shared explore flags and random actions, scheme
    K the baseline (when given).  The resident state afterwards is the one engine K - 1's own eval_steps_mixed leaves.
    -> [EvalResult] per pool with K (+ 1) schemes, the downloads in flight."""
    who = "eval_sweep_mixed"
    check_walk(who, walk)
    channels, T, checked = _check_eval_mixed(who, channels, explore, policy_random, baseline_actions)
    K = _check_sweep_engines(who, engines, K, channels[0].rb)
    _mixed_pools_ready(who, channels)
    baseline = checked[0][3] is not None
    S = K + (1 if baseline else 0)
    table = (Eval * len(channels))()
    blocks = []
    for k, (dc, (_, ex, ra, ba)) in enumerate(zip(channels, checked)):
        io, sw = dc._sweep_io(T, S)
        dc._eval_upload(io, T, ex, ra, ba)
        table[k] = dc.eval_steps_struct(T, v2v_weight, v2i_weight, engine=None, power=power, baseline=baseline)
        offs, _ = eval_result_layout(dc.E, dc.n, dc.rb, T, S)
        for name, o in offs.items():                     # the sweep's own result block, S schemes
            setattr(table[k], 'result_' + name, sw['dev'].data_ptr() + o)
        blocks.append(sw)
    m = EvalSweep(base=EvalMixed(n_pools=len(channels), T=T, pools=table, model=None), K=K, pad_=0, models=None, q=None)
    if engines is not None:
        _mixed_batch_pointers(m.base, channels, T, ('xe', 'graph_off', 'row_ptr', 'col_idx'))
        handles = (C.c_void_p * K)(*[engine._h for engine in engines])
        m.models = handles
        m.q = mixed_sweep_q(channels, T, K).data_ptr()
    sweep = channels[0]._lib.v2x_eval_sweep_mixed            # (one entry point: a null workspace table asks for the serial walk)
    _mixed_trajectory_call(lambda s, stream: sweep(s, None, stream), sweep, m, channels, T, walk)
    return [dc._sweep_download(sw, T, S) for dc, sw in zip(channels, blocks)]


def resident_evaluate_sweep_mixed(envs, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=None, K=None,
                                  walk='serial'):
    """eval_sweep_mixed() on the resident states of one DeviceBatchedEnviron (streams='device') per link count, ascending size:
    the bookkeeping of resident_evaluate_steps_mixed around every environment, the ONE library call in the middle.  Afterwards
    env.trajectory_states(T) of every environment holds that pool's T snapshots.
    -> [EvalResult] per environment with K (+ 1) schemes, the downloads in flight."""
    who = "eval_sweep_mixed"
    check_walk(who, walk)
    envs = _check_mixed_envs(who, envs, dict(explore=explore, policy_random=policy_random, baseline_actions=baseline_actions))
    _check_eval_mixed(who, [_PoolShape(env) for env in envs], explore, policy_random, baseline_actions)   # before any device work
    if envs:
        _check_sweep_engines(who, engines, K, envs[0].n_RB)
    channels = [env._resident_before(who, lambda dc, k=k: dc.check_eval_steps(explore[k], policy_random[k], baseline_actions[k]))
                for k, env in enumerate(envs)]
    results = eval_sweep_mixed(channels, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=engines, K=K,
                               walk=walk)
    for env, result in zip(envs, results):
        env._resident_after(result)
    return results


class _PoolShape(object):
    """what the argument checks of a mixed call read of a DeviceChannels, taken from an environment whose device side may not
    exist yet: the checks then run before the first environment's state is touched"""

    def __init__(self, env):
        self.E, self.n, self.rb = env.E, env.n_Veh, env.n_RB

    def check_eval_steps(self, explore, policy_random, baseline_actions):
        return DeviceChannels.check_eval_steps(self, explore, policy_random, baseline_actions)

    def check_observe(self, n, C_, rb=None):
        return DeviceChannels.check_observe(n, C_, rb)

    def _check_mobility(self, who, mobility):
        return None


class _ResetRow(object):
    """what a device reset knows of the observation it left resident: the regularity flags (the part of a RolloutResult that
    DeviceBatchedEnviron.resident_regular reads)"""

    def __init__(self, regular):
        self.resident_regular = regular


# attribute of BatchedEnviron -> (device tensor, host shape from (E, n, rb))
_DEVICE_ARRAYS = {
    '_v2i_shadow': ('v2i_shadow', lambda E, n, rb: (E, n)),
    '_v2v_shadow': ('v2v_shadow', lambda E, n, rb: (E, n, n)),
    'V2V_channels_abs': ('v2v_abs', lambda E, n, rb: (E, n, n)),
    'V2I_channels_abs': ('v2i_abs', lambda E, n, rb: (E, n)),
    'V2V_channels_with_fastfading': ('v2v_ff', lambda E, n, rb: (E, n, n, rb)),
    'V2I_channels_with_fastfading': ('v2i_ff', lambda E, n, rb: (E, n, rb)),
    'V2V_Interference_all': ('interf_db', lambda E, n, rb: (E, n, 1, rb)),
}


def _device_array(attr):
    tensor, shape_of = _DEVICE_ARRAYS[attr]

    def get(self):
        a = self._host.get(attr)
        if a is None:
            if attr not in self._on_device:
                raise AttributeError(attr)
            dc = self.device_channels
            a = dc.download(tensor).reshape(shape_of(dc.E, dc.n, dc.rb))
            self._host[attr] = a
        # the caller may write into the array it was handed (new_random_game does): it goes up again before the next device call
        self._dirty.add(attr)
        return a

    def set(self, value):
        self._host[attr] = np.asarray(value, np.float64)
        self._dirty.add(attr)

    return property(get, set)


# the state v2x_sim_stream advances: attribute of BatchedEnviron -> device tensor
_STREAM_ARRAYS = {'_mt_keys': 'keys', '_mt_pos': 'mtpos', 'pos': 'pos', 'dirs': 'dirs'}


def _stream_array(attr):
    def get(self):
        self._settle_streams()
        if self.stream_backend == 'device':
            # (as above: the caller may write into what it is handed -- the library's draws of a reset do, MTStream does)
            self._streams_dirty = True
        try:
            return self._stream_host[attr]
        except KeyError:
            raise AttributeError(attr)

    def set(self, value):
        self._settle_streams()
        self._stream_host[attr] = value
        self._streams_dirty = True

    return property(get, set)


class DeviceBatchedEnviron(BatchedEnviron):
    """BatchedEnviron with the channel update, the observable interference, the packed observation and the rates on the GPU
    (DeviceChannels).  Same constructor and public surface.  Mobility, receivers and the MT19937 streams stay on the host
    (libv2xsim.so), so positions, directions, receivers and stream states are those of the host simulator bit for bit; the
    channel arrays and rates agree with it to the rounding of the two math libraries.  Per step the uniforms go up and
    xe / mask / col / regular, the rates and the interference side outputs come down.  The six large channel arrays and
    V2V_Interference_all are properties: reading one downloads it (once per step), assigning one uploads it before the next
    device call -- inherited code keeps working, only slower.  The step is the three-call path (no v2xsim_advance, no
    look-ahead: lookahead=True is refused).

    streams='device': mobility and the MT19937 streams live on the device as well (v2x_sim_stream), and act() is ONE
    enqueue, DeviceChannels.advance(actions), followed by the download of the rates and of the observation; per step only
    the actions go up.  Velocities, receivers and the lane grid go up when they change: at a reset (assign `vel` / `dest`
    anywhere else and call new_random_game, or upload them through device_channels).  _mt_keys, _mt_pos, pos and dirs become
    pull-on-read like the channel arrays: a read after a device step downloads all four into the same numpy arrays, in
    place (the MTStream objects are attached to rows of _mt_keys), and marks them as possibly written, so they go up again
    before the next device call.  The host draws of a reset (reset_vehicles, mt_uniforms, sample_dest, anything through an
    MTStream) therefore cost one pull and one push; a step costs none.  Trajectories are those of streams='host' bit for bit.

    reset='device' (needs streams='device' and a lane grid on multiples of 2^-10 below 2^15; the default is 'host'):
    new_random_game is ONE enqueue on the resident state (DeviceChannels.reset) and one small download of velocities,
    receivers, regularity and status flags -- no pull of the streams, no push of the reset's arrays.  Everything is the host
    reset's bit for bit (the initial shadowing to the rounding of the two math libraries) except the receivers of a state where
    a receiver is tied in squared distance with another vehicle: there numpy's argsort leaves an order that depends on its
    build, the device ranks by (squared distance, index); `reset_ties` counts such states (reset_tie_flags).  `reset_stats`
    counts the resets by who ran them: the host runs the reset when the link count changes in that call or a stream holds a
    cached Gaussian.

    Who holds the newer copy of the stream state (keys, positions in the stream, vehicle positions, directions), with
    streams='device' (with streams='host' the host always does and the flags below stay False):

      _streams_ahead   the device's copy is newer: a device step ran.  Set by act() and by the device channel update; cleared
                       by _settle_streams(), which downloads into the same host arrays.
      _streams_dirty   the host's copy may be newer: somebody was handed one of the four arrays (a read settles first, so
                       the two flags are never set together).  Cleared by _flush(), which uploads before a device call.
      _move_pending    renew_positions() was called and its walk has not been made: the next device channel update makes
                       it (stream(mobility=True)); a read of the four arrays, a flush for anything else or a second
                       renew_positions() makes it on the host instead (_settle_streams, after the download if one is due).
      _static_dirty    velocities, receivers or the lane grid changed (a reset, a new DeviceChannels): _flush() uploads them.
      _in_reset        new_random_game() is running: its draws are the host's, so its channel update takes uniforms,
                       velocities and positions from the host like streams='host' and _flush() uploads no stream state
                       (everything goes up once, at the first device call after the reset).

      event                                   ahead  dirty   copies moved
      read / assign one of the four arrays    -> F   -> T    download if ahead (then the pending move, on the host)
      MTStream draw (on_touch)                -> F   -> T    the same
      _flush() before a device call           F      -> F    upload if dirty (not during a reset)
      act(), device channel update            -> T   F       none: the device advances its own copy
      new_random_game()                       -> F   -> T    download if ahead; the upload waits for the next device call
      new_random_game(), reset='device'       -> T   -> F    upload if dirty, then the device resets its own copy"""

    def __init__(self, down_lane, up_lane, left_lane, right_lane, width, height, n_envs=1, seeds=None, workers=None,
                 native=None, lookahead=False, device=0, streams='host', reset='host'):
        if streams not in ('host', 'device'):
            raise ValueError("streams must be 'host' or 'device', got %r" % (streams,))
        if reset not in RESETS:
            raise ValueError("reset must be 'host' or 'device', got %r" % (reset,))
        if reset == 'device':
            if streams != 'device':
                raise ValueError("reset='device' needs streams='device' (the reset draws from the streams where they live)")
            check_reset_grid("reset='device'", np.concatenate([np.asarray(t, np.float64).ravel() for t in
                                                               (up_lane, down_lane, left_lane, right_lane)]), width, height)
        self.reset_backend = reset
        self.reset_stats = {'device': 0, 'host': 0, 'host_cached_gauss': 0, 'host_links_changed': 0}   # resets, by who ran them and why
        self.reset_ties = 0                                    # states a device reset flagged (status bit 0, reset_tie_flags)
        if lookahead:
            raise ValueError("DeviceBatchedEnviron has no look-ahead step (the channel update runs on the GPU); lookahead=True "
                             "is refused")
        if seeds is None:
            raise ValueError("DeviceBatchedEnviron needs one seed per environment (its streams advance in libv2xsim.so)")
        if native is not None and not native:
            raise ValueError("DeviceBatchedEnviron keeps mobility and the random streams in libv2xsim.so: native=False is refused")
        if not native_sim.available():
            raise RuntimeError("DeviceBatchedEnviron needs libv2xsim.so (python -c 'import __graft_entry__ as g; g.build()')")
        self._host, self._dirty, self._on_device = {}, set(), set()
        self._dc = None
        self._dev_obs = None
        self.device_index = int(device)
        self.stream_backend = streams                          # ('streams' is the list of MTStream objects)
        self._stream_host = {}                                 # the host copies of _STREAM_ARRAYS
        self._streams_dirty = False                            # ... may have been written since they last went up
        self._streams_ahead = False                            # ... are older than the device's (a device step ran)
        self._static_dirty = True                              # vel / dest / the lane grid changed (a reset)
        self._move_pending = False                             # renew_positions() waits for the stream call of the channel update
        self._in_reset = False
        self._rate_host = {}                                   # V2I_Interference / V2V_Interference as last computed or assigned
        self._rates_pending = False                            # ... are older than the device's (a resident rollout step ran)
        self._resident_row = None                              # the RolloutResult of the call that made the current observation
        BatchedEnviron.__init__(self, down_lane, up_lane, left_lane, right_lane, width, height, n_envs=n_envs, seeds=seeds,
                                workers=workers, native=True, lookahead=False)
        if streams == 'device':
            for st in self.streams:                            # a draw through an MTStream reads its row of _mt_keys: pull first
                st.on_touch = self._touch_streams

    lookahead = property(lambda self: False, lambda self, v: DeviceBatchedEnviron._no_lookahead(v))

    @staticmethod
    def _no_lookahead(v):
        if v:
            raise ValueError("DeviceBatchedEnviron has no look-ahead step; lookahead=True is refused")

    def _one_call_step(self):
        return False

    def _wide(self, n=None):
        """more links than the packed observation holds (32..128): the resident observation is kept in receiver form"""
        return int(self.n_Veh if n is None else n) > OBSERVE_MAX_LINKS

    def _check_sizes(self, n=None):
        n = self.n_Veh if n is None else n
        if self._wide(n):
            if self.stream_backend != 'device':
                raise ValueError("DeviceBatchedEnviron serves %d..%d links with streams='device' only (the resident observation "
                                 "is then kept in receiver form), got %d links with streams=%r"
                                 % (OBSERVE_MAX_LINKS + 1, RECV_MAX_LINKS, n, self.stream_backend))
            DeviceChannels.check_observe_recv(int(n), int(self.n_RB))
        else:
            DeviceChannels.check_observe(int(n), int(self.n_RB))
        if uniforms_per_step(n, self.n_RB) & 1:
            raise NotImplementedError("odd number of draws per step")

    def _constants(self):
        return dict(p_v2v=float(self.V2V_power_dB_List[self.fixed_v2v_power_index]), p_v2i=float(self.V2I_power_dB),
                    veh_gain=float(self.vehAntGain), bs_gain=float(self.bsAntGain), bs_nf=float(self.bsNoiseFigure),
                    veh_nf=float(self.vehNoiseFigure), sig2=float(self.sig2))

    @property
    def device_channels(self):
        """the DeviceChannels of the current (E, n_Veh, n_RB), every assigned array uploaded"""
        return self._flush()

    # ------------------------------------------------------------------ streams='device': who holds the newer stream state
    def _touch_streams(self):
        self._drop_lookahead()
        self._settle_streams()
        self._streams_dirty = True

    def _settle_streams(self):
        """the host copies of keys / positions / directions are current: a pending move is made, the device's newer state is
        downloaded IN PLACE"""
        if self._streams_ahead:
            self._streams_ahead = False
            got = self._dc.download(*[_STREAM_ARRAYS[k] for k in ('_mt_keys', '_mt_pos', 'pos', 'dirs')])
            for k, a in zip(('_mt_keys', '_mt_pos', 'pos', 'dirs'), got):
                self._stream_host[k][...] = a.reshape(self._stream_host[k].shape)
        if self._move_pending:                                 # renew_positions() without its channel update: the host's walk
            self._move_pending = False
            BatchedEnviron.renew_positions(self)

    def _flush(self, settle=True, before_reset=False):
        """before_reset: a device reset follows, which writes velocities and receivers itself (only the lane grid goes up)"""
        E, n, rb = self.E, self.n_Veh, self.n_RB
        if settle and self._move_pending:
            self._settle_streams()
        dc = self._dc
        if dc is None or (dc.E, dc.n, dc.rb) != (E, n, rb):
            self._check_sizes()
            if self._streams_ahead:                            # (the old shape's device state is the newer one: keep it)
                self._settle_streams()
            dc = self._dc = DeviceChannels(E, n, rb, device=self.device_index, constants=self._constants())
            self._on_device = set()
            self._dirty = set(k for k in self._host if self._host[k] is not None)
            self._streams_dirty = self._static_dirty = True
        if self.stream_backend == 'device' and not self._in_reset:   # (a reset's channel update takes everything from the host)
            if self._static_dirty:
                p = self._proto
                dc.set_grid((p.up_lanes, p.down_lanes, p.left_lanes, p.right_lanes), p.width, p.height, p.timestep)
                if not before_reset:
                    dc.upload('vel', self.vel)
                    dc.upload('dest', self.dest)
                dc._obs_ready = False                          # (new receivers: the resident observation is of the old ones)
                self._static_dirty = False
            if self._streams_dirty and not self._streams_ahead:
                for k in ('_mt_keys', '_mt_pos', 'pos', 'dirs'):
                    dc.upload(_STREAM_ARRAYS[k], self._stream_host[k])
                self._streams_dirty = False
        for attr in sorted(self._dirty):
            tensor, shape_of = _DEVICE_ARRAYS[attr]
            a = self._host[attr]
            if a.size != int(np.prod(shape_of(E, n, rb))):
                if attr in ('_v2i_shadow', '_v2v_shadow'):
                    raise ValueError("%s of shape %s does not fit %d environments of %d links" % (attr, list(a.shape), E, n))
                self._host.pop(attr)                       # an array of an earlier episode shape: nothing to keep
                continue
            dc.upload(tensor, a.reshape(dc.shapes()[tensor]))
            self._on_device.add(attr)
        self._dirty = set()
        return dc

    # ------------------------------------------------------------------ the overridden steps
    def new_random_game(self, n_Veh=0):
        """reset='device': the whole reset is one call on the resident state (DeviceChannels.reset) and one small download;
        the host reset runs instead (counted in reset_stats) when the link count changes in this call or a stream holds a
        cached Gaussian, which only the host's generator objects can hand out"""
        self._check_sizes(n_Veh if n_Veh > 0 else self.n_Veh)
        if self.reset_backend == 'device':
            if (n_Veh if n_Veh > 0 else self.n_Veh) > RESET_MAX_LINKS:      # (the device reset holds up to 28 links: the host's runs)
                self.reset_stats['host'] += 1
            elif n_Veh > 0 and n_Veh != self.n_Veh:
                self.reset_stats['host_links_changed'] += 1
            elif any(s.gauss_next is not None for s in self.streams):
                self.reset_stats['host_cached_gauss'] += 1
            else:
                self.reset_stats['device'] += 1
                return self._device_reset()
        else:
            self.reset_stats['host'] += 1
        self._dev_obs = None
        self._resident_row = None
        self._settle_streams()                                 # the reset draws on the host: its copy of the streams first
        if n_Veh > 0 and n_Veh != self.n_Veh:
            self._host, self._dirty, self._on_device, self._dc = {}, set(), set(), None
        self._in_reset = True
        try:
            BatchedEnviron.new_random_game(self, n_Veh)
        finally:
            self._in_reset = False
        self._static_dirty = True                              # new velocities and receivers
        self._dev_obs = None                                   # new receivers

    def _device_reset(self):
        """new_random_game on the resident state: what the host holds newer goes up (a re-seeded stream included), the reset is
        enqueued, the device then holds the newer streams, positions, directions, channels and observation, and velocities,
        receivers, regularity and status flags come down in one download"""
        E, n = self.E, self.n_Veh
        self._drop_lookahead()
        self._obs = None
        self._dev_obs = None
        self._resident_row = None
        if self._stream_host.get('pos') is None or self._stream_host['pos'].shape != (E, n, 2):
            self.pos = np.zeros((E, n, 2))                     # (the host copies a later read downloads into)
            self.dirs = np.zeros((E, n), np.int8)
        dc = self._flush(before_reset=True)
        dc.reset()
        self._streams_ahead = True
        self._static_dirty = False                             # velocities and receivers are the device's own
        self._channels_updated()
        self._on_device.add('V2V_Interference_all')
        vel, dest, regular, status = dc.fetch_reset()
        if np.any(status & RESET_NO_DRAW):
            raise RuntimeError("device reset: a draw of environment(s) %s found no value within 64 words of its stream (the "
                               "generator state is broken)" % np.nonzero(status & RESET_NO_DRAW)[0].tolist())
        self.reset_ties += int(np.count_nonzero(status & RESET_TIE))
        self.vel, self.dest = vel, dest
        self.activate_links = np.ones((E, n, 1), dtype=bool)
        self._resident_row = _ResetRow(regular)

    def renew_positions(self):
        if self.stream_backend != 'device':
            return BatchedEnviron.renew_positions(self)
        # the walk rides on the stream call of the channel update that follows (v2x_sim_stream moves, then draws); anything
        # that looks at the streams or the positions first gets the host's walk (_settle_streams)
        self._drop_lookahead()
        if self._move_pending:                                 # a second move with no channel update in between: the first
            self._settle_streams()                             # one is made on the host (one pull); otherwise nothing moves
        self._move_pending = True

    def _channels_updated(self):
        for attr in _DEVICE_ARRAYS:
            self._host.pop(attr, None)
            if attr != 'V2V_Interference_all':
                self._on_device.add(attr)
        self._on_device.discard('V2V_Interference_all')

    def renew_channels_fastfading(self):
        """renew_channel + fast fading for all environments on the device: the streams' uniforms go up, nothing comes down
        (streams='device': they are drawn there, nothing goes up; during a reset, whose other draws are the host's, they are
        drawn on the host like with streams='host')"""
        n, rb = self.n_Veh, self.n_RB
        self._check_sizes()
        self._drop_lookahead()
        self._obs = None
        self._dev_obs = None
        self._resident_row = None
        if self.stream_backend == 'device' and not self._in_reset:
            if any(s.gauss_next is not None for s in self.streams):
                raise RuntimeError("a stream holds a cached gauss value")
            move, self._move_pending = self._move_pending, False
            dc = self._flush(settle=False)
            dc.stream(mobility=move)
            dc.step(dc.tensor('u'))
            self._streams_ahead = True
            self._channels_updated()
            return
        with self._rng() as rs:
            if any(s.gauss_next is not None for s in rs):
                raise RuntimeError("a stream holds a cached gauss value")
            u = native_sim.mt_uniforms(self._mt_keys, self._mt_pos, uniforms_per_step(n, rb))
        dc = self._flush()
        dc.step(u, self.vel, self.pos)
        self._channels_updated()

    def act(self, actions):
        """rates under `actions`, then one simulator step.  streams='device': one enqueue (DeviceChannels.advance) and the
        downloads of the rates and of the observation; the actions are all that goes up."""
        if self.stream_backend != 'device':
            return BatchedEnviron.act(self, actions)
        self.finish_step()
        E, n = self.E, self.n_Veh
        a = np.asarray(actions)
        if a.dtype.kind not in 'iu':
            raise ValueError("actions must be integers, got dtype %s" % a.dtype)
        if a.size != E * n:
            raise ValueError("actions of shape [%d, %d] or [%d, %d, 1] expected, got %s" % (E, n, E, n, list(a.shape)))
        self._check_sizes()
        if any(s.gauss_next is not None for s in self.streams):
            raise RuntimeError("a stream holds a cached gauss value")
        self._obs = None
        self._resident_row = None
        dc = self._flush()
        if self._wide():                                       # v2x_sim_advance's four launches, the observation in receiver form
            dc.rates(a.reshape(E, n))
            dc.stream(mobility=True)
            dc.step(dc.tensor('u'))
            dc.observe_recv()
        else:
            dc.advance(a.reshape(E, n))
        self._streams_ahead = True
        self._channels_updated()
        self._on_device.add('V2V_Interference_all')
        r = dc.fetch_rates()
        self._rates_pending = False
        self._dev_obs = None if self._wide() else dc.fetch_observation()
        self.V2I_Interference = r['v2i_interf']
        self.V2V_Interference = r['v2v_interf'].reshape(E, n, 1)
        return r['v2v_rate'].reshape(E, n, 1), r['v2i_rate'], r['interference']

    def _resident_rollout(self, steps, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine, row_ptr,
                          walk='serial', stream_phase='chain'):
        """rollout_step() / rollout_steps() (steps): DeviceChannels' call of that name with act()'s bookkeeping around it -- the
        device holds the newer streams and channel arrays, the observable interference is on the device, no host copy of the
        observation exists; V2I_Interference / V2V_Interference download the rates when they are next read"""
        def check_args(dc):
            check_walk('rollout_steps' if steps else 'rollout_step', walk)
            check_stream_phase('rollout_steps' if steps else 'rollout_step', stream_phase, walk)
            (dc.check_rollout_steps if steps else dc.check_rollout)(explore, random_actions, storage, head, capacity)

        def call(dc):
            if steps:
                return dc.rollout_steps(explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=engine,
                                        row_ptr=row_ptr, walk=walk, stream_phase=stream_phase)
            return dc.rollout_step(explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=engine,
                                   row_ptr=row_ptr)

        return self._resident_call('rollout_steps' if steps else 'rollout_step', check_args, call)

    def _resident_call(self, who, check_args, call, receiver_form=False):
        """the bookkeeping every call that steps the resident state shares (rollout_step / rollout_steps / evaluate_steps):
        check_args(dc) raises ValueError before any device work of the call, call(dc) makes it -> its result object.  The two
        halves around the call are methods of their own for a call that steps several environments at once
        (resident_rollout_steps_mixed): every environment's first half, the one call, every environment's second half.
        In receiver form (rollout_steps_recv / evaluate_steps / evaluate_sweep) both get own_receivers() as their second
        argument, as _resident_before took them."""
        if receiver_form:
            dc, own = self._resident_before(who, check_args, True)
            return self._resident_after(call(dc, own))
        return self._resident_after(call(self._resident_before(who, check_args)))

    def _resident_before(self, who, check_args, receiver_form=False):
        """_resident_call up to the library call: everything the device needs is on it, the arguments are checked, the
        observation is resident (receiver_form: in receiver form, as rollout_steps_recv() brings it; the host's look at the
        receivers, own_receivers(), is then taken before they go up and handed to check_args) -> the DeviceChannels; in receiver
        form (the DeviceChannels, own)"""
        if self.stream_backend != 'device':
            raise ValueError("%s needs streams='device' (mobility and the MT19937 streams advance inside the call)" % who)
        self.finish_step()
        self._check_sizes()
        if any(s.gauss_next is not None for s in self.streams):
            raise RuntimeError("a stream holds a cached gauss value")
        if receiver_form:
            own = self.own_receivers()
        stale = bool(self._dirty)
        dc = self._flush()
        if receiver_form:
            check_args(dc, own)
            if stale or not dc._recv_ready:
                dc.observe_recv(self.dest)
        else:
            check_args(dc)
            if stale or not dc._obs_ready:                     # (after a reset: the observation of the new channels, left on the device)
                dc.observe(self.dest)
        self._obs = None
        return (dc, own) if receiver_form else dc

    def _resident_after(self, result):
        """_resident_call after the library call: who holds the newer copy of what -> result"""
        self._streams_ahead = True
        self._channels_updated()
        self._on_device.add('V2V_Interference_all')
        self._dev_obs = None
        self._rates_pending = True
        self._resident_row = result
        return result

    def rollout_step(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None):
        """act() of a whole DQN rollout iteration without the host in the loop (streams='device' only; DeviceChannels.rollout_step):
        the resident observation is scored (engine given), the actions are picked from the host's policy draws, the simulators
        step, and the transitions land in the replay slots -- one call, nothing comes back but the result row (-> RolloutResult,
        its download in flight)."""
        return self._resident_rollout(False, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine,
                                      row_ptr)

    def rollout_steps(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None, row_ptr=None,
                      walk='serial', stream_phase='chain'):
        """T iterations of rollout_step() in one call (explore [T, E], random_actions [T, E, n]; DeviceChannels.rollout_steps):
        the same bookkeeping, once.  walk: 'serial' or 'wide', the form of the trajectory; stream_phase: 'chain' or 'split', the
        form of a wide walk's stream phase (the same bits all).  -> the RolloutResult of the block, its download in flight."""
        return self._resident_rollout(True, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine,
                                      row_ptr, walk, stream_phase)

    def own_receivers(self):
        """[E] int32: the links of every state that are their own receiver, from the host's receivers (0 everywhere unless two
        vehicles stand on one spot); ValueError for a receiver outside [0, n) -- the look the host takes before dest goes up"""
        own, bad = own_receiver_counts(self.dest)
        if bad.any():
            raise ValueError("dest of environment(s) %s holds a receiver outside [0, %d)" % (np.nonzero(bad)[0].tolist(), self.n_Veh))
        return own

    def rollout_steps_recv(self, explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight, engine=None,
                           stream_phase='chain', stream_words='serial'):
        """rollout_steps() for 3..128 links into a ReceiverReplay's storage (DeviceChannels.rollout_steps_recv: the wide walk,
        the closed-form CSR, one forward, one finish -- ONE call), with the same bookkeeping around it.  The resident
        observation is brought into receiver form first when it is not (after a reset, or after a packed-form call).
        stream_phase: 'chain' or 'split', the form of the walk's stream phase (the same bits either way); stream_words: 'serial' or
        'jump', how a split stream phase draws its words (DeviceChannels.rollout_steps_recv; the same bits either way).
        -> the RecvRolloutResult of the block, its download in flight."""
        return self._resident_call(
            'rollout_steps_recv',
            lambda dc, own: dc.check_rollout_steps_recv(explore, random_actions, storage, head, capacity, own, stream_phase, stream_words),
            lambda dc, own: dc.rollout_steps_recv(explore, random_actions, storage, head, capacity, v2v_weight, v2i_weight,
                                                  engine=engine, own=own, stream_phase=stream_phase, stream_words=stream_words),
            receiver_form=True)

    def evaluate_steps(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=None, row_ptr=None,
                       walk='serial', stream_phase='chain', receiver_form=None, stream_words='serial'):
        """The T steps of an evaluation episode in one call (streams='device' only; DeviceChannels.eval_steps) with the
        bookkeeping of rollout_steps() around it: explore [T, E], policy_random [T, E, n], baseline_actions [T, E, n] or None.
        walk: 'serial' or 'wide', the form of the trajectory; stream_phase: 'chain' or 'split', the form of a wide walk's stream
        phase (the same bits all).
        Beyond 31 links the call goes through the receiver form (DeviceChannels.eval_steps_recv, the bookkeeping of
        rollout_steps_recv()): walk must then be 'wide' and row_ptr None; receiver_form=True asks for that form at any size
        (None: by the link count); stream_words: 'serial' or 'jump', how the receiver form's split stream phase draws its words.
        -> the EvalResult (receiver form: RecvEvalResult), its download in flight.  trajectory_states(T) then holds the T
        snapshots."""
        if self._wide() if receiver_form is None else receiver_form:
            return self._evaluate_steps_recv(explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine, row_ptr, walk,
                                             stream_phase, stream_words)
        if stream_words != 'serial':
            check_stream_words('evaluate_steps', stream_words, stream_phase)
            raise ValueError("evaluate_steps: stream_words=%r serves the receiver form only (more than %d links, or receiver_form=True)"
                             % (stream_words, OBSERVE_MAX_LINKS))

        def check_args(dc):
            check_walk('evaluate_steps', walk)
            check_stream_phase('evaluate_steps', stream_phase, walk)
            dc.check_eval_steps(explore, policy_random, baseline_actions)

        return self._resident_call(
            'evaluate_steps', check_args,
            lambda dc: dc.eval_steps(explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=engine, row_ptr=row_ptr,
                                     walk=walk, stream_phase=stream_phase))

    def _evaluate_steps_recv(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine, row_ptr, walk,
                             stream_phase, stream_words='serial'):
        """evaluate_steps() in receiver form: rollout_steps_recv()'s bookkeeping around DeviceChannels.eval_steps_recv"""
        who = 'evaluate_steps'
        if walk != 'wide':
            raise ValueError("%s: the receiver form (more than %d links, or receiver_form=True) walks wide only: pass walk='wide', "
                             "got walk=%r" % (who, OBSERVE_MAX_LINKS, walk))
        if row_ptr is not None:
            raise ValueError("%s: the receiver form writes its own CSR (row_ptr must be None)" % who)
        return self._resident_call(
            who, lambda dc, own: dc.check_eval_steps_recv(explore, policy_random, baseline_actions, own, stream_phase, stream_words),
            lambda dc, own: dc.eval_steps_recv(explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engine=engine, own=own,
                                               stream_phase=stream_phase, stream_words=stream_words),
            receiver_form=True)

    def evaluate_sweep(self, explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=None, K=None,
                       stream_phase='chain', stream_words='serial'):
        """K networks scored on the SAME T steps of an evaluation episode in one call (streams='device', more than 31 links:
        DeviceChannels.eval_sweep_recv) with the bookkeeping of evaluate_steps() in receiver form around it: explore [T, E],
        policy_random [T, E, n], baseline_actions [T, E, n] or None, engines: K fixed-size engines of one spec (None: nobody is
        greedy, K identical policy schemes).  Afterwards the resident state is what engine K - 1's own evaluate_steps() leaves.
        -> the RecvEvalResult of K (+ 1) schemes, its download in flight.  trajectory_states(T) then holds the T snapshots."""
        who = 'evaluate_sweep'
        if not self._wide():
            raise ValueError("%s serves the receiver form only (more than %d links, got %d): MixedAgent.evaluate_training scores the "
                             "checkpoints of a shared-weight network at 3..%d links" % (who, OBSERVE_MAX_LINKS, self.n_Veh,
                                                                                        OBSERVE_MAX_LINKS))
        return self._resident_call(
            who,
            lambda dc, own: dc.check_eval_sweep_recv(explore, policy_random, baseline_actions, engines, K, own, stream_phase, stream_words),
            lambda dc, own: dc.eval_sweep_recv(explore, policy_random, baseline_actions, v2v_weight, v2i_weight, engines=engines, K=K,
                                          own=own, stream_phase=stream_phase, stream_words=stream_words),
            receiver_form=True)

    def trajectory_states(self, T):
        """the T snapshots of the last evaluate_steps() / rollout_steps() of block length T as one stacked search problem
        (DeviceChannels.trajectory_states): valid until the next such call"""
        if self._dc is None:
            raise RuntimeError("trajectory_states: no trajectory call has run")
        if not np.all(np.asarray(self.activate_links)):
            raise ValueError("the optimal-allocation search needs every link active")
        return self._dc.trajectory_states(T)

    def resident_regular(self, n_channels=4):
        """the regularity flags [E] of the CURRENT observation, from wherever they are known without a device call: the host copy
        of the observation, or the result row of the resident step that made it (waits for that row); otherwise one download"""
        if self._dev_obs is not None and not self._dirty:
            return self._dev_obs[3]
        if self._resident_row is not None and not self._dirty:
            return self._resident_row.resident_regular
        return self.observe_packed(n_channels)[3]

    def _pull_rates(self):
        self._rates_pending = False
        r = self._dc.fetch_rates()
        self._rate_host['V2I_Interference'] = r['v2i_interf']
        self._rate_host['V2V_Interference'] = r['v2v_interf'].reshape(self.E, self.n_Veh, 1)

    def _observe_device(self):
        dc = self._flush()
        if self._wide():                                       # 32..128 links: receivers and flags stay on the device, no packed copy
            dc.observe_recv(self.dest)
            self._host.pop('V2V_Interference_all', None)
            self._on_device.add('V2V_Interference_all')
            self._dev_obs = None
            return None
        dc.observe(self.dest)
        self._host.pop('V2V_Interference_all', None)
        self._on_device.add('V2V_Interference_all')
        self._dev_obs = dc.fetch_observation()
        return self._dev_obs

    def Compute_Interference(self, actions):
        """the observable interference in dB (V2V_Interference_all, left on the device) -- and, from the same launch, the
        packed observation the agent asks for next"""
        self.finish_step()
        self._observe_device()

    def observe_packed(self, n_channels=4):
        """(3..31 links, as packed_ok() says: beyond them the resident observation is in receiver form and the agent's view is
        the inherited observe())"""
        self.finish_step()
        DeviceChannels.check_observe(self.n_Veh, int(n_channels), self.n_RB)
        if self._dev_obs is None or self._dirty:
            self._observe_device()
        return self._dev_obs

    def packed_ok(self, n_channels=4):
        return bool(n_channels == self.n_RB and 2 < self.n_Veh <= 31 and self.n_RB <= self.n_Veh and 3 * n_channels + 1 <= 16)

    def compute_reward_with_channel_selection(self, actions):
        self.finish_step()
        E, n = self.E, self.n_Veh
        a = np.asarray(actions)
        if a.dtype.kind not in 'iu':
            raise ValueError("actions must be integers, got dtype %s" % a.dtype)
        if a.size != E * n:
            raise ValueError("actions of shape [%d, %d] or [%d, %d, 1] expected, got %s" % (E, n, E, n, list(a.shape)))
        self._check_sizes()
        dc = self._flush()
        dc.rates(a.reshape(E, n), dest=self.dest)
        r = dc.fetch_rates()
        self._rates_pending = False
        self.V2I_Interference = r['v2i_interf']
        self.V2V_Interference = r['v2v_interf'].reshape(E, n, 1)
        return r['v2v_rate'].reshape(E, n, 1), r['v2i_rate'], r['interference']

    # ------------------------------------------------------------------ for OptimalAllocation
    def problem_tensors(self, device=None):
        """the current state's device arrays for OptimalAllocation (no download, no upload but the receivers)"""
        self.finish_step()
        if not np.all(np.asarray(self.activate_links)):
            raise ValueError("the optimal-allocation search needs every link active")
        dc = self._flush()
        dc.upload('dest', self.dest)
        return dc.problem_tensors(device)


def _rate_array(attr):
    def get(self):
        if self._rates_pending:
            self._pull_rates()
        try:
            return self._rate_host[attr]
        except KeyError:
            raise AttributeError(attr)

    def set(self, value):
        self._rate_host[attr] = value

    return property(get, set)


for _attr in ('V2I_Interference', 'V2V_Interference'):
    setattr(DeviceBatchedEnviron, _attr, _rate_array(_attr))
for _attr in _DEVICE_ARRAYS:
    setattr(DeviceBatchedEnviron, _attr, _device_array(_attr))
for _attr in _STREAM_ARRAYS:
    setattr(DeviceBatchedEnviron, _attr, _stream_array(_attr))
del _attr
