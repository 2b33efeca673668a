"""GPU: mobility and the MT19937 streams on the device (v2x_sim_stream, k_sim_stream of csrc/v2xsimdev.hip) and the one-call
step v2x_sim_advance, against the project's CPU library (rl/native_sim.py on libv2xsim.so).  Both are integer or exactly
rounded arithmetic, so positions, directions, key words, stream positions and uniforms are compared byte for byte; channel
arrays and rates carry the tolerances tests/test_gpu_device_sim.py uses for them (dB arrays rtol 1e-11 / atol 1e-9, rates
rtol 1e-9 / atol 1e-12, xe one float32 ulp)."""
import ctypes
import random

import numpy as np
import pytest

from v2xgnn.lib import V2X_EINVAL, OptProblem, SimStep, load_library
from v2xgnn.rl import Agent, BatchedEnviron, DeviceBatchedEnviron, DeviceChannels, RL_Config, native_sim
from v2xgnn.rl.device_sim import DEFAULT_CONSTANTS, uniforms_per_step
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

K = DEFAULT_CONSTANTS
CHANNEL_NAMES = ('v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff')
RATE_NAMES = ('v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf')
STREAM_NAMES = ('keys', 'mtpos', 'pos', 'dirs')

# the project's lane grid (rl/train.py start_env_batched), tables in the order of native_sim.positions: up, down, left, right
UP = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
DOWN = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
LEFT = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
RIGHT = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
LANES = (UP, DOWN, LEFT, RIGHT)
WIDTH, HEIGHT = 750.0, 1299.0


def close_db(a, b):
    return np.allclose(a, b, rtol=1e-11, atol=1e-9)


def seeded_keys(E, seed, start=None):
    """keys [E, 624] of np.random.RandomState(seed + e) and positions: 624 (the state right after seeding) or `start`"""
    keys = np.stack([np.random.RandomState(seed + e).get_state()[1] for e in range(E)]).astype(np.uint32)
    pos = np.full(E, 624, np.int32) if start is None else np.asarray(start, np.int32).copy()
    assert keys.shape == (E, 624) and pos.shape == (E,)
    return np.ascontiguousarray(keys), pos


# ------------------------------------------------------------------------------------------------- the device call, bare
def dev_stream(keys, mtpos, n_u, xy=None, dirs=None, vel=None, timestep=0.01, calls=1):
    """`calls` consecutive v2x_sim_stream calls on device copies -> per call (keys, mtpos, u, xy, dirs) as numpy"""
    import torch
    lib = load_library()
    dev = torch.device('cuda', 0)
    E = keys.shape[0]
    t_keys = torch.from_numpy(keys.view(np.int32).copy()).to(dev)
    t_pos = torch.from_numpy(mtpos.copy()).to(dev)
    t_u = torch.full((E, n_u), -1.0, dtype=torch.float64, device=dev)
    t_xy = t_dirs = t_vel = t_lanes = None
    n = 1
    if xy is not None:
        n = xy.shape[1]
        t_xy, t_dirs, t_vel = (torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev) for a in (xy, dirs, vel))
        t_lanes = torch.from_numpy(np.array(LANES, np.float64)).to(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None            # noqa: E731
    out = []
    for _ in range(calls):
        rc = lib.v2x_sim_stream(E, n, ptr(t_keys), ptr(t_pos), ptr(t_xy), ptr(t_dirs), ptr(t_vel), timestep, len(UP) if xy is not None else 0,
                                ptr(t_lanes), WIDTH, HEIGHT, ptr(t_u), n_u, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.v2x_last_error(None)
        torch.cuda.synchronize()
        out.append((t_keys.cpu().numpy().view(np.uint32), t_pos.cpu().numpy(), t_u.cpu().numpy(),
                    None if xy is None else t_xy.cpu().numpy(), None if xy is None else t_dirs.cpu().numpy()))
    return out


# ------------------------------------------------------------------------------------------------------- 1. uniforms only
STARTS = (0, 1, 226, 227, 396, 397, 622, 623, 624)
N_US = (2, 312, 314, 84, 180, 3780)


@pytest.mark.parametrize("E", [1, 3, 70])
def test_uniforms_are_the_host_librarys_bytes_from_every_start_position(E):
    for n_u in N_US:
        for shift in range(1 if E >= len(STARTS) else len(STARTS)):
            start = [STARTS[(e + shift) % len(STARTS)] for e in range(E)]
            keys, pos = seeded_keys(E, 1000 + 7 * E, start)
            h_keys, h_pos = keys.copy(), pos.copy()
            got = dev_stream(keys, pos, n_u, calls=2)                     # the second call continues the first
            for call in range(2):
                want = native_sim.mt_uniforms(h_keys, h_pos, n_u)
                g_keys, g_pos, g_u = got[call][:3]
                tag = (n_u, start, call)
                assert g_u.tobytes() == want.tobytes(), tag
                assert g_pos.tobytes() == h_pos.tobytes(), (tag, g_pos, h_pos)
                assert g_keys.tobytes() == h_keys.tobytes(), tag


def test_uniforms_ending_exactly_at_a_block_end_do_not_regenerate():
    keys, pos = seeded_keys(2, 5, [0, 312])
    (g_keys, g_pos, g_u, _, _), = dev_stream(keys, pos, 312)
    assert g_pos[0] == 624 and np.array_equal(g_keys[0], keys[0])        # consumed to the end: the block stays as it is
    assert g_pos[1] == 312 and not np.array_equal(g_keys[1], keys[1])    # 312 + 624 words: one regeneration
    rs = np.random.RandomState(5)                                        # and numpy's own generator agrees with the state
    rs.set_state(('MT19937', keys[0], 0))
    assert np.array_equal(rs.random_sample(312), g_u[0])
    assert rs.get_state()[2] == 624 and np.array_equal(rs.get_state()[1], g_keys[0])


# ------------------------------------------------------------------------------------------------------- 2. mobility
def crafted(E, n, seed, scale=1.0, timestep=0.01):
    """positions / directions / velocities: most vehicles within one step of a crossing lane (every third exactly on it), every
    fifth within one step of the map edge it drives towards (all four directions come up over the states)"""
    rng = np.random.default_rng(seed)
    xy = np.zeros((E, n, 2))
    dirs = np.zeros((E, n), np.int8)
    vel = rng.integers(10, 16, size=(E, n)).astype(np.float64) * scale
    for e in range(E):
        for v in range(n):
            d = int(rng.integers(0, 4)) if v % 5 else (v // 5 + e) % 4
            dv = vel[e, v] * timestep
            sg = 1.0 if d in (0, 3) else -1.0
            ax = 1 if d < 2 else 0
            span = (WIDTH, HEIGHT)
            if v % 5 == 0:                                               # about to leave the map
                a = (span[ax] - 0.5 * dv) if sg > 0 else 0.5 * dv
            else:
                tabs = (LEFT + RIGHT) if ax == 1 else (UP + DOWN)
                lane = tabs[int(rng.integers(0, len(tabs)))]
                # on the lane, within one step of it, or (every fourth) within two steps: about half of those reach nothing
                frac = 0.0 if v % 3 == 0 else float(rng.random()) * (2.0 if v % 4 == 1 else 1.0)
                a = lane - sg * frac * dv
            xy[e, v, ax] = a
            xy[e, v, 1 - ax] = float(rng.random()) * span[1 - ax]
            dirs[e, v] = d
    return xy, dirs, vel


def words_between(before, after):
    """words a state consumed (fewer than 624) from its positions before and after"""
    return (int(after) - (0 if before >= 624 else int(before))) % 624 if after != before else 0


def host_walk(keys, pos, xy, dirs, vel, timestep):
    """native_sim.positions on copies -> (keys, mtpos, xy, dirs, draws [E, n]: 53-bit draws of every vehicle).  The walk is
    sequential, so the draws of vehicle v are those of the first v + 1 vehicles less those of the first v."""
    E, n = dirs.shape
    k, p, x, d = keys.copy(), pos.copy(), xy.copy(), dirs.copy()
    native_sim.positions(k, p, x, d, vel, timestep, LANES, WIDTH, HEIGHT)
    cum = np.zeros((E, n + 1), np.int64)
    for m in range(1, n + 1):
        kk, pp = keys.copy(), pos.copy()
        native_sim.positions(kk, pp, xy[:, :m].copy(), dirs[:, :m].copy(), vel[:, :m].copy(), timestep, LANES, WIDTH, HEIGHT)
        cum[:, m] = [words_between(pos[e], pp[e]) // 2 for e in range(E)]
    return k, p, x, d, np.diff(cum, axis=1)


def walk_facts(xy, dirs, vel, timestep, h_xy, h_dirs, draws):
    """what happened in a host walk: turns, draws without a turn, re-entries per direction, the largest draw count"""
    E, n = dirs.shape
    sg = np.where((dirs == 0) | (dirs == 3), 1.0, -1.0)
    ax = np.where(dirs < 2, 1, 0)
    straight = xy.copy()
    moved = np.take_along_axis(xy, ax[..., None], axis=2)[..., 0]
    dv = vel * timestep
    np.put_along_axis(straight, ax[..., None], np.where(sg > 0, moved + dv, moved - dv)[..., None], axis=2)
    out = (straight[..., 0] < 0) | (straight[..., 1] < 0) | (straight[..., 0] > WIDTH) | (straight[..., 1] > HEIGHT)
    turned = ~out & np.any(h_xy != straight, axis=2)
    reentry = [int(np.sum(out & (dirs == d) & (h_dirs == new))) for d, new in ((0, 3), (1, 2), (2, 0), (3, 1))]
    return dict(turns=int(turned.sum()), failed_draws=int(draws.sum() - (turned & (draws > 0)).sum()), reentry=reentry,
                most_draws=int(draws.max()), per_state=draws.sum(axis=1))


MOBILITY_CASES = [(E, n, variant) for (E, n) in ((1, 4), (3, 20), (2, 31)) for variant in ("step", "tenth", "x30", "boundary")]
# the seed of a case's states and streams: the first from 0 up, tried on the CPU, with which the facts asserted below hold
MOBILITY_SEEDS = {(1, 4, "x30"): 4}


def mobility_case(E, n, variant):
    timestep = 0.1 if variant == "tenth" else 0.01
    scale = 30.0 if variant == "x30" else 1.0
    seed = MOBILITY_SEEDS.get((E, n, variant), 0)
    xy, dirs, vel = crafted(E, n, seed, scale, timestep)
    start = [623 if e % 2 == 0 else 621 for e in range(E)] if variant == "boundary" else None
    keys, pos = seeded_keys(E, 300 + seed, start)
    return keys, pos, xy, dirs, vel, timestep


@pytest.fixture(scope="module")
def host_walks():
    out = {}
    for E, n, variant in MOBILITY_CASES:
        keys, pos, xy, dirs, vel, timestep = mobility_case(E, n, variant)
        res = host_walk(keys, pos, xy, dirs, vel, timestep)
        out[(E, n, variant)] = res[:4] + (walk_facts(xy, dirs, vel, timestep, res[2], res[3], res[4]),)
    return out


def test_the_crafted_states_make_the_host_turn_draw_reenter_and_cross_a_block(host_walks):
    reentry = np.zeros(4, np.int64)
    for (E, n, variant), (_, h_pos, _, _, f) in host_walks.items():
        print(E, n, variant, f)
        assert f['turns'] >= 1 and f['failed_draws'] >= 1, (E, n, variant, f)
        reentry += f['reentry']
        if n >= 20:
            assert np.all(np.array(f['reentry']) >= 1), (E, n, variant, f)            # a re-entry in each direction
        if variant == "x30":
            assert f['most_draws'] >= 2, (E, n, f)
        if E > 1:
            assert len(set(f['per_state'].tolist())) > 1, (E, n, variant, f)          # unequal draw counts between states
        if variant == "boundary":
            assert np.all(h_pos < 100) and np.all(f['per_state'] >= 2), (h_pos, f)    # every state crossed the block boundary
    assert np.all(reentry >= 1), reentry


@pytest.mark.parametrize("E,n,variant", MOBILITY_CASES)
def test_mobility_is_the_host_librarys_walk_bytewise(host_walks, E, n, variant):
    keys, pos, xy, dirs, vel, timestep = mobility_case(E, n, variant)
    h_keys, h_pos, h_xy, h_dirs, _ = host_walks[(E, n, variant)]
    h_keys, h_pos = h_keys.copy(), h_pos.copy()
    want_u = native_sim.mt_uniforms(h_keys, h_pos, 2)                    # (a call draws at least one pair)
    (g_keys, g_pos, g_u, g_xy, g_dirs), = dev_stream(keys, pos, 2, xy, dirs, vel, timestep)
    assert g_dirs.tobytes() == h_dirs.tobytes(), (g_dirs, h_dirs)
    assert g_xy.tobytes() == h_xy.tobytes(), np.abs(g_xy - h_xy).max()
    assert g_pos.tobytes() == h_pos.tobytes(), (g_pos, h_pos)
    assert g_keys.tobytes() == h_keys.tobytes() and g_u.tobytes() == want_u.tobytes()


# ------------------------------------------------------------------------------------------------------- 3. both, chained
@pytest.mark.parametrize("E,n,rb,scale", [(3, 20, 4, 1.0), (2, 4, 4, 30.0)])
def test_mobility_then_uniforms_chained_five_calls(E, n, rb, scale):
    xy, dirs, vel = crafted(E, n, 77 + n, scale)
    keys, pos = seeded_keys(E, 900 + n, [620 - 3 * e for e in range(E)])
    n_u = uniforms_per_step(n, rb)
    dc = DeviceChannels(E, n, rb)
    dc.set_grid(LANES, WIDTH, HEIGHT, 0.01)
    for name, a in zip(STREAM_NAMES + ('vel',), (keys, pos, xy, dirs, vel)):
        dc.upload(name, a)
    h_keys, h_pos, h_xy, h_dirs = keys.copy(), pos.copy(), xy.copy(), dirs.copy()
    for call in range(5):
        native_sim.positions(h_keys, h_pos, h_xy, h_dirs, vel, 0.01, LANES, WIDTH, HEIGHT)
        want_u = native_sim.mt_uniforms(h_keys, h_pos, n_u)
        dc.stream(mobility=True)
        g_keys, g_pos, g_xy, g_dirs, g_u = dc.download(*(STREAM_NAMES + ('u',)))
        assert g_keys.dtype == np.uint32 and g_keys.tobytes() == h_keys.tobytes(), call
        assert g_pos.tobytes() == h_pos.tobytes(), (call, g_pos, h_pos)
        assert g_xy.tobytes() == h_xy.tobytes() and g_dirs.tobytes() == h_dirs.tobytes(), call
        assert g_u.tobytes() == want_u.tobytes(), call
    dc.stream(mobility=False)                                            # no mobility: nobody moves, the stream goes on
    want_u = native_sim.mt_uniforms(h_keys, h_pos, n_u)
    g_keys, g_pos, g_xy, g_dirs, g_u = dc.download(*(STREAM_NAMES + ('u',)))
    assert g_xy.tobytes() == h_xy.tobytes() and g_dirs.tobytes() == h_dirs.tobytes()
    assert g_u.tobytes() == want_u.tobytes() and g_keys.tobytes() == h_keys.tobytes() and g_pos.tobytes() == h_pos.tobytes()


# ------------------------------------------------------------------------------------------------------- 4. v2x_sim_advance
def make_dest(E, n, seed):
    rng = np.random.default_rng(seed)
    dest = (np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n
    assert np.all(dest != np.arange(n))
    return dest.astype(np.int64)


def start_state(E, n, rb, seed):
    rng = np.random.default_rng(seed)
    xy, dirs, vel = crafted(E, n, seed + 1)
    keys, pos = seeded_keys(E, seed + 2, [600 + 5 * e for e in range(E)])
    return dict(keys=keys, mtpos=pos, pos=xy, dirs=dirs, vel=vel, dest=make_dest(E, n, seed + 3),
                v2i_shadow=rng.normal(0.0, 8.0, (E, n)), v2v_shadow=rng.normal(0.0, 3.0, (E, n, n)))


def start_channels(E, n, rb, st):
    """a DeviceChannels holding the state `st`, one channel update made (so there are channels to pay rates on)"""
    dc = DeviceChannels(E, n, rb)
    dc.set_grid(LANES, WIDTH, HEIGHT, 0.01)
    for name, a in st.items():
        dc.upload(name, a)
    dc.stream(mobility=False)
    dc.step(dc.tensor('u'))
    return dc


ALL_NAMES = CHANNEL_NAMES + ('interf_db', 'state', 'xe', 'mask', 'col', 'regular') + RATE_NAMES + STREAM_NAMES + ('u',)


@pytest.mark.parametrize("E,n,rb", [(3, 4, 4), (2, 20, 4)])
def test_advance_is_the_four_separate_device_calls_bytewise(E, n, rb):
    st = start_state(E, n, rb, 40 + n)
    one, four = start_channels(E, n, rb, st), start_channels(E, n, rb, st)
    rng = np.random.default_rng(3)
    for step in range(3):
        actions = rng.integers(0, rb, size=(E, n))
        one.advance(actions)
        four.rates(actions)
        four.stream(mobility=True)
        four.step(four.tensor('u'))
        four.observe()
        for name, g, w in zip(ALL_NAMES, one.download(*ALL_NAMES), four.download(*ALL_NAMES)):
            assert g.tobytes() == w.tobytes(), (step, name)
    before = one.download(*RATE_NAMES)
    one.advance(None)                                                    # no actions: no rates, the rest of the step
    four.stream(mobility=True)
    four.step(four.tensor('u'))
    four.observe()
    for name, g, w in zip(ALL_NAMES, one.download(*ALL_NAMES), four.download(*ALL_NAMES)):
        assert g.tobytes() == w.tobytes(), name
    for g, w in zip(one.download(*RATE_NAMES), before):
        assert g.tobytes() == w.tobytes()


def host_advance(E, n, rb, h):
    """native_sim.advance (v2xsim_advance) in place on the host state h"""
    tabs = [np.ascontiguousarray(np.asarray(t, np.float64)) for t in LANES]
    out = {"v2v_abs": np.empty((E, n, n)), "v2i_abs": np.empty((E, n)), "v2v_ff": np.empty((E, n, n, rb)), "v2i_ff": np.empty((E, n, rb)),
           "interf_db": np.empty((E, n, 1, rb)), "state": np.empty((E, n, 3 * rb + 1)), "adj": np.empty((E, n, n)),
           "xe": np.empty((E, n, 16), np.float32), "mask": np.empty((E, n), np.int32), "col": np.empty((E, n * (n - 2)), np.int32),
           "regular": np.empty(E, np.uint8), "scratch": np.empty((E, 2 * uniforms_per_step(n, rb)))}
    a = native_sim.AdvanceArgs()
    a.E, a.n, a.rb, a.n_lanes = E, n, rb, len(tabs[0])
    a.timestep, a.width, a.height = 0.01, WIDTH, HEIGHT
    a.p_v2v, a.p_v2i, a.veh_gain, a.veh_nf, a.sig2 = K['p_v2v'], K['p_v2i'], K['veh_gain'], K['veh_nf'], K['sig2']
    a.up, a.down, a.left, a.right = (t.ctypes.data for t in tabs)
    a.vel, a.dest = h['vel'].ctypes.data, h['dest'].ctypes.data
    for k, name in (("keys", "keys"), ("mtpos", "mtpos"), ("xy", "pos"), ("dirs", "dirs"), ("v2i_shadow", "v2i_shadow"),
                    ("v2v_shadow", "v2v_shadow")):                       # in place: input and output are the same arrays
        setattr(a, k, h[name].ctypes.data)
        setattr(a, k + "_in", h[name].ctypes.data)
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    native_sim.advance(a)
    h.update({k: out[k] for k in ("v2v_abs", "v2i_abs", "v2v_ff", "v2i_ff", "interf_db", "state", "xe", "mask", "col", "regular")})
    return h


@pytest.mark.parametrize("E,n,rb", [(3, 4, 4), (2, 20, 4)])
def test_advance_against_the_host_librarys_advance_and_reward(E, n, rb):
    st = start_state(E, n, rb, 60 + n)
    dc = start_channels(E, n, rb, st)
    h = {k: np.ascontiguousarray(v).copy() for k, v in st.items()}
    u = native_sim.mt_uniforms(h['keys'], h['mtpos'], uniforms_per_step(n, rb))                  # start_channels' update
    (h['v2i_shadow'], h['v2v_shadow'], h['v2v_abs'], h['v2i_abs'], h['v2v_ff'], h['v2i_ff']) = native_sim.channels(
        u, h['vel'], h['pos'], h['v2i_shadow'], h['v2v_shadow'], rb)
    rng = np.random.default_rng(4)
    for step in range(3):
        actions = rng.integers(0, rb, size=(E, n))
        want = native_sim.reward(actions.astype(np.int64), h['dest'], h['v2v_ff'], h['v2i_ff'], h['v2i_abs'], K['p_v2v'], K['p_v2i'],
                                 K['veh_gain'], K['bs_gain'], K['bs_nf'], K['veh_nf'], K['sig2'])
        h = host_advance(E, n, rb, h)
        dc.advance(actions)
        r = dc.fetch_rates()
        xe, mask, col, regular = dc.fetch_observation()
        for name in STREAM_NAMES:
            assert dc.download(name).tobytes() == h[name].tobytes(), (step, name)
        for name in CHANNEL_NAMES:
            g = dc.download(name)
            assert g.shape == h[name].shape and close_db(g, h[name]), (step, name, np.abs(g - h[name]).max())
        assert np.allclose(r['v2v_rate'], want[0][:, :, 0], rtol=1e-9, atol=1e-12), step
        assert np.allclose(r['v2i_rate'], want[1], rtol=1e-9, atol=1e-12), step
        assert np.allclose(r['interference'], want[2], rtol=1e-9, atol=0), step
        assert np.allclose(r['v2i_interf'], want[3], rtol=1e-9, atol=0), step
        assert np.allclose(r['v2v_interf'], want[4][:, :, 0], rtol=1e-9, atol=0), step
        assert np.all(np.abs(xe - h['xe']) <= np.spacing(np.maximum(np.abs(xe), np.abs(h['xe'])))), step
        assert np.array_equal(mask, h['mask']) and np.array_equal(col, h['col']), step
        assert np.array_equal(regular, h['regular'].astype(bool)), step


# ------------------------------------------------------------------------------------------------------- 5. entry-point errors
def test_stream_and_advance_errors_launch_nothing():
    import torch
    lib = load_library()
    E, n, rb, L = 2, 4, 4, 6
    n_u = uniforms_per_step(n, rb)
    dev = torch.device('cuda', 0)
    full = lambda dt, *s: torch.full(s, 7, dtype=dt, device=dev)        # noqa: E731
    f64 = lambda *s: full(torch.float64, *s)                            # noqa: E731
    t = dict(keys=full(torch.int32, E, 624), mtpos=full(torch.int32, E), xy=f64(E, n, 2), dirs=full(torch.int8, E, n), vel=f64(E, n),
             lanes=f64(4, L), u=f64(E, n_u), v2i_shadow=f64(E, n), v2v_shadow=f64(E, n, n), v2v_abs=f64(E, n, n), v2i_abs=f64(E, n),
             v2v_ff=f64(E, n, n, rb), v2i_ff=f64(E, n, rb), interf_db=f64(E, n, rb), state=f64(E, n, 3 * rb + 1),
             xe=full(torch.float32, E, n, 16), mask=full(torch.int32, E, n), col=full(torch.int32, E, n * (n - 2)),
             regular=full(torch.uint8, E), v2v_rate=f64(E, n), v2i_rate=f64(E, rb), interference=f64(E, rb), v2i_interf=f64(E, rb),
             v2v_interf=f64(E, n))
    dest = torch.zeros((E, n), dtype=torch.int64, device=dev)
    actions = torch.zeros((E, n), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def sim_stream(E_=E, n_u_=n_u, n_lanes_=L, null=()):
        p = {k: (None if k in null else t[k].data_ptr()) for k in ('keys', 'mtpos', 'xy', 'dirs', 'vel', 'lanes', 'u')}
        return lib.v2x_sim_stream(E_, n, p['keys'], p['mtpos'], p['xy'], p['dirs'], p['vel'], 0.01, n_lanes_, p['lanes'], 750.0, 1299.0,
                                  p['u'], n_u_, stream)

    def sim_advance(E_=E, n_u_=n_u, n_lanes_=L, null=()):
        prob = OptProblem(E=E_, n=n, rb=rb, pad_=0, v2v_ff=t['v2v_ff'].data_ptr(), v2i_ff=t['v2i_ff'].data_ptr(),
                          v2i_abs=t['v2i_abs'].data_ptr(), dest=dest.data_ptr(), w_v2v=0.0, w_v2i=0.0, **K)
        s = SimStep(problem=prob, n_lanes=n_lanes_, n_u=n_u_, timestep=0.01, width=750.0, height=1299.0, power=10.0,
                    actions=actions.data_ptr(), **{k: (None if k in null else v.data_ptr()) for k, v in t.items()})
        return lib.v2x_sim_advance(ctypes.byref(s), stream)

    cases = ((dict(null=('keys',)), "null"), (dict(null=('dirs',)), "null"), (dict(E_=0), "E = 0"), (dict(n_u_=n_u + 1), "n_u"),
             (dict(n_lanes_=0), "n_lanes"))
    for call in (sim_stream, sim_advance):
        for kwargs, word in cases:
            assert call(**kwargs) == V2X_EINVAL, (call.__name__, kwargs)
            assert word in lib.v2x_last_error(None).decode(), (call.__name__, kwargs, lib.v2x_last_error(None))
    assert sim_advance(n_u_=n_u + 2) == V2X_EINVAL and "n_u" in lib.v2x_last_error(None).decode()      # even, but not this step's
    assert sim_advance(null=('xe',)) == V2X_EINVAL and "null" in lib.v2x_last_error(None).decode()
    assert lib.v2x_sim_advance(None, stream) == V2X_EINVAL
    torch.cuda.synchronize()
    for name, x in t.items():                                            # nothing ran: every tensor still holds its fill value
        assert bool((x == 7).all()), name


# ------------------------------------------------------------------------------------------------------- 6. capture
def test_advance_replays_from_a_captured_graph_bitwise():
    import torch
    E, n, rb = 3, 4, 4
    st = start_state(E, n, rb, 80)
    rng = np.random.default_rng(6)
    actions = [rng.integers(0, rb, size=(E, n)).astype(np.int32) for _ in range(3)]
    names = CHANNEL_NAMES + ('interf_db', 'state', 'xe', 'mask', 'col', 'regular') + RATE_NAMES + STREAM_NAMES
    eager, results = start_channels(E, n, rb, st), []
    for a in actions:
        eager.advance(a)
        results.append([x.copy() for x in eager.download(*names)])

    dc = start_channels(E, n, rb, st)
    a_t = torch.zeros((E, n), dtype=torch.int32, device=torch.device('cuda', 0))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # captured once (capture runs nothing)
        dc.advance(a_t)
    for k in range(3):                                                   # replayed with new actions in the same buffer
        a_t.copy_(torch.from_numpy(actions[k]))
        graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(names, dc.download(*names), results[k]):
            assert got.tobytes() == want.tobytes(), (k, name)


# ------------------------------------------------------------------------------------------------------- 7. the environment
@pytest.mark.parametrize("n,steps", [(4, 6), (20, 2)])
def test_device_streams_environment_against_the_host_environment(n, steps):
    E = 3
    host = start_env_batched(n, E, 77, lookahead=False)
    dev = start_env_batched(n, E, 77, backend="device", streams="device")
    assert type(host) is BatchedEnviron and type(dev) is DeviceBatchedEnviron and dev.stream_backend == 'device'
    rng = np.random.default_rng(5)
    keys_array = dev._mt_keys

    def compare(tag):
        assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev.dirs, host.dirs), tag
        assert np.array_equal(dev.dest, host.dest) and np.array_equal(dev.vel, host.vel), tag
        assert np.array_equal(dev._mt_keys, host._mt_keys) and np.array_equal(dev._mt_pos, host._mt_pos), tag
        assert dev._mt_keys is keys_array, tag                           # pulled in place: the MTStream rows stay attached
        for name in ('_v2i_shadow', '_v2v_shadow', 'V2V_channels_abs', 'V2I_channels_abs', 'V2V_channels_with_fastfading',
                     'V2I_channels_with_fastfading'):
            g, w = getattr(dev, name), getattr(host, name)
            assert g.shape == w.shape and close_db(g, w), (tag, name, np.abs(g - w).max())
        xe, mask, col, regular = dev.observe_packed(4)
        h_xe, h_mask, h_col, h_regular = host.observe_packed(4)
        assert np.all(np.abs(xe - h_xe) <= np.spacing(np.maximum(np.abs(xe), np.abs(h_xe)))), tag
        assert np.array_equal(mask, h_mask) and np.array_equal(col, h_col) and np.array_equal(regular, h_regular), tag

    def step(tag):
        actions = rng.integers(0, 4, size=(E, n, 1))
        got, want = dev.act(actions), host.act(actions)
        for g, w, name in zip(got, want, ("v2v_rate", "v2i_rate", "interference")):
            assert g.shape == w.shape, name
            assert np.allclose(g, w, rtol=1e-9, atol=1e-12 if name != "interference" else 0), (tag, name)
        assert np.allclose(dev.V2I_Interference, host.V2I_Interference, rtol=1e-9, atol=0)
        assert np.allclose(dev.V2V_Interference, host.V2V_Interference, rtol=1e-9, atol=0)

    compare("reset")
    for t in range(steps):
        step(t)
        compare(t)
        assert np.allclose(dev.V2V_Interference_all, host.V2V_Interference_all, rtol=1e-11, atol=1e-10), t
    step("unread")                                                       # two steps with nothing read in between ...
    step("unread 2")
    compare("unread 2")
    host.new_random_game(n)                                              # the reset's host draws pull and push the stream state
    dev.new_random_game(n)
    compare("second game")
    for t in range(2):
        step(("second game", t))
        compare(("second game", t))
    # steady state: only the actions go up, the rates group and the observation group come down
    step("settle")                                                       # (the reads of compare() go up once more)
    dc = dev.device_channels
    # each group comes down as one buffer whose fields start at multiples of 64 bytes: five fp64 rate arrays [E, n], [E, rb],
    # [E, rb], [E, rb], [E, n] (min(rb, n) = rb here); xe [E, n, 16] float32, mask [E, n] int32, col [E, n (n - 2)] int32, regular [E]
    rb = 4
    pad = lambda nbytes: (nbytes + 63) // 64 * 64                      # noqa: E731
    down = (sum(pad(8 * E * k) for k in (n, rb, rb, rb, n))
            + pad(4 * E * n * 16) + pad(4 * E * n) + pad(4 * E * n * (n - 2)) + pad(E))
    for t in range(3):
        before = dict(dc.traffic)
        step(("steady", t))
        assert dc.traffic['bytes_up'] - before['bytes_up'] == E * n * 4, t
        assert dc.traffic['bytes_down'] - before['bytes_down'] == down, t
    compare("end")


def test_device_streams_environment_separate_renew_calls_are_the_hosts():
    """renew_positions / renew_channels_fastfading called one by one, with and without a look at the positions in between"""
    E, n = 3, 4
    host = start_env_batched(n, E, 31, lookahead=False)
    dev = start_env_batched(n, E, 31, backend="device", streams="device")
    for look in (False, True, False):
        host.renew_positions()
        dev.renew_positions()
        if look:
            assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev._mt_pos, host._mt_pos)
        host.renew_channels_fastfading()
        dev.renew_channels_fastfading()
        assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev.dirs, host.dirs)
        assert np.array_equal(dev._mt_keys, host._mt_keys) and np.array_equal(dev._mt_pos, host._mt_pos)
        assert close_db(dev.V2V_channels_with_fastfading, host.V2V_channels_with_fastfading)


# ------------------------------------------------------------------------------------------------------- 8. the agent
def test_agent_trains_on_the_device_streams_environment_with_the_host_runs_draws_and_actions():
    def episode(backend, streams):
        random.seed(21)
        np.random.seed(21)
        env = start_env_batched(4, 3, 21, lookahead=False, backend=backend, streams=streams)
        cfg = RL_Config()
        cfg.set_train_value(16, 0.5, 64, 1, 0.1)
        agent = Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=21, device_replay=True)
        out = agent.train(1, 2)
        rep = agent.device_replay
        rep.flush()
        return env, agent, out, rep.action[:rep.size].cpu().numpy(), np.random.get_state()

    env_d, ag_d, out_d, act_d, rs_d = episode("device", "device")
    env_h, ag_h, out_h, act_h, rs_h = episode("host", "host")
    assert type(env_d) is DeviceBatchedEnviron and env_d.stream_backend == 'device' and type(env_h) is BatchedEnviron
    assert ag_d.num_step == ag_h.num_step > 0 and act_d.shape == act_h.shape and act_d.shape[0] > 0
    assert np.all(np.isfinite(out_d[0])) and np.all(np.isfinite(out_d[1]))
    assert np.array_equal(act_d, act_h)
    assert rs_d[0] == rs_h[0] and np.array_equal(rs_d[1], rs_h[1]) and rs_d[2:] == rs_h[2:]
    assert np.array_equal(env_d.pos, env_h.pos) and np.array_equal(env_d._mt_keys, env_h._mt_keys)
