"""GPU: the episode reset on the resident state (v2x_sim_reset / v2x_sim_reset_draw, k_sim_reset_draw of csrc/v2xsimdev.hip)
against the project's CPU library (rl/native_sim.py on libv2xsim.so) and the host reset of rl/batched_env.py.  The draws are
integer or exactly rounded arithmetic: positions, directions, velocities, receivers, key words, stream positions and uniforms
are compared byte for byte.  The initial shadowing goes through the two math libraries' log / sqrt / cos / sin and carries the
tolerance tests/test_gpu_device_sim.py uses for shadowing (rtol 1e-11 / atol 1e-9); dB arrays, rates and xe further down carry
that file's tolerances too (rates rtol 1e-9 / atol 1e-12, xe one float32 ulp).

The seeds below were chosen on the CPU (host library only) so that reset_tie_flags flags no state -- except FLAGGED_SEED, chosen
so that it flags one: a receiver tied in squared distance with another vehicle is where numpy's argsort and the device's
(d2, index) rule may pick different vehicles.  Measured on the CPU over 20,000 host resets each on the project's lane grid:
1.0 % of 20-link resets are flagged (208), 2.0 % at 28 links (398), none at 4."""
import ctypes
import random

import numpy as np
import pytest

from v2xgnn.lib import V2X_EINVAL, OptProblem, SimReset, SimStep, load_library
from v2xgnn.rl import Agent, DeviceBatchedEnviron, DeviceChannels, RL_Config, native_sim
from v2xgnn.rl.device_sim import DEFAULT_CONSTANTS, reset_tie_flags, uniforms_per_step
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

K = DEFAULT_CONSTANTS
CHANNEL_NAMES = ('v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff')
OBS_NAMES = ('interf_db', 'state', 'xe', 'mask', 'col', 'regular')
DRAW_NAMES = ('pos', 'dirs', 'vel', 'dest', 'keys', 'mtpos', 'u')
ALL_NAMES = DRAW_NAMES + CHANNEL_NAMES + OBS_NAMES + ('status',)

# the project's lane grid (rl/train.py start_env_batched)
UP = [3.5 / 2, 3.5 / 2 + 3.5, 250 + 3.5 / 2, 250 + 3.5 + 3.5 / 2, 500 + 3.5 / 2, 500 + 3.5 + 3.5 / 2]
DOWN = [250 - 3.5 - 3.5 / 2, 250 - 3.5 / 2, 500 - 3.5 - 3.5 / 2, 500 - 3.5 / 2, 750 - 3.5 - 3.5 / 2, 750 - 3.5 / 2]
LEFT = [3.5 / 2, 3.5 / 2 + 3.5, 433 + 3.5 / 2, 433 + 3.5 + 3.5 / 2, 866 + 3.5 / 2, 866 + 3.5 + 3.5 / 2]
RIGHT = [433 - 3.5 - 3.5 / 2, 433 - 3.5 / 2, 866 - 3.5 - 3.5 / 2, 866 - 3.5 / 2, 1299 - 3.5 - 3.5 / 2, 1299 - 3.5 / 2]
LANES = (UP, DOWN, LEFT, RIGHT)                          # the step's order; the host reset takes (down, up, left, right)
WIDTH, HEIGHT, RB = 750, 1299, 4

CASES = [(3, 4), (2, 8), (2, 20), (1, 28)]
STARTS = (0, 1, 397, 623, 624)
CASE_SEED = 0                                            # with it the host reset of every (case, start) is free of ties
FLAGGED_SEED, FLAGGED_E, FLAGGED_N = 9, 4, 20            # the first seed from 0 up whose E states hold exactly one flagged state
ENV_SEEDS = {8: 0, 20: 0}                                # start_env_batched seeds whose three resets are free of ties (E = 3 / 2)
TEST_RUN_SEED = 0                                        # ... and whose three resets of one 8-link simulator are


def close_db(a, b):
    return np.allclose(a, b, rtol=1e-11, atol=1e-9)


def seeded_keys(E, seed, start):
    keys = np.stack([np.random.RandomState(1000 * seed + e).get_state()[1] for e in range(E)]).astype(np.uint32)
    return np.ascontiguousarray(keys), np.full(E, start, np.int32)


# ------------------------------------------------------------------------------------------------- the host side (CPU only)
def ranked_candidates(xy, by_index):
    """[e, i, n - 3]: the vehicles of rank 1 .. n - 3 by distance from vehicle i; by_index: ranked by (d2, index) as the device
    does, otherwise by numpy's argsort of np.abs as the host reset does"""
    n = xy.shape[1]
    if by_index:
        dx, dy = xy[:, :, None, 0] - xy[:, None, :, 0], xy[:, :, None, 1] - xy[:, None, :, 1]
        order = np.argsort(dx * dx + dy * dy, axis=2, kind='stable')                 # [e, i, rank]: ties in ascending index
        return np.ascontiguousarray(order[:, :, 1:n - 2])
    z = xy[:, :, 0] + 1j * xy[:, :, 1]
    order = np.argsort(np.abs(z[:, :, None] - z[:, None, :]), axis=1)                # [e, rank, i], as rl/batched_env.py
    return np.ascontiguousarray(order[:, 1:n - 2, :].transpose(0, 2, 1))


def sample_receivers(keys, pos, cand):
    """random.sample(cand[e][i], 1)[0] in link order on the streams, in place: the library's call up to 21 candidates, the
    stdlib generator itself beyond (rl/batched_env.py does the same)"""
    E, n, m = cand.shape
    if m <= 21:
        return native_sim.sample_dest(keys, pos, cand)
    dest = np.zeros((E, n), np.int64)
    for e in range(E):
        gen = random.Random()
        gen.setstate((3, tuple(int(w) for w in keys[e]) + (int(pos[e]),), None))
        for i in range(n):
            dest[e, i] = gen.sample(cand[e, i].tolist(), 1)[0]
        state = gen.getstate()[1]
        keys[e], pos[e] = np.array(state[:624], np.uint32), state[624]
    return dest


def host_reset_draw(keys, pos, n, rb=RB, by_index=False):
    """reset_vehicles, two mt_uniforms calls, argsort + the receiver draw -> dict of what k_sim_reset_draw writes"""
    k, p = keys.copy(), pos.copy()
    xy, dirs, vel = native_sim.reset_vehicles(k, p, n, (DOWN, UP, LEFT, RIGHT), WIDTH, HEIGHT)
    E, n_g = k.shape[0], 2 * (n * n + n)
    ug = native_sim.mt_uniforms(k, p, n_g)
    x2pi = ug[:, 0::2] * (2.0 * np.pi)
    g2rad = np.sqrt(-2.0 * np.log(1.0 - ug[:, 1::2]))
    zg = np.stack([np.cos(x2pi) * g2rad, np.sin(x2pi) * g2rad], axis=2).reshape(E, n_g)
    o = n * n + n
    u = native_sim.mt_uniforms(k, p, uniforms_per_step(n, rb))
    cand = ranked_candidates(xy, by_index)
    host_cand = cand if not by_index else ranked_candidates(xy, False)
    dest = sample_receivers(k, p, host_cand)
    picked = np.argmax(host_cand == dest[:, :, None], axis=2)                        # the draw j of every link
    return dict(pos=xy, dirs=dirs, vel=vel, dest=np.take_along_axis(cand, picked[:, :, None], axis=2)[:, :, 0], host_dest=dest,
                keys=k, mtpos=p, u=u, v2v_shadow=zg[:, o:o + n * n].reshape(E, n, n) * 3.0, v2i_shadow=zg[:, o + n * n:] * 8.0)


def fresh_channels(E, n, keys, pos, rb=RB):
    dc = DeviceChannels(E, n, rb)
    dc.set_grid(LANES, WIDTH, HEIGHT, 0.01)
    dc.upload('keys', keys)
    dc.upload('mtpos', pos)
    return dc


@pytest.fixture(scope="module")
def host_draws():
    """the host side of every (case, start), computed once"""
    out = {}
    for E, n in CASES:
        for start in STARTS:
            keys, pos = seeded_keys(E, CASE_SEED, start)
            out[(E, n, start)] = (keys, pos, host_reset_draw(keys, pos, n))
    return out


# ------------------------------------------------------------------------------------------------- 1. the draw launch
def test_the_chosen_seeds_hold_no_tie_and_cross_block_ends(host_draws):
    for key, (keys, pos, h) in host_draws.items():
        assert not reset_tie_flags(h['pos'], h['dest']).any(), key
        assert np.array_equal(h['dest'], h['host_dest']), key
    # the integer draws of a reset start right at a block end (623: one word left, 624: none) and inside a block
    assert any(np.any(h['mtpos'] < pos) for _, pos, h in host_draws.values())


@pytest.mark.parametrize("E,n", CASES)
def test_reset_draw_is_the_host_librarys_bytes(E, n, host_draws):
    for start in STARTS:
        keys, pos, h = host_draws[(E, n, start)]
        dc = fresh_channels(E, n, keys, pos)
        dc.reset_draw()
        for name, got in zip(DRAW_NAMES, dc.download(*DRAW_NAMES)):
            assert got.shape == h[name].shape and got.tobytes() == h[name].tobytes(), (start, name)
        for name, got in zip(('v2v_shadow', 'v2i_shadow'), dc.download('v2v_shadow', 'v2i_shadow')):
            err = np.abs(got - h[name]).max()
            print("E=%d n=%d start=%d %s max |dev - host| = %.3e" % (E, n, start, name, err))
            assert np.allclose(got, h[name], rtol=1e-11, atol=1e-9), (start, name, err)
        assert not dc.download('status').any(), start


# ------------------------------------------------------------------------------------------------- 2. the whole reset
@pytest.mark.parametrize("E,n", [(3, 4), (2, 20)])
def test_reset_is_its_three_launches_bytewise(E, n):
    keys, pos = seeded_keys(E, CASE_SEED, 397)
    one, pieces = fresh_channels(E, n, keys, pos), fresh_channels(E, n, keys, pos)
    for game in range(2):                                                # the second reset continues the first one's streams
        one.reset()
        pieces.reset_draw()
        pieces.step(pieces.tensor('u'))
        pieces.observe()
        for name, g, w in zip(ALL_NAMES, one.download(*ALL_NAMES), pieces.download(*ALL_NAMES)):
            assert g.tobytes() == w.tobytes(), (game, name)
    vel, dest, regular, status = one.fetch_reset()
    assert vel.tobytes() == one.download('vel').tobytes() and dest.tobytes() == one.download('dest').tobytes()
    assert np.array_equal(regular, one.download('regular').astype(bool)) and np.array_equal(status, one.download('status'))
    assert np.all(np.isfinite(one.download('v2v_ff'))) and np.all(np.isfinite(one.download('xe')))


# ------------------------------------------------------------------------------------------------- 3. a flagged state
def test_a_flagged_state_takes_the_lower_index_and_everything_else_is_the_hosts():
    E, n = FLAGGED_E, FLAGGED_N
    keys, pos = seeded_keys(E, FLAGGED_SEED, 624)
    h = host_reset_draw(keys, pos, n, by_index=True)
    flags = reset_tie_flags(h['pos'], h['host_dest'])
    assert flags.sum() == 1                                              # (a CPU fact of the seed)
    assert np.array_equal(reset_tie_flags(h['pos'], h['dest']), flags)   # either choice among equals is flagged alike
    dc = fresh_channels(E, n, keys, pos)
    dc.reset_draw()
    assert np.array_equal(dc.download('status'), flags)
    got = dict(zip(DRAW_NAMES, dc.download(*DRAW_NAMES)))
    for name in DRAW_NAMES:                                              # 'dest': the (d2, index) candidate of every link
        assert got[name].tobytes() == h[name].tobytes(), name
    # every link whose receiver is tied with nobody has the host's receiver
    dx, dy = h['pos'][:, :, None, 0] - h['pos'][:, None, :, 0], h['pos'][:, :, None, 1] - h['pos'][:, None, :, 1]
    d2 = dx * dx + dy * dy
    tied = (d2 == np.take_along_axis(d2, h['host_dest'][:, :, None], axis=2)).sum(axis=2) > 1
    assert tied.any() and not tied[flags == 0].any()
    assert np.array_equal(got['dest'][~tied], h['host_dest'][~tied])
    for name in ('v2v_shadow', 'v2i_shadow'):
        assert np.allclose(dc.download(name), h[name], rtol=1e-11, atol=1e-9), name


# ------------------------------------------------------------------------------------------------- 4. the environment
@pytest.mark.parametrize("E,n", [(3, 8), (2, 20)])
def test_two_device_resets_then_two_steps_against_the_host_reset(E, n):
    host = start_env_batched(n, E, ENV_SEEDS[n], backend="device", streams="device")
    dev = start_env_batched(n, E, ENV_SEEDS[n], backend="device", streams="device", reset="device")
    assert type(dev) is DeviceBatchedEnviron and (host.reset_backend, dev.reset_backend) == ('host', 'device')
    assert dev.reset_stats == {'device': 0, 'host': 0, 'host_cached_gauss': 0, 'host_links_changed': 1}      # 4 -> n links: the host's
    rng = np.random.default_rng(5)

    def compare(tag):
        assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev.dirs, host.dirs), tag
        assert np.array_equal(dev.dest, host.dest) and np.array_equal(dev.vel, host.vel), tag
        assert np.array_equal(dev._mt_keys, host._mt_keys) and np.array_equal(dev._mt_pos, host._mt_pos), tag
        assert np.array_equal(dev.activate_links, host.activate_links), tag
        for name in ('_v2i_shadow', '_v2v_shadow', 'V2V_channels_abs', 'V2I_channels_abs', 'V2V_channels_with_fastfading',
                     'V2I_channels_with_fastfading'):
            g, w = getattr(dev, name), getattr(host, name)
            assert g.shape == w.shape and close_db(g, w), (tag, name, np.abs(g - w).max())
        xe, mask, col, regular = dev.observe_packed(4)
        h_xe, h_mask, h_col, h_regular = host.observe_packed(4)
        assert np.all(np.abs(xe - h_xe) <= np.spacing(np.maximum(np.abs(xe), np.abs(h_xe)))), tag
        assert np.array_equal(mask, h_mask) and np.array_equal(col, h_col) and np.array_equal(regular, h_regular), tag

    for game in range(2):
        host.new_random_game(n)
        dev.new_random_game(n)
        assert not reset_tie_flags(host.pos, host.dest).any(), game      # (a CPU fact of the seed)
        assert np.array_equal(dev.resident_regular(4), host.observe_packed(4)[3]), game
        compare(("reset", game))
    for t in range(2):
        actions = rng.integers(0, 4, size=(E, n, 1))
        got, want = dev.act(actions), host.act(actions)
        for g, w, name in zip(got, want, ("v2v_rate", "v2i_rate", "interference")):
            assert g.shape == w.shape and np.allclose(g, w, rtol=1e-9, atol=1e-12 if name != "interference" else 0), (t, name)
        compare(("step", t))
    assert dev.reset_stats['device'] == 2 and dev.reset_ties == 0 and host.reset_stats['host'] == 3
    # a cached Gaussian can only be handed out by the host's generator object: that reset is the host's (which refuses the
    # channel update of a stream with a cached value), and is counted; with the cache drawn empty the device resets again
    for env in (host, dev):
        env.streams[0].gauss_array((1,), 1.0)                           # an odd count: the pair's second value stays cached
        assert env.streams[0].gauss_next is not None
        with pytest.raises(RuntimeError, match="cached gauss"):
            env.new_random_game(n)
    assert dev.reset_stats['host_cached_gauss'] == 1 and dev.reset_stats['device'] == 2
    for env in (host, dev):
        env.streams[0].gauss_array((1,), 1.0)
        assert env.streams[0].gauss_next is None
        env.new_random_game(n)
    assert dev.reset_stats['device'] == 3
    if not reset_tie_flags(host.pos, host.dest).any():
        compare("after a cached Gaussian")


def test_a_reseeded_stream_goes_up_before_the_device_reset():
    E, n = 2, 8
    host = start_env_batched(n, E, 3, backend="device", streams="device")
    dev = start_env_batched(n, E, 3, backend="device", streams="device", reset="device")
    for env in (host, dev):
        env.new_random_game(n)
        env._mt_keys[1] = np.random.RandomState(12345).get_state()[1]    # (the device held the newer streams: pulled, then written)
        env._mt_pos[1] = 624
        env.new_random_game(n)
    assert dev.reset_stats['device'] == 2
    assert np.array_equal(dev._mt_keys, host._mt_keys) and np.array_equal(dev._mt_pos, host._mt_pos)
    assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev.vel, host.vel)
    if not reset_tie_flags(host.pos, host.dest).any():
        assert np.array_equal(dev.dest, host.dest)


# ------------------------------------------------------------------------------------------------- 5. the agent
def test_test_run_with_every_step_exploring_is_the_same_under_both_resets():
    n, T, episodes = 8, 3, 2
    policy = np.random.default_rng(9).integers(0, 4, size=(episodes, T, n))

    def run(reset):
        random.seed(TEST_RUN_SEED)
        np.random.seed(TEST_RUN_SEED)
        env = start_env_batched(n, 1, TEST_RUN_SEED, backend="device", streams="device", reset=reset)
        cfg = RL_Config()
        cfg.set_train_value(16, 0.5, 32, 1, 0.1)
        agent = Agent(n, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=TEST_RUN_SEED, device_replay=False)
        inner, seen = agent._device_episode, []

        def exploring(explore, policy_random, baseline, **kw):           # every step explores: the actions are the draws below
            got = inner(np.ones(T, np.uint8), policy[len(seen)], baseline, **kw)
            seen.append(got['res'].actions.copy())
            return got
        agent._device_episode = exploring
        out = agent.test_run(episodes, T, False, eval_backend='device')
        res = dict(out=[np.asarray(a).copy() for a in out], actions=np.stack(seen), rng=np.random.get_state(), py=random.getstate(),
                   streams=[np.array(a).copy() for a in (env._mt_keys, env._mt_pos, env.pos, env.dirs)], stats=dict(agent.eval_stats),
                   resets=dict(env.reset_stats), ties=env.reset_ties)
        agent.brain.close()
        return res

    h, d = run('host'), run('device')
    assert h['stats'] == d['stats'] == {'device_episodes': episodes, 'host_episodes': 0}
    assert d['resets']['device'] == episodes and d['ties'] == 0 and h['resets']['device'] == 0
    assert np.array_equal(h['actions'], d['actions']) and np.array_equal(d['actions'][:, 0, :, 0, :], policy)
    for a, b in zip(h['streams'], d['streams']):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert h['py'] == d['py'] and np.array_equal(h['rng'][1], d['rng'][1]) and h['rng'][2:] == d['rng'][2:]
    for i, (a, b) in enumerate(zip(h['out'], d['out'])):
        assert a.shape == b.shape and np.all(np.isfinite(a)) and np.allclose(a, b, rtol=1e-9, atol=0), i


# ------------------------------------------------------------------------------------------------- 6. entry-point errors
def test_refused_resets_launch_nothing_and_say_why():
    import torch
    lib = load_library()
    E, rb, L = 2, 4, 6
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream().cuda_stream
    full = lambda dt, *s: torch.full(s, 7, dtype=dt, device=dev)        # noqa: E731
    f64 = lambda *s: full(torch.float64, *s)                            # noqa: E731

    def tensors(n):
        n_u = uniforms_per_step(n, rb)
        return dict(keys=full(torch.int32, E, 624), mtpos=full(torch.int32, E), xy=f64(E, n, 2), dirs=full(torch.int8, E, n),
                    vel=f64(E, n), lanes=f64(4, L), u=f64(E, n_u), v2i_shadow=f64(E, n), v2v_shadow=f64(E, n, n), v2v_abs=f64(E, n, n),
                    v2i_abs=f64(E, n), v2v_ff=f64(E, n, n, rb), v2i_ff=f64(E, n, rb), interf_db=f64(E, n, rb),
                    state=f64(E, n, 3 * rb + 1), xe=full(torch.float32, E, n, 16), mask=full(torch.int32, E, n),
                    col=full(torch.int32, E, n * max(n - 2, 1)), regular=full(torch.uint8, E), v2v_rate=f64(E, n), v2i_rate=f64(E, rb),
                    interference=f64(E, rb), v2i_interf=f64(E, rb), v2v_interf=f64(E, n), dest=full(torch.int64, E, n),
                    status=full(torch.uint8, E), other=f64(E, n), other_dest=full(torch.int64, E, n))

    def call(fn, t, n, width=750.0, height=1299.0, n_u=None, vel='vel', dest='dest', status='status', actions=None, n_lanes=L):
        prob = OptProblem(E=E, n=n, rb=rb, pad_=0, v2v_ff=t['v2v_ff'].data_ptr(), v2i_ff=t['v2i_ff'].data_ptr(),
                          v2i_abs=t['v2i_abs'].data_ptr(), dest=t['dest'].data_ptr(), w_v2v=0.0, w_v2i=0.0, **K)
        step = SimStep(problem=prob, n_lanes=n_lanes, n_u=uniforms_per_step(n, rb) if n_u is None else n_u, timestep=0.01, width=width,
                       height=height, power=10.0, actions=actions,
                       **{k: t[k].data_ptr() for k in t if k not in ('dest', 'status', 'other', 'other_dest')})
        r = SimReset(step=step, vel=t[vel].data_ptr() if vel else None, dest=t[dest].data_ptr() if dest else None,
                     status=t[status].data_ptr() if status else None)
        return fn(ctypes.byref(r), stream)

    texts = []
    for fn in (lib.v2x_sim_reset, lib.v2x_sim_reset_draw):
        mine = []
        for n in (6, 2, 32):
            t = tensors(n)
            assert call(fn, t, n) == V2X_EINVAL, n
            text = lib.v2x_last_error(None).decode()
            assert "n = %d" % n in text and "multiple of 4 in 4..28" in text, text
            mine.append(text)
            torch.cuda.synchronize()
            assert all(bool((x == 7).all()) for x in t.values()), n
        t = tensors(8)
        for kwargs, words in ((dict(width=750.5), "integral"), (dict(height=-1.0), "integral"), (dict(width=2.0 ** 31), "integral"),
                              (dict(vel='other'), "vel must be the step's own vel"),
                              (dict(dest='other_dest'), "dest must be the problem's own dest"), (dict(status=None), "status"),
                              (dict(n_u=uniforms_per_step(8, rb) + 2), "n_u"), (dict(n_u=3 * (8 * 8 + 8)), "n_u"),
                              (dict(actions=t['mask'].data_ptr()), "actions must be NULL"), (dict(n_lanes=0), "n_lanes"),
                              (dict(n_lanes=65), "n_lanes")):
            assert call(fn, t, 8, **kwargs) == V2X_EINVAL, kwargs
            text = lib.v2x_last_error(None).decode()
            assert words in text, (kwargs, text)
            mine.append(text)
        assert fn(None, stream) == V2X_EINVAL
        torch.cuda.synchronize()
        for name, x in t.items():                                        # nothing ran: every tensor still holds its fill value
            assert bool((x == 7).all()), name
        texts.append(mine)
    for mine in texts:                                                   # every refusal has its own message
        assert len(set(mine)) == len(mine), mine
