"""GPU: the simulator's channel step, observation and rates on the device (v2x_sim_* of csrc/v2xsimdev.hip through
rl/device_sim.py) against the project's CPU library (rl/native_sim.py on libv2xsim.so), with the tolerances
tests/test_rl_batched_env.py uses for the same quantities: dB arrays and shadowing rtol 1e-11 / atol 1e-9, rates rtol 1e-9 /
atol 1e-12, interference in dB rtol 1e-11 / atol 1e-10, linear interference rtol 1e-9 / atol 0."""
import ctypes
import random

import numpy as np
import pytest

from v2xgnn.lib import V2X_EINVAL, OptProblem, load_library
from v2xgnn.rl import Agent, BatchedEnviron, DeviceBatchedEnviron, DeviceChannels, OptimalAllocation, RL_Config, native_sim
from v2xgnn.rl.device_sim import DEFAULT_CONSTANTS, uniforms_per_step
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

K = DEFAULT_CONSTANTS
W_V2V, W_V2I = 1.0, 0.1
CHANNEL_NAMES = ('v2i_shadow', 'v2v_shadow', 'v2v_abs', 'v2i_abs', 'v2v_ff', 'v2i_ff')

# crafted neighbours, consecutive points form the pairs: identical points; 2 m, 5 m and 10 m apart on one street (x <= 3,
# x < d_bp = 6.67 and beyond); d1 < 7 <= d2; both >= 7 with one leg > 400 m (the n_j clamp at 1.84)
CRAFTED = np.array([[100.0, 200.0], [100.0, 200.0], [100.0, 202.0], [100.0, 207.0], [100.0, 217.0], [103.0, 277.0],
                    [10.0, 10.0], [30.0, 600.0], [500.0, 90.0], [508.0, 1000.0], [250.0, 250.0], [252.0, 250.0]])


def close_db(a, b):
    return np.allclose(a, b, rtol=1e-11, atol=1e-9)


def make_inputs(E, n, rb, seed):
    """uniforms (one shadowing pair at u = 0, one at the largest double below 1), velocities, positions (random on the
    750 x 1299 grid, the first vehicles of state e on the crafted points from 2 e on) and shadowing states"""
    rng = np.random.default_rng(seed)
    u = rng.random((E, uniforms_per_step(n, rb)))
    u[:, 0:2] = 0.0
    u[:, 2:4] = np.nextafter(1.0, 0.0)
    vel = rng.integers(10, 16, size=(E, n)).astype(np.float64)
    pos = rng.random((E, n, 2)) * np.array([750.0, 1299.0])
    for e in range(E):
        k = min(n, len(CRAFTED))
        pos[e, :k] = np.roll(CRAFTED, -2 * e, axis=0)[:k]
    return u, vel, pos, rng.normal(0.0, 8.0, (E, n)), rng.normal(0.0, 3.0, (E, n, n))


def host_channels(E, n, rb, seed):
    u, vel, pos, s_i, s_v = make_inputs(E, n, rb, seed)
    return native_sim.channels(u, vel, pos, s_i, s_v, rb)


def make_dest(E, n, seed, self_state=None):
    rng = np.random.default_rng(seed)
    dest = (np.arange(n)[None, :] + 1 + rng.integers(0, n - 1, size=(E, n))) % n
    assert np.all(dest != np.arange(n))
    if self_state is not None:
        dest[self_state, n - 1] = n - 1
    return dest.astype(np.int64)


# ------------------------------------------------------------------------------------------------------- 1. channels
@pytest.mark.parametrize("E,n,rb", [(1, 3, 3), (3, 4, 4), (2, 20, 4), (2, 31, 4), (70, 5, 4)])
def test_channels_against_the_host_library(E, n, rb):
    u, vel, pos, s_i, s_v = make_inputs(E, n, rb, 100 * n + E)
    want = native_sim.channels(u, vel, pos, s_i, s_v, rb)
    dc = DeviceChannels(E, n, rb)
    dc.upload('v2i_shadow', s_i)
    dc.upload('v2v_shadow', s_v)
    dc.step(u, vel, pos)
    got = dc.download()
    for name, g, w in zip(CHANNEL_NAMES, got, want):
        err = np.abs(g - w).max()
        print("%s: max |device - host| = %.3g" % (name, err))
        assert g.shape == w.shape and np.all(np.isfinite(g)) and close_db(g, w), (name, err)
    assert np.all(np.diagonal(got[2], axis1=1, axis2=2) > 50.0 - 40.0)          # the + 50 of the diagonal is there


def test_channels_chained_five_steps_each_side_on_its_own_shadowing():
    E, n, rb = 3, 4, 4
    u, vel, pos, s_i, s_v = make_inputs(E, n, rb, 7)
    dc = DeviceChannels(E, n, rb)
    dc.upload('v2i_shadow', s_i)
    dc.upload('v2v_shadow', s_v)
    rng = np.random.default_rng(8)
    for step in range(5):
        u = rng.random(u.shape)
        pos = pos + rng.normal(0.0, 0.15, pos.shape)
        want = native_sim.channels(u, vel, pos, s_i, s_v, rb)
        s_i, s_v = want[0], want[1]                              # the host's own shadowing goes back in
        dc.step(u, vel, pos)                                     # ... and the device keeps its own
        for name, g, w in zip(CHANNEL_NAMES, dc.download(), want):
            assert close_db(g, w), (step, name, np.abs(g - w).max())


# ------------------------------------------------------------------------------------------------------- 2. observation
@pytest.mark.parametrize("E,n,rb,self_state", [(1, 3, 3, None), (1, 3, 3, 0), (3, 4, 4, 1), (2, 31, 4, 1)])
def test_observation_on_identical_inputs_is_the_host_observation_bitwise(E, n, rb, self_state):
    _, _, _, _, v2v_ff, v2i_ff = host_channels(E, n, rb, 200 + n)
    dest = make_dest(E, n, 5, self_state)
    state, adj, xe, mask, col, regular = native_sim.observe_packed(dest, v2v_ff, v2i_ff, K['p_v2v'], rb)
    interf = native_sim.interference_db(dest, v2v_ff, K['p_v2i'], K['veh_gain'], K['veh_nf'], K['sig2'])
    dc = DeviceChannels(E, n, rb)
    dc.upload('v2v_ff', v2v_ff)
    dc.upload('v2i_ff', v2i_ff)
    dc.observe(dest)
    g_xe, g_mask, g_col, g_regular = dc.fetch_observation()
    g_state, g_interf = dc.download('state', 'interf_db')
    assert g_state.tobytes() == state.tobytes()
    assert g_xe.dtype == np.float32 and g_xe.tobytes() == xe.tobytes()
    assert g_mask.dtype == np.int32 and np.array_equal(g_mask, mask)
    assert g_col.dtype == np.int32 and np.array_equal(g_col, col[:, :n * (n - 2)])
    assert g_regular.dtype == bool and np.array_equal(g_regular, regular)
    if self_state is not None:
        assert not g_regular[self_state] and not g_col[self_state].any() and g_regular.sum() == E - 1
    err = np.abs(g_interf - interf[:, :, 0, :]).max()
    print("interf_db: max |device - host| = %.3g" % err)
    assert np.allclose(g_interf, interf[:, :, 0, :], rtol=1e-11, atol=1e-10), err


def test_observation_with_a_receiver_out_of_range_gives_nan_rows_for_that_state_only():
    E, n, rb = 3, 4, 4
    _, _, _, _, v2v_ff, v2i_ff = host_channels(E, n, rb, 31)
    dest = make_dest(E, n, 6)
    dc = DeviceChannels(E, n, rb)
    dc.upload('v2v_ff', v2v_ff)
    dc.upload('v2i_ff', v2i_ff)
    dc.observe(dest)
    clean = dc.fetch_observation()
    bad = dest.copy()
    bad[1, 2] = n
    dc.observe(bad)
    xe, mask, col, regular = dc.fetch_observation()
    state, interf = dc.download('state', 'interf_db')
    assert np.all(np.isnan(state[1])) and np.all(np.isnan(interf[1])) and np.all(np.isnan(xe[1, :, :3 * rb + 1]))
    assert not regular[1] and not col[1].any() and regular[0] and regular[2]
    for e in (0, 2):
        assert np.array_equal(xe[e], clean[0][e]) and np.array_equal(col[e], clean[2][e]) and np.all(np.isfinite(state[e]))


# ------------------------------------------------------------------------------------------------------- 3. rates
def joint_actions(E, n, rb, seed):
    rng = np.random.default_rng(seed)
    return {'one block': np.full((E, n), rb - 2, np.int64), 'spread': np.tile(np.arange(n) % rb, (E, 1)).astype(np.int64),
            'random': rng.integers(0, rb, size=(E, n)).astype(np.int64)}


@pytest.mark.parametrize("E,n,rb", [(3, 4, 4), (2, 20, 4)])
def test_rates_on_identical_inputs_against_the_host_library(E, n, rb):
    _, _, _, v2i_abs, v2v_ff, v2i_ff = host_channels(E, n, rb, 300 + n)
    dest = make_dest(E, n, 9)
    dc = DeviceChannels(E, n, rb)
    for name, a in (('v2v_ff', v2v_ff), ('v2i_ff', v2i_ff), ('v2i_abs', v2i_abs), ('dest', dest)):
        dc.upload(name, a)
    opt = OptimalAllocation()
    for label, ch in joint_actions(E, n, rb, 11).items():
        want = native_sim.reward(ch, dest, v2v_ff, v2i_ff, v2i_abs, K['p_v2v'], K['p_v2i'], K['veh_gain'], K['bs_gain'], K['bs_nf'],
                                 K['veh_nf'], K['sig2'])
        dc.rates(ch)
        r = dc.fetch_rates()
        assert np.allclose(r['v2v_rate'], want[0][:, :, 0], rtol=1e-9, atol=1e-12), label
        assert np.allclose(r['v2i_rate'], want[1], rtol=1e-9, atol=1e-12), label
        assert np.allclose(r['interference'], want[2], rtol=1e-9, atol=0), label
        assert np.allclose(r['v2i_interf'], want[3], rtol=1e-9, atol=0), label
        assert np.allclose(r['v2v_interf'], want[4][:, :, 0], rtol=1e-9, atol=0), label
        reward = W_V2V * r['v2v_rate'].sum(axis=1) + W_V2I * r['v2i_rate'].sum(axis=1)
        assert np.allclose(reward, opt.rewards_of(dc, W_V2V, W_V2I, ch), rtol=1e-9, atol=0), label
    ch = joint_actions(E, n, rb, 12)['random']
    dc.rates(ch)
    clean = dc.fetch_rates()
    ch[1, n - 1] = rb                                           # one channel too far, in state 1
    dc.rates(ch)
    r = dc.fetch_rates()
    for name in ('v2v_rate', 'v2i_rate', 'interference', 'v2i_interf', 'v2v_interf'):
        assert np.all(np.isnan(r[name][1])), name
        for e in set(range(E)) - {1}:
            assert np.array_equal(r[name][e], clean[name][e]), name


# ------------------------------------------------------------------------------------------------------- 4. the environment
@pytest.mark.parametrize("n,steps", [(4, 6), (20, 2)])
def test_device_environment_against_the_host_environment(n, steps):
    E = 3
    host = start_env_batched(n, E, 77, lookahead=False)
    dev = start_env_batched(n, E, 77, backend="device")
    assert type(host) is BatchedEnviron and type(dev) is DeviceBatchedEnviron and host.native
    rng = np.random.default_rng(5)
    opt = OptimalAllocation()

    def compare(tag):
        assert np.array_equal(dev.pos, host.pos) and np.array_equal(dev.dirs, host.dirs), tag
        assert np.array_equal(dev.dest, host.dest) and np.array_equal(dev.vel, host.vel), tag
        assert np.array_equal(dev._mt_keys, host._mt_keys) and np.array_equal(dev._mt_pos, host._mt_pos), tag
        for name in ('_v2i_shadow', '_v2v_shadow', 'V2V_channels_abs', 'V2I_channels_abs', 'V2V_channels_with_fastfading',
                     'V2I_channels_with_fastfading'):
            g, w = getattr(dev, name), getattr(host, name)
            assert g.shape == w.shape and close_db(g, w), (tag, name, np.abs(g - w).max())
        xe, mask, col, regular = dev.observe_packed(4)
        h_xe, h_mask, h_col, h_regular = host.observe_packed(4)
        assert np.all(np.abs(xe - h_xe) <= np.spacing(np.maximum(np.abs(xe), np.abs(h_xe)))), tag
        assert np.array_equal(mask, h_mask) and np.array_equal(col, h_col) and np.array_equal(regular, h_regular), tag

    compare("reset")
    for t in range(steps):
        actions = rng.integers(0, 4, size=(E, n, 1))
        got, want = dev.act(actions), host.act(actions)
        for g, w, name in zip(got, want, ("v2v_rate", "v2i_rate", "interference")):
            assert g.shape == w.shape, name
            assert np.allclose(g, w, rtol=1e-9, atol=1e-12 if name != "interference" else 0), (t, name)
        assert np.allclose(dev.V2I_Interference, host.V2I_Interference, rtol=1e-9, atol=0)
        assert np.allclose(dev.V2V_Interference, host.V2V_Interference, rtol=1e-9, atol=0)
        compare(t)
        assert np.allclose(dev.V2V_Interference_all, host.V2V_Interference_all, rtol=1e-11, atol=1e-10), t
    if n == 4:
        # the search on the device arrays finds what the search on the downloaded state finds
        class Downloaded(object):
            pass
        snap = Downloaded()
        snap.E, snap.n_Veh, snap.n_RB, snap.n_Neighbor = E, n, 4, 1
        dc = dev.device_channels
        snap.V2V_channels_with_fastfading, snap.V2I_channels_with_fastfading, snap.V2I_channels_abs = dc.download(
            'v2v_ff', 'v2i_ff', 'v2i_abs')
        snap.dest, snap.activate_links = dev.dest.copy(), dev.activate_links
        for k in ('V2V_power_dB_List', 'fixed_v2v_power_index', 'V2I_power_dB', 'vehAntGain', 'bsAntGain', 'bsNoiseFigure',
                  'vehNoiseFigure', 'sig2'):
            setattr(snap, k, getattr(dev, k))
        snap.finish_step = lambda: None
        dc.upload('dest', dev.dest)
        i_dc, r_dc = opt.search(dc, W_V2V, W_V2I)
        i_env, r_env = opt.search(dev, W_V2V, W_V2I)
        i_host, r_host = opt.search(snap, W_V2V, W_V2I)
        assert np.array_equal(i_dc, i_host) and r_dc.tobytes() == r_host.tobytes()
        assert np.array_equal(i_env, i_host) and r_env.tobytes() == r_host.tobytes()


# ------------------------------------------------------------------------------------------------------- 5. entry-point errors
def test_entry_point_errors_launch_nothing():
    import torch
    lib = load_library()
    E, n, rb = 2, 4, 4
    n_u = uniforms_per_step(n, rb)
    dev = torch.device('cuda', 0)
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=dev)                # noqa: E731
    u, vel, pos = f64(E, n_u), f64(E, n), f64(E, n, 2)
    outs = [f64(E, n), f64(E, n, n), f64(E, n, n), f64(E, n), f64(E, n, n, rb), f64(E, n, rb)]
    stream = torch.cuda.current_stream().cuda_stream

    def channels(E_=E, n_u_=n_u, u_=u):
        return lib.v2x_sim_channels(E_, n, rb, u_.data_ptr() if u_ is not None else None, n_u_, vel.data_ptr(), pos.data_ptr(),
                                    *[o.data_ptr() for o in outs], stream)

    for kwargs, word in ((dict(u_=None), "null"), (dict(E_=0), "E = 0"), (dict(n_u_=n_u + 2), "n_u")):
        assert channels(**kwargs) == V2X_EINVAL
        assert word in lib.v2x_last_error(None).decode(), kwargs
    dest = torch.zeros((E, n), dtype=torch.int64, device=dev)
    small = [f64(E, n, rb), f64(E, n, 3 * rb + 1), torch.full((E, n, 16), 7.0, device=dev),
             torch.full((E, n), 7, dtype=torch.int32, device=dev), torch.full((E, n * (n - 2),), 7, dtype=torch.int32, device=dev),
             torch.full((E,), 7, dtype=torch.uint8, device=dev)]

    def observe(E_=E, dest_=dest, n_=n):
        return lib.v2x_sim_observe(E_, n_, rb, dest_.data_ptr() if dest_ is not None else None, outs[4].data_ptr(),
                                   outs[5].data_ptr(), 23.0, 3.0, 9.0, 1e-11, 10.0, *[o.data_ptr() for o in small], stream)

    for kwargs, word in ((dict(dest_=None), "null"), (dict(E_=0), "E = 0"), (dict(n_=2), "n = 2")):
        assert observe(**kwargs) == V2X_EINVAL
        assert word in lib.v2x_last_error(None).decode(), kwargs
    rates = [f64(E, n), f64(E, rb)]
    ch = torch.zeros((E, n), dtype=torch.int32, device=dev)

    def problem(E_=E):
        return OptProblem(E=E_, n=n, rb=rb, pad_=0, v2v_ff=outs[4].data_ptr(), v2i_ff=outs[5].data_ptr(), v2i_abs=outs[3].data_ptr(),
                          dest=dest.data_ptr(), w_v2v=1.0, w_v2i=0.1, **K)

    for prob, ch_, word in ((problem(), None, "null"), (problem(0), ch, "E = 0")):
        rc = lib.v2x_sim_rates(ctypes.byref(prob), ch_.data_ptr() if ch_ is not None else None, rates[0].data_ptr(),
                               rates[1].data_ptr(), None, None, None, stream)
        assert rc == V2X_EINVAL and word in lib.v2x_last_error(None).decode()
    assert lib.v2x_sim_rates(None, ch.data_ptr(), rates[0].data_ptr(), rates[1].data_ptr(), None, None, None, stream) == V2X_EINVAL
    torch.cuda.synchronize()
    for t in outs + small + rates:                              # nothing ran: every output still holds its fill value
        assert bool((t == 7).all())


# ------------------------------------------------------------------------------------------------------- 6. capture
def test_step_observe_rates_replay_from_a_captured_graph_bitwise():
    import torch
    E, n, rb = 3, 4, 4
    draws = [make_inputs(E, n, rb, 40 + k) for k in range(3)]
    dest = make_dest(E, n, 3)
    actions = [joint_actions(E, n, rb, 50 + k)['random'].astype(np.int32) for k in range(3)]
    names = CHANNEL_NAMES + ('interf_db', 'state', 'xe', 'mask', 'col', 'regular', 'v2v_rate', 'v2i_rate', 'interference',
                             'v2i_interf', 'v2v_interf')

    def start():
        dc = DeviceChannels(E, n, rb)
        dc.upload('v2i_shadow', draws[0][3])
        dc.upload('v2v_shadow', draws[0][4])
        dc.upload('dest', dest)
        return dc

    eager, results = start(), []
    for (u, vel, pos, _, _), a in zip(draws, actions):
        eager.step(u, vel, pos)
        eager.observe()
        eager.rates(a)
        results.append([x.copy() for x in eager.download(*names)])

    dc = start()
    dev = torch.device('cuda', 0)
    u_t, vel_t, pos_t = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((E, dc.n_u), (E, n), (E, n, 2)))
    a_t = torch.zeros((E, n), dtype=torch.int32, device=dev)

    def load(k):
        for t, a in zip((u_t, vel_t, pos_t, a_t), draws[k][:3] + (actions[k],)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a)))

    load(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # captured once (capture runs nothing)
        dc.step(u_t, vel_t, pos_t)
        dc.observe()
        dc.rates(a_t)
    for k in range(3):                                          # replayed with new uniforms in the same buffers
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(names, dc.download(*names), results[k]):
            assert got.tobytes() == want.tobytes(), (k, name)


# ------------------------------------------------------------------------------------------------------- 7. the agent
def test_agent_trains_on_the_device_environment_with_the_host_runs_draws_and_actions():
    def episode(backend):
        random.seed(21)
        np.random.seed(21)
        env = start_env_batched(4, 3, 21, lookahead=False, backend=backend)
        cfg = RL_Config()
        cfg.set_train_value(16, 0.5, 64, 1, 0.1)
        agent = Agent(4, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=21, device_replay=True)
        out = agent.train(1, 2)
        rep = agent.device_replay
        rep.flush()
        return env, agent, out, rep.action[:rep.size].cpu().numpy(), np.random.get_state()

    env_d, ag_d, out_d, act_d, rs_d = episode("device")
    env_h, ag_h, out_h, act_h, rs_h = episode("host")
    assert type(env_d) is DeviceBatchedEnviron and type(env_h) is BatchedEnviron
    assert ag_d.num_step == ag_h.num_step > 0 and act_d.shape == act_h.shape and act_d.shape[0] > 0
    assert np.all(np.isfinite(out_d[0])) and np.all(np.isfinite(out_d[1]))
    assert np.array_equal(act_d, act_h)
    assert rs_d[0] == rs_h[0] and np.array_equal(rs_d[1], rs_h[1]) and rs_d[2:] == rs_h[2:]
    assert np.array_equal(env_d.pos, env_h.pos) and np.array_equal(env_d._mt_keys, env_h._mt_keys)
