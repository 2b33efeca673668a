"""GPU: K networks scored on the same walked episode in one call (v2x_eval_sweep_mixed: one walk, one k_traj_assemble_mixed, K
ragged forwards, k_eval_finish_sweep_mixed of csrc/v2xsimdev.hip; rl/device_sim.py eval_sweep_mixed /
resident_evaluate_sweep_mixed; MixedAgent.evaluate_training(eval_backend='device')).  The reference is v2x_eval_steps_mixed,
called once per network from a copy of the same resident state -- the kernels share their __device__ functions, so everything is
compared byte for byte -- or the agent's host loop on twin environments.

The shapes: pools of 4 and 8 links with E = (2, 1), rb = 4, T = 3, K = 3 networks and the baseline.  In the finish launch's block
index ((pool, scheme, t, e), S = 4 schemes) the strides are then all different: e 1, t 2 or 1, scheme 6 or 3, pool 24 -- and so
are the strides of the result block's rows (n = 4 or 8) and of the K Q blocks (R = 3 (2 * 4 + 1 * 8) = 48 rows)."""
import ctypes
import random

import numpy as np
import pytest

from test_gpu_eval_device import W_V2I, W_V2V
from test_gpu_eval_mixed import RATES, _pools, _start, _table
from test_gpu_rollout_mixed import RB, _agent, _ragged_engine
from test_gpu_rollout_trajectory import STATE, _same_rng
from v2xgnn import GnnEngine, GnnSpec
from v2xgnn.lib import V2X_EINVAL, EvalMixed, EvalSweep, load_library
from v2xgnn.rl.device_sim import (eval_result_layout, eval_steps_mixed, eval_sweep_mixed, mixed_rollout_buffers, mixed_sweep_q,
                                  resident_evaluate_sweep_mixed)
from v2xgnn.rl.train import start_env_batched

pytestmark = pytest.mark.gpu

SPEC, T3, SEEDS = [(2, 4), (1, 8)], 3, (5, 6, 7)


@pytest.fixture(scope="module")
def engines():
    made = [_ragged_engine(seed) for seed in SEEDS]
    assert len({e.get_flat().tobytes() for e in made}) == len(SEEDS)
    yield made
    for e in made:
        e.close()


def _resident(dc, T):
    """every resident tensor and the whole trajectory workspace, as bytes"""
    import torch
    torch.cuda.synchronize()
    snap = {k: dc.tensor(k).cpu().numpy().tobytes() for k in STATE}
    snap['workspace'] = dc.rollout_steps_buffers(T)['workspace'].cpu().numpy().tobytes()
    return snap


def _single_calls(pools, T, nets, explore, rand, base, walk='serial'):
    """one v2x_eval_steps_mixed call per network, each from a copy of the same resident state (cloned before the first call and
    put back before every other) -> (the channels as the LAST call left them, [rows per pool] per call, [_resident per pool] per call)"""
    ref = _start(pools)
    saved = [{k: dc.tensor(k).clone() for k in STATE} for dc in ref]
    rows, snaps = [], []
    for i, net in enumerate(nets):
        if i:
            for dc, state in zip(ref, saved):
                for k, v in state.items():
                    dc.tensor(k).copy_(v)
        rows.append([r.resolve() for r in eval_steps_mixed(ref, explore, rand, base, W_V2V, W_V2I, engine=net, walk=walk)])
        snaps.append([_resident(dc, T) for dc in ref])
    return ref, rows, snaps


def _assert_sweep_is_the_single_calls(pools, T, nets, explore, rand, base, walk='serial', tag=None):
    K, S = len(nets), len(nets) + (base[0] is not None)
    _, rows, snaps = _single_calls(pools, T, nets, explore, rand, base, walk)
    got = _start(pools)
    engines_arg = None if all(net is None for net in nets) else nets
    got_rows = [r.resolve() for r in eval_sweep_mixed(got, explore, rand, base, W_V2V, W_V2I, engines=engines_arg, K=K, walk=walk)]
    for j, p in enumerate(pools):
        g = got_rows[j]
        assert g.schemes == S and g.actions.shape == (S, T, p['E'], p['n']) and g.reward.shape == (S, T, p['E']), (tag, j)
        for k in range(K):                                               # scheme k: call k's scheme 0, bit for bit
            w = rows[k][j]
            assert g.actions[k].tobytes() == w.actions[0].tobytes(), (tag, j, k)
            for name in RATES:
                a, b = getattr(g, name)[k], getattr(w, name)[0]
                assert a.shape == b.shape and a.tobytes() == b.tobytes() and np.all(np.isfinite(b)), (tag, j, k, name)
            assert np.array_equal(g.regular, w.regular) and g.regular.shape == (T + 1, p['E']) and g.regular.all(), (tag, j, k)
            if base[0] is not None:                                      # the baseline scheme: any call's scheme 1
                assert g.actions[K].tobytes() == w.actions[1].tobytes() == base[j].tobytes(), (tag, j, k)
                for name in RATES:
                    assert getattr(g, name)[K].tobytes() == getattr(w, name)[1].tobytes(), (tag, j, k, name)
            assert snaps[k][j]['workspace'] == snaps[0][j]['workspace'], (tag, j, k)     # (every call walks the same steps)
        after = _resident(got[j], T)                                     # the state and the trajectory: those after call K - 1
        for name, want in snaps[K - 1][j].items():
            assert after[name] == want, (tag, j, name)
        assert got[j].trajectory_states(T).E == T * p['E']
    return got, got_rows, rows


def _draws(pools):
    return [p['policy'][0] for p in pools], [p['policy'][1] for p in pools], [p['baseline'] for p in pools]


def test_the_sweep_is_one_call_per_network_from_the_same_state(engines):
    pools = _pools(SPEC, T3, 1, 41)
    explore, rand, base = _draws(pools)
    for ex in explore:                                                   # both flag values in every pool
        assert ex.any() and not ex.all()
    got, got_rows, rows = _assert_sweep_is_the_single_calls(pools, T3, engines, explore, rand, base)
    for j, p in enumerate(pools):
        g = got_rows[j]
        # explored steps are the same in all K schemes (the draws are shared); greedy ones differ between the networks somewhere,
        # and what the call leaves resident is network K - 1's, not network 0's
        x = explore[j] != 0
        for k in range(1, len(engines)):
            assert np.array_equal(g.actions[k][x], g.actions[0][x]) and np.array_equal(g.actions[k][x], rand[j][x]), (j, k)
            assert g.reward[k][x].tobytes() == g.reward[0][x].tobytes(), (j, k)
        assert np.any(g.actions[1][~x] != g.actions[0][~x]) or np.any(g.actions[2][~x] != g.actions[0][~x]), j
        assert not x[-1, -1]
        assert np.array_equal(got[j].download('actions').reshape(p['E'], p['n']), g.actions[len(engines) - 1][-1]), j
    last = np.concatenate([got_rows[j].actions[2][-1].reshape(-1) for j in range(2)])
    first = np.concatenate([got_rows[j].actions[0][-1].reshape(-1) for j in range(2)])
    assert np.any(last != first)                                         # otherwise "network K - 1's" shows nothing
    # the K Q blocks lie back to back behind one base pointer: block k is network k's forward of the one ragged batch
    q = mixed_sweep_q(got, T3, len(engines)).cpu().numpy()
    R = sum(T3 * E * n for E, n in SPEC)
    assert q.shape == (3, R, RB) and np.all(np.isfinite(q)) and len({q[k].tobytes() for k in range(3)}) == 3


def test_one_network_is_eval_steps_mixed_outright(engines):
    import torch
    pools = _pools(SPEC, T3, 0, 17)
    explore, rand, base = _draws(pools)
    ref = _start(pools)
    eval_steps_mixed(ref, explore, rand, base, W_V2V, W_V2I, engine=engines[1])
    got = _start(pools)
    eval_sweep_mixed(got, explore, rand, base, W_V2V, W_V2I, engines=[engines[1]])
    torch.cuda.synchronize()
    for j, p in enumerate(pools):
        size = eval_result_layout(p['E'], p['n'], RB, T3, 2)[1]
        block = got[j]._sweep_io(T3, 2)[1]['dev'].cpu().numpy().tobytes()
        assert len(block) == size and block == ref[j]._eval_io(T3)['eval_result_dev'][:size].cpu().numpy().tobytes(), j
        assert _resident(got[j], T3) == _resident(ref[j], T3), j


@pytest.mark.parametrize("variant", ["T1", "no_baseline", "everybody_greedy", "one_pool"])
def test_shapes_and_flags(engines, variant):
    spec, T = ([(2, 4)] if variant == "one_pool" else SPEC), (1 if variant == "T1" else T3)
    pools = _pools(spec, T, 2, 23)
    explore, rand, base = _draws(pools)
    if variant == "T1":
        explore = [np.array([[1, 0]], np.uint8), np.array([[0]], np.uint8)]
    if variant == "everybody_greedy":
        explore = [np.zeros_like(x) for x in explore]
    if variant == "no_baseline":
        base = [None] * len(pools)
    _assert_sweep_is_the_single_calls(pools, T, engines, explore, rand, base, tag=variant)


def test_everybody_explores_without_models_all_schemes_are_the_same(engines):
    pools = _pools(SPEC, T3, 1, 29)
    _, rand, base = _draws(pools)
    explore = [np.ones((T3, p['E']), np.uint8) for p in pools]
    _, got_rows, _ = _assert_sweep_is_the_single_calls(pools, T3, [None] * 3, explore, rand, base, tag='explore')
    for j in range(len(pools)):
        g = got_rows[j]
        for k in range(3):
            assert np.array_equal(g.actions[k], rand[j]), (j, k)
            for name in RATES:
                assert getattr(g, name)[k].tobytes() == getattr(g, name)[0].tobytes(), (j, k, name)
    # ... and with models the flags alone keep everybody from the Q-values: the same bits
    got = _start(pools)
    with_models = [r.resolve() for r in eval_sweep_mixed(got, explore, rand, base, W_V2V, W_V2I, engines=engines)]
    for j in range(len(pools)):
        for name in RATES + ('actions',):
            assert getattr(with_models[j], name).tobytes() == getattr(got_rows[j], name).tobytes(), (j, name)


def test_the_wide_walk_leaves_the_bits_of_the_serial_walk(engines):
    pools = _pools(SPEC, T3, 1, 41)
    explore, rand, base = _draws(pools)
    serial = _start(pools)
    s_rows = [r.resolve() for r in eval_sweep_mixed(serial, explore, rand, base, W_V2V, W_V2I, engines=engines)]
    wide, w_rows, _ = _assert_sweep_is_the_single_calls(pools, T3, engines, explore, rand, base, walk='wide', tag='wide')
    for j in range(len(pools)):
        assert _resident(wide[j], T3) == _resident(serial[j], T3), j
        for name in RATES + ('actions', 'regular'):
            assert getattr(w_rows[j], name).tobytes() == getattr(s_rows[j], name).tobytes(), (j, name)
        assert wide[j].walk_calls == {'serial': 0, 'wide': 1} and wide[j].stream_phase_calls['split'] == 1, j
        assert serial[j].walk_calls == {'serial': 1, 'wide': 0}, j


# ------------------------------------------------------------------------------------------------------- refusals
def test_a_refused_sweep_names_what_is_wrong_and_launches_nothing(engines):
    import torch
    lib = load_library()
    T = 2
    pools = _pools(SPEC, T, 0, 9)
    chans = _start(pools)
    fixed = GnnEngine(GnnSpec(n_nodes=4, feat_dim=16, n_mp_layers=2))
    wider = GnnEngine(GnnSpec(n_nodes=1, n_channels=RB, feat_dim=32, n_mp_layers=2, share_weights=True, variable_graphs=True))
    buf = mixed_rollout_buffers(chans, T)
    q = mixed_sweep_q(chans, T, 3)
    q.fill_(7)
    for dc in chans:
        dc._eval_io(T)['eval_result_dev'].fill_(7)
    before = [_resident(dc, T) for dc in chans]
    blocks = lambda: [dc._eval_io(T)['eval_result_dev'].cpu().numpy().tobytes() for dc in chans]     # noqa: E731
    blocks_before = blocks()
    stream = torch.cuda.current_stream().cuda_stream

    def refused(text, K=3, models=engines, no_q=False, n_pools=2, table=None, ws=None):
        table = _table(chans, T) if table is None else table
        base = EvalMixed(n_pools=n_pools, T=T, pools=table, model=None)
        for name in ('xe', 'graph_off', 'row_ptr', 'col_idx'):
            setattr(base, name, buf[name].data_ptr())
        s = EvalSweep(base=base, K=K, pad_=0, q=None if no_q else q.data_ptr())
        if models is not None:
            handles = (ctypes.c_void_p * len(models))(*[None if m is None else m._h for m in models])
            s.models = handles
        assert lib.v2x_eval_sweep_mixed(ctypes.byref(s), ws, stream) == V2X_EINVAL, text
        err = lib.v2x_last_error(None).decode()
        assert err.startswith("eval_sweep_mixed: ") and text in err, (text, err)

    refused("1..64 networks supported, got K = 0", K=0)
    refused("1..64 networks supported, got K = 65", K=65)
    refused("models[1] is NULL", models=[engines[0], None, engines[2]])
    refused("models[2] has fixed-size graphs", models=[engines[0], engines[1], fixed])
    refused("models[1] has 4 channels, feature width 32", models=[engines[0], wider, engines[2]])
    refused("models need the Q workspace", no_q=True)
    # ... and everything v2x_eval_steps_mixed checks, under the sweep's name
    refused("1..8 pools", n_pools=0)
    t = _table(chans, T)
    t[0], t[1] = _table(chans, T)[1], _table(chans, T)[0]
    refused("the link counts must ascend strictly", table=t)
    t = _table(chans, T)
    t[1].T = T + 1
    refused("pool 1 (8 links) walks T = 3 steps, the call T = 2", table=t)
    t = _table(chans, T)
    t[1].baseline_actions = None
    refused("one number of schemes for all pools", table=t)
    t = _table(chans, T)
    t[1].explore = None
    refused("Q-values need the explore flags", table=t)
    t = _table(chans, T)
    t[0].result_reward = None
    refused("null result pointer", table=t)
    from v2xgnn.lib import TrajWs
    refused("pool 0 (4 links): ", ws=(TrajWs * 2)())                     # the wide walk's workspaces are checked per pool
    torch.cuda.synchronize()
    assert [_resident(dc, T) for dc in chans] == before and blocks() == blocks_before and bool((q == 7).all())
    # the Python entry points refuse before any device work, too
    explore, rand, base = _draws(pools)
    with pytest.raises(ValueError, match="1..64 networks, got 0"):
        eval_sweep_mixed(chans, explore, rand, base, W_V2V, W_V2I, engines=[])
    with pytest.raises(ValueError, match="1..64 networks, got 65"):
        eval_sweep_mixed(chans, explore, rand, base, W_V2V, W_V2I, engines=list(engines) * 21 + [engines[0], engines[1]])
    with pytest.raises(ValueError, match=r"variable_graphs engines of 4 channels \(engine 1\)"):
        eval_sweep_mixed(chans, explore, rand, base, W_V2V, W_V2I, engines=[engines[0], fixed])
    with pytest.raises(ValueError, match="engine 2 has another spec than engine 0"):
        eval_sweep_mixed(chans, explore, rand, base, W_V2V, W_V2I, engines=[engines[0], engines[1], wider])
    with pytest.raises(ValueError, match="ascend strictly"):
        eval_sweep_mixed(chans[::-1], explore[::-1], rand[::-1], base[::-1], W_V2V, W_V2I, engines=engines)
    host_env = start_env_batched(4, 2, 5, backend="device", streams="host")
    with pytest.raises(ValueError, match="needs streams='device' in every environment"):
        resident_evaluate_sweep_mixed([host_env], explore[:1], rand[:1], base[:1], W_V2V, W_V2I, engines=engines)
    torch.cuda.synchronize()
    assert [_resident(dc, T) for dc in chans] == before and blocks() == blocks_before
    fixed.close()
    wider.close()


# ------------------------------------------------------------------------------------------------------- the agent
def _training_run(backend, T, eps, walk='serial', sizes=(4, 8), Es=(2, 1), trials=2, seed=12):
    import torch
    agent = _agent(sizes, Es, seed, 'host', 0, 20)
    agent.trajectory_walk = walk
    nets = [_ragged_engine(s) for s in SEEDS]
    envs = agent.envs
    books = agent.evaluate_training(envs, None, T, trials, eps, opt_flag=True, opt_backend='device', eval_backend=backend, engines=nets)
    torch.cuda.synchronize()
    run = dict(books=books, rng=np.random.get_state(), py=random.getstate(), num_step=agent.num_step, stats=dict(agent.eval_stats),
               streams=[[np.array(a).copy() for a in (e._mt_keys, e._mt_pos, e.pos, e.dirs)] for e in envs],
               resident=[{k: e._dc.tensor(k).cpu().numpy().tobytes() for k in STATE} for e in envs])
    for net in nets:
        net.close()
    agent.close()
    return run


@pytest.mark.parametrize("T,eps,walk", [(1, 0.0, 'serial'), (1, 0.5, 'serial'), (3, 1.0, 'serial'), (3, 1.0, 'wide')])
def test_evaluate_training_on_the_device_equals_the_host_loop(T, eps, walk):
    """4 and 8 links with E = (2, 1), K = 3 checkpoints, 2 trials, with the optimum of every state (exhaustive search).  As for
    test_run (tests/test_gpu_eval_mixed.py) the greedy cases hold one step per trial, so that both forms score the same batch,
    and the longer episode has nobody greedy: the check does not lean on a ragged forward being independent of what else is in
    the batch."""
    sizes, Es, trials, K = (4, 8), (2, 1), 2, len(SEEDS)
    h = _training_run('host', T, eps)
    d = _training_run('device', T, eps, walk)
    assert h['stats'] == {'device_episodes': 0, 'host_episodes': trials} and d['stats'] == {'device_episodes': trials, 'host_episodes': 0}
    assert sorted(h['books']) == sorted(d['books']) == list(sizes)
    for n, E in zip(sizes, Es):
        assert sorted(h['books'][n]) == sorted(d['books'][n]) == ['gnn', 'optimal', 'random']
        for s in ('gnn', 'random', 'optimal'):
            lead = (trials, K, E) if s == 'gnn' else (trials, E)
            shapes = [lead, lead + (T,), lead + (T, n), lead + (T, RB), lead + (T, RB)]
            for a, b, shape in zip(h['books'][n][s], d['books'][n][s], shapes):
                assert a.shape == b.shape == shape and a.tobytes() == b.tobytes() and np.all(np.isfinite(a)), (n, s)
            assert np.all(h['books'][n][s][1] > 0), (n, s)
        best, gnn = h['books'][n]['optimal'][1], h['books'][n]['gnn'][1]
        assert np.all(best[:, None] >= gnn - 1e-9) and np.all(best >= h['books'][n]['random'][1] - 1e-9), n
        if eps == 0.0:                # the checkpoints do not all pick alike (two of three may, on so few states), nor like the baseline
            assert len({gnn[:, k].tobytes() for k in range(K)}) > 1 and gnn[:, 0].tobytes() != h['books'][n]['random'][1].tobytes(), n
        if eps == 1.0:
            assert all(gnn[:, k].tobytes() == gnn[:, 0].tobytes() for k in range(K)), n
    assert _same_rng(h['rng'], d['rng']) and h['py'] == d['py'] and h['num_step'] == d['num_step'] == trials * T * sum(Es)
    for a, b in zip(h['streams'], d['streams']):
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
    for k, (a, b) in enumerate(zip(h['resident'], d['resident'])):
        for name in STATE:
            assert a[name] == b[name], (k, name)


def test_checkpoints_saved_by_train_are_the_networks_the_sweep_scores(tmp_path):
    """train(save_interval=1) leaves a checkpoint per episode; evaluate_training loads them by their tags and scores what a
    sweep over engines holding those weights scores"""
    from v2xgnn.bs_brain import load_weight_file
    from v2xgnn.rl.evaluate import saved_checkpoints
    folder = str(tmp_path / 'run')
    agent = _agent((4, 8), (2, 1), 5, 'host', 0, 20)
    agent.train(2, 1, save_dir=folder, save_interval=1)
    assert saved_checkpoints(folder, 5, 1, 32) == [1, 2]
    # (the simulators own their streams: twins from one seed face the same episode, one agent's second run does not)
    twin_a, twin_b = _agent((4, 8), (2, 1), 9, 'host', 0, 20), _agent((4, 8), (2, 1), 9, 'host', 0, 20)
    by_tag = twin_a.evaluate_training(twin_a.envs, [1, 2], 1, 1, 0.0, save_dir=folder, num_train_steps=1)
    nets = []
    for tag in (1, 2):
        net = GnnEngine(agent.spec)
        net.set_weights(load_weight_file(agent._weight_paths(folder, tag, 1)[0]))
        nets.append(net)
    assert nets[0].get_flat().tobytes() != nets[1].get_flat().tobytes() and nets[1].get_flat().tobytes() == agent.online.get_flat().tobytes()
    by_engine = twin_b.evaluate_training(twin_b.envs, None, 1, 1, 0.0, engines=nets)
    assert by_tag[4]['gnn'][1].shape == (1, 2, 2, 1) and np.all(by_tag[8]['gnn'][1] > 0)
    for n in (4, 8):
        for s in ('gnn', 'random'):
            for a, b in zip(by_tag[n][s], by_engine[n][s]):
                assert a.tobytes() == b.tobytes(), (n, s)
    for net in nets:
        net.close()
    for a in (agent, twin_a, twin_b):
        a.close()
