"""GPU: the one-call DQN replay step on RAGGED batches (v2x_dqn_step with two variable_graphs models: graphs of 3-31 links in
one minibatch, one reward per graph, one action per node row) against the float64 oracle -- targets, the single Huber mean, the
GRADIENT and the weights after Adam -- by the scheme of test_gpu_dqn_step.py, whose helpers and bounds are used as they are.

The draw (_draw; one seeded draw per case, nothing redrawn): pools of reference-topology graphs, random_inputs per size,
concatenated in the order given (an empty pool draws nothing); f32_params for both networks, the last Dense layer of each
divided by the standard deviation of the network's float64 output; actions uniform in 0..3; reward[g] = median over the rows of
graph g of (q[r, a] - gamma max_c q'[r, c]) + U(-w, w), gamma = 0.5.  Asserted in every case from the oracle's own numbers: at
least 25 % of the R replaced entries on either Huber branch (each case prints its share).

    seed  pools (n x count)          F   L  w  B   R    covers
    2001  4x5, 12x3, 20x7, 31x2      64  2  1  17  258  graphs below and above the 16-node complement threshold
    2002  3x1, 8x0, 16x4, 31x9       32  1  1  14  346  an empty pool; R crosses the 320-row tile
    2003  20x17                      64  2  1  17  340  a single pool
    2004  4x12, 15x6, 16x6, 31x2     16  3  2  26  296  deep and narrow (w = 1 would leave the linear branch 10-15 %)

A  every case: y (assert_fwd_close), the single loss within LOSS_RTOL / LOSS_ATOL, the gradient (assert_grads_match_oracle), the
   weights after the oracle's Adam step, a twin engine's forward_backward on the step's own y (assert_grad_close).
B  the two target forms (k_dqn_tq_ragged inside k_mlp_train_wg / V2X_DQN_FUSED_TARGETS=0: forward, k_dqn_targets_ragged, the
   training launch): replaced entries bit for bit; y_out=None bit for bit a call with a buffer.
C  n_global = 2 R: the loss and the gradient are one half of the default's.
D  three steps on the same buffers with new contents, a target sync after the second: hipGraph replay == eager, bit for bit.
E  v2x_dqn_targets_ragged on ties, signed zeros, +-inf, values near +-3e38 and NaN (test D's table of test_gpu_dqn_step.py,
   with per-graph rewards on graphs of different sizes) against numpy's scalar expression, bit for bit.
F  refusals, matched on their text: another graph_off pointer, a variable online model with a fixed target, dqn_step_dp.
"""
import functools

import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnSpec, PackedBatch
from v2xgnn.engine import DeviceBatch
from oracle import compact as oc
from util import ospec, f32_params, random_inputs, oracle_step, assert_close, assert_grad_close
from test_gpu_dqn_step import (GAMMA, LOSS_RTOL, LOSS_ATOL, MIN_BRANCH_SHARE, SPECIAL_ROWS, SPECIAL_REWARDS, SPECIAL_GAMMAS,
                               _check_against_oracle, _assert_same_floats)
from test_gpu_launch_sizes import _engine

pytestmark = pytest.mark.gpu

CASES = {  # seed: (pools (n, count), F, L, w, B, R)
    2001: (((4, 5), (12, 3), (20, 7), (31, 2)), 64, 2, 1.0, 17, 258),
    2002: (((3, 1), (8, 0), (16, 4), (31, 9)), 32, 1, 1.0, 14, 346),
    2003: (((20, 17),), 64, 2, 1.0, 17, 340),
    2004: (((4, 12), (15, 6), (16, 6), (31, 2)), 16, 3, 2.0, 26, 296),
}


# ------------------------------------------------------------------------------------------------ the draw (host only)
def _spec(F, L):
    return GnnSpec(n_nodes=1, feat_dim=F, n_mp_layers=L, share_weights=True, variable_graphs=True)


def _inputs(rng, pools):
    """s and s' of the pools' transitions as node rows: x, e, x2, e2 [R, .], one ragged CSR (graph_off, row_ptr, col_idx)"""
    xs, es, x2s, e2s, sizes, rps, cols, edges = [], [], [], [], [], [np.zeros(1, np.int32)], [], 0
    for n, count in pools:
        if count == 0:
            continue
        x, e, adj = random_inputs(rng, count, n)
        x2, e2, _ = random_inputs(rng, count, n)
        _, rp, ci = oc.adj_to_csr(adj)
        assert len(ci) == count * n * (n - 2)
        xs.append(x.reshape(count * n, -1)); es.append(e.reshape(count * n, -1))
        x2s.append(x2.reshape(count * n, -1)); e2s.append(e2.reshape(count * n, -1))
        sizes += [n] * count
        rps.append(rp[1:] + edges)
        cols.append(ci)
        edges += len(ci)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cat = lambda v: np.ascontiguousarray(np.concatenate(v))
    return dict(x=cat(xs), e=cat(es), x2=cat(x2s), e2=cat(e2s), offs=offs, row_ptr=cat(rps).astype(np.int32),
                col_idx=cat(cols).astype(np.int32))


def _graph(t):
    return t['offs'], t['row_ptr'], t['col_idx']


def _oracle_q(spec, P, x, e, graph):
    M = oc.csr_to_matrix(*graph, dtype=np.float64)
    return oc.forward(ospec(spec), P, np.asarray(x, np.float64), np.asarray(e, np.float64), M)[0]


def _unit_scale_head(spec, P, x, e, graph):
    q = _oracle_q(spec, P, x, e, graph)
    s = q.std()
    P['dense'][3] = {k: (v / s).astype(np.float32).astype(np.float64) for k, v in P['dense'][3].items()}
    return P, q / s


def _graph_of_row(offs):
    return np.repeat(np.arange(len(offs) - 1), np.diff(offs))


def _actions_rewards(rng, q, qn, offs, w):
    """actions [R] uniform in 0..3; reward[g] = median over the graph's rows of (q[r, a] - gamma max q'[r]) + U(-w, w)"""
    R, B = q.shape[0], len(offs) - 1
    action = rng.integers(0, 4, size=R)
    d = q[np.arange(R), action] - GAMMA * qn.max(axis=1)
    reward = np.array([np.median(d[offs[g]:offs[g + 1]]) for g in range(B)]) + rng.uniform(-w, w, size=B)
    return action.astype(np.int32), reward.astype(np.float64)


def _oracle_of(spec, P_on, P_tg, t, n_global, what, min_share=MIN_BRANCH_SHARE):
    """targets by the rule row by row (the reward of the row's graph), util.oracle_step on them, the branch shares asserted"""
    graph = _graph(t)
    R = t['x'].shape[0]
    q, qn = _oracle_q(spec, P_on, t['x'], t['e'], graph), _oracle_q(spec, P_tg, t['x2'], t['e2'], graph)
    y = q.copy()
    y[np.arange(R), t['action']] = t['reward'][_graph_of_row(t['offs'])] + GAMMA * qn.max(axis=1)
    step = oracle_step(spec, P_on, t['x'], t['e'], graph, y, n_denominator=n_global)
    assert np.array_equal(step['q'], q)
    untouched = np.ones(q.shape, bool)
    untouched[np.arange(R), t['action']] = False
    err = (y - q)[~untouched]
    quad = float((np.abs(err) < 1.0).mean())
    print("%s: Huber branches of the %d replaced entries: quadratic %.3f, linear %.3f (|err| median %.3f, max %.3f; q std %.3f)"
          % (what, err.size, quad, 1.0 - quad, np.median(np.abs(err)), np.abs(err).max(), q.std()))
    assert quad >= min_share and 1.0 - quad >= min_share, (what, quad)
    return dict(y=y, step=step, untouched=untouched)


def _draw(seed):
    pools, F, L, w, B, R = CASES[seed]
    spec = _spec(F, L)
    rng = np.random.default_rng(seed)
    P_on, P_tg = f32_params(spec, rng), f32_params(spec, rng)
    t = _inputs(rng, pools)
    assert len(t['offs']) - 1 == B and t['x'].shape[0] == R == t['offs'][-1]
    P_on, q = _unit_scale_head(spec, P_on, t['x'], t['e'], _graph(t))
    P_tg, qn = _unit_scale_head(spec, P_tg, t['x2'], t['e2'], _graph(t))
    t['action'], t['reward'] = _actions_rewards(rng, q, qn, t['offs'], w)
    t.update(spec=spec, P_on=P_on, P_tg=P_tg)
    return t


@functools.lru_cache(maxsize=None)
def _case(seed, n_global=None):
    """(draw, oracle) of a case -- computed once, shared by the tests on that draw and never modified"""
    d = _draw(seed)
    return d, _oracle_of(d['spec'], d['P_on'], d['P_tg'], d, n_global, "case %d" % seed)


# ------------------------------------------------------------------------------------------------ the engines
def _device_batches(eng, t):
    """s and s' in HBM: two batches that share graph_off, row_ptr and col_idx (the contract of the ragged replay step)"""
    import torch
    B = len(t['offs']) - 1
    sb = eng.to_device(PackedBatch(B, 0, v2xgnn.pack_xe(t['x'], t['e']), t['row_ptr'], t['col_idx'], graph_off=t['offs']))
    xe2 = torch.from_numpy(v2xgnn.pack_xe(t['x2'], t['e2'])).to(sb.device)
    sn = DeviceBatch.from_tensors(B, 0, xe2, sb.row_ptr, sb.col_idx, sb.max_edges, graph_off=sb.graph_off, max_nodes=sb.max_nodes)
    return sb, sn


def _run_step(t, switches, n_global=None, y_buffer=True, twin=False, what=""):
    """One dqn_step of a fresh engine pair created under `switches` -> dict(y, loss, grad, weights, info[, twin_*])"""
    import torch
    spec = t['spec']
    online, target = _engine(spec, switches), _engine(spec, switches)
    w_on = oc.params_to_list(t['P_on'])
    online.set_weights(w_on)
    target.set_weights(oc.params_to_list(t['P_tg']))
    sb, sn = _device_batches(online, t)
    online.validate(sb)
    info = online.path_info(sb)
    print("%s: F=%d L=%d B=%d R=%d %s  %s" % (what, spec.feat_dim, spec.n_mp_layers, sb.n_graphs, sb.n_rows, switches or "",
                                               " ".join("%s=%s" % kv for kv in sorted(info.items()))))
    a_dev = torch.from_numpy(t['action']).cuda()
    r_dev = torch.from_numpy(t['reward']).cuda()
    y = torch.empty((sb.n_rows, 4), dtype=torch.float32, device="cuda") if y_buffer else None
    loss = online.dqn_step(target, sb, sn, a_dev, r_dev, GAMMA, y_out=y, n_global=n_global)
    online.check_errors()
    out = dict(info=info, loss=loss.cpu().numpy(), grad=online.get_grad_flat(), weights=online.get_weights(),
               y=None if y is None else y.cpu().numpy())
    assert out['loss'].shape == (1,) and online.get_optimizer_state()[2] == 1
    if twin:
        tw = _engine(spec, switches)
        tw.set_weights(w_on)
        out['twin_loss'] = tw.forward_backward(sb, y, n_global=n_global or sb.n_rows).cpu().numpy()
        out['twin_grad'] = tw.get_grad_flat()
        tw.close()
    online.close()
    target.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("seed", sorted(CASES))
def test_a_one_step_vs_oracle(seed):
    what = "A%d" % seed
    d, ref = _case(seed)
    if seed == 2001:
        assert min(np.diff(d['offs'])) < 16 < max(np.diff(d['offs']))
    if seed == 2002:
        assert d['x'].shape[0] > 320 and CASES[seed][0][1][1] == 0
    out = _run_step(d, {}, twin=True, what=what)
    _check_against_oracle(d['spec'], d['P_on'], ref, out, what)
    assert_grad_close(out['grad'], out['twin_grad'], what + ": gradient of the replay step against forward_backward on its targets")
    assert_close(out['loss'], out['twin_loss'], LOSS_RTOL, LOSS_ATOL, what + ": loss of the replay step against forward_backward")


# ---------------------------------------------------------------------------------------------------------------- B
def test_b_two_target_forms_agree():
    d, ref = _case(2001)
    outs = {}
    for form, sw in (("in-kernel", {}), ("k_dqn_targets_ragged", dict(V2X_DQN_FUSED_TARGETS=0))):
        outs[form] = _run_step(d, sw, what="B " + form)
        _check_against_oracle(d['spec'], d['P_on'], ref, outs[form], "B " + form)
        nobuf = _run_step(d, sw, y_buffer=False, what="B %s, y_out=None" % form)
        assert np.array_equal(nobuf['loss'], outs[form]['loss']), form
        assert all(np.array_equal(a, b) for a, b in zip(nobuf['weights'], outs[form]['weights'])), form
        assert np.array_equal(nobuf['grad'], outs[form]['grad']), form
    assert outs["in-kernel"]['info']['mlp'] == "train_wg"          # (otherwise both runs took the three-launch form)
    ya, yb = outs["in-kernel"]['y'], outs["k_dqn_targets_ragged"]['y']
    replaced = ~ref['untouched']
    assert np.array_equal(ya[replaced].view(np.uint32), yb[replaced].view(np.uint32))
    assert_grad_close(outs["in-kernel"]['grad'], outs["k_dqn_targets_ragged"]['grad'], "B: gradients of the two forms")


# ---------------------------------------------------------------------------------------------------------------- C
def test_c_n_global_of_twice_the_rows_halves_loss_and_gradient():
    d, _ = _case(2001)
    R = d['x'].shape[0]
    one = _run_step(d, {}, what="C default")
    explicit = _run_step(d, {}, n_global=R, what="C n_global=R")
    assert np.array_equal(one['loss'], explicit['loss']) and np.array_equal(one['grad'], explicit['grad'])    # the default counts ROWS
    two = _run_step(d, {}, n_global=2 * R, what="C n_global=2R")
    assert np.array_equal(one['y'], two['y'])
    # 1 / (n C) is rounded to fp32 once per launch: a power of two apart, up to that rounding and the sums' own
    assert_close(two['loss'], 0.5 * one['loss'], 1e-6, 0.0, "C: loss at twice the denominator")
    assert_grad_close(two['grad'], 0.5 * one['grad'], "C: gradient at twice the denominator")
    _, ref2 = _case(2001, 2 * R)
    _check_against_oracle(d['spec'], d['P_on'], ref2, two, "C n_global=2R")


# ---------------------------------------------------------------------------------------------------------------- D
def test_d_three_steps_hipgraph_replay_is_bitwise_eager():
    import torch
    pools, F, L, w = CASES[2001][:4]
    d, _ = _case(2001)
    spec = d['spec']
    rng = np.random.default_rng(2101)
    data = [d]
    for _ in range(2):
        t = _inputs(rng, pools)
        t['action'] = rng.integers(0, 4, size=t['x'].shape[0]).astype(np.int32)
        t['reward'] = rng.normal(0.0, 1.0, size=len(t['offs']) - 1)
        data.append(t)
    res = []
    for use_graph in (False, True):
        online, target = _engine(spec, {}, use_graph=use_graph), _engine(spec, {}, use_graph=use_graph)
        online.set_weights(oc.params_to_list(d['P_on']))
        target.set_weights(oc.params_to_list(d['P_tg']))
        with torch.cuda.stream(torch.cuda.Stream()):
            sb, sn = _device_batches(online, d)
            a_dev = torch.zeros(sb.n_rows, dtype=torch.int32, device="cuda")
            r_dev = torch.zeros(sb.n_graphs, dtype=torch.float64, device="cuda")
            y = torch.empty((sb.n_rows, 4), dtype=torch.float32, device="cuda")
            out = []
            for step, t in enumerate(data):
                sb.xe.copy_(torch.from_numpy(v2xgnn.pack_xe(t['x'], t['e'])))          # same device buffers, new contents
                sn.xe.copy_(torch.from_numpy(v2xgnn.pack_xe(t['x2'], t['e2'])))
                sb.col_idx.copy_(torch.from_numpy(t['col_idx']))
                a_dev.copy_(torch.from_numpy(t['action']))
                r_dev.copy_(torch.from_numpy(t['reward']))
                loss = online.dqn_step(target, sb, sn, a_dev, r_dev, GAMMA, y_out=y)
                out.append((loss.cpu().numpy(), y.cpu().numpy().copy()))
                if step == 1:
                    target.copy_weights_from(online)
            torch.cuda.synchronize()
        online.check_errors()
        assert online.get_optimizer_state()[2] == 3
        res.append((out, online.get_flat()))
        online.close()
        target.close()
    for (l0, y0), (l1, y1) in zip(res[0][0], res[1][0]):
        assert np.isfinite(l0).all() and np.array_equal(l0, l1) and np.array_equal(y0, y1)
    assert np.array_equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------- E
def test_e_target_rule_on_special_values_per_graph_rewards():
    """graphs of 1, 2, 3, 4 and 6 rows (the 16 crafted rows in order), one reward each; a 70-row graph behind them, whose rows
    the wave reaches in its second pass"""
    import ctypes as C
    import torch
    lib = v2xgnn.load_library()
    rng = np.random.default_rng(33)
    sizes = [1, 2, 3, 4, 6, 70]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    R, B = int(offs[-1]), len(sizes)
    qn = np.concatenate([SPECIAL_ROWS, SPECIAL_ROWS[rng.integers(0, len(SPECIAL_ROWS), size=70)]])
    assert qn.shape[0] == R
    reward = np.concatenate([SPECIAL_REWARDS, [0.375]])
    q = rng.normal(0.0, 1.0, size=(R, 4)).astype(np.float32)
    action = rng.integers(0, 4, size=R).astype(np.int32)
    action[:16] = np.arange(16) % 4
    g = _graph_of_row(offs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q_d, qn_d, a_d, r_d, o_d = dev(q), dev(qn), dev(action), dev(reward), dev(offs)
    for gamma in SPECIAL_GAMMAS:
        y = torch.full((R + 1, 4), -77.0, dtype=torch.float32, device="cuda")
        rc = lib.v2x_dqn_targets_ragged(q_d.data_ptr(), qn_d.data_ptr(), a_d.data_ptr(), r_d.data_ptr(), C.c_double(gamma),
                                        o_d.data_ptr(), B, R, 4, y.data_ptr(), None)
        v2xgnn.lib.check(lib, rc, None)
        torch.cuda.synchronize()
        want = np.array(q, np.float32)
        with np.errstate(all="ignore"):
            for row in range(R):
                want[row, action[row]] = np.float32(reward[g[row]] + gamma * np.float64(np.amax(qn[row])))
        got = y.cpu().numpy()
        _assert_same_floats(got[:R], want, "k_dqn_targets_ragged, gamma %g" % gamma)
        assert (got[R] == -77.0).all()
    with pytest.raises(v2xgnn.lib.V2XInvalidArgument, match="dqn_targets_ragged: bad argument"):
        v2xgnn.lib.check(lib, lib.v2x_dqn_targets_ragged(q_d.data_ptr(), qn_d.data_ptr(), a_d.data_ptr(), r_d.data_ptr(),
                                                         C.c_double(0.5), None, B, R, 4, q_d.data_ptr(), None), None)


# ---------------------------------------------------------------------------------------------------------------- F
def test_f_refusals():
    import torch
    d, _ = _case(2003)
    spec = d['spec']
    online, target = _engine(spec, {}), _engine(spec, {})
    sb, sn = _device_batches(online, d)
    a_dev = torch.from_numpy(d['action']).cuda()
    r_dev = torch.from_numpy(d['reward']).cuda()
    other = DeviceBatch.from_tensors(sn.n_graphs, 0, sn.xe, sn.row_ptr, sn.col_idx, sn.max_edges, graph_off=sb.graph_off.clone(),
                                     max_nodes=sn.max_nodes)
    with pytest.raises(v2xgnn.lib.V2XInvalidArgument, match="graph_off must be the same device pointer"):
        online.dqn_step(target, sb, other, a_dev, r_dev, GAMMA)
    fixed_spec = GnnSpec(n_nodes=20, feat_dim=spec.feat_dim, n_mp_layers=spec.n_mp_layers, share_weights=True)
    fixed = _engine(fixed_spec, {})
    with pytest.raises(v2xgnn.lib.V2XInvalidArgument, match="both be variable_graphs models or both fixed-size"):
        online.dqn_step(fixed, sb, sn, a_dev, r_dev, GAMMA)
    comm = v2xgnn.lib.Comm()
    with pytest.raises(v2xgnn.lib.V2XInvalidArgument, match="dqn_step_dp: variable_graphs models are not supported"):
        online.dqn_step_dp(target, sb, sn, a_dev, r_dev, GAMMA, comm, sb.n_rows)
    assert online.get_optimizer_state()[2] == 0                   # no refusal took a step
    online.dqn_step(target, sb, sn, a_dev, r_dev, GAMMA)          # ... and the pair still works
    online.check_errors()
    assert online.get_optimizer_state()[2] == 1
    for e in (online, target, fixed):
        e.close()
