"""Host: the draws of tests/test_gpu_links_41_128.py (whole-model oracle parity at 41 to 128 links) held to their conditions
with the oracle alone, so that a draw is known to be usable before it reaches a GPU.  This file owns the two case tables and
the draws; the GPU file imports them.

A  fit-step cases (CASES_A, draw_a).  Every case is ONE seeded draw, default_rng(4100 + case number): f32_params,
   random_inputs for x and e, the case's adjacency, for case 13 a Neighbor_Input ~ N(0, 0.5) (test_gpu_depth._draw's), and the
   N(0, 1.2) noise that is added to the forward's own q to give the targets.  Here the forward whose q the targets sit around
   is an fp32 restatement of the oracle -- the same oracle.compact functions with parameters and inputs cast to float32 --
   and the float64 loss is differentiated at that q (q_at), exactly what the GPU file does with the kernels' q.  Asserted:
   the restatement's forward within FWD_RTOL / FWD_ATOL, its gradient within GRAD_RTOL / GRAD_ATOL_REL with at most
   MAX_GATE_FLIPS gates (assert_grads_match_oracle), and every gradient array of the oracle with a scale above 1e-12 -- but
   for the one array that is zero by construction: stage 0's W3 multiplies the Neighbor_Input, which only case 13 feeds,
   and must then be exactly zero.  All cases have L <= 3: at 128 links and L = 4 the activations reach 4e8 and this very
   restatement fails the gradient bound on an array of scale 1e-18.
   The topologies: "reference" (oracle.compact.random_topology), "random" (density 0.5), "indegree2", "receivers" (case 4:
   Agent.adjacency of random receivers, links 0, 31, 32 and 64 of graphs 1 and 5 their own receivers: in-degree n - 1 beside
   n - 2) and "mixed" (case 14, mixed_adjacency below).  forms_of gives the form k_agg_dense takes per graph, from its rule
   n * n - n_edges <= 8 * n and the edge counts.

B  one-call DQN steps (CASES_B): the draw of test_gpu_dqn_step._draw, default_rng(1000 + case number), through that module's
   own case table, which this file extends.  _oracle_of asserts at least MIN_BRANCH_SHARE of the replaced entries on either
   Huber branch and prints the shares.

C  three DQN steps on cases 102 and 105 by section C of test_gpu_dqn_step.py, at learning rate C_LR = 1e-5 instead of the
   default 1e-3.  At 128 links the scheme is unusable at 1e-3, and that shows from the oracle alone (its own float64 Adam in
   the engine's place): one step of 1e-3 on every weight takes the standard deviation of q from 1.0 to 114 (case 102) and
   to 5279 (case 105, shared weights: 1024 rows move every weight the same way).  Case 102's later steps then have 0.010
   and 0.023 of the replaced entries on the quadratic branch, against the 0.10 that section C asks of them
   (MIN_BRANCH_SHARE_LATER_STEPS); case 105 keeps its shares, but target - q[a] of order 1 is then the difference of two
   fp32 numbers of order 5e3, and the fp32 restatement of the oracle misses the gradient bound 6.8 and 7.6 times over at
   steps 1 and 2.  At 1e-5 q stays at unit scale for case 102 (std 1.0, 1.7, 1.0) and within 60 for case 105, the
   quadratic shares are 0.64, 0.37, 0.68 and 0.59, 0.52, 0.26, and the restatement's gradient is within 0.11 of the bound at
   every step.  The test below holds the three draws per case to section C's shares and the restatement to the gradient
   bound."""
import functools

import numpy as np
import pytest

from v2xgnn import GnnSpec
from oracle import compact as oc
from util import (ospec, f32_params, random_inputs, fixed_indegree_adj, oracle_step, assert_fwd_close,
                  assert_grads_match_oracle, FWD_RTOL, FWD_ATOL, MAX_GATE_FLIPS)
import test_gpu_dqn_step as T

AD_COMPL_PER_ROW = 8          # csrc/kernels_wide.hpp: a graph with at most 8 n non-edges takes the complement walk
MIN_GRAD_SCALE = 1e-12
OWN_LINKS, OWN_GRAPHS = (0, 31, 32, 64), (1, 5)
SPARSE_DESTS, SPARSE_INDEGREE = (0, 33, 79), 3

LW = dict(graph_layers="layerwise", handoff="row-major")
DENSE, GATHER = "dense(complement-or-mfma-per-graph)", "edge-gather"
# (dense0_dw, from dense0_rides of csrc/v2xgnn.hip: k_wgrad needs F = 64, the embed layer riding on the stage roles and whole
#  16-row groups per slot -- B % 16 == 0 with per-node weights, B N % 16 == 0 with shared ones -- at no more than 12 tiles per
#  MLP workgroup)
CASES_A = {  # number: (N, F, L, shared, B, topology, n_global, path_info fields the case must show)
    1: (41, 64, 2, False, 32, "reference", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    2: (64, 64, 2, False, 17, "reference", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    3: (65, 64, 2, False, 16, "random", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    4: (65, 64, 2, False, 9, "receivers", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    5: (96, 32, 2, False, 9, "reference", None, dict(LW, aggregation=GATHER, mlp="train_wg")),
    6: (97, 64, 3, False, 5, "reference", 15, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    7: (100, 128, 2, False, 5, "reference", None, dict(LW, aggregation=DENSE, mlp="fwd+bwd", dense0_dw="k_wide_wgrad")),
    8: (128, 64, 2, False, 17, "reference", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    9: (128, 64, 2, False, 16, "random", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    10: (128, 64, 2, True, 8, "reference", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    11: (128, 16, 2, False, 3, "random", None, dict(LW, aggregation=GATHER, mlp="train_wg")),
    12: (128, 64, 2, False, 8, "indegree2", None, dict(LW, aggregation=GATHER, mlp="train_wg")),
    13: (100, 64, 2, False, 9, "reference+nbr", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    14: (80, 64, 2, False, 8, "mixed", None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
}

CASES_B = {  # the layout of test_gpu_dqn_step.CASES
    101: (64, 64, 2, False, 16, "reference", {}, None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    102: (128, 64, 2, False, 17, "reference", {}, None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    103: (65, 64, 2, False, 16, "random", {}, None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    104: (100, 32, 1, False, 9, "indegree2", {}, None, dict(LW, aggregation=GATHER, mlp="train_wg")),
    105: (128, 64, 2, True, 8, "reference", {}, None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
    106: (97, 64, 3, False, 5, "reference", {}, 15, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_mlp_train_wg")),
    107: (128, 16, 2, False, 3, "random", {}, None, dict(LW, aggregation=GATHER, mlp="train_wg")),
    108: (41, 64, 2, False, 32, "reference", {}, None, dict(LW, aggregation=DENSE, mlp="train_wg", dense0_dw="k_wgrad")),
}
T.CASES.update(CASES_B)


# ------------------------------------------------------------------------------------------------ adjacencies
def receiver_adjacency(recv):
    """Agent.adjacency of receivers [B, n] -> [B, n, n]: ones, except the diagonal and Adj[receiver of q, q]"""
    B, n = recv.shape
    adj = np.ones((B, n, n)) - np.eye(n)[None]
    adj[np.arange(B)[:, None], recv, np.arange(n)[None, :]] = 0
    return adj


def _receivers(rng, B, n):
    r = rng.integers(0, n - 1, size=(B, n))
    return r + (r >= np.arange(n)[None, :])


def _with_non_edges(rng, n, count):
    """the complete graph without its diagonal, random edges removed until it has `count` non-edges, diagonal included"""
    adj = np.ones((n, n)) - np.eye(n)
    p, q = np.nonzero(adj)
    drop = rng.choice(p.size, size=count - n, replace=False)
    adj[p[drop], q[drop]] = 0
    assert n * n - int(adj.sum()) == count
    return adj


def mixed_adjacency(rng, n):
    """Case 14's eight graphs: 0 and 6 reference; 1 random 0.5; 2 with exactly 8 n non-edges (the last adjacency of the
    complement form); 3 with 8 n + 1 (the first of the MFMA product); 4 without edges; 5 complete; 7 reference, but
    destinations 0, 33 and 79 keep three in-edges each (rows summed directly inside a complement-form graph)"""
    adj = oc.random_topology(rng, 8, n)
    adj[1] = (rng.uniform(size=(n, n)) < 0.5).astype(np.float64)
    adj[2] = _with_non_edges(rng, n, AD_COMPL_PER_ROW * n)
    adj[3] = _with_non_edges(rng, n, AD_COMPL_PER_ROW * n + 1)
    adj[4] = 0.0
    adj[5] = np.ones((n, n)) - np.eye(n)
    for q in SPARSE_DESTS:
        src = np.nonzero(adj[7, :, q])[0]
        adj[7, :, q] = 0.0
        adj[7, rng.choice(src, size=SPARSE_INDEGREE, replace=False), q] = 1.0
    return adj


def forms_of(adj):
    """per graph the form k_agg_dense takes, from its rule and the edge counts"""
    n = adj.shape[1]
    non_edges = n * n - adj.reshape(adj.shape[0], -1).sum(axis=1).astype(np.int64)
    return ["complement" if k <= AD_COMPL_PER_ROW * n else "mfma" for k in non_edges]


# ------------------------------------------------------------------------------------------------ the draw of an A case
@functools.lru_cache(maxsize=None)
def draw_a(n):
    """-> dict(spec, P, x [B, N, 9], e [B, N, 4], adj, nbr [B, N, F] or None, noise [B N, 4], n_global); computed once, shared
    by the tests on that draw and never modified"""
    N, F, L, shared, B, topo, n_global, _ = CASES_A[n]
    rng = np.random.default_rng(4100 + n)
    spec = GnnSpec(n_nodes=N, feat_dim=F, n_mp_layers=L, share_weights=shared)
    P = f32_params(spec, rng)
    x, e, adj = random_inputs(rng, B, N, ref_topology=topo.startswith("reference"), density=0.5)
    nbr = None
    if topo == "receivers":
        recv = _receivers(rng, B, N)
        for g in OWN_GRAPHS:
            recv[g, list(OWN_LINKS)] = OWN_LINKS
        adj = receiver_adjacency(recv)
    elif topo == "indegree2":
        adj = fixed_indegree_adj(rng, B, N, 2)
    elif topo == "mixed":
        adj = mixed_adjacency(rng, N)
    elif topo == "reference+nbr":
        nbr = rng.normal(0, 0.5, size=(B, N, F)).astype(np.float32)
    else:
        assert topo in ("reference", "random"), topo
    noise = rng.normal(0, 1.2, size=(B * N, 4))
    return dict(spec=spec, P=P, x=x, e=e, adj=adj, nbr=nbr, noise=noise, n_global=n_global)


def rows(a):
    return None if a is None else a.reshape(a.shape[0] * a.shape[1], -1)


def oracle_of_a(d, q):
    """targets around q (the forward under test's own output) and the float64 oracle's step differentiated at that q
    -> (y float32 [R, 4], oracle_step(...)); every gradient array's scale asserted from the oracle alone"""
    y = (q + d['noise']).astype(np.float32)
    step = oracle_step(d['spec'], d['P'], rows(d['x']), rows(d['e']), oc.adj_to_csr(d['adj']), y, q_at=q,
                       n_denominator=d['n_global'], nbr=rows(d['nbr']))
    g = step['grads']
    for kind in ('gnn', 'dense'):
        for i, layer in enumerate(g[kind]):
            for name, arr in layer.items():
                if kind == 'gnn' and i == 0 and name == 'W3' and d['nbr'] is None:
                    assert not arr.any()              # multiplies the Neighbor_Input, which this case does not feed
                    continue
                for k in range(arr.shape[0]):
                    assert np.abs(arr[k]).max() > MIN_GRAD_SCALE, ("unusable draw", kind, i, name, k, np.abs(arr[k]).max())
    return y, step


def _fp32_restatement(d):
    """forward, Huber and reverse pass of oracle.compact in float32 -> (q, gradient as a Keras-shaped list)"""
    f4 = np.float32
    os_ = ospec(d['spec'])
    P4 = oc.cast_params(d['P'], f4)
    M = oc.csr_to_matrix(*oc.adj_to_csr(d['adj']), dtype=f4)
    nbr = None if d['nbr'] is None else rows(d['nbr']).astype(f4)
    q, cache = oc.forward(os_, P4, rows(d['x']).astype(f4), rows(d['e']).astype(f4), M, nbr)
    assert q.dtype == f4
    y = (q + d['noise']).astype(f4)
    _, dq = oc.huber_loss_and_grad(os_, q, y, d['n_global'])
    g = oc.backward(os_, P4, cache, dq.astype(f4), probe={})
    return q, oc.params_to_list(oc.cast_params(g, np.float64))


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("n", sorted(CASES_A))
def test_a_draw_is_usable(n):
    N, F, L, shared, B, topo, n_global, _ = CASES_A[n]
    assert 41 <= N <= 128 and L <= 3
    d = draw_a(n)
    adj = d['adj']
    assert adj.shape == (B, N, N)
    if topo == "receivers":
        indeg = adj.sum(axis=1)
        for g in range(B):
            own = list(OWN_LINKS) if g in OWN_GRAPHS else []
            assert (indeg[g, own] == N - 1).all() and (np.delete(indeg[g], own) == N - 2).all()
        assert set(forms_of(adj)) == {"complement"}
    if topo == "mixed":
        non_edges = N * N - adj.reshape(B, -1).sum(axis=1)
        assert non_edges[2] == 8 * N and non_edges[3] == 8 * N + 1 and non_edges[4] == N * N and non_edges[5] == N
        assert forms_of(adj) == ["complement", "mfma", "complement", "mfma", "mfma", "complement", "complement", "complement"]
        assert (adj[7].sum(axis=0)[list(SPARSE_DESTS)] == SPARSE_INDEGREE).all() and 2 * SPARSE_INDEGREE < N
    if topo == "random":
        assert set(forms_of(adj)) == {"mfma"}
    if topo == "indegree2":
        assert (adj.sum(axis=1) == 2).all() and 4 * 2 * N < N * N          # 4 * max_edges < N * N: the edge-gather
    q32, g32 = _fp32_restatement(d)
    _, step = oracle_of_a(d, q32.astype(np.float64))
    ref = step['q']
    ratio = (np.abs(q32 - ref) / (FWD_RTOL * np.abs(ref) + FWD_ATOL * max(1.0, np.abs(ref).max()))).max()
    assert_fwd_close(q32, ref, "A%d: fp32 restatement, forward" % n)
    _, n_cand, n_flip = assert_grads_match_oracle(g32, d['P'], step, "A%d: fp32 restatement, gradient" % n)
    assert n_flip <= MAX_GATE_FLIPS
    print("A%d: N=%d F=%d L=%d B=%d %s: max|q| %.3g, fp32 restatement forward error / bound %.3f, %d gates flipped of %d candidates"
          % (n, N, F, L, B, topo, np.abs(ref).max(), ratio, n_flip, n_cand))


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("n", sorted(CASES_B))
def test_b_draw_has_both_huber_branches(n):
    d, ref = T._case(n)                              # _oracle_of asserts MIN_BRANCH_SHARE on either branch and prints both
    N, B = CASES_B[n][0], CASES_B[n][4]
    assert ref['y'].shape == (B, N, 4) and T.MIN_BRANCH_SHARE == 0.25


# ------------------------------------------------------------------------------------------------ C
C_LR = 1e-5
C_CASES = (102, 105)


def _fp32_dqn_gradient(spec, P_on, P_tg, t):
    """the replay step's gradient from oracle.compact in float32 (both forwards, the target rule, Huber, the reverse pass)
    -> a Keras-shaped list"""
    f4 = np.float32
    os_ = ospec(spec)
    B, N = t['x'].shape[:2]
    M = oc.csr_to_matrix(*oc.adj_to_csr(t['adj']), dtype=f4)
    P4 = oc.cast_params(P_on, f4)
    q, cache = oc.forward(os_, P4, T._flat(t['x']).astype(f4), T._flat(t['e']).astype(f4), M)
    qn, _ = oc.forward(os_, oc.cast_params(P_tg, f4), T._flat(t['x2']).astype(f4), T._flat(t['e2']).astype(f4), M)
    y = q.copy()
    y[np.arange(B * N), t['action'].reshape(-1)] = (np.repeat(t['reward'], N) + T.GAMMA * qn.max(axis=1).astype(np.float64)).astype(f4)
    _, dq = oc.huber_loss_and_grad(os_, q, y, None)
    return oc.params_to_list(oc.cast_params(oc.backward(os_, P4, cache, dq.astype(f4), probe={}), np.float64))


@pytest.mark.parametrize("n", C_CASES)
def test_c_three_steps_keep_both_huber_branches_at_c_lr(n):
    """section C's loop with the oracle's float64 Adam (weights rounded to fp32 after every step) in the engine's place"""
    from oracle.keras_semantics import KerasAdam
    N, F, L, shared, B, topo = CASES_B[n][:6]
    d, _ = T._case(n)
    spec = d['spec']
    rng = np.random.default_rng(2000 + n)
    P_on, P_tg = d['P_on'], d['P_tg']
    opt = KerasAdam(lr=C_LR)
    for step in range(3):
        x, e, adj, x2, e2 = T._inputs(spec, rng, B, topo)
        action, reward = T._actions_rewards(rng, T._oracle_q(spec, P_on, x, e, adj), T._oracle_q(spec, P_tg, x2, e2, adj))
        t = dict(x=x, e=e, adj=adj, x2=x2, e2=e2, action=action, reward=reward)
        ref = T._oracle_of(spec, P_on, P_tg, t, None, "C%d step %d" % (n, step),
                           T.MIN_BRANCH_SHARE if step == 0 else T.MIN_BRANCH_SHARE_LATER_STEPS)
        assert_grads_match_oracle(_fp32_dqn_gradient(spec, P_on, P_tg, t), P_on, ref['step'], "C%d step %d: fp32 restatement" % (n, step))
        P_new = oc.cast_params(P_on, np.float64)
        opt.step(oc.param_arrays(P_new), oc.param_arrays(ref['step']['grads']))
        P_on = oc.cast_params(oc.cast_params(P_new, np.float32), np.float64)
        if step == 1:
            P_tg = P_on
