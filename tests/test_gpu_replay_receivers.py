"""GPU: the replay memory that stores a transition's adjacency as its receivers (rl/replay.py ReceiverReplay) and its
one-launch gather (v2x_replay_gather_recv, csrc/kernels.hpp k_replay_gather_recv) -- byte for byte the existing
DeviceReplay where both hold the graphs (up to 31 links), the host packer beyond, the replay step of an Agent against the
host path at 32 and 40 links, and a short training run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _adjacency(recv):
    """Agent.adjacency (BS_brain.py:441-445) for given receivers [n]: ones, except the diagonal and Adj[receiver of q, q]"""
    n = len(recv)
    adj = np.ones((n, n)) - np.eye(n)
    for q in range(n):
        if recv[q] != q:
            adj[recv[q], q] = 0
    return adj


def _receivers(rng, n, own=()):
    r = rng.integers(0, n - 1, size=n)
    r = r + (r >= np.arange(n))
    r[list(own)] = list(own)
    return r


def _transition(rng, n, own=()):
    return dict(x=rng.normal(size=(n, 9)), e=rng.normal(size=(n, 4)), adj=_adjacency(_receivers(rng, n, own)),
                a=rng.integers(0, 4, size=n), r=float(rng.normal()), x2=rng.normal(size=(n, 9)), e2=rng.normal(size=(n, 4)))


def _feed(reps, log, flush_rule):
    """the same add / add_many calls into every memory of reps: single transitions, and blocks of three through add_many"""
    i = 0
    while i < len(log):
        block = log[i:i + 3] if i % 5 == 2 else log[i:i + 1]
        for rep in reps:
            if len(block) == 1:
                t = block[0]
                rep.add(t['x'], t['e'], t['adj'], t['a'], t['r'], t['x2'], t['e2'])
            else:
                st = lambda k: np.stack([t[k] for t in block])
                rep.add_many(st('x'), st('e'), st('adj'), st('a'), np.array([t['r'] for t in block]), st('x2'), st('e2'))
            if flush_rule(i):
                rep.flush()
        i += len(block)


def _arrays(sample):
    sb, sb_next, action, reward = sample
    c = lambda t: t.cpu().numpy()
    return dict(xe=c(sb.xe), xe_next=c(sb_next.xe), action=c(action), reward=c(reward), row_ptr=c(sb.row_ptr),
                col_idx=c(sb.col_idx)[:sb.n_edges], n_edges=sb.n_edges, n_edges_next=sb_next.n_edges,
                col_idx_next=c(sb_next.col_idx)[:sb_next.n_edges], row_ptr_next=c(sb_next.row_ptr))


# ---------------------------------------------------------------------------- 1. against the existing memory
@pytest.mark.parametrize("n", [5, 20])
@pytest.mark.parametrize("own", [False, True])
def test_receiver_memory_is_the_existing_memory_byte_for_byte(n, own):
    """ring capacity 37, 90 transitions, uneven flushes, 50 draws with repeats: every array of the minibatch equal.  own:
    transitions with a link that is its own receiver at the first, a middle and the last position of the minibatch, one
    of them with two such links; then a regular minibatch from the same memories (the buffers change roles)."""
    from v2xgnn.rl.replay import DeviceReplay, ReceiverReplay
    rng = np.random.default_rng(3 + n)
    cap = 37
    # FIFO position i of the full ring = log[90 - 37 + i]
    special = {60: (3,), 70: (0, n - 1), 85: (n - 2,)} if own else {}
    log = [_transition(rng, n, special.get(i, ())) for i in range(90)]
    old, new = DeviceReplay(cap, n), ReceiverReplay(cap, n)
    _feed((old, new), log, lambda i: i % 7 == 3)
    assert len(old) == len(new) == cap
    idx = rng.integers(0, cap, size=50)
    if own:
        idx[idx == 7] = 8
        idx[idx == 17] = 18
        idx[idx == 32] = 31
        idx[0], idx[25], idx[49] = 7, 17, 32                             # log[60], log[70] (two own links), log[85]
    draws = [idx]
    if own:
        reg = rng.integers(0, cap, size=50)
        reg[np.isin(reg, (7, 17, 32))] = 1
        draws.append(reg)                                                # ... and an all-regular minibatch afterwards
        draws.append(idx)
    for d in draws:
        a, b = _arrays(old.sample(d)), _arrays(new.sample(d))
        for k in a:
            assert np.array_equal(a[k], b[k]), (k, n, own)
        regular = not np.isin(d, (7, 17, 32)).any() or not own
        sb = new.sample(d)[0]
        assert sb.max_edges == (n * (n - 2) if regular else n * (n - 1))
        assert sb.n_edges == 50 * n * (n - 2) + (0 if regular else 4)


def test_receiver_memory_keeps_its_output_buffers():
    """two regular minibatches of one size come back in the same tensors and the same batch descriptors (what a captured
    replay step replays on)"""
    from v2xgnn.rl.replay import ReceiverReplay
    rng = np.random.default_rng(1)
    rep = ReceiverReplay(64, 12)
    _feed((rep,), [_transition(rng, 12) for _ in range(30)], lambda i: False)
    s0 = rep.sample(rng.integers(0, 30, size=16))
    first = _arrays(s0)
    s1 = rep.sample(rng.integers(0, 30, size=16))
    assert s0[0] is s1[0] and s0[1] is s1[1] and s0[2].data_ptr() == s1[2].data_ptr()
    assert not np.array_equal(first['xe'], _arrays(s1)['xe'])


# ---------------------------------------------------------------------------- 2. beyond 31 links, against the host packer
def _check_against_packer(rep, kept, idx):
    from v2xgnn import PackedBatch
    got = _arrays(rep.sample(idx))
    st = lambda k: np.stack([kept[i][k] for i in idx])
    ref, ref_next = PackedBatch.from_dense(st('x'), st('e'), st('adj')), PackedBatch.from_dense(st('x2'), st('e2'), st('adj'))
    assert got['n_edges'] == ref.n_edges == got['n_edges_next']
    assert np.array_equal(got['row_ptr'], ref.row_ptr) and np.array_equal(got['col_idx'], ref.col_idx)
    assert np.array_equal(got['row_ptr_next'], ref.row_ptr) and np.array_equal(got['col_idx_next'], ref.col_idx)
    assert got['xe'].dtype == np.float32 and np.array_equal(got['xe'], ref.xe) and np.array_equal(got['xe_next'], ref_next.xe)
    assert np.array_equal(got['action'], st('a')) and np.array_equal(got['reward'], np.array([kept[i]['r'] for i in idx]))
    return ref


@pytest.mark.parametrize("n", [32, 33, 64, 65, 128])
@pytest.mark.parametrize("K", [1, 5, 17])
def test_receiver_memory_beyond_31_links_is_the_host_packer(n, K):
    """the first refused size, an odd one, one wave of sources and one past it, the limit; rings that wrap; regular and
    own-receiver graphs mixed (own receivers at link 0, at the last link, at links 63 / 64 where the masks meet)"""
    from v2xgnn.rl.replay import ReceiverReplay
    rng = np.random.default_rng(100 * n + K)
    cap, total = 11, 29                                                  # wraps the ring twice
    edge = [q for q in (0, 63, 64, n - 1) if q < n]
    own_of = {20: (0,), 22: tuple(edge), 25: (n - 1, n // 2), 27: (1, 2, 3)}
    log = [_transition(rng, n, own_of.get(i, ())) for i in range(total)]
    rep = ReceiverReplay(cap, n)
    _feed((rep,), log, lambda i: i % 4 == 1)
    assert len(rep) == cap
    kept = log[-cap:]                                                    # FIFO position i = log[18 + i]: own at 2, 4, 7, 9
    regular = [i for i in range(cap) if i not in (2, 4, 7, 9)]
    _check_against_packer(rep, kept, rng.choice(regular, size=K))        # every graph regular
    idx = rng.integers(0, cap, size=K)
    idx[0] = 4                                                           # own-receiver graphs first ...
    idx[-1] = (4, 9)[K > 1]                                              # ... and last
    if K > 2:
        idx[K // 2] = 7
    ref = _check_against_packer(rep, kept, idx)
    assert ref.n_edges > K * n * (n - 2)
    _check_against_packer(rep, kept, rng.choice(regular, size=K))        # and regular again, in the same buffers


@pytest.mark.parametrize("n,feat,layers", [(33, 32, 1), (40, 16, 2), (65, 64, 2), (128, 64, 2)])
def test_forward_of_a_sampled_batch_is_the_forward_of_the_host_batch(n, feat, layers):
    """(65 and 128 links at F = 64: the CSR v2x_csr_from_recv builds on the device feeds k_adj_masks and the dense
    aggregation, own-receiver rows of in-degree n - 1 included; the forward is also held to the float64 oracle)"""
    from v2xgnn import GnnEngine, GnnSpec
    from v2xgnn.rl.replay import ReceiverReplay
    from oracle import compact as oc
    from util import f32_params, ospec, assert_fwd_close
    rng = np.random.default_rng(n)
    log = [_transition(rng, n, (5,) if i == 6 else ()) for i in range(12)]
    assert log[6]['adj'][:, 5].sum() == n - 1 and all(t['adj'].sum() == n * (n - 2) for i, t in enumerate(log) if i != 6)
    rep = ReceiverReplay(32, n)
    _feed((rep,), log, lambda i: False)
    spec = GnnSpec(n_nodes=n, feat_dim=feat, n_mp_layers=layers)
    eng = GnnEngine(spec)
    P = f32_params(spec, np.random.default_rng(1))
    eng.set_weights(oc.params_to_list(P))
    for idx in (np.array([0, 1, 2, 3, 3, 11, 9]), np.array([4, 6, 6, 0, 10])):      # regular; with an own-receiver graph
        ref = _check_against_packer(rep, log, idx)
        sb = rep.sample(idx)[0]
        q = eng.forward(sb).cpu().numpy()
        assert np.array_equal(q, eng.forward(ref))
        if n > 40:
            assert eng.path_info(sb)["aggregation"].startswith("dense"), eng.path_info(sb)
        f32 = lambda k: np.concatenate([log[i][k] for i in idx]).astype(np.float32).astype(np.float64)
        M = oc.csr_to_matrix(*oc.adj_to_csr(np.stack([log[i]['adj'] for i in idx])), dtype=np.float64)
        assert_fwd_close(q, oc.forward(ospec(spec), P, f32('x'), f32('e'), M)[0], "forward of the sampled batch against the oracle")
    eng.close()


# ---------------------------------------------------------------------------- 3. the replay step
@pytest.mark.parametrize("n_veh,feat,batch,n_trans", [(32, 16, 64, 40), (40, 32, 48, 130)])
def test_receiver_replay_step_equals_host_replay(n_veh, feat, batch, n_trans):
    """test_gpu_rl.test_device_replay_equals_host_replay's procedure and bounds, host Memory against the receiver memory:
    same sampled transitions, same targets, same update."""
    from test_gpu_rl import _setup
    from v2xgnn.rl.replay import ReceiverReplay
    out = []
    for dev in (False, 'receivers'):
        agent, env, cfg = _setup(21, batch=batch, n_veh=n_veh, feat=feat, device_replay=dev)
        assert isinstance(agent.device_replay, ReceiverReplay) == (dev == 'receivers')
        assert (agent.device_replay is None) == (dev is False)
        agent.num_Episodes, agent.num_Train_Step = 1, 4
        steps = []
        for _ in range(3):                                  # first replay samples with replacement, later ones without
            agent.generate_d2d_transition(n_trans)
            result, q_mean, q_max, _, _ = agent.replay()
            steps.append((np.array([result.history['D%d_Decide_Output_loss' % (k + 1)][0] for k in range(n_veh)]),
                          q_mean, q_max))
        out.append((steps, np.concatenate([w.ravel() for w in agent.brain.model.get_weights()])))
    rel = lambda a, b: float(np.max(np.abs(a - b) / (1e-30 + np.abs(a))))
    for s, ((l0, m0, x0), (l1, m1, x1)) in enumerate(zip(out[0][0], out[1][0])):
        print("step %d: loss max rel %.3e abs %.3e, q mean rel %.3e, q max rel %.3e"
              % (s, rel(l0, l1), np.max(np.abs(l0 - l1)), rel(m0, m1), rel(x0, x1)))
    print("weights: max abs %.3e, max rel %.3e" % (np.max(np.abs(out[0][1] - out[1][1])), rel(out[0][1], out[1][1])))
    for (l0, m0, x0), (l1, m1, x1) in zip(out[0][0], out[1][0]):
        assert np.allclose(l0, l1, rtol=2e-4, atol=1e-6)
        assert np.allclose(m0, m1, rtol=1e-5, atol=1e-6) and np.allclose(x0, x1, rtol=1e-5, atol=1e-6)
    assert np.allclose(out[0][1], out[1][1], rtol=1e-3, atol=2e-5)


# ---------------------------------------------------------------------------- 4. a short training run
@pytest.mark.parametrize("envs", [0, 5])
def test_training_run_at_32_links_stores_in_the_device_memory(envs):
    """Agent.train(1, 3) at 32 links (one simulator: add(); five batched simulators: add_many() through the array path of the
    batched rollout): 150 transitions in the HBM memory, none on the host (its list holds only the FIFO bookkeeping's
    placeholders), finite losses."""
    import random
    from test_gpu_rl import _setup
    from v2xgnn.rl import Agent, RL_Config
    from v2xgnn.rl.replay import ReceiverReplay
    if envs:
        from v2xgnn.rl.train import start_env_batched
        random.seed(5)
        np.random.seed(5)
        cfg = RL_Config()
        cfg.set_train_value(16, 0.5, 64, 1, 0.1)
        env = start_env_batched(32, envs, 5)
        agent = Agent(32, env.n_RB, env.n_Neighbor, 16, env, cfg, seed=5, device_replay='receivers')
        assert agent._packed_rollouts() is False
    else:
        agent, env, cfg = _setup(5, batch=64, n_veh=32, feat=16, device_replay='receivers')
    rep = agent.device_replay
    assert isinstance(rep, ReceiverReplay)
    loss, reward_step, reward_ep, q_mean, q_max, _, _ = agent.train(1, 3)
    assert len(rep) == 150 and rep.size + rep._n_staged == 150
    assert all(s is None for s in agent.memory.samples)                  # no transition lives on the host
    assert loss.shape == (32, 1, 3) and np.all(np.isfinite(loss)) and np.all(loss >= 0)
    assert np.all(np.isfinite(q_mean)) and np.all(np.isfinite(q_max)) and np.all(np.isfinite(reward_step))
    assert rep.recv.shape[1] == 32 and not hasattr(rep, 'col') and not hasattr(rep, 'mask')
