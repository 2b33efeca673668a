"""GPU: rl/mixed.py's MixedAgent -- one shared-weight Q-network trained on scenarios of 4 and 8 links at once (3 and 2
simulators, minibatches of 16 graphs, 16 features).

  * train(1, 10) collects 10 x 10 x 5 = 500 transitions: finite non-negative losses, the target network synced at the 500th,
    stored = 500 - dropped;
  * one replay() equals a fresh engine pair's dqn_step on the numpy assembly of last_minibatch (the pools' storage read back),
    bit for bit in loss and weights;
  * the Q rows of each environment in the ONE mixed forward agree with a forward of that environment's graphs alone.
"""
import numpy as np
import pytest

import v2xgnn
from v2xgnn import GnnEngine, PackedBatch
from v2xgnn.engine import DeviceBatch
from util import assert_fwd_close
from test_gpu_replay_mixed import numpy_assembly

pytestmark = pytest.mark.gpu

SIZES, SIMS, BATCH, FEAT = (4, 8), (3, 2), 16, 16


def _agent(seed):
    from v2xgnn.rl.mixed import MixedAgent
    from v2xgnn.rl.sim_config import RL_Config
    from v2xgnn.rl.train import start_env_batched
    np.random.seed(seed)
    cfg = RL_Config()
    cfg.set_train_value(FEAT, 0.5, BATCH, 1, 0.1)
    envs = [start_env_batched(n, E, seed + 1000 * k) for k, (n, E) in enumerate(zip(SIZES, SIMS))]
    return MixedAgent(envs[::-1], cfg, FEAT, seed=seed)             # (handed over largest first: the agent sorts)


def test_train_reaches_500_transitions_and_syncs_the_target():
    agent = _agent(11)
    assert [e.n_Veh for e in agent.envs] == [4, 8] and agent.n_iter == 10 and agent.num_transition == 50
    before = agent.target.get_flat()
    loss, rewards, q_mean, q_max = agent.train(1, 10)
    assert agent.num_step == 500
    assert loss.shape == (1, 1, 10) and np.isfinite(loss).all() and (loss >= 0).all()
    assert q_mean.shape == (1, 10) and np.isfinite(q_mean).all() and (q_max >= q_mean).all()
    assert rewards[4].shape == (1, 10, 30) and rewards[8].shape == (1, 10, 20) and np.isfinite(rewards[8]).all()
    on, tg = agent.online.get_flat(), agent.target.get_flat()
    assert np.array_equal(on, tg) and not np.array_equal(tg, before)              # synced when the 500th transition was in
    dropped = sum(agent.memory.dropped_irregular.values())
    assert len(agent.memory) == 500 - dropped
    assert agent.memory.stored(4) + agent.memory.dropped_irregular[4] == 300
    assert agent.online.get_optimizer_state()[2] == 10 and agent.epsilon < 1.0
    assert sum(len(v) for v in agent.last_minibatch.values()) == BATCH
    agent.close()


def test_replay_equals_dqn_step_on_the_numpy_assembly():
    import torch
    agent = _agent(12)
    agent.num_Episodes, agent.num_Train_Step = 1, 10
    for _ in range(2):
        agent.generate_transitions()
    w_on, w_tg = agent.online.get_flat(), agent.target.get_flat()
    loss, qm, qx = agent.replay()
    drawn = agent.last_minibatch
    assert sorted(drawn) == [4, 8] and [len(drawn[4]), len(drawn[8])] == [10, 6]     # 16 x 3 / 5 = 9.6, 16 x 2 / 5 = 6.4
    pools, slots = [], []
    for n in (4, 8):
        p = agent.memory.pools[n]
        pools.append(dict(n=n, **{k: getattr(p, k).cpu().numpy() for k in ("xe", "xe_next", "col", "action", "reward")}))
        slots.append(p.logical_to_slot(drawn[n]))
    m = numpy_assembly(pools, slots)
    online, target = GnnEngine(agent.spec), GnnEngine(agent.spec)
    online.set_flat(w_on)
    target.set_flat(w_tg)
    B = len(m['reward'])
    sb = online.to_device(PackedBatch(B, 0, m['xe'], m['row_ptr'], m['col_idx'], graph_off=m['graph_off']))
    sn = DeviceBatch.from_tensors(B, 0, torch.from_numpy(m['xe_next']).cuda(), sb.row_ptr, sb.col_idx, sb.max_edges,
                                  graph_off=sb.graph_off, max_nodes=sb.max_nodes)
    y = torch.empty((sb.n_rows, 4), dtype=torch.float32, device="cuda")
    ref = online.dqn_step(target, sb, sn, torch.from_numpy(m['action']).cuda(), torch.from_numpy(m['reward']).cuda(), agent.gamma, y_out=y)
    assert np.float32(loss) == ref.cpu().numpy()[0]
    assert np.array_equal(agent.online.get_flat(), online.get_flat()) and not np.array_equal(online.get_flat(), w_on)
    yn = y.cpu().numpy().astype(np.float64)
    assert np.isclose(qm, yn.mean(), rtol=1e-12) and np.isclose(qx, yn.max(axis=1).mean(), rtol=1e-12)
    for e in (online, target):
        e.close()
    agent.close()


def test_mixed_forward_scores_each_environment_like_its_own_forward():
    agent = _agent(13)
    obs = agent.observe()
    qs = agent.score(obs)
    for env, (xe, mask, col, regular), q in zip(agent.envs, obs, qs):
        E, n = env.E, env.n_Veh
        assert q.shape == (E, n, 4) and regular.all()
        offs = (np.arange(E + 1) * n).astype(np.int32)
        rp = (np.arange(E * n + 1) * (n - 2)).astype(np.int32)
        alone = agent.online.forward(PackedBatch(E, 0, np.ascontiguousarray(xe.reshape(E * n, 16)), rp, col.reshape(-1), graph_off=offs))
        assert_fwd_close(q.reshape(E * n, 4), alone, "%d links: rows of the mixed forward against the environment alone" % n)
    agent.close()
