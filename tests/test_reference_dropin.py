"""CPU: `v2xgnn.BS` driven through the reference `Agent`'s real call sites -- `predict_one_step` in the rollout
(BS_brain.py:336), `predict` x 2 and `train_dnn` in `replay` (:664-665, :728), `update_target_model` (:847) -- with the
payloads that Agent built: the dict inputs and the dense kron(Adj, I_F) adjacency captured from the reference's own code
on its simulator (golden_agent_n4.npz, tests/golden/make_golden.py).  The compute engine injected here is the float64
oracle (no GPU needed); the boundary code under test (BS / GnnQModel / packing) is the product's."""
import os

import numpy as np

from util import GOLDEN


def test_reference_agent_drives_v2xgnn_bs():
    from oracle_engine import OracleEngine
    from oracle import compact as oc
    from oracle import literal as ol
    from util import ospec
    import v2xgnn
    g = np.load(os.path.join(GOLDEN, 'golden_agent_n4.npz'))

    def payload(prefix):
        return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}
    init, states, states_ = payload('init/'), payload('replay_s/'), payload('replay_s_next/')
    x, y = payload('fit_x/'), payload('fit_y/')
    batch = int(g['batch_size'])

    # the Agent's constructor call: BS(num_D2D, input_Node_Info, input_Edge_Info, num_Feedback, num_Neighbor, num_CH)
    # with the one-line swap of INTEGRATION.md section 1
    brain = v2xgnn.BS(4, 3, 1, 16, 1, 4, seed=5, engine_factory=lambda spec: OracleEngine(spec))
    assert g['mem_states'].shape[1] == brain.num_D2D_Input == 4 * 13 + 16     # the Agent's num_States

    def literal(model, feed):
        osp = ospec(brain._spec)
        params = oc.params_from_list(osp, [np.asarray(w, np.float64) for w in model.get_weights()], np.float64)
        return ol.forward_literal(osp, params, feed)

    def check(got, ref, rows):
        assert len(got) == 4
        for a, b in zip(got, ref):
            assert a.shape == (rows, 4) and np.allclose(a, b, rtol=2e-5, atol=2e-6)

    # rollout: the greedy branch's predict_one_step on a single state (B = 1)
    check(brain.predict_one_step(init, target=False), literal(brain.model, init), 1)
    # replay: online network on s, target network on s', then one fit step on the Agent's x / y
    p = brain.predict(states)
    check(p, literal(brain.model, states), batch)
    q = np.stack(p)
    assert np.all(q.max(axis=2) >= q.mean(axis=2))                          # the Agent's Q statistics are well-formed
    check(brain.predict(states_, target=True), literal(brain.target_model, states_), batch)
    w0 = np.concatenate([w.ravel() for w in brain.model.get_weights()])
    result = brain.train_dnn(x, y, batch)
    for k in range(1, 5):
        loss = result.history['D%d_Decide_Output_loss' % k][0]
        assert np.isfinite(loss) and loss >= 0
    w1 = np.concatenate([w.ravel() for w in brain.model.get_weights()])
    assert not np.array_equal(w0, w1)                                       # train_dnn really stepped the online network
    # the Agent's own state dict through BS.predict == the literal (dense kron) restatement on the trained weights
    check(brain.predict(init), literal(brain.model, init), 1)
    brain.update_target_model()
    for a, b in zip(brain.model.get_weights(), brain.target_model.get_weights()):
        assert np.array_equal(a, b)
