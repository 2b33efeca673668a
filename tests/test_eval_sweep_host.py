"""No GPU needed: the C ABI of the checkpoint sweep (v2x_eval_sweep_mixed) is declared, exported and bound alike, the ctypes
struct has the header's layout, the first argument checks come back as V2X_EINVAL before anything is launched;
MixedAgent.evaluate_training(eval_backend='host') on host simulators with recording stand-in networks: one set of draws per
trial in the order of draw_eval_episode_ahead, every checkpoint scored on the same observations, the simulators stepped under
the last checkpoint's actions; MixedAgent.train(save_interval=...) writes the checkpoints' files; and the evaluation-of-training
driver refuses with --mixed-links what holds one link count."""
import ctypes as C
import os
import random
import re
import types

import numpy as np
import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL
from v2xgnn.rl import evaluate as rl_evaluate
from v2xgnn.rl import mixed
from v2xgnn.rl import train as rl_train
from v2xgnn.rl.device_sim import eval_result_layout
from v2xgnn.rl.run import weight_file_names
from v2xgnn.rl.train import start_env_batched
from v2xgnn.spec import GnnSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_V2V, W_V2I = 0.9, 0.1


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_the_entry_point_is_declared_exported_and_bound_alike():
    m = re.search(r'\bint\s+v2x_eval_sweep_mixed\s*\(([^)]*)\)\s*;', _header())
    assert m, "v2x_eval_sweep_mixed is not declared in include/v2xgnn.h"
    assert [a.strip() for a in m.group(1).split(',')] == ['const v2x_eval_sweep* s', 'const v2x_traj_ws* ws', 'void* stream']
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    so = C.CDLL(vlib.library_path())
    assert hasattr(so, 'v2x_eval_sweep_mixed') and hasattr(so, 'v2x_eval_sweep_result_bytes')
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert bound['v2x_eval_sweep_mixed'][0] is C.c_int and len(bound['v2x_eval_sweep_mixed'][1]) == 3
    assert bound['v2x_eval_sweep_mixed'][1][0]._type_ is vlib.EvalSweep and bound['v2x_eval_sweep_mixed'][1][1]._type_ is vlib.TrajWs


def test_the_binding_has_the_layout_of_the_declared_struct():
    body = re.search(r'typedef struct v2x_eval_sweep \{(.*?)\} v2x_eval_sweep;', _header(), flags=re.S).group(1)
    decls = [d.strip() for d in body.split(';') if d.strip()]
    assert decls == ['v2x_eval_mixed base', 'int32_t K, pad_', 'v2x_model* const* models', 'float* q']
    S = vlib.EvalSweep
    assert [f[0] for f in S._fields_] == ['base', 'K', 'pad_', 'models', 'q'] and S._fields_[0][1] is vlib.EvalMixed
    base = C.sizeof(vlib.EvalMixed)
    assert (S.base.offset, S.K.offset, S.pad_.offset, S.models.offset, S.q.offset) == (0, base, base + 4, base + 8, base + 16)
    assert C.sizeof(S) == base + 24 == 88                                # no padding anywhere


@pytest.mark.parametrize("E,n,rb,T,S", [(2, 4, 4, 3, 4), (1, 8, 4, 3, 3), (1, 20, 4, 50, 9), (1, 31, 5, 2, 65), (3, 4, 4, 1, 1)])
def test_result_bytes_is_the_layout_of_eval_steps_with_more_schemes(E, n, rb, T, S):
    m = min(rb, n)
    want = -(-(8 * S * T * E * (n + m + rb + 1) + 4 * S * T * E * n + (T + 1) * E) // 8) * 8
    lib = vlib.load_library()
    assert lib.v2x_eval_sweep_result_bytes(E, n, rb, T, S) == want == eval_result_layout(E, n, rb, T, S)[1]
    if S <= 2:
        assert lib.v2x_eval_steps_result_bytes(E, n, rb, T, S) == want


@pytest.mark.parametrize("E,n,rb,T,S", [(1, 4, 4, 3, 0), (1, 4, 4, 3, 66), (1, 4, 4, 0, 3), (2, 4, 4, 32768, 3), (1, 2, 1, 1, 3)])
def test_result_bytes_is_negative_outside_the_limits(E, n, rb, T, S):
    assert vlib.load_library().v2x_eval_sweep_result_bytes(E, n, rb, T, S) == V2X_EINVAL < 0


def test_the_first_checks_refuse_before_anything_is_launched():
    lib = vlib.load_library()

    def refused(s, *words):
        assert lib.v2x_eval_sweep_mixed(C.byref(s) if s is not None else None, None, None) == V2X_EINVAL
        err = lib.v2x_last_error(None).decode()
        assert err.startswith("eval_sweep_mixed: ") and all(w in err for w in words), err

    table = (vlib.Eval * 9)()
    sweep = lambda K, n_pools=2, T=1, pools=table, **kw: vlib.EvalSweep(   # noqa: E731
        base=vlib.EvalMixed(n_pools=n_pools, T=T, pools=pools), K=K, **kw)
    refused(None, "null sweep")
    refused(sweep(0), "1..64 networks", "K = 0")
    refused(sweep(65), "1..64 networks", "K = 65")
    refused(sweep(-1), "1..64 networks")
    none = (C.c_void_p * 2)(None, None)
    refused(sweep(2, models=none), "models[0] is NULL")
    refused(sweep(3, n_pools=0), "1..8 pools", "n_pools = 0")
    refused(sweep(3, n_pools=9), "1..8 pools", "n_pools = 9")
    refused(sweep(3, pools=None), "non-null pool table")
    refused(sweep(3, T=3), "pool 0", "walks T = 0 steps, the call T = 3")
    table[0].T = table[1].T = 3
    refused(sweep(3, T=3), "pool 0 (0 links): eval_steps: null pointer (actions is required)")
    table[0].model = 0x10000
    refused(sweep(3, T=3), "pool 0", "has a model of its own")


# ------------------------------------------------------------------------------------------------------- the agent on the host
class _Net(object):
    """a stand-in for a GnnEngine: Q-values that depend on the observation row and on the network's seed; records what it scored"""

    def __init__(self, seed):
        self.w = np.random.default_rng(seed).normal(size=(16, 4))
        self.seen = []

    def forward(self, pb):
        xe = np.asarray(pb.xe, np.float64).reshape(-1, 16)
        self.seen.append((xe.tobytes(), np.asarray(pb.graph_off).tobytes(), np.asarray(pb.col_idx).tobytes()))
        return np.sin(xe @ self.w * 37.0).astype(np.float32)

    def get_weights(self):
        from v2xgnn.bs_brain import _glorot_list
        return _glorot_list(self.spec, np.random.default_rng(3))


class _HostAgent(mixed.MixedAgent):
    """MixedAgent without its engines and its replay memory: what evaluate_training and train's save logic read"""

    def __init__(self, envs, batch=32):
        self.envs = sorted(envs, key=lambda e: e.n_Veh)
        self.sizes = [e.n_Veh for e in self.envs]
        self.num_CH, self.batch_size = 4, batch
        self.n_sims = sum(e.E for e in self.envs)
        self.v2v_weight, self.v2i_weight = W_V2V, W_V2I
        self.spec = GnnSpec(n_nodes=1, n_channels=4, feat_dim=16, n_mp_layers=2, share_weights=True, variable_graphs=True)
        self.online, self.target = _Net(1), _Net(2)
        self.online.spec = self.target.spec = self.spec
        self.trajectory_walk = 'serial'
        self.eval_stats = {'device_episodes': 0, 'host_episodes': 0}
        self.num_step, self._sync_mark, self.num_Episodes, self.num_Train_Step = 0, 0, 1, 1
        self.n_iter = -(-50 // self.n_sims)
        self._eval_opt = self._regular_look = None


def _envs():
    return [start_env_batched(4, 2, 5), start_env_batched(8, 1, 6)]


def _state(envs):
    return [tuple(np.array(a).tobytes() for a in e.observe_packed(4)) + (np.array(e.V2V_channels_with_fastfading).tobytes(),)
            for e in envs]


def _run(seeds, T, trials, eps, monkeypatch):
    envs, nets = _envs(), [_Net(s) for s in seeds]
    agent = _HostAgent(envs)
    calls = []
    ahead = mixed.draw_eval_episode_ahead

    def spy(*a):
        before = np.random.get_state()
        out = ahead(*a)
        calls.append((before, out, np.random.get_state(), a[1:]))
        return out
    monkeypatch.setattr(mixed, 'draw_eval_episode_ahead', spy)
    books = agent.evaluate_training(envs, None, T, trials, eps, engines=nets)
    monkeypatch.setattr(mixed, 'draw_eval_episode_ahead', ahead)
    return dict(books=books, calls=calls, nets=nets, rng=np.random.get_state(), py=random.getstate(), state=_state(envs),
                num_step=agent.num_step, stats=agent.eval_stats)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_every_checkpoint_is_scored_on_the_one_episode_of_its_trial(monkeypatch):
    T, trials, eps, seeds = 4, 2, 0.4, (11, 12, 13)
    run = _run(seeds, T, trials, eps, monkeypatch)
    K, shapes = len(seeds), ((2, 4), (1, 8))
    # one set of draws per trial, right after the re-seed (a reset draws from the simulators' own streams), in the order of
    # draw_eval_episode_ahead; nothing draws after it: the generators end where the last trial's draws left them
    assert len(run['calls']) == trials and run['stats'] == {'device_episodes': 0, 'host_episodes': trials}
    for tr, (before, out, after, args) in enumerate(run['calls']):
        np.random.seed(tr + 1)
        assert _same_state(before, np.random.get_state()) and args == (4, eps, T)
        again = mixed.draw_eval_episode_ahead([types.SimpleNamespace(E=E, n_Veh=n) for E, n in shapes], 4, eps, T)
        assert _same_state(after, np.random.get_state())
        for part, part_again in zip(out, again):
            assert all(np.array_equal(x, y) for x, y in zip(part, part_again))
    assert _same_state(run['rng'], run['calls'][-1][2]) and run['num_step'] == trials * T * 3
    random.seed(trials)
    assert run['py'] == random.getstate()
    # every checkpoint scored the same observations, once per step with a greedy simulator
    greedy_steps = sum(int(not all(x[st].all() for x in out[1])) for _, out, _, _ in run['calls'] for st in range(T))
    assert 0 < greedy_steps
    for net in run['nets']:
        assert len(net.seen) == greedy_steps and net.seen == run['nets'][0].seen
    # shapes; explored (trial, step, simulator) entries are the same in all K schemes, greedy ones differ somewhere
    differ = 0
    for k_env, (E, n) in enumerate(shapes):
        b = run['books'][n]
        assert sorted(b) == ['gnn', 'random']
        assert [a.shape for a in b['gnn']] == [(trials, K, E), (trials, K, E, T), (trials, K, E, T, n), (trials, K, E, T, 4), (trials, K, E, T, 4)]
        assert [a.shape for a in b['random']] == [(trials, E), (trials, E, T), (trials, E, T, n), (trials, E, T, 4), (trials, E, T, 4)]
        assert all(np.all(np.isfinite(a)) for a in b['gnn'] + b['random']) and np.all(b['gnn'][1] > 0) and np.all(b['random'][1] > 0)
        assert np.allclose(b['gnn'][0], b['gnn'][1].sum(axis=3), rtol=1e-12)
        for tr in range(trials):
            explore = run['calls'][tr][1][1][k_env]                       # [T, E]
            for st in range(T):
                for e in range(E):
                    rows = [b['gnn'][1][tr, k, e, st] for k in range(K)]
                    if explore[st, e]:
                        assert rows[0] == rows[1] == rows[2]
                    else:
                        differ += len(set(rows)) > 1
    assert differ > 0


def test_a_sweep_is_its_checkpoints_evaluated_alone_and_steps_under_the_last(monkeypatch):
    """nothing in an episode depends on the actions but the rates paid for them: checkpoint k of a sweep of three has the books of
    a sweep of that checkpoint alone, the random scheme is the same in all, and the simulators are left where the last
    checkpoint alone leaves them"""
    T, trials, eps, seeds = 3, 2, 0.3, (21, 22, 23)
    sweep = _run(seeds, T, trials, eps, monkeypatch)
    for k, seed in enumerate(seeds):
        alone = _run((seed,), T, trials, eps, monkeypatch)
        for n in (4, 8):
            for a, b in zip(sweep['books'][n]['gnn'], alone['books'][n]['gnn']):
                assert a[:, k].tobytes() == b[:, 0].tobytes(), (k, n)
            for a, b in zip(sweep['books'][n]['random'], alone['books'][n]['random']):
                assert a.tobytes() == b.tobytes(), (k, n)
        assert _same_state(sweep['rng'], alone['rng'])
        if k == len(seeds) - 1:
            assert sweep['state'] == alone['state']
    other = _run((21, 22, 21), T, trials, eps, monkeypatch)               # ... and it is the LAST checkpoint they step under
    for n in (4, 8):
        assert other['books'][n]['gnn'][1][:, 2].tobytes() == sweep['books'][n]['gnn'][1][:, 0].tobytes()


def test_evaluate_training_refuses_before_any_draw_reset_or_load(tmp_path):
    resets = []
    env = types.SimpleNamespace(E=2, n_Veh=8, n_RB=4, observe_packed=None, packed_ok=lambda c: True,
                                new_random_game=lambda n: resets.append(n))
    agent = _HostAgent([env])
    np.random.seed(3)
    before = np.random.get_state()
    nets = [_Net(1)]
    for kw, text in ((dict(engines=nets, eval_backend='device'), "evaluate_training: eval_backend='device' steps every environment on the device"),
                     (dict(engines=nets, opt_backend='host'), "opt_backend must be one of"),
                     (dict(engines=nets, eval_backend='graph'), "eval_backend must be one of"),
                     (dict(), "the checkpoints' episode tags"),
                     (dict(engines=nets, checkpoints=[5]), "one of the two"),
                     (dict(checkpoints=[5]), "checkpoints are loaded from save_dir"),
                     (dict(engines=[]), "1..64 checkpoints, got 0"),
                     (dict(engines=nets * 65), "1..64 checkpoints, got 65"),
                     (dict(engines=nets, T=0), "at least one step and one trial"),
                     (dict(checkpoints=[5], save_dir=str(tmp_path)), "no checkpoint ")):
        kw = dict(kw)
        with pytest.raises(ValueError, match=text):
            agent.evaluate_training([env], kw.pop('checkpoints', None), kw.pop('T', 5), 2, 0.1, **kw)
    assert not resets and _same_state(np.random.get_state(), before)


# ------------------------------------------------------------------------------------------------------- checkpoints of a run
def _train(tmp_path, name, **kw):
    """MixedAgent.train with the rollout and the replay step stubbed out: its episode loop and its saves"""
    import torch
    agent = _HostAgent(_envs())
    agent.memory = types.SimpleNamespace(torch=torch, pools={})
    agent.generate_transitions = lambda defer=False: {e.n_Veh: np.zeros(agent.n_iter * e.E) for e in agent.envs}
    agent.replay = lambda defer=False: (torch.zeros(1), torch.zeros((2, 1), dtype=torch.float64), 8)
    folder = str(tmp_path / name)
    agent.train(7, 2, save_dir=folder, **kw)
    return sorted(os.listdir(folder))


def test_save_interval_writes_a_pair_of_files_per_interval_and_the_final_pair(tmp_path):
    names = lambda eps: sorted(f for ep in eps for f in weight_file_names(ep, 2, 32))     # noqa: E731
    assert _train(tmp_path, 'none') == names([7])                        # today's behaviour: the final pair alone
    assert _train(tmp_path, 'three', save_interval=3) == names([3, 6, 7])
    assert _train(tmp_path, 'seven', save_interval=7) == names([7])
    assert _train(tmp_path, 'one', save_interval=1) == names(range(1, 8))
    assert rl_evaluate.saved_checkpoints(str(tmp_path / 'three'), 10, 2, 32) == [3, 6, 7]
    assert rl_evaluate.saved_checkpoints(str(tmp_path / 'three'), 6, 2, 32) == [3, 6]
    assert rl_evaluate.saved_checkpoints(str(tmp_path / 'three'), 10, 3, 32) == []
    for bad in (0, -2, 2.5):
        with pytest.raises(ValueError, match="save_interval must be a positive integer or None"):
            _train(tmp_path, 'bad', save_interval=bad)


# ------------------------------------------------------------------------------------------------------- the drivers
BASE = ["--save-dir", "D", "--mixed-links", "8,12"]


@pytest.mark.parametrize("extra,message", [
    (["--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device", "--trajectory-walk", "wide"],
     "--mixed-links walks serially"),
    (["--opt", "--opt-backend", "host"], "--mixed-links searches the optimum on the GPU"),
    (["--envs", "0"], "--envs must be at least 1"),
    (["--trials", "0"], "--trials and --test-steps must be at least 1"),
    (["--eval-backend", "device"], "--eval-backend device needs --sim-backend device --sim-streams device"),
    (["--sim-streams", "device"], "--sim-streams device needs --sim-backend device"),
    (["--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --eval-backend device"),
    (["--eval-links", "8,10"], "--eval-links: every link count must be a multiple of 4"),
    (["--eval-links", "8,8"], "--eval-links: the link counts must be distinct"),
])
def test_the_evaluation_driver_refuses_with_a_message_of_its_own(extra, message, capsys):
    with pytest.raises(SystemExit) as exit_:
        rl_evaluate.parse_args(BASE + extra)
    assert exit_.value.code == 2
    assert message in capsys.readouterr().err


def test_the_mixed_options_of_the_evaluation_driver_need_mixed_links(capsys):
    for extra, message in ((["--eval-links", "8"], "--eval-links / --envs need --mixed-links"),
                           (["--envs", "2"], "--eval-links / --envs need --mixed-links"),
                           (["--mixed-trajectory-walk", "wide"], "--mixed-trajectory-walk wide needs --mixed-links")):
        with pytest.raises(SystemExit):
            rl_evaluate.parse_args(["--save-dir", "D"] + extra)
        assert message in capsys.readouterr().err


def test_the_evaluation_driver_defaults():
    _, args = rl_evaluate.parse_args(["--save-dir", "D", "--mixed-links", "20,8,12"])
    assert args.mixed_links == [8, 12, 20] and args.eval_links == [8, 12, 20] and args.envs == 1
    assert args.opt_backend == "device" and args.eval_backend == "host" and args.mixed_trajectory_walk == "serial"
    _, args = rl_evaluate.parse_args(["--save-dir", "D", "--mixed-links", "8,12", "--eval-links", "28,16", "--envs", "3", "--opt",
                                      "--opt-backend", "bound"])
    assert args.eval_links == [16, 28] and args.envs == 3 and args.opt_backend == "bound"
    _, args = rl_evaluate.parse_args(["--save-dir", "D"])                # without --mixed-links nothing changes
    assert args.mixed_links is None and args.opt_backend == "host" and args.links == 4


def test_a_missing_checkpoint_folder_is_an_argument_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as exit_:
        rl_evaluate.main(["--save-dir", str(tmp_path), "--mixed-links", "8,12", "--episodes", "10"])
    assert exit_.value.code == 2 and "no checkpoint of episodes 1..10" in capsys.readouterr().err


def test_save_interval_of_the_training_driver_needs_mixed_links_and_a_folder(capsys):
    _, args = rl_train.parse_args(["--mixed-links", "8,12", "--envs", "2", "--save-dir", "D", "--save-interval", "5"])
    assert args.save_interval == 5
    _, args = rl_train.parse_args(["--mixed-links", "8,12", "--envs", "2", "--save-dir", "D"])
    assert args.save_interval is None
    for argv, message in ((["--save-interval", "5", "--save-dir", "D"], "--save-interval needs --mixed-links"),
                          (["--mixed-links", "8,12", "--envs", "2", "--save-interval", "5"], "needs --save-dir"),
                          (["--mixed-links", "8,12", "--envs", "2", "--save-dir", "D", "--save-interval", "0"], "must be at least 1")):
        with pytest.raises(SystemExit):
            rl_train.parse_args(argv)
        assert message in capsys.readouterr().err
