"""Host side of mixed-size DQN (rl/mixed.py, rl/train.py --mixed-links, the bindings of the two new entry points): no GPU."""
import ctypes as C
import os
import re

import pytest

from v2xgnn import lib as vlib
from v2xgnn.rl.mixed import MixedAgent, MixedReplay, mixed_quotas
from v2xgnn.rl import train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------------- the quota rule
@pytest.mark.parametrize("batch,weights,want", [
    (16, [3, 2], [10, 6]),                   # 9.6 and 6.4: the graph left over goes to the larger remainder
    (4096, [10, 10, 10, 10], [1024] * 4),
    (4096, [10, 10, 10], [1366, 1365, 1365]),          # equal remainders: the earlier entry
    (7, [1, 1, 5], [1, 1, 5]),
    (2, [1, 1, 1], [1, 1, 0]),               # a zero quota is allowed
    (5, [0, 4], [0, 5]),                     # a pool that holds nothing yet
    (0, [1, 2], [0, 0]),
    (100, [7, 1, 3, 9], [35, 5, 15, 45]),
])
def test_quota_rule_is_largest_remainder(batch, weights, want):
    got = mixed_quotas(batch, weights)
    assert got == want and sum(got) == batch
    total = sum(weights)
    assert all(batch * w // total <= q <= -(-batch * w // total) for q, w in zip(got, weights))


def test_quota_rule_refuses_nonsense():
    for batch, weights in ((4, []), (4, [0, 0]), (-1, [1]), (4, [2, -1])):
        with pytest.raises(ValueError, match="mixed_quotas"):
            mixed_quotas(batch, weights)


# ------------------------------------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("sizes,text", [
    ([], r"1\.\.8 link counts, got 0"),
    (list(range(3, 12)), r"1\.\.8 link counts, got 9"),
    ([4, 8, 4], "the link counts must be distinct"),
    ([2, 8], r"2 links -- a pool holds 3\.\.31 links"),
    ([8, 32], r"32 links -- a pool holds 3\.\.31 links"),
])
def test_mixed_replay_refuses_bad_sizes(sizes, text):
    with pytest.raises(ValueError, match="MixedReplay: " + text):
        MixedReplay(64, sizes)


class _FakeEnv(object):
    def __init__(self, n, batched=True, n_rb=4):
        self.n_Veh, self.n_RB = n, n_rb
        if batched:
            self.E = 2
            self.observe_packed = lambda c: None
        self.packed_ok = lambda c: c == self.n_RB


def test_mixed_agent_refuses_bad_environments():
    with pytest.raises(ValueError, match="MixedAgent: the link counts must be distinct"):
        MixedAgent([_FakeEnv(8), _FakeEnv(8)], None, 16)
    with pytest.raises(ValueError, match=r"MixedAgent: 40 links -- a pool holds 3\.\.31 links"):
        MixedAgent([_FakeEnv(8), _FakeEnv(40)], None, 16)
    with pytest.raises(ValueError, match=r"MixedAgent: 1\.\.8 link counts, got 0"):
        MixedAgent([], None, 16)
    with pytest.raises(ValueError, match="steps BatchedEnviron simulators, got _FakeEnv"):
        MixedAgent([_FakeEnv(8), _FakeEnv(12, batched=False)], None, 16)
    with pytest.raises(ValueError, match="environment of 12 links must have n_RB = 4"):
        MixedAgent([_FakeEnv(8), _FakeEnv(12, n_rb=3)], None, 16)


@pytest.mark.parametrize("text,want", [("8,12,20", [8, 12, 20]), ("20, 4", [4, 20]), ("28", [28])])
def test_mixed_links_are_parsed_and_sorted(text, want):
    assert train.parse_mixed_links(text) == want


@pytest.mark.parametrize("argv,text", [
    (["--mixed-links", "8,12", "--envs", "2", "--sim-backend", "device"], "--mixed-links steps host simulators"),
    (["--mixed-links", "8,12", "--envs", "2", "--sim-backend", "device", "--sim-streams", "device", "--rollout", "trajectory"],
     "--mixed-links steps host simulators"),
    (["--mixed-links", "8,12", "--envs", "2", "--rollout", "device"], "--mixed-links scores through the host"),
    (["--mixed-links", "8,12", "--envs", "2", "--rollouts", "sharded"], "--mixed-links runs on one GPU"),
    (["--mixed-links", "8,12"], "give --envs"),
    (["--mixed-links", "8,x", "--envs", "2"], "link counts separated by commas"),
    (["--mixed-links", "8,8", "--envs", "2"], "must be distinct"),
    (["--mixed-links", "8,10", "--envs", "2"], r"multiple of 4 between 4 and 28 \(got 10\)"),
    (["--mixed-links", "8,32", "--envs", "2"], r"multiple of 4 between 4 and 28 \(got 32\)"),
    (["--mixed-links", ",".join(str(4 * k) for k in range(1, 8)) + ",4,8", "--envs", "2"], "1 to 8 link counts, got 9"),
])
def test_mixed_links_flag_is_refused_with_a_message(argv, text, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("V2X_FORCE_DP", raising=False)
    with pytest.raises(SystemExit) as exc:
        train.main(argv)
    assert exc.value.code == 2
    assert re.search(text, capsys.readouterr().err)


def test_mixed_links_flag_is_refused_under_data_parallelism(capsys, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        train.main(["--mixed-links", "8,12", "--envs", "2"])
    assert "--mixed-links runs on one GPU" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------- the bindings
@pytest.mark.parametrize("name,argtypes", [
    ("v2x_dqn_targets_ragged", [C.c_void_p] * 4 + [C.c_double, C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 2),
    ("v2x_replay_gather_mixed", [C.c_int32, C.POINTER(vlib.ReplayPool), C.POINTER(vlib.MixedBatch), C.c_void_p]),
])
def test_new_entry_points_are_declared_exported_and_bound_alike(name, argtypes):
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == len(argtypes)
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is C.c_int and bound[name][1] == argtypes


@pytest.mark.parametrize("struct,binding", [("v2x_replay_pool", vlib.ReplayPool), ("v2x_mixed_batch", vlib.MixedBatch)])
def test_bindings_have_the_fields_of_the_declared_structs_in_order(struct, binding):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), _header(), flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[\s*]', '', part).replace('const', '') for part in decl.split(None, 1)[1].split(',')]
    names = [re.sub(r'^(double|float|u?int\d+_t)', '', n) for n in names]
    assert names == [f[0] for f in binding._fields_], (names, [f[0] for f in binding._fields_])
    is_ptr = [f[1] is C.c_void_p for f in binding._fields_]
    assert C.sizeof(binding) == 8 * sum(is_ptr) + 4 * (len(is_ptr) - sum(is_ptr))
