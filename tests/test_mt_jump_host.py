"""No GPU needed: the jump-ahead polynomials of MT19937 (v2x_mt_jump_polys: x^J mod phi, phi by Berlekamp-Massey on the library's
own word stream) enter numpy's stream at any position; the C ABI of the jump form (v2x_mt_jump, v2x_mt_jump_scratch_bytes,
v2x_rollout_steps_recv_jump, v2x_eval_steps_recv_jump, v2x_eval_sweep_recv_jump) is declared, exported and bound alike and
refuses what the header says before anything is launched (the pointers handed over are never dereferenced by the host); and
the Python layers take stream_words / receiver_words / --receiver-words with the split stream phase only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_eval_recv_host
import test_eval_sweep_recv_host
import test_rollout_recv_split_host
from test_rollout_recv_split_host import LANES, P, _dev_env, _mk
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL, MtJump
from v2xgnn.rl import DeviceChannels
from v2xgnn.rl import evaluate as rl_evaluate
from v2xgnn.rl import run as rl_run
from v2xgnn.rl.device_sim import JUMP_FIRST, JUMP_STRIDE, STREAM_PHASES, STREAM_WORDS, jump_plan
from v2xgnn.rl.train import parse_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_FIRST = 20561                                        # 1 + 19936 + 624: the prefix the seeds of a chunk read


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'v2xgnn.h')).read(), flags=re.S)


@pytest.mark.parametrize("name,ret,restype,count", [("v2x_mt_jump_polys", "int", C.c_int, 4),
                                                    ("v2x_mt_jump_scratch_bytes", "int64_t", C.c_int64, 2),
                                                    ("v2x_rollout_steps_recv_jump", "int", C.c_int, 7),
                                                    ("v2x_eval_steps_recv_jump", "int", C.c_int, 7),
                                                    ("v2x_eval_sweep_recv_jump", "int", C.c_int, 7)])
def test_entry_points_are_declared_exported_and_bound_alike(name, ret, restype, count):
    m = re.search(r'\b%s\s+%s\s*\(([^)]*)\)\s*;' % (ret, name), _header())
    assert m, "%s is not declared in include/v2xgnn.h" % name
    assert len([a for a in m.group(1).split(',') if a.strip()]) == count
    assert os.path.exists(vlib.library_path()), "build the HIP extension first (__graft_entry__.build())"
    assert hasattr(C.CDLL(vlib.library_path()), name), "libv2xgnn.so does not export %s" % name
    bound = {n: (r, a) for n, r, a in vlib.SYMBOLS}
    assert name in bound and bound[name][0] is restype and len(bound[name][1]) == count


def test_the_struct_is_declared_and_bound_field_for_field():
    m = re.search(r'typedef struct v2x_mt_jump \{(.*?)\} v2x_mt_jump;', _header(), flags=re.S)
    assert m, "v2x_mt_jump is not declared in include/v2xgnn.h"
    declared = [re.sub(r'[*\s]', '', name) for decl in m.group(1).split(';') if decl.strip()
                for name in decl.strip().split(None, 1)[1].replace('uint32_t', '').replace('const', '').split(',')]
    assert declared == [f[0] for f in MtJump._fields_] == ['first', 'stride', 'count', 'pad_', 'polys', 'scratch', 'scratch_bytes']
    assert C.sizeof(MtJump) == 48 and MtJump.polys.offset == 24 and MtJump.scratch_bytes.offset == 40


# ------------------------------------------------------------------------------------------------------- the identity
def _stream(seed, total):
    """numpy's key array of `seed`, then w[i + 624] = twist(w[i], w[i + 1], w[i + 397]) up to `total` words"""
    w = np.zeros(total, np.uint32)
    w[:624] = np.random.RandomState(seed).get_state()[1]
    for i in range(0, total - 624, 227):                                 # 227 words at a time: their operands are all older
        m = min(227, total - 624 - i)
        y = (w[i:i + m] & np.uint32(0x80000000)) | (w[i + 1:i + 1 + m] & np.uint32(0x7fffffff))
        w[i + 624:i + 624 + m] = w[i + 397:i + 397 + m] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908b0df), np.uint32(0))
    return w


def _temper(y):
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9d2c5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xefc60000))
    return y ^ (y >> np.uint32(18))


SEEDS = (7, 20201)
TOTAL = 30000 + 4 * 58112 + 624


@pytest.fixture(scope="module")
def streams():
    return {seed: _stream(seed, TOTAL) for seed in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_the_reference_stream_is_numpys(streams, seed):
    w = streams[seed]
    want = np.random.RandomState(seed).randint(0, 2 ** 32, TOTAL - 624, dtype=np.uint64)
    assert np.array_equal(_temper(w[624:]).astype(np.uint64), want)


@pytest.mark.parametrize("first,stride,count", [(20561, 624, 3), (20561, 1000, 2), (30000, 58112, 4)])
def test_the_polynomials_enter_the_stream_at_every_chunk(streams, first, stride, count):
    lib = vlib.load_library()
    out = np.full((count + 1, 624), 0xA5A5A5A5, np.uint32)
    assert lib.v2x_mt_jump_polys(first, stride, count, out.ctypes.data) == 0, lib.v2x_last_error(None)
    assert (out[count] == 0xA5A5A5A5).all()                              # nothing behind the table is written
    assert (out[:count, 623] >> 1 == 0).all()                            # the 31 unused top bits
    k = np.arange(624)
    for p in range(count):
        c = first + p * stride
        idx = np.nonzero(np.unpackbits(out[p].view(np.uint8), bitorder='little'))[0]
        assert 0 < len(idx) and idx[-1] < 19937
        for seed in SEEDS:
            w = streams[seed]
            got = np.bitwise_xor.reduce(w[1 + idx[:, None] + k[None, :]], axis=0)
            assert np.array_equal(got, w[c:c + 624]), (seed, p, c)
    again = np.zeros((count, 624), np.uint32)                            # the cached field gives the same table
    assert lib.v2x_mt_jump_polys(first, stride, count, again.ctypes.data) == 0 and np.array_equal(again, out[:count])


@pytest.mark.parametrize("args,word", [((20560, 624, 1), "first = 20560"), ((0, 624, 1), "first = 0"), ((20561, 623, 1), "stride = 623"),
                                       ((20561, 624, 0), "count = 0"), ((20561, 624, -2), "count = -2")])
def test_the_table_refuses_what_the_identity_cannot_serve(args, word):
    lib = vlib.load_library()
    out = np.zeros((1, 624), np.uint32)
    assert lib.v2x_mt_jump_polys(*args, out.ctypes.data) == V2X_EINVAL
    text = lib.v2x_last_error(None).decode()
    assert text.startswith("mt_jump_polys:") and word in text, text
    assert not out.any()
    assert lib.v2x_mt_jump_polys(20561, 624, 1, None) == V2X_EINVAL
    assert lib.v2x_last_error(None).decode() == "mt_jump_polys: null out"


def test_scratch_bytes_is_the_documented_formula():
    lib = vlib.load_library()
    for E, count in ((1, 1), (3, 7), (10, 256), (1, 0)):
        assert lib.v2x_mt_jump_scratch_bytes(E, count) == -(-4 * E * count * 8 * 624 // 256) * 256
    for E, count in ((0, 1), (1, -1), (1, 65536)):
        assert lib.v2x_mt_jump_scratch_bytes(E, count) == V2X_EINVAL
        assert lib.v2x_last_error(None).decode().startswith("mt_jump_scratch_bytes:")


# ------------------------------------------------------------------------------------------------------- the argument checks
NBW = (1 + -(-3 * (2 * (40 + 1600 + 320 + 12800) + 4 * 40 * 2) // 624)) * 624    # of the _call defaults: E = 2, n = 40, rb = 4, T = 3, 2 lanes
JUMP = dict(first=MIN_FIRST, stride=624, count=3, polys=P + (2 << 30), scratch=P + (3 << 30), scratch_bytes=1 << 30)
ENTRY = {"rollout_steps_recv_jump": (test_rollout_recv_split_host._call, ()), "eval_steps_recv_jump": (test_eval_recv_host._call, (True,)),
         "eval_sweep_recv_jump": (test_eval_sweep_recv_host._call, (True,))}


class _JumpLibrary:
    """the library with every _recv_split call sent to its _jump form with `jump`: the made-up structs of the split forms' own
    host tests serve the jump forms"""

    def __init__(self, lib, jump):
        self._lib, self._jump = lib, jump

    def __getattr__(self, name):
        if not name.endswith("_recv_split"):
            return getattr(self._lib, name)
        call = getattr(self._lib, name[:-len("split")] + "jump")
        ref = None if self._jump is None else C.byref(self._jump)
        return lambda r, ws, ws_bytes, sws, sws_bytes, stream: call(r, ws, ws_bytes, sws, sws_bytes, ref, stream)


def _call(monkeypatch, entry, jump, **over):
    lib = vlib.load_library()
    call, args = ENTRY[entry]
    with monkeypatch.context() as m:
        m.setattr(vlib, "load_library", lambda: _JumpLibrary(lib, None if jump is None else MtJump(pad_=0, **jump)))
        return call(*args, **over)


JUMP_REFUSALS = [
    (None, "null jump"), (dict(JUMP, first=MIN_FIRST - 1), "first = 20560"), (dict(JUMP, stride=623), "stride = 623"),
    (dict(JUMP, count=-1), "count = -1"), (dict(JUMP, polys=None), "polys is null"), (dict(JUMP, polys=P + 64), "polys is null or not 256"),
    (dict(JUMP, scratch=None), "scratch is null"), (dict(JUMP, scratch=P + 8), "scratch is null or not 256"),
    (dict(JUMP, stride=NBW - MIN_FIRST, count=2), "last chunk is empty"), (dict(JUMP, first=NBW - 2 * 624), "last chunk is empty"),
    (dict(JUMP, scratch_bytes=2 * 3 * 8 * 624 * 4 - 1), "needs 119808 bytes"),
    # count = 0 asks for no chunk, but first and stride are checked all the same
    (dict(JUMP, count=0, polys=None, scratch=None, first=5), "first = 5"), (dict(JUMP, count=0, polys=None, scratch=None, stride=0), "stride = 0"),
]


@pytest.mark.parametrize("entry", sorted(ENTRY))
@pytest.mark.parametrize("jump,word", JUMP_REFUSALS)
def test_a_bad_jump_table_is_refused_before_anything_is_launched(monkeypatch, entry, jump, word):
    rc, text = _call(monkeypatch, entry, jump)
    assert rc == V2X_EINVAL and text.startswith(entry + ":") and word in text, (rc, text)


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_the_split_forms_checks_come_first(monkeypatch, entry):
    for over, word in ((dict(split_ws=None), "split-stream workspace is null"), (dict(split_bytes=1024), "split-stream workspace of E = 2"),
                       (dict(n=129), "n = 129"), (dict(ws=None), "workspace")):
        rc, text = _call(monkeypatch, entry, dict(JUMP, first=0), **over)
        assert rc == V2X_EINVAL and word in text and ": jump:" not in text, (rc, text)
    lib = vlib.load_library()
    assert getattr(lib, "v2x_" + entry)(None, P, 1 << 20, P, 1 << 20, None, None) == V2X_EINVAL
    assert lib.v2x_last_error(None).decode().startswith(entry + ": null")


# ------------------------------------------------------------------------------------------------------- the Python layers
def test_jump_plan_covers_the_array_with_a_non_empty_last_chunk():
    assert STREAM_WORDS == ('serial', 'jump') and STREAM_PHASES == ('chain', 'split')
    assert JUMP_FIRST >= MIN_FIRST and (JUMP_FIRST - 624) % 227 == 0 and JUMP_STRIDE % 227 == 0 and JUMP_STRIDE >= 624
    assert DeviceChannels.jump_plan(100) == jump_plan(JUMP_FIRST) == (JUMP_FIRST, JUMP_STRIDE, 0)
    for nbw in (JUMP_FIRST + 1, JUMP_FIRST + JUMP_STRIDE, JUMP_FIRST + JUMP_STRIDE + 1, 79872, 14_922_832):
        first, stride, count = jump_plan(nbw)
        assert (first, stride) == (JUMP_FIRST, JUMP_STRIDE) and count >= 1
        assert first + (count - 1) * stride < nbw <= first + count * stride


def test_channels_check_stream_words_before_any_device_work():
    import types
    dc = DeviceChannels(2, 40, 4)
    dc.set_grid(LANES, 750.0, 1299.0, 0.01)
    assert dc.stream_words_calls == {'serial': 0, 'jump': 0}
    tensor = lambda *shape: types.SimpleNamespace(shape=(8,) + shape, is_contiguous=lambda: True)        # noqa: E731
    st = {'xe': tensor(40, 16), 'xe_next': tensor(40, 16), 'recv': tensor(40), 'action': tensor(40), 'reward': tensor()}
    ex, ra, own = np.ones((3, 2), np.uint8), np.zeros((3, 2, 40), np.int32), [0, 0]
    assert dc.check_rollout_steps_recv(ex, ra, st, 5, 8, own, stream_phase='split', stream_words='jump')[0] == 3
    assert dc.check_eval_steps_recv(ex, ra, None, own, 'split', 'jump')[0] == 3
    assert dc.check_eval_sweep_recv(ex, ra, None, None, 2, own, 'split', 'jump')[-1] == 2
    for words in ('split', 'chain', None, 1):
        with pytest.raises(ValueError, match="stream_words must be one of 'serial', 'jump'"):
            dc.check_rollout_steps_recv(ex, ra, st, 5, 8, own, stream_phase='split', stream_words=words)
        with pytest.raises(ValueError, match="eval_steps_recv: stream_words must be one of 'serial', 'jump'"):
            dc.eval_steps_recv(ex, ra, None, 1.0, 0.1, own=own, stream_phase='split', stream_words=words)
    needs = "stream_words='jump' needs stream_phase='split'"
    with pytest.raises(ValueError, match="rollout_steps_recv: " + needs):
        dc.rollout_steps_recv(ex, ra, st, 5, 8, 1.0, 0.1, own=own, stream_words='jump')
    with pytest.raises(ValueError, match="eval_steps_recv: " + needs):
        dc.eval_steps_recv(ex, ra, None, 1.0, 0.1, own=own, stream_phase='chain', stream_words='jump')
    with pytest.raises(ValueError, match="eval_sweep_recv: " + needs):
        dc.eval_sweep_recv(ex, ra, None, 1.0, 0.1, K=2, own=own, stream_words='jump')
    assert dc.stream_words_calls == {'serial': 0, 'jump': 0} and dc.stream_phase_calls == {'chain': 0, 'split': 0}
    with pytest.raises(ValueError, match="receiver form only"):
        _dev_env('device').evaluate_steps(np.ones((1, 2), np.uint8), np.zeros((1, 2, 4), np.int32), None, 1.0, 0.1, walk='wide',
                                          stream_phase='split', stream_words='jump')


def test_agent_takes_receiver_words_with_the_split_stream_phase_only():
    how = dict(device_replay='receivers', rollout_backend='trajectory')
    agent = _mk(_dev_env('device'), receiver_streams='split', receiver_words='jump', **how)
    assert (agent.receiver_streams, agent.receiver_words) == ('split', 'jump')
    assert _mk(_dev_env('device'), receiver_streams='split', **how).receiver_words == 'serial'
    assert _mk(_dev_env('device'), n=20).receiver_words == 'serial'      # 'serial' is valid everywhere: nothing existing changes
    with pytest.raises(ValueError, match="receiver_words='jump' needs receiver_streams='split'"):
        _mk(_dev_env('device'), receiver_words='jump', **how)
    with pytest.raises(ValueError, match="receiver_words must be one of"):
        _mk(_dev_env('device'), receiver_streams='split', receiver_words='split', **how)


def test_command_lines_take_receiver_words_with_receiver_streams_split_only(capsys):
    dev = ["--sim-backend", "device", "--sim-streams", "device", "--envs", "1"]
    recv = ["--links", "100", "--replay", "receivers", "--rollout", "trajectory"]
    _, args = parse_args(recv + ["--receiver-streams", "split", "--receiver-words", "jump"] + dev)
    assert (args.receiver_streams, args.receiver_words) == ("split", "jump")
    assert parse_args(recv + ["--receiver-streams", "split"] + dev)[1].receiver_words == "serial"
    needs = "--receiver-words jump needs --receiver-streams split"
    for argv, word in ((recv + ["--receiver-words", "jump"] + dev, needs), (["--receiver-words", "jump"], needs),
                       (recv + ["--receiver-streams", "split", "--receiver-words", "wide"] + dev, "invalid choice")):
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert word in capsys.readouterr().err, argv
    ev = ["--links", "40", "--save-dir", "x", "--sim-backend", "device", "--sim-streams", "device", "--eval-backend", "device"]
    for mod in (rl_run, rl_evaluate):
        _, args = mod.parse_args(ev + ["--receiver-streams", "split", "--receiver-words", "jump"])
        assert (args.receiver_streams, args.receiver_words) == ("split", "jump")
        with pytest.raises(SystemExit):
            mod.parse_args(ev + ["--receiver-words", "jump"])
        assert needs in capsys.readouterr().err, mod.__name__
