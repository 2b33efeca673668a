"""No GPU needed: what the host tests of the single families do not pin across them.  Every resident trajectory entry point of
the C ABI refuses a null struct under its own name; the four result-block sizes are one formula with four names and two scheme
limits; and in every receiver-form family a _jump call whose split-stream workspace and jump table are both wrong hears from the
split form's check (the pointers handed over are never dereferenced by the host)."""
import ctypes as C

import pytest

from test_mt_jump_host import ENTRY, JUMP, _call
from test_rollout_recv_split_host import P
from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL

TRAJECTORY_CALLS = ["rollout_steps", "rollout_steps_wide", "rollout_steps_split", "rollout_steps_mixed", "rollout_steps_mixed_wide",
                    "eval_steps", "eval_steps_wide", "eval_steps_split", "eval_steps_mixed", "eval_steps_mixed_wide", "eval_sweep_mixed",
                    "rollout_steps_recv", "rollout_steps_recv_split", "rollout_steps_recv_jump",
                    "eval_steps_recv", "eval_steps_recv_split", "eval_steps_recv_jump",
                    "eval_sweep_recv", "eval_sweep_recv_split", "eval_sweep_recv_jump"]


@pytest.mark.parametrize("entry", TRAJECTORY_CALLS)
def test_a_null_struct_is_refused_under_the_entry_points_own_name(entry):
    lib = vlib.load_library()
    argtypes = {name: args for name, _, args in vlib.SYMBOLS}["v2x_" + entry]
    # every workspace a plausible pointer of plausible size, so that the struct is the one thing wrong; the stream last
    rest = [(1 << 20) if t is C.c_int64 else None if t is not C.c_void_p else P for t in argtypes[1:-1]]
    assert getattr(lib, "v2x_" + entry)(None, *rest, None) == V2X_EINVAL
    text = lib.v2x_last_error(None).decode()
    assert text.startswith(entry + ": null "), text


RESULT_BYTES = {"v2x_eval_steps_result_bytes": ("eval_steps", 2), "v2x_eval_sweep_result_bytes": ("eval_sweep", 65),
                "v2x_eval_recv_result_bytes": ("eval_steps_recv", 2), "v2x_eval_sweep_recv_result_bytes": ("eval_sweep_recv", 65)}


@pytest.mark.parametrize("E,n,rb,T,S", [(1, 3, 1, 1, 1), (2, 31, 4, 3, 2)])
def test_the_four_result_sizes_agree(E, n, rb, T, S):
    lib = vlib.load_library()
    ste = S * T * E
    want = -(-(8 * ste * (n + min(rb, n) + rb + 1) + 4 * ste * n + (T + 1) * E) // 8) * 8      # the layout include/v2xgnn.h documents
    assert {name: getattr(lib, name)(E, n, rb, T, S) for name in RESULT_BYTES} == dict.fromkeys(RESULT_BYTES, want)


@pytest.mark.parametrize("name", sorted(RESULT_BYTES))
def test_each_result_size_refuses_under_its_own_name(name):
    lib = vlib.load_library()
    who, most = RESULT_BYTES[name]
    call = getattr(lib, name)
    assert call(256, 3, 1, 256, 1) == V2X_EINVAL                         # E and T fine alone, T E = 65536
    text = lib.v2x_last_error(None).decode()
    assert text.startswith(who + ": T E <= 65535 needed") and "T = 256, E = 256" in text, text
    for schemes in (0, most + 1):
        assert call(2, 4, 2, 3, schemes) == V2X_EINVAL
        text = lib.v2x_last_error(None).decode()
        assert text.startswith(who + ": ") and "schemes supported, got %d" % schemes in text, text
    assert call(2, 4, 2, 3, most) > 0


@pytest.mark.parametrize("entry", sorted(ENTRY))
@pytest.mark.parametrize("over,word", [(dict(split_ws=None), "split-stream workspace is null"),
                                       (dict(split_ws=P + 8), "split-stream workspace is null or not 256-byte aligned"),
                                       (dict(split_bytes=1024), "split-stream workspace of E = 2")])
@pytest.mark.parametrize("jump", [None, dict(JUMP, first=0), dict(JUMP, polys=None)])
def test_a_bad_split_workspace_speaks_before_a_bad_jump_table(monkeypatch, entry, over, word, jump):
    rc, text = _call(monkeypatch, entry, jump, **over)
    assert rc == V2X_EINVAL and text.startswith(entry + ":") and word in text and "jump" not in text.split(":", 1)[1], (rc, text)
