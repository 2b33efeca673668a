"""Host: the rule that cuts a wide GEMM launch into 128-row tiles and 64-row half tiles (wide_tiling_plan of csrc/v2xgnn.hip,
through the model-free v2x_wide_tiling_plan -- the function launch_wide_gemm itself calls).  No GPU.

The rule, for T = n_rb * ny workgroup tiles on C resident slots, rem = T % C:
  ny   = ceil(n_out / 64), Dense-0's 80 columns one 5-tile strip (ny = 1);  mbs = ceil(n_idx / 128);  n_rb = mbs * grid_z
  tail >= 1, T > C, rem > 0 and 4 rem < 3 C:  the last rem / ny row blocks run as two half tiles each
  tail == 2, C / 2 < T < C:                   every row block does
Every expected tuple below is worked from that text, not read off the library."""
import ctypes as C

import pytest

from v2xgnn import lib as vlib
from v2xgnn.lib import V2X_EINVAL


def _plan(n_idx, grid_z, n_out, slots, tail):
    out = (C.c_int32 * 4)()
    lib = vlib.load_library()
    rc = lib.v2x_wide_tiling_plan(n_idx, grid_z, n_out, slots, tail, out)
    assert rc == 0, (rc, lib.v2x_last_error(None))
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("what,args,want", [
    # 8 x 100 = 800 row blocks x 4 = 3200 tiles on 1280 slots: rem 640, 2560 < 3840 -> the last 640 / 4 = 160 blocks
    ("cfg3 node update", (1024, 100, 256, 1280, 1), (4, 8, 640, 800)),
    ("cfg3 node update, whole tiles only", (1024, 100, 256, 1280, 0), (4, 8, 800, 800)),
    # 800 tiles < 1280 slots: the first rule needs T > C
    ("cfg3 Dense-0", (1024, 100, 80, 1280, 1), (1, 8, 800, 800)),
    ("cfg3 Dense-0, all half tiles", (1024, 100, 80, 1280, 2), (1, 8, 0, 800)),      # 640 < 800 < 1280
    ("cfg3 node update, tail 2 is tail 1 above one round", (1024, 100, 256, 1280, 2), (4, 8, 640, 800)),
    # 2 x 5 = 10 row blocks x 2 = 20 tiles on 12 slots: rem 8, 32 < 36 -> 4 blocks
    ("small, stage", (140, 5, 128, 12, 1), (2, 2, 6, 10)),
    # x 4 = 40 tiles: rem 4, 16 < 36 -> 1 block
    ("small, dgrad", (140, 5, 256, 12, 1), (4, 2, 9, 10)),
    ("small, Dense-0", (140, 5, 80, 12, 1), (1, 2, 10, 10)),                         # 10 tiles < 12 slots
    ("small, Dense-0, tail 2", (140, 5, 80, 12, 2), (1, 2, 0, 10)),                  # 6 < 10 < 12
    # 3 x 5 = 15 row blocks x 2 = 30 tiles on 20 slots: rem 10, 40 < 60 -> 5 blocks = 10 half units: one run of 8, 2 in plain order
    ("three blocks per slot", (300, 5, 128, 20, 1), (2, 3, 10, 15)),
    # 512 columns: 8 column tiles; 10 x 8 = 80 tiles on 24 slots: rem 8, 32 < 72 -> 1 block
    ("512-column dgrad", (140, 5, 512, 24, 1), (8, 2, 9, 10)),
    # one weight slot, 300 rows: 3 row blocks x 2 on 4 slots: rem 2, 8 < 12 -> 1 block
    ("shared weights", (300, 1, 128, 4, 1), (2, 3, 2, 3)),
    # a remainder smaller than one row block's column tiles: 40 tiles on 13 slots, rem 1 -> 1 / 4 = 0 blocks
    ("remainder below one row block", (140, 5, 256, 13, 1), (4, 2, 10, 10)),
    # 99 links x 801 graphs x 128 features on 256 CUs: 7 x 99 = 693 blocks x 2 = 1386 on 1280: rem 106 -> 53 blocks
    ("99 links x 801 graphs", (801, 99, 128, 1280, 1), (2, 7, 640, 693)),
], ids=lambda v: v if isinstance(v, str) else None)
def test_tiling_of_known_launches(what, args, want):
    assert _plan(*args) == want, what


def test_a_launch_of_at_most_one_round_keeps_whole_tiles():
    """T <= slots: 13 row blocks x 2 = 26 tiles; 26 and 27 slots -> whole tiles, 25 slots -> rem 1 -> 0 blocks, 24 -> rem 2 -> 1"""
    assert _plan(100, 13, 128, 26, 1) == (2, 1, 13, 13)              # T == C
    assert _plan(100, 13, 128, 27, 1) == (2, 1, 13, 13)              # T < C, tail 1
    assert _plan(100, 13, 128, 25, 1) == (2, 1, 13, 13)
    assert _plan(100, 13, 128, 24, 1) == (2, 1, 12, 13)
    # tail 2 below one round: only above half a round (2 T > C)
    assert _plan(100, 13, 128, 27, 2) == (2, 1, 0, 13)
    assert _plan(100, 13, 128, 51, 2) == (2, 1, 0, 13)               # 52 > 51
    assert _plan(100, 13, 128, 52, 2) == (2, 1, 13, 13)              # 2 T == C
    assert _plan(100, 13, 128, 26, 2) == (2, 1, 13, 13)              # T == C: neither rule


def test_a_last_round_at_least_three_quarters_full_keeps_whole_tiles():
    """16 slots: 28 tiles leave rem 12, 48 >= 48 -> whole tiles; 26 tiles leave rem 10, 40 < 48 -> 5 blocks"""
    assert _plan(140, 7, 128, 16, 1) == (2, 2, 14, 14)
    assert _plan(100, 13, 128, 16, 1) == (2, 1, 8, 13)
    assert _plan(100, 13, 128, 16, 2) == (2, 1, 8, 13)
    # rem == 0: nothing to fill
    assert _plan(140, 5, 128, 10, 1) == (2, 2, 10, 10)
    assert _plan(140, 5, 128, 20, 2) == (2, 2, 10, 10)


def test_half_tiles_are_a_suffix_for_every_slot_count():
    """0 <= n_full_rb <= n_rb, whole tiles at tail 0, and ny / mbs / n_rb do not depend on slots or tail"""
    for n_idx, gz, n_out in ((140, 5, 128), (300, 5, 256), (300, 1, 128), (1, 1, 80), (129, 3, 512)):
        base = _plan(n_idx, gz, n_out, 7, 0)
        assert base[2] == base[3] == base[1] * gz and base[1] == (n_idx + 127) // 128
        for slots in range(1, 70):
            for tail in (0, 1, 2):
                ny, mbs, full, n_rb = _plan(n_idx, gz, n_out, slots, tail)
                assert (ny, mbs, n_rb) == (base[0], base[1], base[3])
                assert 0 <= full <= n_rb and (tail or full == n_rb)


def test_the_library_refuses_bad_arguments():
    lib = vlib.load_library()
    out = (C.c_int32 * 4)()
    assert lib.v2x_wide_tiling_plan(140, 5, 128, 12, 1, None) == V2X_EINVAL
    for bad in ((0, 5, 128, 12, 1), (140, 0, 128, 12, 1), (140, 5, 0, 12, 1), (140, 5, 128, 0, 1), (140, 5, 128, 12, 3),
                (140, 5, 128, 12, -1), (2 ** 31 - 1, 2 ** 20, 128, 12, 1)):
        assert lib.v2x_wide_tiling_plan(*bad, out) == V2X_EINVAL, bad
        assert b"wide_tiling_plan" in lib.v2x_last_error(None)
