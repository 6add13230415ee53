"""sd_tome_plan (no device): the cells, the destination draw and the counts against tests/tome_oracle.py."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tome_oracle  # noqa: E402

GEOMS = [(16, 16, 2, 2), (8, 8, 2, 2), (6, 10, 2, 2), (5, 7, 2, 2), (7, 5, 3, 2), (2, 2, 2, 2), (1, 9, 2, 2)]
RATIOS = [0.0, 0.1, 0.25, 0.5, 0.75]
TRIPLES = [(0, 0, 0), (1234, 7, 3), (0xFFFFFFFF, 49, 15)]


def engine_plan(lib, H, W, sx, sy, ratio, use_rand, seed, step, site):
    info = (C.c_int32 * 4)()
    assert lib.sd_tome_plan(H, W, sx, sy, ratio, use_rand, seed, step, site, info, None) == 0, lib.sd_last_error()
    dst = (C.c_int32 * max(info[0], 1))()
    assert lib.sd_tome_plan(H, W, sx, sy, ratio, use_rand, seed, step, site, info, dst) == 0, lib.sd_last_error()
    return tuple(info), list(dst)[:info[0]]


@pytest.mark.parametrize("H,W,sx,sy", GEOMS)
@pytest.mark.parametrize("use_rand", [0, 1])
def test_plan_matches_oracle(engine_lib, H, W, sx, sy, use_rand):
    for ratio in RATIOS:
        for seed, step, site in TRIPLES:
            info, dst = engine_plan(engine_lib, H, W, sx, sy, ratio, use_rand, seed, step, site)
            Nd, Ns, r, Tm, odst, osrc = tome_oracle.plan(H, W, sx, sy, ratio, use_rand, seed, step, site)
            assert info == (Nd, Ns, r, Tm), (ratio, seed, step, site)
            assert dst == odst, (ratio, seed, step, site)
            assert Nd == (H // sy) * (W // sx) and Nd + Ns == H * W and Tm == H * W - r
            assert r == min(Ns, int(H * W * ratio))
            # one destination per whole cell, inside its cell
            cells = sorted(((t // W) // sy) * (W // sx) + (t % W) // sx for t in dst)
            assert cells == list(range(Nd))
            if not use_rand:
                assert all((t // W) % sy == 0 and (t % W) % sx == 0 for t in dst)


def test_every_hash_input_changes_the_draw(engine_lib):
    base = engine_plan(engine_lib, 16, 16, 2, 2, 0.5, 1, 5, 6, 7)[1]
    assert engine_plan(engine_lib, 16, 16, 2, 2, 0.5, 1, 5, 6, 7)[1] == base
    assert engine_plan(engine_lib, 16, 16, 2, 2, 0.5, 1, 6, 6, 7)[1] != base
    assert engine_plan(engine_lib, 16, 16, 2, 2, 0.5, 1, 5, 7, 7)[1] != base
    assert engine_plan(engine_lib, 16, 16, 2, 2, 0.5, 1, 5, 6, 8)[1] != base
    # and the draw uses every position of the cell
    assert {((t // 16) % 2) * 2 + (t % 16) % 2 for t in base} == {0, 1, 2, 3}


def test_plan_bytes_grow_with_the_problem(engine_lib):
    lib = engine_lib
    assert lib.sd_tome_plan_bytes(1, 16) > 0
    assert lib.sd_tome_plan_bytes(2, 256) > lib.sd_tome_plan_bytes(1, 256) > lib.sd_tome_plan_bytes(1, 64)
    assert lib.sd_tome_plan_bytes(0, 16) == 0 and lib.sd_tome_plan_bytes(1, 0) == 0


@pytest.mark.parametrize("args", [
    (16, 16, 2, 2, 0.76, 1), (16, 16, 2, 2, -0.1, 1), (16, 16, 2, 2, float("nan"), 1), (16, 16, 0, 2, 0.5, 1),
    (16, 16, 2, 9, 0.5, 1), (0, 16, 2, 2, 0.5, 1), (16, -1, 2, 2, 0.5, 1)])
def test_plan_rejects_bad_arguments(engine_lib, args):
    info = (C.c_int32 * 4)()
    H, W, sx, sy, ratio, use_rand = args
    assert engine_lib.sd_tome_plan(H, W, sx, sy, ratio, use_rand, 0, 0, 0, info, None) == 1
    assert b"tome" in engine_lib.sd_last_error()


def test_plan_rejects_null(engine_lib):
    assert engine_lib.sd_tome_plan(16, 16, 2, 2, 0.5, 1, 0, 0, 0, None, None) == 1
