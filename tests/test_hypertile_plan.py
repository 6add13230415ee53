"""sd_hypertile_plan (no device): the candidate counts and the per-step draw against stablediffusion_amd.hypertile, the
helper oracle and the tables of the feature's definition; the new C entries are declared and exported."""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hypertile_oracle  # noqa: E402
from stablediffusion_amd import hypertile  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, tile_size, swap_size) -> counts, written by hand from the rule
COUNTS = [
    (128, 32, 2, [4, 2]), (64, 32, 2, [2, 1]), (96, 32, 2, [3, 2]), (96, 32, 3, [3, 2, 1]), (20, 32, 2, [1]),
    (30, 8, 4, [3, 2, 1]), (37, 8, 3, [1]), (16, 8, 2, [2, 1]), (8, 8, 2, [1]), (8, 4, 2, [2, 1]), (24, 8, 3, [3, 2, 1]),
    (12, 6, 2, [2, 1]),
]
TRIPLES = [(0, 0, 0), (1234, 7, 3), (0xFFFFFFFF, 49, 15), (1, 63, 9)]
NEW_SYMBOLS = ["sd_unet_set_hypertile", "sd_unet_hypertile_step", "sd_unet_hypertile_sites", "sd_unet_hypertile_read",
               "sd_hypertile_plan", "sd_op_hypertile_gather", "sd_op_hypertile_scatter"]


def engine_plan(lib, Hs, Ws, tile, swap, seed, step, site):
    out = (C.c_int32 * 4)()
    assert lib.sd_hypertile_plan(Hs, Ws, tile, swap, seed, step, site, out) == 0, lib.sd_last_error()
    return tuple(out)


@pytest.mark.parametrize("n,tile,swap,want", COUNTS)
def test_counts_table(engine_lib, n, tile, swap, want):
    assert hypertile.counts(n, tile, swap) == want == hypertile_oracle.counts(n, tile, swap)
    # per axis through the engine: with the other axis a single token, every draw is one of the axis's candidates and
    # over 64 steps all of them appear
    seen_h, seen_w = set(), set()
    for step in range(64):
        nh, nw, th, tw = engine_plan(engine_lib, n, 1, tile, swap, 1, step, 2)
        assert nw == 1 and tw == 1 and nh * th == n
        seen_h.add(nh)
        nh, nw, th, tw = engine_plan(engine_lib, 1, n, tile, swap, 1, step, 2)
        assert nh == 1 and th == 1 and nw * tw == n
        seen_w.add(nw)
    assert seen_h == set(want) == seen_w


@pytest.mark.parametrize("Hs,Ws,tile,swap", [(16, 16, 8, 2), (128, 128, 32, 2), (96, 64, 32, 3), (12, 20, 6, 2), (30, 24, 8, 4),
                                             (37, 16, 8, 3), (8, 8, 4, 1), (16, 24, 8, 2), (16, 24, 4, 2)])
def test_plan_matches_python(engine_lib, Hs, Ws, tile, swap):
    for seed, step, site in TRIPLES:
        got = engine_plan(engine_lib, Hs, Ws, tile, swap, seed, step, site)
        assert got == hypertile.plan(Hs, Ws, tile, swap, seed, step, site), (seed, step, site)
        assert got == hypertile_oracle.plan(Hs, Ws, tile, swap, seed, step, site), (seed, step, site)
        nh, nw, th, tw = got
        assert nh * th == Hs and nw * tw == Ws
        assert nh in hypertile.counts(Hs, tile, swap) and nw in hypertile.counts(Ws, tile, swap)


def test_draws_of_the_definition(engine_lib):
    """Seed 0, site 0, 16 x 16, tile_size 8, swap_size 2 (counts [2, 1] on both axes)."""
    want = {0: (2, 2), 2: (1, 2), 3: (2, 1), 4: (1, 1)}
    for step, div in want.items():
        assert engine_plan(engine_lib, 16, 16, 8, 2, 0, step, 0)[:2] == div, step
        assert hypertile.plan(16, 16, 8, 2, 0, step, 0)[:2] == div, step


@pytest.mark.parametrize("n,tile,swap", [(16, 8, 2), (24, 8, 3)])       # a 2- and a 3-candidate axis
def test_every_candidate_is_drawn(engine_lib, n, tile, swap):
    cands = hypertile.counts(n, tile, swap)
    assert len(cands) == swap
    for seed in (0, 1, 12345):
        for site in range(16):
            for axis in (0, 1):
                drawn = [engine_plan(engine_lib, n, n, tile, swap, seed, step, site)[axis] for step in range(64)]
                assert set(drawn) == set(cands), (seed, site, axis)


def test_every_hash_input_changes_the_draw(engine_lib):
    seq = lambda seed, site: [engine_plan(engine_lib, 24, 24, 8, 3, seed, step, site)[:2] for step in range(32)]
    base = seq(5, 7)
    assert seq(5, 7) == base
    assert seq(6, 7) != base and seq(5, 8) != base
    assert len(set(base)) > 1                       # the step
    assert any(nh != nw for nh, nw in base)         # the two axes draw independently


@pytest.mark.parametrize("args", [(0, 16, 8, 2), (16, -1, 8, 2), (16, 16, 0, 2), (16, 16, -3, 2), (16, 16, 8, 0), (16, 16, 8, 9),
                                  (8192, 4096, 32, 2)])
def test_plan_rejects_bad_arguments(engine_lib, args):
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert engine_lib.sd_hypertile_plan(*args, 0, 0, 0, out) == 1
    assert b"hypertile" in engine_lib.sd_last_error()
    assert tuple(out) == (-7, -7, -7, -7)


def test_plan_rejects_null(engine_lib):
    assert engine_lib.sd_hypertile_plan(16, 16, 8, 2, 0, 0, 0, None) == 1


def test_python_rule_rejects_bad_arguments():
    for bad in ((0, 8, 2), (16, 0, 2), (16, 8, 0), (16, 8, 9)):
        with pytest.raises(ValueError):
            hypertile.counts(*bad)


def test_handle_entries_reject_null(engine_lib):
    lib = engine_lib
    assert lib.sd_unet_set_hypertile(None, 32, 2, 0, 0) == 1
    assert lib.sd_unet_hypertile_step(None, 3) == 1
    assert lib.sd_unet_hypertile_sites(None) == 0
    assert lib.sd_unet_hypertile_read(None, 0, (C.c_int32 * 8)()) == 1


def test_header_declares_and_library_exports(engine_lib):
    header = open(os.path.join(ROOT, "include", "sd_engine.h")).read()
    raw = C.CDLL(engine_lib._name)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|int64_t)\s+%s\(" % name, header), name
        assert getattr(engine_lib, name) is not None and getattr(raw, name) is not None, name
