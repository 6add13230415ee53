"""CPU half of the temporal attention tests: what sd_temporal_attention_plan names for a shape, that the GPU case list
covers every instantiation, and that the bound of tests/tattn_cases.py holds for an emulation of the kernel's arithmetic
while four one-defect mutants of that emulation break it."""
import ctypes as C

import pytest
import torch

import tattn_cases as tc


def plan(lib, V, F, HW, heads, d):
    out = (C.c_int64 * 7)()
    rc = lib.sd_temporal_attention_plan(V, F, HW, heads, d, out)
    return rc, tuple(out)


def test_plan_sd15_shapes(engine_lib):
    """Two videos of 16 frames at 512 px: the four levels of SD 1.5 with eight motion heads."""
    for C_, hw in ((320, 64 * 64), (640, 32 * 32), (1280, 16 * 16), (1280, 8 * 8)):
        d = C_ // 8
        rc, got = plan(engine_lib, 2, 16, hw, 8, d)
        assert rc == 0, engine_lib.sd_last_error()
        assert got == (d, 1, tc.PIXELS, tc.WAVES, 16, tc.WAVES * 16 * tc.vstr_halves(d) * 2, 2 * hw // tc.PIXELS)
        rc, got = plan(engine_lib, 2, 32, hw, 8, d)
        assert rc == 0 and got[:5] == (d, 2, tc.PIXELS, tc.WAVES, 32) and got[5] <= 64 * 1024


def test_plan_thresholds_and_refusals(engine_lib):
    for d in tc.HEAD_DIMS:
        assert plan(engine_lib, 1, 16, 5, 2, d)[1][:2] == (d, 1)
        assert plan(engine_lib, 1, 17, 5, 2, d)[1][:2] == (d, 2)
        assert plan(engine_lib, 1, 1, 1, 1, d)[1][6] == 1
        assert plan(engine_lib, 3, 1, 2 * tc.PIXELS + 1, 1, d)[1][6] == 9
    for bad in ((1, 0, 4, 2, 40), (1, 33, 4, 2, 40), (1, 8, 4, 2, 48), (1, 8, 4, 2, 128), (0, 8, 4, 2, 40), (1, 8, 0, 2, 40),
                (1, 8, 4, 0, 40)):
        rc, _ = plan(engine_lib, *bad)
        assert rc == 4, bad                     # SD_ERR_UNSUPPORTED
        assert b"temporal_attention" in engine_lib.sd_last_error()
    assert engine_lib.sd_temporal_attention_plan(1, 8, 4, 2, 40, None) == 1


def test_cases_cover_every_instantiation(engine_lib):
    seen = set()
    for c in tc.GPU_CASES:
        rc, got = plan(engine_lib, c.V, c.F, c.HW, c.heads, c.d)
        assert rc == 0 and got == tc.expected_plan(c), tc.case_id(c)
        seen.add(got[:2])
    assert seen == set(tc.INSTANTIATIONS)
    # the whole cross product of the shape sets is there
    shapes = {(c.F, c.HW, c.V, c.heads, c.d) for c in tc.GPU_CASES if c.kind == "randn"}
    assert len(shapes) == len(tc.FRAMES) * len(tc.PIXEL_COUNTS) * len(tc.VIDEOS) * len(tc.HEADS) * len(tc.HEAD_DIMS)
    assert {c.kind for c in tc.GPU_CASES} == {"randn", "stress", "nobias"}
    assert {c.presc for c in tc.GPU_CASES} == {0, 1}


# the emulation runs the two-head cases of every (d, F, HW, V) and the stress / zero-table cases
EMULATED = [c for c in tc.GPU_CASES if c.heads == 2]


def test_emulation_within_bound():
    worst, worst_case, worst_round = 0.0, None, 0.0
    for case in EMULATED:
        q, k, v, bias = tc.make_inputs(case)
        qo, ko, vo = tc.operands(case, q, k, v, bias)
        O, A = tc.reference(case, qo, ko, vo)
        rnd = tc.score_rounding(case, qo, ko)
        worst_round = max(worst_round, rnd)
        assert rnd <= 2.0 ** -11, (tc.case_id(case), rnd)        # what elementwise_bound grants the scores
        out = tc.emulate(case, q, k, v, bias).double()
        assert torch.isfinite(out).all()
        ratio = ((out - O).abs() / tc.elementwise_bound(O, A, case.F, vo.abs().max().double())).max().item()
        if ratio > worst:
            worst, worst_case = ratio, case
        assert ratio <= 1.0, tc.case_id(case)
        if case.F == 1:
            assert torch.equal(out.half(), vo)
    print("emulation: worst |err| / bound %.3f (%s); worst score rounding %.2e of 2^-11 = %.2e"
          % (worst, tc.case_id(worst_case), worst_round, 2.0 ** -11))


MUTANTS = {
    "padded key not masked": dict(mask_pad=False),
    "bias added to q but not to k": dict(bias_k=False),
    "frame stride off by one row": dict(row_stride=+1),
    "table of frame f + 1 used for frame f": dict(table_shift=1),
}


@pytest.mark.parametrize("name", list(MUTANTS))
@pytest.mark.parametrize("d", (40, 160))
def test_mutants_break_the_bound(name, d):
    case = tc.Case(3, 15, 5, 2, d, 1, "randn")
    kw = dict(MUTANTS[name])
    if "row_stride" in kw:
        kw["row_stride"] = case.HW + kw["row_stride"]
    q, k, v, bias = tc.make_inputs(case)
    qo, ko, vo = tc.operands(case, q, k, v, bias)
    O, A = tc.reference(case, qo, ko, vo)
    bound = tc.elementwise_bound(O, A, case.F, vo.abs().max().double())
    good = ((tc.emulate(case, q, k, v, bias).double() - O).abs() / bound).max().item()
    bad = ((tc.emulate(case, q, k, v, bias, **kw).double() - O).abs() / bound).max().item()
    print("%s, d = %d: |err| / bound %.3f -> %.1f" % (name, d, good, bad))
    assert good <= 1.0 < bad


@pytest.mark.parametrize("C_", (64, 320, 1280))
def test_position_table_closed_form(C_):
    """The package's table (what the loader compares a stored one with, and the reference of sd_op_motion_pos_bias in the
    GPU suite) against the stated formula, element by element, written with pow instead of exp."""
    import math
    from stablediffusion_amd.motion import position_table
    pe = position_table(32, C_)
    assert pe.shape == (32, C_) and pe.dtype == torch.float64
    assert torch.equal(pe[0, 0::2], torch.zeros(C_ // 2, dtype=torch.float64))
    assert torch.equal(pe[0, 1::2], torch.ones(C_ // 2, dtype=torch.float64))
    for f in range(32):
        for i in range(C_ // 2):
            a = f * 10000.0 ** (-2.0 * i / C_)
            assert abs(pe[f, 2 * i].item() - math.sin(a)) < 1e-12 and abs(pe[f, 2 * i + 1].item() - math.cos(a)) < 1e-12
