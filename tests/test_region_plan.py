"""sd_region_plan (host only) and the cases of tests/region_cases.py: the plan stays inside the LDS and covers every
segment, the GPU cases run the form they were written for and cover both forms at every head dim, the emulation of
region_xattn_kernel's arithmetic stays inside the element-wise bound the GPU suite asserts, and unsupported arguments
are rejected."""
import ctypes as C

import pytest
import torch

import region_cases as rc


def plan(lib, R, L, d):
    out = (C.c_int * 4)()
    code = lib.sd_region_plan(R, L, d, out)
    return code, tuple(out)


@pytest.mark.parametrize("d", rc.HEAD_DIMS)
def test_plan_fits_the_lds_and_covers_every_segment(engine_lib, d):
    for R in range(1, 9):
        for L in (1, 77, 96, 160):
            code, (per, groups, lds, tiles) = plan(engine_lib, R, L, d)
            assert code == 0, engine_lib.sd_last_error()
            assert 0 < lds <= rc.LDS_LIMIT, (R, L, lds)
            assert per >= 1 and groups >= 1 and per * groups >= R and per * (groups - 1) < R, (R, L, per, groups)
            assert tiles == (1 if groups > 1 else 0)
            if groups > 1:                          # split only when one more segment would not fit
                assert lds // per * R > rc.LDS_LIMIT - 16, (R, L, per, lds)


def test_plan_matches_the_stated_segment_sizes(engine_lib):
    """One 77-key segment (96 rows): 24.6 KB at d = 40, 30.7 KB at d = 64, 67.6 KB at d = 160; so two fit at d = 160."""
    for d, kb in ((40, 24576), (64, 30720), (160, 67584)):
        code, (per, groups, lds, _) = plan(engine_lib, 1, 77, d)
        assert (code, per, groups, lds) == (0, 1, 1, kb + 16)
    assert plan(engine_lib, 2, 77, 160)[1][:2] == (2, 1)
    assert plan(engine_lib, 3, 77, 160)[1][:2] == (2, 2)
    assert plan(engine_lib, 5, 77, 160)[1][:2] == (2, 3)
    assert plan(engine_lib, 8, 160, 160)[1][:2] == (1, 8)


def test_cases_run_the_form_they_name_and_cover_both(engine_lib):
    seen = set()
    for c in rc.GPU_CASES:
        code, (per, groups, lds, _) = plan(engine_lib, c.R, c.L, c.d)
        assert code == 0
        assert ("grouped" if groups > 1 else "resident") == c.form, rc.case_id(c)
        seen.add((c.d, c.form))
    for d in rc.HEAD_DIMS:
        can_group = any(plan(engine_lib, R, L, d)[1][1] > 1 for R in range(1, 9) for L in (77, 160))
        assert (d, "resident") in seen
        assert not can_group or (d, "grouped") in seen, d
    ids = [rc.case_id(c) for c in rc.GPU_CASES]
    assert len(set(ids)) == len(ids)
    # the stated coverage
    assert {c.Tq for c in rc.GPU_CASES} >= {64, 100, 257} and {c.L for c in rc.GPU_CASES} >= {5, 77}
    assert {c.R for c in rc.GPU_CASES} >= {1, 2, 3, 5}
    assert {(c.d, c.R) for c in rc.GPU_CASES if c.form == "grouped"} >= {(160, 3), (160, 5)}
    assert any(c.Bw < c.B for c in rc.GPU_CASES) and any(c.presc for c in rc.GPU_CASES)
    idx = rc.disjoint_regions(100, 3)
    assert idx[22] == 0 and idx[23] == 1            # a boundary inside the second 16-query tile


@pytest.mark.parametrize("case", rc.GPU_CASES, ids=[rc.case_id(c) for c in rc.GPU_CASES])
def test_emulation_is_inside_the_bound(case):
    """The bound of attn_cases.elementwise_bound with Tk = R L and A = sum_r w_r sum_k p_rk |v_rk| holds for the
    kernel's arithmetic without an extra term: P = fp16(p w / l) is rounded to nearest (2^-11 relative, below the
    2^-10 of a truncation the bound was written for), the weight multiplies before the rounding, and the fp32
    accumulator runs over R L keys."""
    q, k, v, w, O, A = rc.inputs_and_reference(case)
    assert torch.allclose(w.sum(-1), torch.ones(case.Bw, case.Tq), atol=1e-6)
    out = rc.emulate(case, q, k, v, w).double()
    assert torch.isfinite(out).all()
    bound = rc.elementwise_bound(O, A, case.R * case.L, v.abs().max().double())
    ratio = ((out - O).abs() / bound).max().item()
    assert ratio <= 1.0, ratio


def test_unsupported_arguments_are_rejected(engine_lib):
    for R, L, d in [(1, 77, 48), (1, 77, 128), (0, 77, 40), (9, 77, 40), (-1, 77, 40), (2, 0, 40), (2, 161, 40)]:
        code, _ = plan(engine_lib, R, L, d)
        assert code == 4, (R, L, d)
        assert engine_lib.sd_last_error()
    assert engine_lib.sd_region_plan(2, 77, 40, None) == 1
