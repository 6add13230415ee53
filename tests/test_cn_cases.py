"""The cases of tests/cn_cases.py without a GPU: they cover what they state, an emulation of cn_cond_conv_kernel's
arithmetic stays inside the element-wise bound the GPU suite asserts, and an emulation that mishandles the padding
breaks it on the border ring of every case that has taps outside the image."""
import pytest
import torch

import cn_cases as cc

_IDS = [cc.case_id(c) for c in cc.CASES]


def test_cases_cover_what_they_state():
    cs = cc.CASES
    assert len(set(_IDS)) == len(_IDS)
    assert {(c.Cin, c.stride) for c in cs} == {(ci, s) for ci in (3, 16, 32, 96) for s in (1, 2)}
    assert {c.Cout for c in cs} == {16, 32, 96} and {c.N for c in cs} == {1, 3}
    pix = [c.N * cc.out_hw(c)[0] * cc.out_hw(c)[1] for c in cs]
    assert any(p < 256 for p in pix) and any(p > 256 and p % 256 for p in pix) and any(p % 256 == 0 for p in pix)
    assert any((c.IH, c.IW) == (1, 1) for c in cs) and any(c.IH == 1 and c.IW > 1 for c in cs)
    assert any(c.stride == 2 and c.IH % 2 and c.IW % 2 and cc.out_hw(c) == (5, 7) for c in cs)
    assert any(not c.silu for c in cs)
    for c in cs:
        assert cc.border_ring(c).any()


def test_residual_tables_cover_what_they_state():
    t = cc.RES_TABLES["sixteen"]
    assert len(t) == 16 and len(cc.RES_TABLES["one"]) == 1
    assert {M for M, _ in t} == set(cc.RES_M) and {C_ for _, C_ in t} == set(cc.RES_C)
    assert all(len({C_ for M_, C_ in t if M_ == M}) == 2 for M in cc.RES_M)


@pytest.mark.parametrize("case", cc.CASES, ids=_IDS)
def test_emulation_is_inside_the_bound(case):
    x, w, b, out, y, A = cc.inputs_and_reference(case)
    got = cc.emulate(case, x, w, b).double()
    assert torch.isfinite(got).all()
    ratio = (got - out).abs() / cc.bound(case, out, y, A)
    ring = cc.border_ring(case)
    print("%s: emulation worst |err| / bound %.3f, on the border ring %.3f" % (cc.case_id(case), ratio.max(), ratio[:, ring].max()))
    assert ratio.max() <= 1.0
    if case.silu:
        assert y.min() < -1.0 and y.max() > 1.0 or case.IH * case.IW == 1       # both branches of the activation


@pytest.mark.parametrize("case", cc.CASES, ids=_IDS)
def test_wrong_padding_breaks_the_bound_on_the_border(case):
    """Taps outside the image that add the clamped pixel (the kernel reads it, and multiplies by zero) are seen on the
    border ring and nowhere else."""
    x, w, b, out, y, A = cc.inputs_and_reference(case)
    got = cc.emulate(case, x, w, b, "no_pad").double()
    bad = (got - out).abs() > cc.bound(case, out, y, A)
    ring = cc.border_ring(case)
    assert bad[:, ring].any()
    assert not bad[:, ~ring].any()
