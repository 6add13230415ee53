"""sd_ip_attention_plan (host only) and the cases of tests/ip_cases.py: the plan's numbers, the cases in the form
their ids claim (one tile per block, or a walk in uneven rounds with a ragged last tile), the stated coverage, the
emulation of ip_xattn_kernel's arithmetic inside the element-wise bound the GPU suite asserts, and one-defect mutants
of that emulation outside it -- the proof, without a GPU, that the GPU tests fail for a subtly wrong kernel."""
import ctypes as C

import pytest
import torch

import ip_cases as ic

LDS_LIMIT = 160 * 1024
_IDS = [ic.case_id(c) for c in ic.GPU_CASES]


def plan(lib, B, Tq, L, Tip, heads, d, lam):
    out = (C.c_int * 4)()
    code = lib.sd_ip_attention_plan(B, Tq, L, Tip, heads, d, lam, out)
    return code, tuple(out)


def form_of(lib, c):
    code, (rows, qtiles, qblocks, lds) = plan(lib, c.B, c.Tq, c.L, c.Tip, c.heads, c.d, c.lam)
    assert code == 0, lib.sd_last_error()
    assert rows == 64 and qtiles == -(-c.Tq // rows) and 1 <= qblocks <= qtiles and 0 < lds <= LDS_LIMIT
    if qblocks == qtiles:
        return "single"
    # a walk worth the name: uneven rounds and a ragged last tile
    assert qtiles % qblocks != 0 and c.Tq % rows != 0, (qtiles, qblocks)
    return "walk"


def test_plan_numbers(engine_lib):
    """64 rows per tile; ceil(1024 / (B heads)) blocks per (batch, head), at most one per tile; LDS = the padded key rows
    of both segments (of the text alone at lambda = 0) times the K and V row strides."""
    assert plan(engine_lib, 8, 4096, 77, 4, 8, 40, 1.0) == (0, (64, 64, 16, (96 + 32) * (80 + 48) * 2))    # SD1.5, 64 x 64
    assert plan(engine_lib, 8, 4096, 77, 4, 8, 40, 0.0) == (0, (64, 64, 16, 96 * (80 + 48) * 2))
    assert plan(engine_lib, 2, 67, 77, 4, 3, 64, 0.6)[1][:3] == (64, 2, 2)
    assert plan(engine_lib, 2000, 4096, 77, 4, 8, 40, 1.0)[1][1:3] == (64, 1)
    assert plan(engine_lib, 2, 1, 160, 64, 2, 160, 1.0) == (0, (64, 1, 1, 224 * (176 + 176) * 2))
    for d in ic.HEAD_DIMS:
        assert plan(engine_lib, 2, 300, 160, 64, 2, d, 1.0)[1][3] <= LDS_LIMIT
    assert plan(engine_lib, 0, 64, 77, 4, 8, 40, 1.0) == (0, (64, 0, 0, 0))          # nothing to launch


def test_plan_rejects_what_the_launch_rejects(engine_lib):
    for L, Tip, d in [(161, 4, 64), (0, 4, 64), (77, 65, 64), (77, 0, 64), (77, 4, 128), (77, 4, 48)]:
        assert plan(engine_lib, 1, 8, L, Tip, 8, d, 1.0)[0] == 4, (L, Tip, d)
        assert engine_lib.sd_last_error()
    assert plan(engine_lib, 1, 8, 77, 4, 8, 64, float("nan"))[0] == 1
    assert engine_lib.sd_ip_attention_plan(1, 8, 77, 4, 8, 64, 1.0, None) == 1


def test_cases_have_the_form_they_name(engine_lib):
    for c in ic.GPU_CASES:
        assert form_of(engine_lib, c) == c.form, ic.case_id(c)
    assert len(set(_IDS)) == len(_IDS)


def test_cases_cover_what_they_state():
    cs = ic.GPU_CASES
    for d in ic.HEAD_DIMS:
        edge = [c for c in cs if c.group == "edge" and c.d == d]
        assert {c.Tq for c in edge} == set(ic.TQ_EDGES)
        assert {c.L for c in edge} == set(ic.L_EDGES)
        assert {c.Tip for c in edge} == set(ic.TIP_EDGES)
        assert all(c.B >= 2 and c.heads >= 2 for c in edge)
        assert {c.lam for c in cs if c.group == "lambda" and c.d == d} == set(ic.LAMBDAS)
        assert {c.kind for c in cs if c.group == "scores" and c.d == d} == {"big_text", "big_ip", "neg_text", "neg_ip"}
        assert any(c.group == "walk" and c.d == d for c in cs) and any(c.group == "constv" and c.d == d for c in cs)
        assert {c.presc for c in cs if c.d == d} == {0, 1}
    assert {c.lam for c in cs} >= set(ic.LAMBDAS)
    assert sum(c.form == "walk" for c in cs) >= 2


@pytest.mark.parametrize("case", ic.GPU_CASES, ids=_IDS)
def test_emulation_is_inside_the_bound(case):
    q, k, v, kip, vip, O, A = ic.inputs_and_reference(case)
    out = ic.emulate(case, q, k, v, kip, vip).double()
    assert torch.isfinite(out).all()
    ratio = ((out - O).abs() / ic.bound_of(case, v, vip, O, A)).max().item()
    print("%s: emulation worst |err| / bound %.3f" % (ic.case_id(case), ratio))
    assert ratio <= 1.0, ratio


def _breaks(case, mutant):
    q, k, v, kip, vip, O, A = ic.inputs_and_reference(case)
    out = ic.emulate(case, q, k, v, kip, vip, mutant).double()
    return not bool(((out - O).abs() <= ic.bound_of(case, v, vip, O, A)).all())     # (a NaN breaks it too)


# the small cases first: any() stops at the first case that catches the mutant
_BY_SIZE = sorted(ic.GPU_CASES, key=lambda c: c.B * c.heads * c.Tq * (c.L + c.Tip) * c.d)


@pytest.mark.parametrize("mutant", [m for m in ic.MUTANTS if m != "lambda_after_rounding"])
def test_a_listed_case_catches_each_mutant(mutant):
    """lambda left off the image segment's last 32-key step; the last valid key of a segment masked; the key just past
    the end let in; one 16-query sub-tile's rows taken from the next tile; both segments normalised by one joint sum."""
    caught = next((ic.case_id(c) for c in _BY_SIZE if _breaks(c, mutant)), None)
    print(mutant, "caught by", caught)
    assert caught is not None, mutant


@pytest.mark.parametrize("mutant,group", [("lambda_off_last_step", "edge"), ("last_key_masked", "edge"),
                                          ("key_past_end", "edge"), ("joint_sum", "lambda")])
@pytest.mark.parametrize("d", ic.HEAD_DIMS)
def test_key_and_lambda_mutants_are_caught_at_every_head_dim(mutant, group, d):
    assert any(_breaks(c, mutant) for c in _BY_SIZE if c.d == d and c.group == group), (mutant, d)


@pytest.mark.parametrize("d", ic.HEAD_DIMS)
def test_mutants_are_caught_where_they_are_hardest_to_see(d):
    """At every head dim: lambda off the last step where that step is the second of two (T_ip = 33: one key of 33;
    T_ip = 64), a masked last key and a key let in among 77 or more text keys, and the swapped sub-tile."""
    mine = [c for c in _BY_SIZE if c.d == d and c.group != "walk"]
    assert any(_breaks(c, "lambda_off_last_step") for c in mine if c.Tip > 32 and c.lam != 1.0)
    assert any(_breaks(c, "last_key_masked") for c in mine if c.L >= 77 and c.Tip >= 4)
    assert any(_breaks(c, "key_past_end") for c in mine if c.L in (77, 154) and c.Tip >= 4 and c.Tip % 32 != 0)
    assert any(_breaks(c, "subtile_from_next_tile") for c in mine if c.Tq >= 96)


def test_lambda_after_the_rounding_is_not_distinguishable():
    """P = lambda * fp16(p / l) instead of fp16(p lambda / l) is the same arithmetic to within the bound: both round
    the probability once, 2^-11 relative, and the mutant is the more accurate of the two where lambda pushes
    p lambda / l into fp16's subnormal range.  So the bound cannot tell them apart, and this mutant is not in the
    list above; that it stays inside the bound on every small case is what this test records."""
    for c in _BY_SIZE:
        if c.group != "walk":
            assert not _breaks(c, "lambda_after_rounding"), ic.case_id(c)
