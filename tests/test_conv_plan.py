"""The cases of tests/conv_cases.py checked on the CPU: each plans (sd_igemm_plan, host code only) to the kernel it names,
together they reach every kernel igemm2_plan can pick and both split-K reducers, none is skipped anywhere, and the
references hold what the GPU suite relies on: exact cases are representable in fp16, and an fp32 emulation of the
kernels' arithmetic stays inside the element-wise bound of every randn case."""
import ctypes as C
import os

import pytest
import torch

import conv_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(lib, c):
    geom, flags = cc.plan_args(c)
    out = (C.c_int64 * 12)()
    name = C.create_string_buffer(64)
    lib.sd_igemm_force(*(c.force or (-1, 0)))
    try:
        rc = lib.sd_igemm_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*flags), out, name)
    finally:
        lib.sd_igemm_force(-1, 0)
    assert rc == 0, (cc.case_id(c), lib.sd_last_error())
    return list(out), name.value.decode()


def test_case_ids_are_unique():
    ids = [cc.case_id(c) for c in cc.CASES]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1][:5]
    assert len({cc.small_cout_id(s) for s in cc.SMALL_COUT_CASES}) == len(cc.SMALL_COUT_CASES) == 12


def test_every_case_plans_to_the_kernel_it_names(engine_lib):
    moved = []
    for c in cc.CASES:
        out, name = plan(engine_lib, c)
        kind, splits, gn_emit, scales_ok = out[0], out[2], out[7], out[9]
        M, K = cc.gemm_dims(c)
        slabs = c.Cin // 64 if kind in cc.HALO else K // 64
        want = (kind,) + cc.launched(slabs, splits, gn_emit) if splits > 1 else (kind, 1, 0)
        if want != c.want:
            moved.append((cc.case_id(c), c.want, want, name))
        if c.acc_scale != 1.0 or c.bias_scale != 1.0:
            assert scales_ok, cc.case_id(c)
    assert not moved, "the plan moved: these cases no longer run the kernel they were written for: %r" % moved[:8]


def test_conv_ex_rejects_bad_arguments(engine_lib):
    """A stride below the dense width or a wider one that is no multiple of 8, an unknown activation, a padding outside
    -1..1 and a missing `ran` are refused before anything touches a device."""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    ran = (C.c_int * 4)()

    def call(ldx=64, ldres=8, ldy=8, res=None, pad=-1, act=0, ran=ran, geglu=0, Cout=8):
        return engine_lib.sd_op_conv2d_ex(p, p, None, None, res, p, 1, 4, 1, 64, Cout, 1, 1, 0, geglu, ldx, ldres, ldy, pad, act,
                                          1.0, 1.0, 0, ran, None)
    for kw in (dict(ldx=63), dict(ldx=68), dict(ldy=7), dict(ldy=12), dict(ldres=12, res=p), dict(ldres=4, res=p),
               dict(geglu=1, Cout=256, ldy=256 + 4), dict(geglu=1, Cout=256, ldy=120), dict(act=3), dict(pad=2), dict(pad=-2),
               dict(ran=None)):
        assert call(**kw) == 1, kw                      # SD_ERR_INVALID
        assert b"sd_op_conv2d_ex" in engine_lib.sd_last_error(), kw


def test_cases_reach_every_kernel_and_both_reducers():
    kinds = {c.want[0] for c in cc.CASES}
    assert kinds == cc.ALL_KINDS, sorted(cc.ALL_KINDS - kinds)
    assert {c.want[2] for c in cc.CASES} == {0, 1, 2}
    # each reducer behind a streamed tile and reducer 1 behind a halo tile
    assert {(c.want[0] in cc.HALO, c.want[2]) for c in cc.CASES if c.want[2]} >= {(False, 1), (False, 2), (True, 1)}
    by_group = lambda g: [c for c in cc.CASES if c.group == g]       # noqa: E731
    # ring: every streamed tile and igemm3 at 1, 2, STAGES - 1, STAGES, STAGES + 1 slabs (igemm3: from STAGES), and a
    # last split-K slice shorter than the ring
    for v, (bm, bn, st) in cc.TILE.items():
        ks = {c.Cin // 64 for c in by_group("ring") if c.want == (v, 1, 0)}
        assert ks == {1, 2, st - 1, st, st + 1}, (v, ks)
        short = [c for c in by_group("ring") if c.want == (v, 2, 1)]
        assert short and all((c.Cin // 64) - cc.cdiv(c.Cin // 64, 2) < st for c in short), v
    assert {c.Cin // 64 for c in by_group("ring") if c.want[0] == cc.REG} == {cc.REG_TILE[2], cc.REG_TILE[2] + 1}
    # edges: M and Cout around the tile for every streamed tile
    for v, (bm, bn, st) in cc.TILE.items():
        got = {(c.H, c.Cout) for c in by_group("edges") if c.want[0] == v and c.ks == 1}
        assert got == {(m, n) for m in (1, bm - 1, bm, bm + 1) for n in (8, bn - 8, bn, bn + 8)}, v
        assert {(c.N, c.H, c.W) for c in by_group("edges") if c.want[0] == v and c.ks == 3} == {(3, 7, 9), (3, 9, 7)}
    # gather: the three patch widths on both halo tiles, with and without the upsample, every split of three slabs
    for v in cc.HALO:
        got = {(cc.halo_patch_width(*cc.out_size(c)), c.up, c.want[1]) for c in by_group("gather") if c.want[0] == v}
        assert got == {(wt, up, sp) for wt in (16, 32, 64) for up in (0, 1) for sp in (1, 2, 3)}, (v, got)
    assert {(c.stride, c.pad, c.up) for c in by_group("gather") if c.want[0] in cc.TILE} == {(1, -1, 0), (2, -1, 0), (2, 0, 0), (1, -1, 1)}
    assert all(c.N >= 2 and c.kind == "tap" for c in by_group("gather"))
    # strided: one case per family, all three layouts
    fam = {c.want[0] for c in by_group("strided")}
    assert fam >= {3, 2, 10, 15, 13, 14, cc.REG, 100, -1} and all(c.layouts == ("dense", "left", "right") for c in by_group("strided"))
    assert {c.want[2] for c in by_group("strided")} == {0, 1, 2}
    # GEGLU kernels with the saturated gate, and a randn case each
    for kind in ("sat", "randn"):
        assert {c.want[0] for c in cc.CASES if c.geglu and c.kind == kind} >= {0, 1, 6, 14, 100}
    assert {c.act for c in cc.CASES if c.kind == "randn"} == {0, 1, 2}
    assert all(cc.gemm_dims(c)[1] <= 1152 for c in cc.CASES if c.kind == "randn")
    # small Cout: all nine taps between the tap cases
    taps = {cc.tap_of(cc.small_cout_case(s), co) for s in cc.SMALL_COUT_CASES if s[5] == "tap" for co in range(s[4])}
    assert taps == set(range(9)), taps


def test_no_case_is_skipped_or_expected_to_fail():
    """The cap on omitted cases is zero: the GPU module and the case list hold no skip / xfail mark or call (this
    module has none either: nothing here is conditional), and every group is parametrised into a GPU test."""
    for mod in ("test_conv_gpu.py", "conv_cases.py"):
        src = open(os.path.join(ROOT, "tests", mod)).read()
        for word in ("skip", "xfail"):
            assert word not in src, (mod, word)
    src = open(os.path.join(ROOT, "tests", "test_conv_gpu.py")).read()
    for group in {c.group for c in cc.CASES}:
        assert '"%s"' % group in src, group
    assert "SMALL_COUT_CASES" in src


def _exact_cases():
    cs = [c for c in cc.CASES if c.kind != "randn"] + [cc.small_cout_case(s) for s in cc.SMALL_COUT_CASES]
    seen, out = set(), []
    for c in cs:                        # the same problem under another force / layout has the same reference
        key = c._replace(group="", force=None, want=None, layouts=(), gn_groups=0)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_exact_references_are_representable_in_fp16():
    n = 0
    for c in _exact_cases():
        x, w, bias, rowadd, res = cc.make_inputs(c)
        r, _ = cc.reference(c, x, w, bias, rowadd, res)
        assert torch.isfinite(r).all()
        assert torch.equal(r.half().double(), r), (cc.case_id(c), r.abs().max().item())
        if c.kind in ("grid", "sat"):
            # every partial sum is a multiple of 1/16 (1/128 scaled down) far below 2^20 of them: exact in fp32
            M, K = cc.gemm_dims(c)
            assert K * 2 * 1 < 2 ** 20 / 16 and r.abs().max() < 2048
            unit = 16.0 / min(c.acc_scale, c.bias_scale, 1.0)
            assert torch.equal((r * unit).round(), r * unit), cc.case_id(c)
        if c.res and not c.geglu:
            # the value rounded to fp16 ahead of the residual add is representable as well
            p = r - res.double()
            assert torch.equal(p.half().double(), p), cc.case_id(c)
        n += 1
    assert n >= 100


@pytest.mark.parametrize("case", [c for c in cc.CASES if c.kind == "randn"],
                         ids=[cc.case_id(c) for c in cc.CASES if c.kind == "randn"])
def test_fp32_emulation_stays_inside_the_bound(case):
    """Slab by slab in K order, and as four split partials summed afterwards."""
    x, w, bias, rowadd, res, r, bound = cc.inputs_and_reference(case)
    assert (bound > 0).all() and torch.isfinite(bound).all()
    # not vacuous: for the typical element the bound is a few fp16 steps of the result (two roundings of two values with
    # a residual, the hidden value's step times the gate under GEGLU)
    assert (bound / U16_STEP(r)).median().item() <= 8.0
    for nsplit in (1, 4):
        got = cc.emulate(case, x, w, bias, rowadd, res, nsplit).double()
        ratio = ((got - r).abs() / bound).max().item()
        assert ratio <= 1.0, (cc.case_id(case), nsplit, ratio)


def U16_STEP(r):
    """fp16 spacing at |r| (at least that of the smallest normal)."""
    return 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14))) - 10)


def test_bound_sees_one_wrong_element():
    """What the whole-tensor metric lets through: one element 10 % off passes rel-L2 < 2e-3 and breaks the bound."""
    from conftest import rel_l2
    case = next(c for c in cc.CASES if c.kind == "randn" and c.want[0] in cc.HALO and c.res)
    x, w, bias, rowadd, res, r, bound = cc.inputs_and_reference(case)
    got = cc.emulate(case, x, w, bias, rowadd, res, 1).clone()
    i = int(r.abs().argmax())
    got.view(-1)[i] = (got.view(-1)[i].float() * 1.1).half()
    assert rel_l2(got, r) < 2e-3
    assert ((got.double() - r).abs() / bound).max().item() > 10.0
