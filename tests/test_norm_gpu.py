"""Every normalisation kernel launch_groupnorm can pick, through sd_op_groupnorm_ex, and the LayerNorm / row-statistics
kernels through sd_op_layernorm_ex / sd_op_row_stats, against a float64 CPU reference of the same fp16 operands, element
by element (tests/norm_cases.py holds the cases, the references and the bound; the CPU suite tests/test_norm_plan.py
proves the bound on an emulation of every kernel's summation order, that six plausible kernel bugs break it, and that
the cases reach every kernel form and prologue path).

Per run, in this order: rc == 0; the kernels that ran are the ones the case names (and what sd_norm_plan says); nothing
outside the output was written; the input is untouched; every element is finite; every element lies within the bound.
A second run must then give the same bits: the kernels reduce in a fixed order.

Guards: y lives in an int16 buffer pre-filled with an fp16 NaN bit pattern, GUARD rows in front and behind, and the
other columns of the concatenation buffer when strided; x sits in a NaN-filled buffer of the same build, so a read out
of range turns up as a non-finite output (or summary)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GUARD = 64                     # guard rows in front of and behind x and y
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
OTHER = 24                     # columns of the other tensor in a concatenation buffer
XOFF = 16                      # column offset of x inside its wider buffer


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def place(x2d, layout):
    """x [rows, C] fp16 (CPU) inside a NaN buffer: (buffer, view, row stride)."""
    rows, Cc = x2d.shape
    xw, xo = (Cc, 0) if layout == "dense" else (Cc + OTHER, XOFF)
    buf = torch.full((GUARD + rows + GUARD, xw), float("nan"), dtype=torch.float16, device="cuda")
    view = buf[GUARD:GUARD + rows, xo:xo + Cc]
    view.copy_(x2d)
    return buf, view, xw


def out_buffer(rows, Cc, layout):
    yw = Cc if layout == "dense" else Cc + OTHER
    yo = OTHER if layout == "right" else 0
    buf = torch.full((GUARD + rows + GUARD, yw), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, buf[GUARD:GUARD + rows, yo:yo + Cc], yw, yo


def collect(ybuf, rows, Cc, yo):
    """The output region as fp16 on the CPU, after checking that nothing around it was written."""
    yb = ybuf.cpu()
    out = yb[GUARD:GUARD + rows, yo:yo + Cc].clone()
    yb[GUARD:GUARD + rows, yo:yo + Cc] = SENTINEL
    assert (yb[:GUARD] == SENTINEL).all(), "rows in front of the output were written"
    assert (yb[GUARD + rows:] == SENTINEL).all(), "rows behind the output were written"
    assert (yb == SENTINEL).all(), "columns beside the output were written"
    return out.view(torch.float16)


def plan_of(lib, c):
    out = (C.c_int64 * 10)()
    rc = lib.sd_norm_plan(c.N, c.HW, c.C, c.G, 1 if c.pre else 0, nc.cdiv(c.HW, c.pre) if c.pre else 0, out)
    assert rc == 0, lib.sd_last_error()
    return list(out)


def run(lib, c, x, gamma, beta, layout, summaries=None):
    """Launches the case in one operand layout and returns the [N, HW, C] fp16 output on the CPU, after checking rc,
    what ran, the guards and the input.
      dense   ldx = ldy = C
      left    x a slice at column 16 of a [rows, C + 24] buffer; y the left columns of a buffer 24 wider
      right   the same x; y behind 24 columns of another tensor"""
    rows = c.N * c.HW
    xbuf, xv, ldx = place(x.view(rows, c.C), layout)
    ybuf, yv, ldy, yo = out_buffer(rows, c.C, layout)
    gd, bd = gamma.cuda(), beta.cuda()
    sd = summaries.cuda().contiguous() if summaries is not None else None
    S = summaries.shape[1] if summaries is not None else 0
    x_before = xbuf.view(torch.int16).clone()
    ran = (C.c_int64 * 10)()
    rc = lib.sd_op_groupnorm_ex(P(xv), ldx, P(gd), P(bd), P(yv), ldy, c.N, c.HW, c.C, c.G, c.eps, c.silu, P(sd), S, c.pre,
                                ran, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    ran = list(ran)
    assert tuple(ran[:5]) == c.want, \
        "the plan moved: this case no longer runs the kernels it was written for (ran %r, written for %r)" % (ran, c.want)
    want = plan_of(lib, c)
    if c.pre and want[9]:
        want[6] = c.pre                                # the plan entry is not told the tile height
    assert ran == want, (ran, want)
    out = collect(ybuf, rows, c.C, yo)
    assert torch.equal(xbuf.view(torch.int16), x_before), "the input buffer was written"
    return out.view(c.N, c.HW, c.C)


def check(c, out, r, bound):
    bad = ~torch.isfinite(out.float())
    assert not bad.any(), "%d non-finite elements, first at %r" % (int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]))
    err = (out.double() - r).abs()
    ratio = err / bound
    worst = int(ratio.argmax())
    print("%s <stats %d, apply %d, T %d, NV %d, finalize %d>: rel_l2 %.2e, worst |err| / bound %.3f, fp32 terms used %.3f"
          % ((nc.case_id(c),) + c.want + (rel_l2(out, r), ratio.flatten()[worst].item(), nc.error_ratios(out, r, bound)[1])))
    assert ratio.flatten()[worst].item() <= 1.0, \
        (nc.case_id(c), "element", np.unravel_index(worst, tuple(out.shape)), out.flatten()[worst].item(), r.flatten()[worst].item(),
         bound.flatten()[worst].item())


def _cases(*groups):
    cs = [c for c in nc.CASES if c.group in groups]
    return pytest.mark.parametrize("case", cs, ids=[nc.case_id(c) for c in cs])


def _summaries(c, x):
    return nc.tile_summaries(x, c.G, c.pre)[0] if c.pre else None


@_cases("fused", "twopass", "apply1", "narrow", "groups", "large", "defect", "supplied")
def test_groupnorm_against_float64(engine_lib, case):
    """fused: every HW edge of the three single-kernel forms, the UNets' widths, the fall-off at C = 5120.  twopass: both
    statistics kernels at channels per group 1, 2, 3, 6 and 4.  apply1: gn_apply_kernel (256 groups).  narrow: a last
    channel block narrower than the others.  groups: 1, 8, 16 groups.  large: NV = 8, 4, 2 and 256 slabs.  defect: the
    map sizes whose last slabs used to be empty.  supplied: the caller's summaries, with and without the finalize."""
    x, gamma, beta, r, bound = nc.inputs_and_reference(case)
    s = _summaries(case, x)
    out = run(engine_lib, case, x, gamma, beta, "dense", s)
    check(case, out, r, bound)
    cg = nc.constant_group(case)
    if cg:
        assert torch.isfinite(out[0, :, cg[0]:cg[1]].float()).all()
    again = run(engine_lib, case, x, gamma, beta, "dense", s)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "a second run gave other bits"


@_cases("strided")
def test_groupnorm_strided_operands(engine_lib, case):
    """The engine's layouts: x a column slice of a wider buffer, y the left, then the right columns of a concatenation
    buffer, NaN / sentinels in every other column.  Bit-identical to the dense run, itself checked."""
    x, gamma, beta, r, bound = nc.inputs_and_reference(case)
    assert case.layouts == ("dense", "left", "right")
    s = _summaries(case, x)
    dense = run(engine_lib, case, x, gamma, beta, "dense", s)
    check(case, dense, r, bound)
    for layout in case.layouts[1:]:
        out = run(engine_lib, case, x, gamma, beta, layout, s)
        assert torch.isfinite(out.float()).all(), layout
        assert torch.equal(dense.view(torch.int16), out.view(torch.int16)), layout


def test_supplied_summaries_with_an_empty_tile_are_refused(engine_lib):
    """(S - 1) rows < HW <= S rows or SD_ERR_INVALID, and nothing is launched: the sentinels stay."""
    x = torch.zeros(1000, 64, dtype=torch.float16, device="cuda")
    y = torch.full((1000, 64), SENTINEL, dtype=torch.int16, device="cuda")
    g = torch.ones(64, device="cuda")
    summ = torch.zeros(16 * 32 * 2, device="cuda")
    ran = (C.c_int64 * 10)()
    for S, rows in ((9, 128), (7, 128), (17, 63), (16, 67), (2, 1000)):
        rc = engine_lib.sd_op_groupnorm_ex(P(x), 64, P(g), P(g), P(y), 64, 1, 1000, 64, 32, 1e-5, 0, P(summ), S, rows, ran, stream())
        assert rc == 1, (S, rows)
        assert b"no empty one" in engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()


DEFECT = [c for c in nc.CASES if c.group == "defect"]


@pytest.mark.parametrize("case", DEFECT, ids=[nc.case_id(c) for c in DEFECT])
def test_gn_stats_summaries_match_their_own_rows(engine_lib, case):
    """sd_op_gn_stats on the map sizes whose last slabs used to be empty: S slabs cover HW with none empty, every
    summary is finite (x sits between NaN rows and columns) and is the float64 (mean, M2) of its own rows within the
    statistics terms of the bound."""
    c = case
    x = nc.make_inputs(c)[0]
    xbuf, xv, ldx = place(x.view(c.N * c.HW, c.C), "left")
    p = plan_of(engine_lib, c._replace(pre=0))
    out = np.full(p[8], np.nan, np.float32)
    S, rows, kernel = C.c_int(), C.c_int64(), C.c_int()
    rc = engine_lib.sd_op_gn_stats(P(xv), ldx, c.N, c.HW, c.C, c.G, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(S),
                                   C.byref(rows), C.byref(kernel), stream())
    assert rc == 0, engine_lib.sd_last_error()
    S, rows = S.value, rows.value
    assert (S, rows) == (p[5], p[6]) and kernel.value == c.want[0]
    assert (S - 1) * rows < c.HW <= S * rows
    got = torch.from_numpy(out[:c.N * S * c.G * 2]).view(c.N, S, c.G, 2).double()
    assert torch.isfinite(got).all(), "%d non-finite summaries" % int((~torch.isfinite(got)).sum())
    _, want = nc.tile_summaries(x, c.G, rows)
    dm, dq = nc.summary_errors(got, want, nc.slab_counts(c.HW, S, rows, c.C // c.G))
    print("%s: S %d x %d rows, worst mean error %.3f, worst M2 error %.3f of the bound's terms" % (nc.case_id(c), S, rows, dm, dq))
    assert dm <= 1.0 and dq <= 1.0


@pytest.mark.parametrize("N,HW,Ca,Cb", [(1, 4289, 320, 320), (2, 5776, 640, 320)])
def test_groupnorm_concat_at_map_sizes_with_a_short_last_slab(engine_lib, N, HW, Ca, Cb):
    """sd_op_groupnorm_concat at the 76 x 76 level of SDXL at 1216 px (HW = 4289 stands for every size whose halves'
    slabs used to end past the map): gn_cat_finalize_kernel merges slabs of unequal size, none of them empty."""
    c = nc.Case("concat", N, HW, Ca + Cb, 32, 1, 1e-5, "randn", 0, None, ("dense",))
    x, gamma, beta, r, bound = nc.inputs_and_reference(c)
    rows = N * HW
    xbuf, xv, _ = place(x.view(rows, c.C), "dense")
    ybuf, yv, _, yo = out_buffer(rows, c.C, "dense")
    gd, bd = gamma.cuda(), beta.cuda()
    outs = []
    for _ in range(2):
        rc = engine_lib.sd_op_groupnorm_concat(P(xv), Ca, Cb, P(gd), P(bd), P(yv), N, HW, 32, 1e-5, 1, stream())
        assert rc == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        outs.append(collect(ybuf, rows, c.C, yo).view(N, HW, c.C))
    c = c._replace(want=(2, 2, 0, 0, 0))
    check(c, outs[0], r, bound)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_groupnorm_conv2d_at_65x65(engine_lib):
    """GroupNorm -> SiLU -> 3x3 conv on the VAE's 65 x 65 mid-block map (a 520 x 520 image), C = 128: the statistics
    pass in front of the convolution runs on HW = 4225.  Against F.group_norm -> F.silu -> F.conv2d in fp32, with the
    tolerance of test_ops_gpu.test_groupnorm_conv2d."""
    N, H, W, Cin, Cout, G = 1, 65, 65, 128, 128, 32
    g = torch.Generator().manual_seed(65)
    x = (torch.randn(N, Cin, H, W, generator=g) + 0.3 * torch.randn(1, Cin, 1, 1, generator=g)).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half()
    gamma = 1.0 + 0.3 * torch.randn(Cin, generator=g)
    beta = 0.3 * torch.randn(Cin, generator=g)
    bias = torch.randn(Cout, generator=g) * 0.5
    ref = F.conv2d(F.silu(F.group_norm(x.float(), G, gamma, beta, 1e-5)), w.float(), bias, padding=1)
    xbuf, xv, _ = place(x.permute(0, 2, 3, 1).reshape(H * W, Cin), "dense")
    y = torch.empty(N, H, W, Cout, dtype=torch.float16, device="cuda")
    wd, bd, gd, btd = w.cuda().contiguous(), bias.cuda(), gamma.cuda(), beta.cuda()
    fused = C.c_int(-1)
    rc = engine_lib.sd_op_groupnorm_conv2d(P(xv), P(gd), P(btd), G, 1e-5, 1, P(wd), P(bd), None, None, P(y), N, H, W, Cin, Cout,
                                           3, 0, None, C.byref(fused), stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    out = y.float().cpu().permute(0, 3, 1, 2)
    assert torch.isfinite(out).all()
    print("groupnorm_conv2d 65 x 65: fused %d, rel_l2 %.2e" % (fused.value, rel_l2(out, ref)))
    assert rel_l2(out, ref) < 3e-3


# ------------------------------------------------------------------------------------------- LayerNorm, row statistics
@pytest.mark.parametrize("t", nc.LN_CASES, ids=[nc.ln_id(t) for t in nc.LN_CASES])
def test_layernorm_against_float64(engine_lib, t):
    rows, Cc, profile, strided = t
    x, gamma, beta, r, bound, _ = nc.ln_inputs_and_reference(rows, Cc, profile)
    layout = "right" if strided else "dense"
    xbuf, xv, ldx = place(x, layout)
    ybuf, yv, ldy, yo = out_buffer(rows, Cc, layout)
    gd, bd = gamma.cuda(), beta.cuda()
    x_before = xbuf.view(torch.int16).clone()
    outs = []
    for _ in range(2):
        rc = engine_lib.sd_op_layernorm_ex(P(xv), ldx, P(gd), P(bd), P(yv), ldy, rows, Cc, 1e-5, stream())
        assert rc == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        outs.append(collect(ybuf, rows, Cc, yo))
    assert torch.equal(xbuf.view(torch.int16), x_before), "the input buffer was written"
    out = outs[0]
    assert torch.isfinite(out.float()).all()
    ratio, used = nc.error_ratios(out, r, bound)
    print("layernorm %s: worst |err| / bound %.3f, fp32 terms used %.3f" % (nc.ln_id(t), ratio, used))
    assert ratio <= 1.0
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("Cc", [2056, 4, 12, 2052])
def test_layernorm_refuses_widths_it_cannot_hold(engine_lib, Cc):
    """C > 2048 (a wave holds four 16-byte chunks per lane) and C % 8 != 0: SD_ERR_INVALID, nothing written."""
    ld = (Cc + 7) // 8 * 8
    x = torch.zeros(4, ld, dtype=torch.float16, device="cuda")
    y = torch.full((4, ld), SENTINEL, dtype=torch.int16, device="cuda")
    g = torch.ones(ld, device="cuda")
    assert engine_lib.sd_op_layernorm_ex(P(x), ld, P(g), P(g), P(y), ld, 4, Cc, 1e-5, stream()) == 1
    if Cc % 8 == 0:
        assert engine_lib.sd_op_layernorm(P(x), P(g), P(g), P(y), 4, Cc, 1e-5, stream()) == 1
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()


@pytest.mark.parametrize("t", nc.ROW_STATS_CASES, ids=[nc.ln_id(t) for t in nc.ROW_STATS_CASES])
def test_row_stats_against_float64(engine_lib, t):
    """sd_op_row_stats: (mean, M2) per row, x a column slice between NaN rows and columns, the statistics between
    sentinels; within the statistics terms of the bound."""
    rows, Cc, profile = t
    x, _, _, _, _, want = nc.ln_inputs_and_reference(rows, Cc, profile)
    xbuf, xv, ldx = place(x, "left")
    sbuf = torch.full((GUARD + rows + GUARD, 2), float("inf"), dtype=torch.float32, device="cuda")
    sv = sbuf[GUARD:GUARD + rows]
    rc = engine_lib.sd_op_row_stats(P(xv), ldx, P(sv), rows, Cc, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    sb = sbuf.cpu()
    assert torch.isinf(sb[:GUARD]).all() and torch.isinf(sb[GUARD + rows:]).all(), "statistics outside the rows were written"
    got = sb[GUARD:GUARD + rows].double()
    assert torch.isfinite(got).all()
    dm, dq = nc.summary_errors(got, want, float(Cc))
    print("row_stats %s: worst mean error %.3f, worst M2 error %.3f of the bound's terms" % (nc.ln_id(t), dm, dq))
    assert dm <= 1.0 and dq <= 1.0
