"""Every convolution / linear kernel igemm2_plan can pick, through sd_op_conv2d_ex, against a float64 CPU reference of
the same operands, element by element (tests/conv_cases.py holds the cases, the references and the bound; the CPU suite
tests/test_conv_plan.py proves the bound on an emulation of the kernels' arithmetic, that exact references are fp16
numbers, and that the cases reach every kernel and both split-K reducers).

Per run, in this order: rc == 0; the kernel, split-K slices and reduction kernel that ran are the ones the case names;
nothing outside the output was written; every element is finite; the result equals the reference bit for bit (grid,
tap and saturated-gate inputs) or lies within the element-wise bound with rel-L2 < 2e-3 (randn).

Guards: y lives in an int16 buffer pre-filled with an fp16 NaN bit pattern, 256 rows (the tallest tile) in front and
behind, and the other columns of the concatenation buffer when strided, so a whole-tile overrun stays inside memory the
test owns; x and res sit in NaN-filled buffers of the same build, so a read out of range turns up as a non-finite
output."""
import ctypes as C

import pytest
import torch

import conv_cases as cc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GUARD = 256                    # guard rows in front of and behind x, res and y
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
OTHER = 24                     # columns of the other tensor in a concatenation buffer
XOFF = 16                      # column offset of x inside its wider buffer
FLAT_GUARD = 4096              # guard elements around the NCHW output of the small-Cout kernel


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan_buffer(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16, device="cuda")


def _round8(n):
    return (n + 7) // 8 * 8


def _first_mismatch(got, want):
    bad = (got.view(torch.int16) != want.view(torch.int16)).flatten().nonzero()
    i = int(bad[0])
    return "%d of %d elements differ, first at %s: got %r, reference %r" % (
        len(bad), got.numel(), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)),
        got.flatten()[i].item(), want.flatten()[i].item())


def run(lib, c, ins, layout):
    """Launches the case in one operand layout and returns the [N, OH, OW, out_cols] fp16 output on the CPU, after
    checking rc, what ran, and the guards.
      dense   ldx = Cin, ldy = ldres = the output width
      left    x a slice at column 16 of a [rows, Cin + 24] buffer; y and res the left columns of a buffer 24 wider
      right   the same x; y and res behind 24 columns of another tensor"""
    x, w, bias, rowadd, res = ins
    OH, OW = cc.out_size(c)
    M, _ = cc.gemm_dims(c)
    oc = cc.out_cols(c)
    rows_x = c.N * c.H * c.W
    if layout == "dense":
        xw, xo, yw, yo = c.Cin, 0, oc, 0
    else:
        xw, xo, yw = c.Cin + OTHER, XOFF, _round8(oc) + OTHER
        yo = 0 if layout == "left" else OTHER
    xbuf = _nan_buffer(GUARD + rows_x + GUARD, xw)
    xv = xbuf[GUARD:GUARD + rows_x, xo:xo + c.Cin]
    xv.copy_(x.reshape(rows_x, c.Cin))
    rbuf = rv = None
    if res is not None:
        rbuf = _nan_buffer(GUARD + M + GUARD, yw)
        rv = rbuf[GUARD:GUARD + M, yo:yo + oc]
        rv.copy_(res.reshape(M, oc))
    ybuf = torch.full((GUARD + M + GUARD, yw), SENTINEL, dtype=torch.int16, device="cuda")
    yv = ybuf[GUARD:GUARD + M, yo:yo + oc]
    wd = w.cuda().contiguous()
    bd = bias.cuda() if bias is not None else None
    ad = rowadd.cuda().contiguous() if rowadd is not None else None
    x_before = xbuf.view(torch.int16).clone()
    r_before = rbuf.view(torch.int16).clone() if rbuf is not None else None
    ran = (C.c_int * 4)()
    lib.sd_igemm_force(*(c.force or (-1, 0)))
    try:
        rc = lib.sd_op_conv2d_ex(P(xv), P(wd), P(bd), P(ad), P(rv), P(yv), c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride,
                                 c.up, c.geglu, xw, yw, yw, c.pad, c.act, c.acc_scale, c.bias_scale, c.gn_groups, ran,
                                 stream())
    finally:
        lib.sd_igemm_force(-1, 0)
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert (ran[0], ran[2], ran[3]) == c.want, \
        "the plan moved: this case no longer runs the kernel it was written for (ran %r, written for %r)" % (tuple(ran), c.want)
    yb = ybuf.cpu()
    out = yb[GUARD:GUARD + M, yo:yo + oc].clone()
    yb[GUARD:GUARD + M, yo:yo + oc] = SENTINEL
    assert (yb[:GUARD] == SENTINEL).all(), "rows in front of the output were written"
    assert (yb[GUARD + M:] == SENTINEL).all(), "rows behind the output were written"
    assert (yb == SENTINEL).all(), "columns beside the output were written"
    assert torch.equal(xbuf.view(torch.int16), x_before), "the input buffer was written"
    assert rbuf is None or torch.equal(rbuf.view(torch.int16), r_before), "the residual buffer was written"
    return out.view(torch.float16).view(c.N, OH, OW, oc)


def check(c, out, r, bound):
    assert torch.isfinite(out.float()).all(), "%d non-finite elements" % int((~torch.isfinite(out.float())).sum())
    if c.kind != "randn":
        want = r.half()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), _first_mismatch(out, want)
        return
    err = (out.double() - r).abs()
    ratio = (err / bound).max().item()
    rl2 = rel_l2(out, r)
    print("%s <kind %d>: rel_l2 %.2e, worst |err| / bound %.3f" % (cc.case_id(c), c.want[0], rl2, ratio))
    assert rl2 < 2e-3
    worst = (err / bound).argmax()
    assert ratio <= 1.0, (cc.case_id(c), "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())


def _cases(*groups):
    cs = [c for c in cc.CASES if c.group in groups]
    return pytest.mark.parametrize("case", cs, ids=[cc.case_id(c) for c in cs])


@_cases("ring", "edges", "gather", "epilogue", "routes")
def test_conv_against_float64(engine_lib, case):
    """ring: every streamed tile and igemm3 at 1, 2, STAGES - 1, STAGES, STAGES + 1 slabs of K and with a last split-K
    slice shorter than the ring.  edges: M and Cout around one tile, 3x3 on odd images.  gather: the nine taps as a
    pure copy under stride, padding and upsample, streamed and halo tiles, every halo split.  epilogue: the operand
    sets and scales fused, behind both reducers, on halo, wsgemm and igemm3; the activations.  routes: what the planner
    sends to wsgemm, the persistent GEGLU and the old igemm kernel, GEGLU tiles, and a randn case per family."""
    ins = cc.inputs_and_reference(case)
    out = run(engine_lib, case, ins[:5], "dense")
    check(case, out, ins[5], ins[6])


@_cases("strided")
def test_conv_strided_operands(engine_lib, case):
    """The engine's layouts: x a column slice of a wider buffer, y and res the left, then the right columns of a
    concatenation buffer, NaN / sentinels in every other column.  Bit-identical to the dense run, itself checked."""
    ins = cc.inputs_and_reference(case)
    assert case.layouts == ("dense", "left", "right")
    dense = run(engine_lib, case, ins[:5], "dense")
    check(case, dense, ins[5], ins[6])
    for layout in case.layouts[1:]:
        out = run(engine_lib, case, ins[:5], layout)
        assert torch.isfinite(out.float()).all(), layout
        assert torch.equal(dense.view(torch.int16), out.view(torch.int16)), (layout, _first_mismatch(out, dense))


def test_conv_ex_reports_an_unsplit_launch(engine_lib):
    """A wider output stride that is a multiple of 8 runs; `ran` of an unsplit launch ends in (1 slice, no reducer)."""
    x = torch.zeros(4, 64, dtype=torch.float16, device="cuda")
    w = torch.zeros(8, 64, 1, 1, dtype=torch.float16, device="cuda")
    y = torch.ones(4, 16, dtype=torch.float16, device="cuda")
    ran = (C.c_int * 4)()
    rc = engine_lib.sd_op_conv2d_ex(P(x), P(w), None, None, None, P(y), 1, 4, 1, 64, 8, 1, 1, 0, 0, 64, 8, 16, -1, 0, 1.0, 1.0,
                                    0, ran, stream())
    assert rc == 0, engine_lib.sd_last_error()
    assert tuple(ran)[2:] == (1, 0) and ran[0] in cc.TILE
    assert (y[:, :8] == 0).all() and (y[:, 8:] == 1).all()


@pytest.mark.parametrize("sc", cc.SMALL_COUT_CASES, ids=[cc.small_cout_id(s) for s in cc.SMALL_COUT_CASES])
def test_conv3x3_small_cout_exact(engine_lib, sc):
    """sd_op_conv3x3_small_cout (conv_out, NHWC in, NCHW out) with grid and one-hot tap inputs: bit for bit, the NCHW
    output guarded on both sides, x inside NaN rows."""
    c = cc.small_cout_case(sc)
    x, w, bias, _, _, r, _ = cc.inputs_and_reference(c)
    N, H, W, Cin, Cout = c.N, c.H, c.W, c.Cin, c.Cout
    rows = N * H * W
    xbuf = _nan_buffer(GUARD + rows + GUARD, Cin)
    xv = xbuf[GUARD:GUARD + rows]
    xv.copy_(x.reshape(rows, Cin))
    n = N * Cout * H * W
    ybuf = torch.full((FLAT_GUARD + n + FLAT_GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    yv = ybuf[FLAT_GUARD:FLAT_GUARD + n]
    wd, bd = w.cuda().contiguous(), bias.cuda()
    rc = engine_lib.sd_op_conv3x3_small_cout(P(xv), P(wd), P(bd), P(yv), N, H, W, Cin, Cout, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    yb = ybuf.cpu()
    assert (yb[:FLAT_GUARD] == SENTINEL).all(), "elements in front of the output were written"
    assert (yb[FLAT_GUARD + n:] == SENTINEL).all(), "elements behind the output were written"
    out = yb[FLAT_GUARD:FLAT_GUARD + n].clone().view(torch.float16).view(N, Cout, H, W)
    assert torch.isfinite(out.float()).all()
    want = r.permute(0, 3, 1, 2).contiguous().half()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)), _first_mismatch(out, want)
