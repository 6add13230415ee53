"""conv_head_kernel, conv_tail_kernel and the two time-embedding linear kernels through their operator entries
(sd_op_unet_conv_in, sd_op_unet_conv_out_ex, sd_op_small_linear) on the cases of tests/edge_cases.py: rc == 0; exact
cases bit for bit, the others inside the element bound derived from the float64 reference alone (no element excused);
16-element guards around every output and around the summaries untouched, the inputs unchanged, the spare columns of a
wide row stride still NaN; the refused shapes launch nothing.  Prints the worst |err| / bound and the share of the fp32
terms used per group of cases."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_cases as ec  # noqa: E402
import norm_cases as nc  # noqa: E402
from test_edge_plan import refusals  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = ec.GUARD
NAN = float("nan")
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    """The worst figures of every group of cases, printed once behind the module's last test."""
    yield
    for group, w in sorted(_worst.items()):
        print("\n[edge] %-20s worst %s" % (group, ", ".join("%.3f" % v if isinstance(v, float) else "%d cases" % v for v in w)), end="")
    print()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def note(group, ratio, used=0.0):
    w = _worst.setdefault(group, [0.0, 0.0, 0])
    w[0], w[1], w[2] = max(w[0], ratio), max(w[1], used), w[2] + 1
    return "(%s, %d cases so far: worst |err| / bound %.3f, fp32 terms used %.3f)" % (group, w[2], w[0], w[1])


def guarded(n, dtype, fill):
    """A device buffer of n elements between two guards of GUARD elements: (whole, inside)."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def unchanged(dev, host):
    return same_bits(dev.cpu(), host.contiguous())


# ------------------------------------------------------------------------------------------------------------ conv_in
def run_head(lib, c, x, w, bias):
    """-> (y [N, H, W, 320] fp16, summaries [N, S, G, 2] fp32 | None), on the CPU."""
    M, S = c.N * c.H * c.W, c.H * c.W // 128
    ybuf, y = guarded(M * ec.COUT_IN, torch.float16, NAN)
    n_s = c.N * S * max(c.G, 1) * 2
    sbuf, summ = guarded(n_s, torch.float32, 13.0)
    xd, wd, bd = x.cuda().contiguous(), w.cuda().contiguous(), bias.cuda().contiguous()
    rc = lib.sd_op_unet_conv_in(P(xd), P(wd), P(bd), P(y), P(summ), c.G, c.N, c.Cin, c.H, c.W, ec.COUT_IN, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert guards_intact(ybuf, NAN) and guards_intact(sbuf, 13.0)
    assert unchanged(xd, x) and unchanged(wd, w) and unchanged(bd, bias)
    if not c.G:
        assert (sbuf == 13.0).all()                      # groups = 0: the pointer is not touched
    return y.cpu().reshape(c.N, c.H, c.W, ec.COUT_IN), (summ.cpu().reshape(c.N, S, c.G, 2) if c.G else None)


def check_head_summaries(c, y, summ):
    if not c.G:
        return
    assert torch.isfinite(summ).all()
    dm, dq = ec.head_summary_errors(c, summ, ec.head_summary_reference(c, y))
    w = _worst.setdefault("conv_in summaries", [0.0, 0.0])
    w[0], w[1] = max(w[0], dm), max(w[1], dq)
    print("%s: summaries: worst mean error %.3f, worst M2 error %.3f of SLAB x the terms (so far %.3f, %.3f)"
          % (ec.head_id(c), dm, dq, w[0], w[1]))
    assert dm <= 1.0 and dq <= 1.0, (ec.head_id(c), dm, dq)


@pytest.mark.parametrize("case", ec.HEAD_CASES, ids=[ec.head_id(c) for c in ec.HEAD_CASES])
def test_conv_in(engine_lib, case):
    x, w, bias, r, bound = ec.head_inputs_and_reference(case)
    got, summ = run_head(engine_lib, case, x, w, bias)
    if case.kind == "randn":
        assert torch.isfinite(got.float()).all()
        ratio, used = nc.error_ratios(got, r, bound)
        print("%s: worst |err| / bound %.3f, fp32 terms used %.3f %s" % (ec.head_id(case), ratio, used, note("conv_in", ratio, used)))
        assert ratio <= 1.0, (ec.head_id(case), ratio)
    else:
        want = ec.head_tap_gather(case, x) if case.kind == "tap" else r.half()
        diff = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        print("%s: %d of %d elements differ in bits" % (ec.head_id(case), diff, got.numel()))
        assert diff == 0, (ec.head_id(case), diff)
    check_head_summaries(case, got, summ)


# ----------------------------------------------------------------------------------------------------------- conv_out
def run_tail(lib, c, x, gamma, beta, w, bias):
    """-> y [N, Cout, H, W] fp16 on the CPU."""
    HW = c.H * c.W
    ldx = 328 if c.layout == "ld328" else ec.C_OUT
    xw = torch.full((c.N * HW, ldx), NAN, dtype=torch.float16)
    xw[:, :ec.C_OUT] = x.reshape(c.N * HW, ec.C_OUT)
    xd, gd, btd, wd, bd = xw.cuda(), gamma.cuda(), beta.cuda(), w.cuda().contiguous(), bias.cuda()
    ybuf, y = guarded(c.N * c.Cout * HW, torch.float16, NAN)
    sbuf = summ = part = None
    if c.S:
        part = ec.tail_supplied(c, x)
        sbuf, summ = guarded(part.numel(), torch.float32, 13.0)
        summ.copy_(part.reshape(-1))
    rc = lib.sd_op_unet_conv_out_ex(P(xd), ldx, P(gd), P(btd), c.G, 1e-5, c.silu, P(wd), P(bd), P(y), c.N, c.H, c.W, ec.C_OUT,
                                    c.Cout, P(summ) if c.S else None, c.S, c.rows, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert guards_intact(ybuf, NAN)
    back = xd.cpu()
    assert same_bits(back[:, :ec.C_OUT].contiguous(), xw[:, :ec.C_OUT].contiguous()) and torch.isnan(back[:, ec.C_OUT:]).all()
    assert unchanged(gd, gamma) and unchanged(btd, beta) and unchanged(wd, w) and unchanged(bd, bias)
    if c.S:
        assert guards_intact(sbuf, 13.0) and unchanged(summ, part.reshape(-1))
    return y.cpu().reshape(c.N, c.Cout, c.H, c.W)


@pytest.mark.parametrize("case", ec.TAIL_CASES, ids=[ec.tail_id(c) for c in ec.TAIL_CASES])
def test_conv_out(engine_lib, case):
    x, gamma, beta, w, bias, r, bound, outside = ec.tail_inputs_and_reference(case)
    got = run_tail(engine_lib, case, x, gamma, beta, w, bias)
    assert torch.isfinite(got.float()).all()
    ratio = ec.worst_ratio(got, r, bound)
    if case.kind == "tap":
        nz = int((got[outside].view(torch.int16) != 0).sum())
        print("%s: worst |err| / bound %.3f, %d of %d out-of-image taps not zero bits %s"
              % (ec.tail_id(case), ratio, nz, int(outside.sum()), note("conv_out tap", ratio)))
        assert nz == 0, (ec.tail_id(case), nz)
    else:
        used = nc.error_ratios(got, r, bound)[1]
        print("%s: worst |err| / bound %.3f, fp32 terms used %.3f %s" % (ec.tail_id(case), ratio, used, note("conv_out", ratio, used)))
    assert ratio <= 1.0, (ec.tail_id(case), ratio)


def test_conv_out_is_the_ex_entry_without_summaries(engine_lib):
    """sd_op_unet_conv_out became a call of sd_op_unet_conv_out_ex (ldx = C, own statistics pass): the same bits."""
    case = next(c for c in ec.TAIL_CASES if c.kind == "randn" and c.layout == "dense" and not c.S)
    x, gamma, beta, w, bias, r, bound, _ = ec.tail_inputs_and_reference(case)
    want = run_tail(engine_lib, case, x, gamma, beta, w, bias)
    xd, gd, btd, wd, bd = x.cuda().contiguous(), gamma.cuda(), beta.cuda(), w.cuda().contiguous(), bias.cuda()
    ybuf, y = guarded(want.numel(), torch.float16, NAN)
    rc = engine_lib.sd_op_unet_conv_out(P(xd), P(gd), P(btd), case.G, 1e-5, case.silu, P(wd), P(bd), P(y), case.N, case.H, case.W,
                                        ec.C_OUT, case.Cout, 0, None, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert guards_intact(ybuf, NAN) and same_bits(y.cpu().reshape(want.shape), want)


# ------------------------------------------------------------------------------------------------------- small_linear
def run_linear(lib, c, x, w, bias):
    xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
    bd = bias.cuda() if bias is not None else None
    ybuf, y = guarded(c.B * c.n_out, torch.float32, 13.0)
    rc = lib.sd_op_small_linear(P(xd), P(wd), P(bd) if bd is not None else None, P(y), c.B, c.K, c.n_out, c.silu_in, c.silu_out,
                                stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert guards_intact(ybuf, 13.0)
    assert unchanged(xd, x) and unchanged(wd, w) and (bd is None or unchanged(bd, bias))
    return y.cpu().reshape(c.B, c.n_out)


@pytest.mark.parametrize("case", ec.LIN_CASES, ids=[ec.lin_id(c) for c in ec.LIN_CASES])
def test_small_linear(engine_lib, case):
    assert engine_lib.sd_small_linear_plan(case.B, case.K, case.n_out) == case.want      # the kernel the case was written for
    x, w, bias, r, bound = ec.lin_inputs_and_reference(case)
    got = run_linear(engine_lib, case, x, w, bias)
    group = ("skinny" if case.want else "gemv") + " " + case.kind
    if case.kind == "randn":
        assert torch.isfinite(got).all()
        ratio = ec.worst_ratio(got, r, bound)
        print("%s: worst |err| / bound %.3f %s" % (ec.lin_id(case), ratio, note(group, ratio)))
        assert ratio <= 1.0, (ec.lin_id(case), ratio)
    else:
        diff = int((got.view(torch.int32) != r.float().view(torch.int32)).sum())
        print("%s: %d of %d elements differ in bits %s" % (ec.lin_id(case), diff, got.numel(), note(group, float(diff))))
        assert diff == 0, (ec.lin_id(case), diff)
        if case.kind == "split":                        # and not what fp16(x) alone gives: lo is carried
            assert not same_bits(got, ec.lin_reference(case, x.half().float(), w, bias)[0].float())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_other_shapes_are_refused_and_nothing_is_launched(engine_lib):
    buf = torch.zeros(4096, dtype=torch.float16, device="cuda")
    ybuf, y = guarded(4096, torch.float16, NAN)
    for label, call in refusals(engine_lib, P(buf), P(y), stream()):
        assert call() == 1, label
        assert b"sd_op_unet_conv" in engine_lib.sd_last_error(), label
    torch.cuda.synchronize()
    assert torch.isnan(ybuf).all() and not buf.any()
    assert engine_lib.sd_op_small_linear(P(buf), P(buf), None, P(y), 4, 12, 16, 0, 0, stream()) != 0      # K % 8
    torch.cuda.synchronize()
    assert torch.isnan(ybuf).all()
