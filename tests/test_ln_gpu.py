"""The folded-LayerNorm chain element by element: every consumer of row statistics (the igemm2 streamed tiles plain and
GEGLU, igemm3, wsgemm 13 / 14, geglu_persist_kernel, ffn_fused_kernel) on statistics the host computed in float64 and
laid out in layouts no producer emits today, every producer (igemm2 tile epilogue, wsgemm, igemm3, row_stats_kernel)
against float64 statistics of the fp16 y1 it stored, and one chain per producer family into a consumer of another.
tests/ln_cases.py holds the cases, operands, references and the bound; tests/test_ln_plan.py proves the bound on an
emulation of the kernels' arithmetic and that it sees the defects it is for.

Per consumer run, in this order: rc == 0; the kernel named ran; nothing outside the output was written; the input and the
statistics are unchanged; every element is finite; |got - ref| <= bound element by element; rel-L2 < 3e-3; a second run on
fresh buffers is bit-identical.

Guards: y lives in an int16 buffer pre-filled with an fp16 NaN bit pattern, 256 rows in front and behind; x and the
statistics sit between 256 NaN rows each, so a row read out of range turns up as a non-finite output."""
import ctypes as C

import pytest
import torch

import conv_cases as cc
import ln_cases as lc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = 0x7E5A               # an fp16 NaN pattern, compared as int16
STAT_SENTINEL = -123456.0
STAT_GUARD = 4096               # floats behind the producer's statistics


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(t, dtype=None):
    """t [M, n] inside a NaN buffer with GUARD rows in front and behind: (buffer, view)."""
    M, n = t.shape
    buf = torch.full((GUARD + M + GUARD, n), float("nan"), dtype=dtype or t.dtype, device="cuda")
    view = buf[GUARD:GUARD + M]
    view.copy_(t)
    return buf, view


def _bits(buf):
    return buf.view(torch.int16 if buf.dtype == torch.float16 else torch.int32)


def _take_output(ybuf, M):
    """The [M, n] fp16 output out of its sentinel buffer, after checking that nothing around it was written."""
    assert (ybuf[:GUARD] == SENTINEL).all(), "rows in front of the output were written"
    assert (ybuf[GUARD + M:] == SENTINEL).all(), "rows behind the output were written"
    return ybuf[GUARD:GUARD + M].clone().view(torch.float16)


def run_consumer(lib, c, ops, x, stat, lay):
    """One launch of a consumer case on x [M, C] fp16 and stat [M, parts, 2] fp32 (CPU or device tensors): the [M, n]
    fp16 output on the device, after rc, the kernel id, the guards and the unchanged inputs."""
    parts, w = lay
    M = c.M
    xbuf, xv = _guarded(x)
    sbuf, sv = _guarded(stat.reshape(M, parts * 2))
    n = c.C if c.entry == "ffn" else c.O
    ybuf = torch.full((GUARD + M + GUARD, n), SENTINEL, dtype=torch.int16, device="cuda")
    yv = ybuf[GUARD:GUARD + M]
    dev = [t.cuda().contiguous() if t is not None else None for t in (ops.gamma, ops.beta, ops.w1, ops.b1, ops.w2, ops.b2)]
    gamma, beta, w1, b1, w2, b2 = dev
    x_before, s_before = _bits(xbuf).clone(), _bits(sbuf).clone()
    ran = C.c_int(-9)
    lib.sd_igemm_force(*(c.force or (-1, 0)))
    try:
        if c.entry == "ffn":
            rc = lib.sd_op_ln_ffn_geglu(P(xv), P(sv), parts, w, P(gamma), P(beta), lc.EPS, P(w1), P(b1), P(w2), P(b2), P(yv),
                                        M, c.C, C.byref(ran), stream())
        else:
            rc = lib.sd_op_ln_linear(P(xv), P(sv), parts, w, P(gamma), P(beta), lc.EPS, P(w1), P(b1), P(yv), M, c.C, c.O,
                                     c.geglu, ops.rows_scaled, ops.row_scale, C.byref(ran), stream())
    finally:
        lib.sd_igemm_force(-1, 0)
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    if c.want is not None:
        assert ran.value == c.want, \
            "the plan moved: this case no longer runs the kernel it was written for (ran %d, written for %d)" % (ran.value, c.want)
    else:
        assert ran.value not in c.avoid and ran.value in cc.TILE, "a layout beyond the kernel's capacity ran on %d" % ran.value
    out = _take_output(ybuf, M)
    assert torch.equal(_bits(xbuf), x_before), "the input buffer was written"
    assert torch.equal(_bits(sbuf), s_before), "the statistics buffer was written"
    return out, ran.value


def check(name, kind, out, r, bound):
    """Finite, inside the bound element by element, rel-L2 under the family's threshold; prints the figures first."""
    out = out.to(r.device)
    finite = torch.isfinite(out.float())
    assert finite.all(), "%s: %d non-finite elements" % (name, int((~finite).sum()))
    ratio = (out.double() - r).abs() / bound
    worst = int(ratio.argmax())
    rl2 = (torch.linalg.vector_norm(out.double() - r) / torch.linalg.vector_norm(r)).item()
    print("%s <kind %d>: rel_l2 %.2e, worst |err| / bound %.3f" % (name, kind, rl2, ratio.flatten()[worst].item()))
    assert ratio.flatten()[worst].item() <= 1.0, (name, "element", tuple(int(v) for v in divmod(worst, out.shape[1])),
                                                  out.flatten()[worst].item(), r.flatten()[worst].item(),
                                                  bound.flatten()[worst].item())
    assert rl2 < 3e-3, (name, rl2)


_RUNS = [(c, lay, prof) for c in lc.CONSUMERS for lay, prof in c.runs]


@pytest.mark.parametrize("case,lay,prof", _RUNS, ids=[lc.run_id(*r) for r in _RUNS])
def test_consumer_against_float64(engine_lib, case, lay, prof):
    """Host-computed statistics in the given layout into the kernel the case names.  The float64 reference of the two
    feed-forward cases (M >= 8192) is evaluated on the device (test_device_evaluation_of_the_reference_equals_the_cpu's)."""
    ops = lc.consumer_operands(case, prof)
    stat = lc.supplied_stats(ops.x, lay)
    out, kind = run_consumer(engine_lib, case, ops, ops.x, stat, lay)
    name = lc.run_id(case, lay, prof)
    if case.entry == "ffn":
        y, branch, bound = lc.consumer_reference(case, prof, lay, device="cuda")
        check(name, kind, out, y, bound)
        got_branch = out.double() - ops.x.cuda().double()
        err = (torch.linalg.vector_norm(got_branch - branch) / torch.linalg.vector_norm(branch)).item()
        print("  branch rel-L2 %.2e" % err)
        assert err < 3e-3, (name, err)
    else:
        r, bound = lc.consumer_reference(case, prof, lay)
        check(name, kind, out.cpu(), r, bound)
    again, kind2 = run_consumer(engine_lib, case, ops, ops.x, stat, lay)
    assert kind2 == kind and torch.equal(out.view(torch.int16), again.view(torch.int16)), "a second run differs"


def test_device_evaluation_of_the_reference_equals_the_cpu(engine_lib):
    """The feed-forward reference on the device in float64 against its CPU evaluation, on the first and last 64 rows."""
    case = next(c for c in lc.CONSUMERS if c.entry == "ffn")
    lay, prof = case.runs[-1]
    ops = lc.consumer_operands(case, prof)
    rows = torch.cat((torch.arange(64), torch.arange(case.M - 64, case.M)))
    dev = lc.reference_ffn(ops.x.cuda(), ops, lay)
    cpu = lc.reference_ffn(ops.x[rows], ops, lay)
    for a, b in zip(dev, cpu):
        torch.testing.assert_close(a[rows.cuda()].cpu(), b, rtol=1e-10, atol=1e-12)


def run_producer(lib, p, profile):
    """sd_op_linear_rowstats in guarded buffers: (y1 [M, C] fp16, stat [M, parts, 2] fp32) on the device, after rc, the
    kernel and layout reported, the guards (statistics slots past M * parts included) and the unchanged inputs."""
    x, w0, b0, res = lc.producer_operands(p, profile)
    xbuf, xv = _guarded(x)
    rbuf = rv = None
    if res is not None:
        rbuf, rv = _guarded(res)
    ybuf = torch.full((GUARD + p.M + GUARD, p.C), SENTINEL, dtype=torch.int16, device="cuda")
    yv = ybuf[GUARD:GUARD + p.M]
    nstat = p.M * ((p.C + 63) // 64) * 2                # what the entry asks for
    sbuf = torch.full((nstat + STAT_GUARD,), STAT_SENTINEL, dtype=torch.float32, device="cuda")
    w0d, b0d = w0.cuda().contiguous(), b0.cuda()
    x_before = _bits(xbuf).clone()
    r_before = _bits(rbuf).clone() if rbuf is not None else None
    parts, part_w, prod = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    lib.sd_igemm_force(*p.force)
    try:
        rc = lib.sd_op_linear_rowstats(P(xv), P(w0d), P(b0d), P(rv), P(yv), P(sbuf), p.M, p.K, p.C, C.byref(parts),
                                       C.byref(part_w), C.byref(prod), stream())
    finally:
        lib.sd_igemm_force(-1, 0)
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert (prod.value, parts.value, part_w.value) == (p.want, p.parts, p.part_w), \
        "the plan moved: ran %r, written for %r" % ((prod.value, parts.value, part_w.value), (p.want, p.parts, p.part_w))
    y1 = _take_output(ybuf, p.M)
    assert torch.equal(_bits(xbuf), x_before), "the input buffer was written"
    assert rbuf is None or torch.equal(_bits(rbuf), r_before), "the residual buffer was written"
    used = p.M * p.parts * 2
    assert (sbuf[used:] == STAT_SENTINEL).all(), "statistics slots beyond M * parts were written"
    return y1, sbuf[:used].clone().view(p.M, p.parts, 2)


_PRODS = [(p, prof) for p in lc.PRODUCERS for prof in lc.PRODUCER_PROFILES]


@pytest.mark.parametrize("prod,prof", _PRODS, ids=["%s-%s" % (lc.producer_id(p), prof) for p, prof in _PRODS])
def test_producer_statistics_against_float64(engine_lib, prod, prof):
    """y1 within the conv suite's bound; every stored (mean, M2) part against float64 statistics of the stored fp16 y1 over
    exactly its columns, at the tolerances asserted for epilogue summaries elsewhere (mean atol 2e-5 rtol 1e-4, M2 atol
    1e-3 rtol 1e-4); M2 is never negative, and exactly 0 on the constant rows of offset:50."""
    y1, stat = run_producer(engine_lib, prod, prof)
    y1, stat = y1.cpu(), stat.cpu()
    r, bound = lc.producer_reference(prod, prof)
    assert torch.isfinite(y1.float()).all() and torch.isfinite(stat).all()
    ratio = ((y1.double() - r).abs() / bound).max().item()
    mk, qk = lc.part_stats(y1, (prod.parts, prod.part_w))
    dm = (stat[:, :, 0].double() - mk).abs()
    dq = (stat[:, :, 1].double() - qk).abs()
    print("%s-%s <producer %d>: y1 worst |err| / bound %.3f, mean worst |err| %.2e (of %.1f), M2 worst |err| %.2e (of %.1f)"
          % (lc.producer_id(prod), prof, prod.want, ratio, dm.max().item(), mk.abs().max().item(), dq.max().item(),
             qk.max().item()))
    assert ratio <= 1.0 and rel_l2(y1, r) < 2e-3
    assert (dm <= 2e-5 + 1e-4 * mk.abs()).all(), ("mean", dm.max().item())
    assert (dq <= 1e-3 + 1e-4 * qk.abs()).all(), ("M2", dq.max().item())
    assert (stat[:, :, 1] >= 0).all(), "a negative M2"
    if prof == "offset:50":
        for m in (0, prod.M - 1):
            assert (y1[m] == 50.0).all()
            assert (stat[m, :, 0] == 50.0).all() and (stat[m, :, 1] == 0.0).all(), (m, stat[m])


@pytest.mark.parametrize("chain", lc.CHAINS, ids=[ch.name for ch in lc.CHAINS])
def test_producer_statistics_into_a_consumer_of_another_family(engine_lib, chain):
    """The producer's own statistics into a consumer of another kernel family, element by element against the LayerNorm of
    the stored y1.  The bound's statistics terms are widened by what a one-pass fp32 summary of n_k values may be off by
    (ln_cases.stat_errors, produced=True); everything else is the consumer bound."""
    y1, stat = run_producer(engine_lib, chain.prod, "rows")
    case = lc.chain_consumer(chain)
    ops = lc.chain_operands(chain)
    lay = (chain.prod.parts, chain.prod.part_w)
    out, kind = run_consumer(engine_lib, case, ops, y1, stat, lay)
    r, bound = lc.reference_linear(y1.cpu(), ops, lay, case.geglu, produced=True)
    check("chain-" + chain.name, kind, out.cpu(), r, bound)
    again, _ = run_consumer(engine_lib, case, ops, y1, stat, lay)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "a second run differs"


@pytest.mark.parametrize("Cc,parts,w", lc.OVER_CAPACITY, ids=["c%d-%dx%d" % t for t in lc.OVER_CAPACITY])
def test_layouts_beyond_capacity_leave_the_output_untouched(engine_lib, Cc, parts, w):
    """More parts than a consumer holds per row: both entries return an error with nothing written to the output (all the
    operands are real buffers, so a launch that went ahead would show)."""
    M = 256
    g = torch.Generator().manual_seed(parts)
    x = lc.make_x(M, Cc, "rows", g)
    _, xv = _guarded(x)
    _, sv = _guarded(lc.supplied_stats(x, (parts, w)).reshape(M, parts * 2))
    gamma, beta = torch.ones(Cc, device="cuda"), torch.full((Cc,), 0.1, device="cuda")
    w1 = (torch.randn(8 * Cc, Cc, generator=g) / Cc ** 0.5).half().cuda()
    b1 = torch.zeros(8 * Cc, device="cuda")
    w2 = (torch.randn(Cc, 4 * Cc, generator=g) / Cc ** 0.5).half().cuda()
    b2 = torch.zeros(Cc, device="cuda")
    got = C.c_int(-7)
    for geglu in (0, 1):
        ybuf = torch.full((GUARD + M + GUARD, 128), SENTINEL, dtype=torch.int16, device="cuda")
        rc = engine_lib.sd_op_ln_linear(P(xv), P(sv), parts, w, P(gamma), P(beta), lc.EPS, P(w1), P(b1), P(ybuf[GUARD:]), M, Cc,
                                        128, geglu, 0, 1.0, C.byref(got), stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"ln_parts" in engine_lib.sd_last_error(), rc
        assert (ybuf == SENTINEL).all(), "the output was written"
    ybuf = torch.full((GUARD + M + GUARD, Cc), SENTINEL, dtype=torch.int16, device="cuda")
    rc = engine_lib.sd_op_ln_ffn_geglu(P(xv), P(sv), parts, w, P(gamma), P(beta), lc.EPS, P(w1), P(b1), P(w2), P(b2),
                                       P(ybuf[GUARD:]), M, Cc, C.byref(got), stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"ln_parts" in engine_lib.sd_last_error(), rc
    assert (ybuf == SENTINEL).all(), "the output was written"
    assert got.value == -7
