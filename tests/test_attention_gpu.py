"""Every attn_kernel instantiation launch_attention can pick, through sd_op_attention_ex, against a float64 CPU
reference of the same fp16 operands (tests/attn_cases.py holds the cases, the reference and the bound; the CPU suite
proves the bound on an emulation of the kernel's arithmetic and that the cases cover every instantiation).

Per run: the instantiation sd_attention_plan names is the one the case was written for; rel-L2 < 3e-3; every element
finite and within the element-wise bound; and nothing outside the B * Tq x heads * d output is written.  Every run
puts `out` inside a buffer pre-filled with a bit pattern (64 tail rows, 8 pad columns when strided) and K / V in front
of 64 rows of NaN in the same allocation; the pad columns of strided inputs hold NaN too."""
import ctypes as C

import pytest
import torch

import attn_cases as ac
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TAIL = 64                      # guard rows behind out / K / V
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan_buffer(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16, device="cuda")


def run(lib, case, q, k, v, layout):
    """Launches the case in one operand layout; returns the [B, Tq, C] fp16 output on the CPU after checking that
    everything around it in its buffer is untouched."""
    B, H, Tq, Tk, d = case.B, case.heads, case.Tq, case.Tk, case.d
    Cw = H * d
    q2, k2, v2 = q.reshape(B * Tq, Cw).cuda(), k.reshape(B * Tk, Cw).cuda(), v.reshape(B * Tk, Cw).cuda()
    if layout == "contig":
        qv = q2
        kbuf, vbuf = _nan_buffer(B * Tk + TAIL, Cw), _nan_buffer(B * Tk + TAIL, Cw)
        kv, vv = kbuf[:B * Tk], vbuf[:B * Tk]
        ldo = Cw
    elif layout == "qkv":
        assert Tq == Tk
        buf = _nan_buffer(B * Tk + TAIL, 3 * Cw + 8)
        qv, kv, vv = buf[:B * Tq, 0:Cw], buf[:B * Tk, Cw:2 * Cw], buf[:B * Tk, 2 * Cw:3 * Cw]
        ldo = Cw + 8
    else:
        assert layout == "textkv"
        qbuf = _nan_buffer(B * Tq, Cw + 8)
        buf = _nan_buffer(B * Tk + TAIL, 4 * Cw + 24)
        qv, kv, vv = qbuf[:, :Cw], buf[:B * Tk, 2 * Cw + 8:3 * Cw + 8], buf[:B * Tk, 3 * Cw + 8:4 * Cw + 8]
        ldo = Cw + 8
    if qv is not q2:
        qv.copy_(q2)
    kv.copy_(k2)
    vv.copy_(v2)
    obuf = torch.full((B * Tq + TAIL, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    got = (C.c_int * 5)()
    assert lib.sd_attention_plan(B, Tq, Tk, H, d, case.causal, case.presc, got) == 0, lib.sd_last_error()
    assert tuple(got) == case.inst, "the dispatch moved: this case no longer runs the kernel it was written for"
    rc = lib.sd_op_attention_ex(P(qv), P(kv), P(vv), P(obuf), B, Tq, Tk, H, d, qv.stride(0), kv.stride(0), vv.stride(0),
                                ldo, case.causal, case.presc, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    ob = obuf.cpu()
    assert (ob[B * Tq:] == SENTINEL).all(), "rows behind the output were written"
    assert (ob[:, Cw:] == SENTINEL).all(), "pad columns of the output were written"
    return ob[:B * Tq, :Cw].contiguous().view(torch.float16).view(B, Tq, Cw)


def check(case, out, O, A, v):
    o = out.double()
    assert torch.isfinite(o).all()
    err = (o - O).abs()
    bound = ac.elementwise_bound(O, A, case.Tk, v.abs().max().double())
    ratio = (err / bound).max().item()
    r = rel_l2(out, O)
    print("%s: rel_l2 %.2e, worst |err| / bound %.3f" % (ac.case_id(case), r, ratio))
    assert r < 3e-3
    worst = (err - bound).argmax()
    assert ratio <= 1.0, (ac.case_id(case), "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())


def _cases(*groups):
    cs = [c for c in ac.GPU_CASES if c.group in groups]
    return pytest.mark.parametrize("case", cs, ids=[ac.case_id(c) for c in cs])


@_cases("threshold", "edge", "extreme")
def test_attention_against_float64(engine_lib, case):
    """The instantiations at their thresholds and one step below, Tq / Tk at block and tile edges for every
    instantiation, and a late score spike / scores far below zero on the eight-wave and long-block kernels."""
    q, k, v, O, A = ac.inputs_and_reference(case)
    out = run(engine_lib, case, q, k, v, "contig")
    check(case, out, O, A, v)
    if case.Tk == 1:                                   # one key: the output is that key's V row, bit for bit
        assert torch.equal(out, v.expand(case.B, case.Tq, -1))


@_cases("strided", "causal")
def test_attention_strided_operands(engine_lib, case):
    """The engine's operand layouts: q / k / v as column slices of one wide buffer (UNet, VAE and CLIP self-attention)
    or K / V inside the wide text-KV row, NaN in every pad column and behind the last K / V row.  Bit-identical to
    the dense layout, and both within the bounds."""
    q, k, v, O, A = ac.inputs_and_reference(case)
    assert case.layouts[0] == "contig" and len(case.layouts) == 2
    dense = run(engine_lib, case, q, k, v, "contig")
    check(case, dense, O, A, v)
    strided = run(engine_lib, case, q, k, v, case.layouts[1])
    assert torch.isfinite(strided.float()).all()
    assert torch.equal(dense.view(torch.int16), strided.view(torch.int16))


@_cases("constv")
def test_attention_constant_v(engine_lib, case):
    """Every V row equal to c (1.0, or a row of mixed signs and magnitudes) under random scores: softmax weights sum
    to one, so out = c up to the truncation of the probabilities (2^-10, where the denominator is summed from the
    un-truncated values; it cancels where it rides on the PV product) and one fp16 step of c.  Prints the signed mean
    of (out - c) / |c| per instantiation (DESIGN.md records them)."""
    q, k, v, O, A = ac.inputs_and_reference(case)
    out = run(engine_lib, case, q, k, v, "contig")
    check(case, out, O, A, v)
    c = v[0, 0].double()
    step = torch.maximum(2.0 ** (torch.floor(torch.log2(c.abs().clamp_min(2.0 ** -14))) - 10),
                         torch.tensor(2.0 ** -24, dtype=torch.float64))       # fp16 spacing at c
    dev = out.double() - c
    rel = (dev / c.abs())[..., c != 0]
    print("constant V %s <%s>: signed mean of (out - c) / |c| = %+.3e, min %+.3e, max %+.3e"
          % (case.kind, ",".join(map(str, case.inst)), rel.mean().item(), rel.min().item(), rel.max().item()))
    assert (dev.abs() <= 2.0 ** -10 * c.abs() + step).all(), (dev.abs() - 2.0 ** -10 * c.abs() - step).max().item()
    if case.d not in ac.EXACT_DENOMINATOR and case.kind == "const1":
        assert torch.equal(out, v[:, :1].expand_as(out))       # the truncation cancels exactly
