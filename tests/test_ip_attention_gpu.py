"""ip_xattn_kernel through sd_op_ip_cross_attention, element by element against a float64 CPU reference of the same fp16
operands (tests/ip_cases.py holds the cases, the reference and the bound; tests/test_ip_attention_plan.py proves the
bound on an emulation of the kernel's arithmetic and that one-defect mutants of it break the bound on these cases).

Per run: the form sd_ip_attention_plan reports is the one the case was written for (one tile per block, or the walk in
uneven rounds); rel-L2 < 3e-3; every element finite and within the element-wise bound; nothing outside the
B * Tq x heads * d output is written.  The strided layout gives every operand its own row stride, with NaN in the pad
columns and in 64 rows behind the last K / V row, and puts `out` inside a wider buffer pre-filled with a bit pattern:
guard rows above and below, guard columns to the right."""
import ctypes as C

import pytest
import torch

import ip_cases as ic
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TAIL = 64                      # guard rows behind out / K / V
HEAD = 3                       # guard rows in front of out
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
PADS = {"q": 8, "k": 16, "v": 24, "kip": 32, "vip": 40, "out": 24}        # pad columns of the strided layout


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _operand(t, pad, tail):
    """A [rows, Cw] device view of the CPU tensor `t` inside a NaN buffer with `pad` more columns and `tail` more rows."""
    rows, Cw = t.shape
    buf = torch.full((rows + tail, Cw + pad), float("nan"), dtype=torch.float16, device="cuda")
    view = buf[:rows, :Cw]
    view.copy_(t)
    return view


def launch(lib, q, k, v, kip, vip, B, Tq, L, Tip, H, d, lam, presc, layout="strided", col0=0, heads_run=None):
    """One launch on CPU operands q [B, Tq, C], k / v [B, L, C], k_ip / v_ip [B, T_ip, C]; returns (code, the int16 bits
    of the [B, Tq, Cr] output on the CPU) after checking that everything around the output in its buffer is untouched.
    "dense": every operand its own dense matrix, guard rows around out; "strided": see the module docstring.
    col0 / heads_run: run only heads_run heads starting at column col0 of every operand (same buffers and strides)."""
    Cw = H * d
    strided = layout == "strided"
    pad = PADS if strided else dict.fromkeys(PADS, 0)
    qv = _operand(q.reshape(B * Tq, Cw), pad["q"], 0)
    kv, vv = _operand(k.reshape(B * L, Cw), pad["k"], TAIL), _operand(v.reshape(B * L, Cw), pad["v"], TAIL)
    kiv, viv = _operand(kip.reshape(B * Tip, Cw), pad["kip"], TAIL), _operand(vip.reshape(B * Tip, Cw), pad["vip"], TAIL)
    Hr = heads_run or H
    Cr = Hr * d
    ldo = Cr + pad["out"]
    obuf = torch.full((HEAD + B * Tq + TAIL, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    code = lib.sd_op_ip_cross_attention(P(qv[:, col0:]), P(kv[:, col0:]), P(vv[:, col0:]), P(kiv[:, col0:]),
                                        P(viv[:, col0:]), P(obuf[HEAD:]), B, Tq, L, Tip, Hr, d, qv.stride(0),
                                        kv.stride(0), vv.stride(0), kiv.stride(0), viv.stride(0), ldo, lam, presc, 0, None,
                                        stream())
    torch.cuda.synchronize()
    ob = obuf.cpu()
    assert (ob[:HEAD] == SENTINEL).all(), "rows in front of the output were written"
    assert (ob[HEAD + B * Tq:] == SENTINEL).all(), "rows behind the output were written"
    assert (ob[:, Cr:] == SENTINEL).all(), "guard columns of the output were written"
    return code, ob[HEAD:HEAD + B * Tq, :Cr].contiguous()


def run(lib, case, q, k, v, kip, vip, layout="strided"):
    got = (C.c_int * 4)()
    assert lib.sd_ip_attention_plan(case.B, case.Tq, case.L, case.Tip, case.heads, case.d, case.lam, got) == 0
    walks = got[2] < got[1]
    assert walks == (case.form == "walk"), "the plan moved: this case no longer runs the form it was written for"
    assert not walks or (got[1] % got[2] != 0 and case.Tq % got[0] != 0), "the walk's rounds are no longer uneven"
    code, ob = launch(lib, q, k, v, kip, vip, case.B, case.Tq, case.L, case.Tip, case.heads, case.d, case.lam, case.presc,
                      layout)
    assert code == 0, lib.sd_last_error()
    return ob.view(torch.float16).view(case.B, case.Tq, case.heads * case.d)


def check(case, out, O, bound, what=""):
    o = out.double()
    assert torch.isfinite(o).all()
    err = (o - O).abs()
    ratio = (err / bound).max().item()
    r = rel_l2(out, O)
    print("%s%s: rel_l2 %.2e, worst |err| / bound %.3f" % (ic.case_id(case), what, r, ratio))
    assert r < 3e-3
    worst = (err - bound).argmax()
    assert ratio <= 1.0, (ic.case_id(case), "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())


def _cases(pred):
    cs = [c for c in ic.GPU_CASES if pred(c)]
    return pytest.mark.parametrize("case", cs, ids=[ic.case_id(c) for c in cs])


@_cases(lambda c: True)
def test_ip_attention_against_float64(engine_lib, case):
    """Every head dim in every group: Tq, L and T_ip at the edges of the 16- and 64-row tiles and of the 32-key step, the
    walk over query tiles in uneven rounds, every lambda, scores of std 60 and of about -150 in either segment,
    pre-scaled queries, constant V; all in the strided layout with guards."""
    q, k, v, kip, vip, O, A = ic.inputs_and_reference(case)
    check(case, run(engine_lib, case, q, k, v, kip, vip), O, ic.bound_of(case, v, vip, O, A))


@_cases(lambda c: c.group in ("lambda", "walk") or (c.group == "edge" and c.Tq in (17, 129)))
def test_dense_and_strided_runs_are_bit_identical(engine_lib, case):
    q, k, v, kip, vip = ic.make_inputs(case)
    dense = run(engine_lib, case, q, k, v, kip, vip, "dense")
    wide = run(engine_lib, case, q, k, v, kip, vip, "strided")
    assert torch.isfinite(wide.float()).all()
    assert torch.equal(dense.view(torch.int16), wide.view(torch.int16))


@_cases(lambda c: c.lam == 0.0)
def test_zero_lambda_never_reads_the_image_operands(engine_lib, case):
    """lambda = 0 with k_ip all +inf and v_ip all NaN: finite, inside the bound, and bit-equal to the run on finite image
    operands."""
    q, k, v, kip, vip, O, A = ic.inputs_and_reference(case)
    poisoned = run(engine_lib, case, q, k, v, torch.full_like(kip, float("inf")), torch.full_like(vip, float("nan")))
    check(case, poisoned, O, ic.bound_of(case, v, vip, O, A), " (non-finite image operands)")
    finite = run(engine_lib, case, q, k, v, kip, vip)
    assert torch.equal(poisoned.view(torch.int16), finite.view(torch.int16))


@_cases(lambda c: c.group == "walk")
def test_a_slice_run_alone_equals_the_walking_run(engine_lib, case):
    """One (batch, head) of a walking case run on its own -- B = 1, one head, that head's columns through the same
    strides, so one block per tile and no walk -- gives that slice of the big run bit for bit: a row's result does not
    depend on which block computed it, nor in which round."""
    q, k, v, kip, vip = ic.make_inputs(case)
    big = run(engine_lib, case, q, k, v, kip, vip).view(torch.int16)
    d = case.d
    for b, h in ((case.B - 1, case.heads - 1), (0, 1)):
        got = (C.c_int * 4)()
        assert engine_lib.sd_ip_attention_plan(1, case.Tq, case.L, case.Tip, 1, d, case.lam, got) == 0
        assert got[2] == got[1], "the single slice walks too"
        code, alone = launch(engine_lib, q[b:b + 1], k[b:b + 1], v[b:b + 1], kip[b:b + 1], vip[b:b + 1], 1, case.Tq, case.L,
                             case.Tip, case.heads, d, case.lam, case.presc, col0=h * d, heads_run=1)
        assert code == 0, engine_lib.sd_last_error()
        assert torch.equal(alone, big[b, :, h * d:(h + 1) * d]), (b, h)


@_cases(lambda c: c.kind == "constv")
def test_constant_v_gives_a_plus_lambda_b(engine_lib, case):
    """v = a and v_ip = b in every row: out = a + lambda b whatever the scores, a reference that needs no softmax.  The
    bound is the same one with O = a + lambda b and A = |a| + |lambda| |b|."""
    q, k, v, kip, vip = ic.make_inputs(case)
    a, b = v[0, 0].double(), vip[0, 0].double()
    assert torch.equal(v, v[:1, :1].expand_as(v)) and torch.equal(vip, vip[:1, :1].expand_as(vip))
    O = (a + case.lam * b).expand(case.B, case.Tq, -1)
    A = (a.abs() + abs(case.lam) * b.abs()).expand(case.B, case.Tq, -1)
    check(case, run(engine_lib, case, q, k, v, kip, vip), O, ic.bound_of(case, v, vip, O, A), " (a + lambda b)")


def test_rejections_return_their_codes_and_write_nothing(engine_lib):
    B, Tq, H = 2, 40, 2

    def attempt(L, Tip, d, lam=1.0, ld_off=0):
        Cw = H * d
        x = torch.zeros(B * 160, Cw + ld_off, dtype=torch.float16, device="cuda")
        obuf = torch.full((B * Tq + TAIL, Cw), SENTINEL, dtype=torch.int16, device="cuda")
        code = engine_lib.sd_op_ip_cross_attention(P(x), P(x), P(x), P(x), P(x), P(obuf), B, Tq, L, Tip, H, d, Cw + ld_off,
                                                   Cw + ld_off, Cw + ld_off, Cw + ld_off, Cw + ld_off, Cw, lam, 0, 0, None,
                                                   stream())
        torch.cuda.synchronize()
        assert (obuf == SENTINEL).all()
        assert engine_lib.sd_last_error()
        got = (C.c_int * 4)()
        if not ld_off:          # the plan entry answers with the same code
            assert engine_lib.sd_ip_attention_plan(B, Tq, L, Tip, H, d, lam, got) == code
        return code

    for L, Tip, d in [(161, 4, 64), (0, 4, 64), (77, 65, 64), (77, 0, 64), (77, 4, 128), (77, 4, 48)]:
        assert attempt(L, Tip, d) == 4, (L, Tip, d)
    assert attempt(77, 4, 64, lam=float("nan")) == 1
    assert attempt(77, 4, 64, ld_off=4) == 1            # a row stride that is no multiple of 8
