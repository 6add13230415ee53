"""region_xattn_kernel through sd_op_region_cross_attention, against a float64 CPU reference of the same fp16 operands
(tests/region_cases.py holds the cases, the reference and the bound; tests/test_region_plan.py proves the bound on an
emulation of the kernel's arithmetic and that the cases cover the all-resident and the grouped form at every head dim).

Per run: the form sd_region_plan names is the one the case was written for; rel-L2 < 3e-3; every element finite and
within the element-wise bound; nothing outside the B * Tq x heads * d output is written.  Every run puts `out` inside
a buffer pre-filled with a bit pattern (64 tail rows, 8 pad columns when strided) and K / V in front of 64 rows of NaN
in the same allocation; the pad columns of strided inputs hold NaN too."""
import ctypes as C

import pytest
import torch

import region_cases as rc
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


def launch(lib, q, k, v, w, B, Tq, L, R, H, d, Bw, presc, layout="contig"):
    """One launch on CPU operands q [B, Tq, C], k / v [B, R L, C], w [Bw, Tq, R]; returns (code, [B, Tq, C] fp16 output
    on the CPU) after checking that everything around the output in its buffer is untouched.
      "contig"  every operand its own dense matrix;
      "textkv"  k, v slices at a non-zero column offset of a [B R L, 4C + 24] row (the UNet's text K / V), q and out in
                rows 8 columns wider than C."""
    Cw = H * d
    Tk = R * L
    q2, k2, v2 = q.reshape(B * Tq, Cw).cuda(), k.reshape(B * Tk, Cw).cuda(), v.reshape(B * Tk, Cw).cuda()
    if layout == "contig":
        qv = q2
        kbuf, vbuf = _nan_buffer(B * Tk + TAIL, Cw), _nan_buffer(B * Tk + TAIL, Cw)
        kv, vv = kbuf[:B * Tk], vbuf[:B * Tk]
        ldo = Cw
    else:
        assert layout == "textkv"
        qbuf = _nan_buffer(B * Tq, Cw + 8)
        buf = _nan_buffer(B * Tk + TAIL, 4 * Cw + 24)
        qv, kv, vv = qbuf[:, :Cw], buf[:B * Tk, 2 * Cw + 8:3 * Cw + 8], buf[:B * Tk, 3 * Cw + 8:4 * Cw + 8]
        ldo = Cw + 8
        qv.copy_(q2)
    kv.copy_(k2)
    vv.copy_(v2)
    wd = w.contiguous().cuda()
    obuf = torch.full((B * Tq + TAIL, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    code = lib.sd_op_region_cross_attention(P(qv), P(kv), P(vv), P(wd), P(obuf), B, Tq, L, R, H, d, qv.stride(0),
                                            kv.stride(0), vv.stride(0), ldo, Bw, presc, stream())
    torch.cuda.synchronize()
    ob = obuf.cpu()
    assert (ob[B * Tq:] == SENTINEL).all(), "rows behind the output were written"
    assert (ob[:, Cw:] == SENTINEL).all(), "pad columns of the output were written"
    return code, ob[:B * Tq, :Cw].contiguous()


def run(lib, case, q, k, v, w, layout="contig"):
    got = (C.c_int * 4)()
    assert lib.sd_region_plan(case.R, case.L, case.d, got) == 0, lib.sd_last_error()
    assert ("grouped" if got[1] > 1 else "resident") == case.form, "the plan moved: this case no longer runs the form it was written for"
    code, ob = launch(lib, q, k, v, w, case.B, case.Tq, case.L, case.R, case.heads, case.d, case.Bw, case.presc, layout)
    assert code == 0, lib.sd_last_error()
    return ob.view(torch.float16).view(case.B, case.Tq, case.heads * case.d)


def check(case, out, O, A, v):
    o = out.double()
    assert torch.isfinite(o).all()
    err = (o - O).abs()
    bound = rc.elementwise_bound(O, A, case.R * case.L, v.abs().max().double())
    ratio = (err / bound).max().item()
    r = rel_l2(out, O)
    print("%s: rel_l2 %.2e, worst |err| / bound %.3f" % (rc.case_id(case), r, ratio))
    assert r < 3e-3
    worst = (err - bound).argmax()
    assert ratio <= 1.0, (rc.case_id(case), "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())


def _cases(pred):
    cs = [c for c in rc.GPU_CASES if pred(c)]
    return pytest.mark.parametrize("case", cs, ids=[rc.case_id(c) for c in cs])


@_cases(lambda c: True)
def test_region_attention_against_float64(engine_lib, case):
    """Every head dim in both forms: disjoint weights whose boundary falls inside a 16-query tile, soft overlapping
    ones, a region that is zero everywhere, Bw < B, pre-scaled queries, one segment with scores of std 60 and one with
    every score about -150."""
    q, k, v, w, O, A = rc.inputs_and_reference(case)
    check(case, run(engine_lib, case, q, k, v, w), O, A, v)


@_cases(lambda c: c.weights == "disjoint" and c.kind == "randn")
def test_one_hot_weights_equal_the_single_region_run(engine_lib, case):
    """With one-hot weights every row is, bit for bit, the R = 1 run on the K / V of that row's region: a skipped
    segment adds nothing, and a segment that runs for a neighbour in the tile adds an exact zero."""
    q, k, v, w, O, A = rc.inputs_and_reference(case)
    out = run(engine_lib, case, q, k, v, w).view(torch.int16)
    B, Tq, L, R = case.B, case.Tq, case.L, case.R
    ones = torch.ones(1, Tq, 1)
    seen = torch.zeros(B, Tq, dtype=torch.bool)
    for r in range(R):
        code, single = launch(engine_lib, q, k[:, r * L:(r + 1) * L].contiguous(), v[:, r * L:(r + 1) * L].contiguous(), ones,
                              B, Tq, L, 1, case.heads, case.d, 1, case.presc)
        assert code == 0, engine_lib.sd_last_error()
        single = single.view(B, Tq, -1)
        for b in range(B):
            rows = w[b % case.Bw, :, r] == 1.0
            assert torch.equal(out[b, rows], single[b, rows]), (r, b)
            seen[b] |= rows
    assert seen.all()


@_cases(lambda c: c.kind == "randn" and c.Tq == 100 and c.weights in ("disjoint", "soft"))
def test_wide_text_kv_layout_is_bit_identical(engine_lib, case):
    """K / V inside the wide text-KV row, q and out in padded rows, NaN in every pad column and behind the last K / V
    row: bit-identical to the dense layout."""
    q, k, v, w, O, A = rc.inputs_and_reference(case)
    dense = run(engine_lib, case, q, k, v, w)
    wide = run(engine_lib, case, q, k, v, w, "textkv")
    assert torch.isfinite(wide.float()).all()
    assert torch.equal(dense.view(torch.int16), wide.view(torch.int16))


def test_rejections_return_their_codes_and_write_nothing(engine_lib):
    B, Tq, L, H = 2, 40, 8, 2

    def attempt(R, L, d, Bw=1, ld_off=0, null=None):
        Cw = H * d
        q = torch.zeros(B * Tq, Cw + ld_off, dtype=torch.float16, device="cuda")
        k = torch.zeros(B * max(R, 1) * max(L, 1), Cw, dtype=torch.float16, device="cuda")
        w = torch.ones(max(Bw, 1), Tq, max(R, 1), device="cuda")
        obuf = torch.full((B * Tq + TAIL, Cw), SENTINEL, dtype=torch.int16, device="cuda")
        ptr = {"q": P(q), "k": P(k), "v": P(k), "w": P(w), "out": P(obuf)}
        if null:
            ptr[null] = None
        code = engine_lib.sd_op_region_cross_attention(ptr["q"], ptr["k"], ptr["v"], ptr["w"], ptr["out"], B, Tq, L, R, H, d,
                                                       Cw + ld_off, Cw, Cw, Cw, Bw, 0, stream())
        torch.cuda.synchronize()
        assert (obuf == SENTINEL).all()
        assert code == 0 or engine_lib.sd_last_error()
        return code

    for R, L_, d in [(2, L, 48), (2, L, 128), (0, L, 40), (9, L, 40), (2, 0, 40), (2, 161, 40)]:
        assert attempt(R, L_, d) == 4, (R, L_, d)
    assert attempt(2, L, 40, ld_off=4) == 1         # a row stride that is no multiple of 8
    assert attempt(2, L, 40, Bw=0) == 1
    assert attempt(2, L, 40, Bw=3) == 1             # does not divide B = 2
    for name in ("q", "k", "v", "w", "out"):
        assert attempt(2, L, 40, null=name) == 1, name
