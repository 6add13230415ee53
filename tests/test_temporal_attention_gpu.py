"""sd_op_temporal_attention against a float64 CPU reference of the same fp16 operands, per element, under the bound of
tests/tattn_cases.py (the CPU suite proves it on an emulation of the kernel's arithmetic), and sd_op_motion_pos_bias
against the float64 closed form.

Every run reads q | k | v as column slices of one [M, 3C + 8] buffer whose pad columns and 64 rows behind the last row
hold NaN, and writes `out` inside a buffer pre-filled with a bit pattern (64 rows in front, 64 behind, 8 pad columns):
nothing outside the M x C output may change."""
import ctypes as C
import math

import pytest
import torch

import tattn_cases as tc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TAIL = 64
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(lib, case, q, k, v, bias):
    """One launch; returns the [M, C] fp16 output on the CPU after checking its surroundings."""
    V, F, HW, H, d = case.V, case.F, case.HW, case.heads, case.d
    Cw, M = H * d, V * F * HW
    buf = torch.full((M + TAIL, 3 * Cw + 8), float("nan"), dtype=torch.float16, device="cuda")
    buf[:M, 0:Cw] = q.cuda()
    buf[:M, Cw:2 * Cw] = k.cuda()
    buf[:M, 2 * Cw:3 * Cw] = v.cuda()
    table = bias.cuda().contiguous()
    ldo = Cw + 8
    obuf = torch.full((TAIL + M + TAIL, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    oview = obuf[TAIL:]
    got = (C.c_int64 * 7)()
    assert lib.sd_temporal_attention_plan(V, F, HW, H, d, got) == 0, lib.sd_last_error()
    assert tuple(got) == tc.expected_plan(case), "the plan moved: this case no longer runs what it was written for"
    ld = buf.stride(0)
    rc = lib.sd_op_temporal_attention(P(buf[:, 0:]), P(buf[:, Cw:]), P(buf[:, 2 * Cw:]), P(oview), P(table), ld, ld, ld, ldo,
                                      table.stride(0), V, F, HW, H, d, case.presc, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    ob = obuf.cpu()
    assert (ob[:TAIL] == SENTINEL).all(), "rows in front of the output were written"
    assert (ob[TAIL + M:] == SENTINEL).all(), "rows behind the output were written"
    assert (ob[:, Cw:] == SENTINEL).all(), "pad columns of the output were written"
    return ob[TAIL:TAIL + M, :Cw].contiguous().view(torch.float16)


def check(case, out, O, A, vo):
    o = out.double()
    assert torch.isfinite(o).all(), tc.case_id(case)
    err = (o - O).abs()
    bound = tc.elementwise_bound(O, A, case.F, vo.abs().max().double())
    ratio = (err / bound).max().item()
    worst = (err - bound).argmax()
    assert ratio <= 1.0, (tc.case_id(case), "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())
    assert rel_l2(out, O) < 3e-3, tc.case_id(case)
    return ratio


_GROUPS = [(d, F) for d in tc.HEAD_DIMS for F in tc.FRAMES]


@pytest.mark.parametrize("d,F", _GROUPS, ids=["d%d-F%d" % g for g in _GROUPS])
def test_temporal_attention_against_float64(engine_lib, d, F):
    """Every HW in {1, P - 1, P, P + 1, 2P + 3}, V in {1, 3} and heads in {2, 8} of one (head dim, frame count)."""
    cases = [c for c in tc.GPU_CASES if c.kind == "randn" and (c.d, c.F) == (d, F)]
    assert len(cases) == len(tc.PIXEL_COUNTS) * len(tc.VIDEOS) * len(tc.HEADS)
    worst = 0.0
    for case in cases:
        q, k, v, bias = tc.make_inputs(case)
        qo, ko, vo = tc.operands(case, q, k, v, bias)
        O, A = tc.reference(case, qo, ko, vo)
        out = run(engine_lib, case, q, k, v, bias)
        worst = max(worst, check(case, out, O, A, vo))
        if F == 1:                                     # one frame: the output is v + bias_v rounded once, bit for bit
            assert torch.equal(out.view(torch.int16), vo.view(torch.int16)), tc.case_id(case)
    print("d %d, F %d: worst |err| / bound %.3f over %d shapes" % (d, F, worst, len(cases)))


_STRESS = [c for c in tc.GPU_CASES if c.kind == "stress"]


@pytest.mark.parametrize("case", _STRESS, ids=[tc.case_id(c) for c in _STRESS])
def test_temporal_attention_stress_scores(engine_lib, case):
    """Key frames whose scores lie 0, 10, 20, 30 or 40 (log2 units) below the best: most probabilities are below fp16's
    normal range or zero."""
    q, k, v, bias, O, A = tc.inputs_and_reference(case)
    vo = tc.operands(case, q, k, v, bias)[2]
    out = run(engine_lib, case, q, k, v, bias)
    print("%s: worst |err| / bound %.3f" % (tc.case_id(case), check(case, out, O, A, vo)))


_NOBIAS = [c for c in tc.GPU_CASES if c.kind == "nobias"]


@pytest.mark.parametrize("case", _NOBIAS, ids=[tc.case_id(c) for c in _NOBIAS])
def test_temporal_attention_zero_bias_equals_attention(engine_lib, case):
    """A zero table (and a NULL one, bit for bit the same): the launch computes what sd_op_attention_ex computes on the
    operands permuted to [V HW, F, C], under the same bound."""
    V, F, HW, H, d = case.V, case.F, case.HW, case.heads, case.d
    Cw = H * d
    q, k, v, bias, O, A = tc.inputs_and_reference(case)
    assert not bias.any()
    out = run(engine_lib, case, q, k, v, bias)
    check(case, out, O, A, v)

    M = V * F * HW
    qkv = torch.cat([q, k, v], dim=1).cuda()
    o2 = torch.empty(M, Cw, dtype=torch.float16, device="cuda")
    rc = engine_lib.sd_op_temporal_attention(P(qkv[:, 0:]), P(qkv[:, Cw:]), P(qkv[:, 2 * Cw:]), P(o2), None, 3 * Cw, 3 * Cw,
                                             3 * Cw, Cw, 0, V, F, HW, H, d, case.presc, stream())
    assert rc == 0, engine_lib.sd_last_error()
    assert torch.equal(o2.cpu().view(torch.int16), out.view(torch.int16))

    perm = qkv.view(V, F, HW, 3 * Cw).permute(0, 2, 1, 3).contiguous().view(V * HW * F, 3 * Cw)
    o3 = torch.empty(V * HW * F, Cw, dtype=torch.float16, device="cuda")
    rc = engine_lib.sd_op_attention_ex(P(perm[:, 0:]), P(perm[:, Cw:]), P(perm[:, 2 * Cw:]), P(o3), V * HW, F, F, H, d, 3 * Cw,
                                       3 * Cw, 3 * Cw, Cw, 0, case.presc, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    back = o3.view(V, HW, F, Cw).permute(0, 2, 1, 3).reshape(M, Cw).cpu()
    check(case, back, O, A, v)
    diff = (back.double() - out.double()).abs()
    bound = tc.elementwise_bound(O, A, F, v.abs().max().double())
    print("%s: worst |fused - permuted route| / bound %.3f" % (tc.case_id(case), (diff / bound).max().item()))
    assert (diff <= bound).all()


def test_temporal_attention_rejections(engine_lib):
    """Nothing is launched for arguments the kernel's indexing does not cover."""
    lib = engine_lib
    buf = torch.zeros(64, 3 * 80 + 8, dtype=torch.float16, device="cuda")
    out = torch.full((64, 80), SENTINEL, dtype=torch.int16, device="cuda")
    tab = torch.zeros(32, 240, device="cuda")

    def call(F=2, d=40, ldq=248, ldo=80, ldb=240, qoff=0, heads=2):
        return lib.sd_op_temporal_attention(P(buf[:, qoff:]), P(buf[:, 80:]), P(buf[:, 160:]), P(out), P(tab), ldq, 248, 248, ldo,
                                            ldb, 2, F, 4, heads, d, 1, stream())
    assert call() == 0, lib.sd_last_error()
    assert call(F=0) == 4 and call(F=33) == 4 and call(d=48) == 4
    assert call(ldq=244) == 1 and call(ldo=72) == 1 and call(ldb=232) == 1 and call(qoff=4) == 1
    torch.cuda.synchronize()
    assert (out.cpu()[16:] == SENTINEL).all()


@pytest.mark.parametrize("C_,F", [(320, 32), (1280, 32), (64, 5), (1280, 1)])
def test_motion_pos_bias_closed_form(engine_lib, C_, F):
    """The table of a q|k|v weight against float64, with the query rows carrying the pre-scale; fp32 rounding only."""
    g = torch.Generator().manual_seed(C_ + F)
    w = (torch.randn(3 * C_, C_, generator=g) / math.sqrt(C_)).half()
    scale = tc.LOG2E / math.sqrt(C_ // 8)
    ldo = 3 * C_ + 4
    out = torch.full((F + 1, ldo), float("nan"), device="cuda")
    rc = engine_lib.sd_op_motion_pos_bias(P(w.cuda()), 3 * C_, C_, F, scale, C_, P(out), ldo, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    o = out.cpu()
    assert torch.isnan(o[F:]).all() and torch.isnan(o[:, 3 * C_:]).all()
    ref = tc.pos_bias_reference(w, F, float(torch.tensor(scale, dtype=torch.float32)), C_)
    err = (o[:F, :3 * C_].double() - ref).abs()
    tol = 2.0 ** -23 * ref.abs() + 1e-12 * C_
    print("C %d, F %d: worst error %.2e" % (C_, F, err.max().item()))
    assert (err <= tol).all()
    assert engine_lib.sd_op_motion_pos_bias(P(w.cuda()), 3 * C_, C_ + 4, F, scale, C_, P(out), ldo, stream()) == 1
