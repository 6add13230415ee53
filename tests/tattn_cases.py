"""Cases, inputs, float64 reference, emulation and error bound shared by tests/test_temporal_attention_plan.py (CPU) and
tests/test_temporal_attention_gpu.py (GPU).  Nothing here touches a device.

Row order everywhere: frame f of pixel p of video v is row (v F + f) HW + p, as the UNet's row-wise GEMMs leave it."""
import collections
import functools
import math
import zlib

import torch

from stablediffusion_amd.motion import position_table

LOG2E = 1.4426950408889634
HEAD_DIMS = (32, 40, 64, 80, 160)
# Every instantiation launch_temporal_attention can reach, as (D, FT): the answers of temporal_attention_plan() in
# stablediffusion_amd/csrc/temporal_attention.hip.  FT = 1 for F <= 16 (PV product on 16x16x16 MFMAs), 2 for F <= 32.
INSTANTIATIONS = [(d, ft) for d in HEAD_DIMS for ft in (1, 2)]
PIXELS = 2              # pixels per block of every instantiation
WAVES = 4
F_MAX = 32

FRAMES = (1, 2, 8, 15, 16, 17, 24, 31, 32)
PIXEL_COUNTS = tuple(sorted({1, PIXELS - 1, PIXELS, PIXELS + 1, 2 * PIXELS + 3} - {0}))
VIDEOS = (1, 3)
HEADS = (2, 8)

# kind: "randn" | "stress" (frames whose scores differ by multiples of 10 in log2 units) | "nobias" (a zero table)
Case = collections.namedtuple("Case", "V F HW heads d presc kind")


def case_id(c):
    return "d%d-F%d-V%dxHW%dxH%d%s-%s" % (c.d, c.F, c.V, c.HW, c.heads, "-presc" if c.presc else "", c.kind)


def inst_of(c):
    return (c.d, 1 if c.F <= 16 else 2)


def vstr_halves(d):
    """LDS row stride of the V tile: the head dim padded to 16, as an odd multiple of 32 bytes."""
    b = (d + 15) // 16 * 16 * 2
    return (((b + 31) // 32) | 1) * 32 // 2


def expected_plan(c):
    ft = 1 if c.F <= 16 else 2
    return (c.d, ft, PIXELS, WAVES, 16 if ft == 1 else 32, WAVES * 16 * ft * vstr_halves(c.d) * 2,
            c.V * ((c.HW + PIXELS - 1) // PIXELS))


def _build():
    """The whole cross product of the shape sets; pre-scaled queries (what the UNet runs) alternate with plain ones."""
    cases = []
    n = 0
    for d in HEAD_DIMS:
        for F in FRAMES:
            for HW in PIXEL_COUNTS:
                for V in VIDEOS:
                    for heads in HEADS:
                        cases.append(Case(V, F, HW, heads, d, n % 2, "randn"))
                        n += 1
    for d in HEAD_DIMS:
        for F in (2, 15, 17, 32):
            cases.append(Case(3, F, 2 * PIXELS + 3, 2, d, F % 2, "stress"))
            cases.append(Case(3, F, 2 * PIXELS + 3, 2, d, 1 - F % 2, "nobias"))
    return cases


GPU_CASES = _build()


def seed_of(case):
    return zlib.crc32(case_id(case).encode()) & 0x7fffffff


def frame_of_row(case):
    M = case.V * case.F * case.HW
    return (torch.arange(M) // case.HW) % case.F


def make_inputs(case):
    """fp16 q, k, v [V F HW, heads d] as the q|k|v GEMM would leave them and the fp32 table [F_MAX, 3C]; with
    case.presc q and the table's q columns carry log2(e) / sqrt(d)."""
    V, F, HW, H, d = case.V, case.F, case.HW, case.heads, case.d
    C, M = H * d, V * F * HW
    g = torch.Generator().manual_seed(seed_of(case))
    c = LOG2E / math.sqrt(d) if case.presc else 1.0
    q = torch.randn(M, C, generator=g)
    k = torch.randn(M, C, generator=g)
    v = torch.randn(M, C, generator=g)
    bias = 0.5 * torch.randn(F_MAX, 3 * C, generator=g)
    if case.kind == "nobias":
        bias.zero_()
    if case.kind == "stress":
        # q = a u + small noise, k_g = b_g u + noise with u = 1 / sqrt(d) per head: the log2-domain score of key frame g
        # is about off_g = -10 ((7 g) mod 5), and sum |q_i k_i| stays near |score| (score_rounding below)
        a = 4.0
        off = -10.0 * ((7 * torch.arange(F)) % 5).float()
        b = off / (a * LOG2E / math.sqrt(d))
        u = 1.0 / math.sqrt(d)
        q = 0.25 * q + a * u
        k = k + (b[frame_of_row(case)] * u)[:, None]
        bias[:, :2 * C] *= 0.1
    q = q * c
    bias[:, :C] *= c
    return q.half(), k.half(), v.half(), bias


def operands(case, q, k, v, bias, table_shift=0, bias_k=True):
    """The fp16 operands the kernel multiplies: the table row of the frame added in fp32, rounded once.  The two
    arguments are the mutants' defects."""
    C = case.heads * case.d
    f = (frame_of_row(case) + table_shift) % F_MAX
    qo = (q.float() + bias[f, 0:C]).half()
    ko = (k.float() + bias[f, C:2 * C]).half() if bias_k else k
    vo = (v.float() + bias[f, 2 * C:3 * C]).half()
    return qo, ko, vo


def _problems(case, t, row_stride=None):
    """[M, C] -> [V, HW, heads, F, d]; row_stride: the rows one frame lies apart (the mutant's: HW + 1)."""
    V, F, HW, H, d = case.V, case.F, case.HW, case.heads, case.d
    rs = HW if row_stride is None else row_stride
    idx = (torch.arange(V)[:, None, None] * F + torch.arange(F)[None, None, :]) * rs + torch.arange(HW)[None, :, None]
    idx = idx % t.shape[0]
    return t[idx].view(V, HW, F, H, d).transpose(2, 3)


def _rows(case, o):
    """[V, HW, heads, F, d] -> [M, C]"""
    V, F, HW, H, d = case.V, case.F, case.HW, case.heads, case.d
    return o.transpose(2, 3).reshape(V, HW, F, H * d).transpose(1, 2).reshape(V * F * HW, H * d)


def reference(case, qo, ko, vo):
    """float64 of the fp16 operands: O = softmax(q k^T / sqrt(d)) v over the F frames of a pixel, A = softmax(..) |v|,
    both [M, C].  Pre-scaled queries are un-scaled first."""
    d = case.d
    unscale = math.sqrt(d) / LOG2E if case.presc else 1.0
    qd, kd, vd = (_problems(case, t.double()) for t in (qo, ko, vo))
    S = (qd * unscale) @ kd.transpose(-1, -2) / math.sqrt(d)
    P = torch.softmax(S, dim=-1)
    return _rows(case, P @ vd), _rows(case, P @ vd.abs())


def score_rounding(case, qo, ko):
    """An upper bound of the relative error the fp32 score arithmetic leaves in a probability: the MFMA sums d products
    in fp32 ((d + 1) 2^-24 of sum |q_i k_i|), the scale multiply and the subtraction of the maximum round once each
    (2^-24 of |score| <= sum |q_i k_i| each), all in log2 units, so times ln 2; the hardware exp2 adds 2^-22."""
    d = case.d
    s = 1.0 if case.presc else LOG2E / math.sqrt(d)
    X = (_problems(case, qo.double()).abs() @ _problems(case, ko.double()).abs().transpose(-1, -2)).max().item() * s
    return math.log(2.0) * (d + 4) * 2.0 ** -24 * X + 2.0 ** -22


def elementwise_bound(O, A, F, vmax):
    """|out - O| may not exceed this.  From the kernel's arithmetic:
      * probabilities rounded to nearest fp16 (2^-11 relative) and the denominator summed from the same rounded values;
        the fp32 score arithmetic moves a probability by at most score_rounding(), which the CPU suite holds below
        2^-11 for every case.  Relative errors of at most e in the probabilities move a weight w_i = p_i / sum p by at
        most 2 e w_i: together 2 (2^-11 + 2^-11) A = 2^-9 A;
      * the fp16 store, 2^-11 |O| (the bound grants 2^-10);
      * fp32 accumulation over F keys and the normalisation, below F 2^-23 max|V|, which also covers probabilities in
        fp16's subnormal range (they lose at most 2^-25 each against a denominator of at least 1);
      * 2^-24, the smallest fp16 step."""
    return 2.0 ** -9 * A + 2.0 ** -10 * O.abs() + F * 2.0 ** -23 * vmax + 2.0 ** -24


def emulate(case, q, k, v, bias, mask_pad=True, bias_k=True, row_stride=None, table_shift=0):
    """The kernel's arithmetic in torch on the CPU: table added in fp32 and the operand rounded to fp16, fp32 scores on a
    16-key tile grid, keys >= F masked, exact maximum, probabilities exp2 rounded to nearest fp16, fp32 sums of the
    rounded values, fp16 store.  The keyword arguments switch in ONE defect each (the mutants of the CPU suite)."""
    F, d = case.F, case.d
    qo, ko, vo = operands(case, q, k, v, bias, table_shift=table_shift, bias_k=bias_k)
    qf, kf, vf = (_problems(case, t.float(), row_stride) for t in (qo, ko, vo))
    KEYS = 16 * (1 if F <= 16 else 2)
    pad = KEYS - F
    kf = torch.nn.functional.pad(kf, (0, 0, 0, pad))            # padded keys load as zeros
    vf = torch.nn.functional.pad(vf, (0, 0, 0, pad))
    S = qf @ kf.transpose(-1, -2)
    S = S * torch.tensor(1.0 if case.presc else LOG2E / math.sqrt(d), dtype=torch.float32)
    if mask_pad:
        S[..., F:] = float("-inf")
    p = torch.exp2(S - S.amax(dim=-1, keepdim=True)).half().float()
    o = (p @ vf) * (1.0 / p.sum(dim=-1, keepdim=True))
    return _rows(case, o.half())


@functools.lru_cache(maxsize=4)
def inputs_and_reference(case):
    """(q, k, v, bias, O, A) of a case, computed once for the tests that run it; callers must not modify them."""
    q, k, v, bias = make_inputs(case)
    return (q, k, v, bias) + reference(case, *operands(case, q, k, v, bias))


def pos_bias_reference(w, F, scale, scale_rows):
    """float64 [F, N] of sd_op_motion_pos_bias for the fp16 weight w [N, C]."""
    out = position_table(F, w.shape[1]) @ w.double().t()
    out[:, :scale_rows] *= scale
    return out
