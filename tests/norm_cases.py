"""Cases, inputs, float64 references, fp32 emulations and the element-wise error bound shared by tests/test_norm_plan.py
(CPU) and tests/test_norm_gpu.py (GPU) for the normalisation kernels of csrc/norm.hip.  Nothing here touches a device.

A GroupNorm case names what it was written for as want = (statistics kernel, apply kernel, T, NV, finalize) in
sd_norm_plan's numbering (statistics 0 none / 1 gn_stats_kernel / 2 gn_stats2_kernel; apply 0 gn_fused_kernel<T, NV> /
1 gn_apply_kernel / 2 gn_apply2_kernel<NV>): the CPU suite checks that sd_norm_plan gives exactly that for every case
and that the cases reach every kernel form and every path inside them, the GPU suite compares it with what
sd_op_groupnorm_ex reports to have run.

Profiles
  randn   x = fp16(1.5 randn + 0.7)
  p50     x = fp16(50 + 0.1 randn), group 1 of image 0 the constant 50: |mean| / std = 500, the case E[x^2] - mean^2
  m30     x = fp16(-30 + 0.1 randn), the same constant group     loses; the constant group's output is act(beta)

Reference: float64 on the fp16 inputs, y = act((x - mean) rstd gamma + beta), biased variance.

Bound per element, with u = 2^-24, sc = rstd gamma, pre = (x - mean) sc + beta, the kernels' form y = act(x sc + sh),
sh = beta - mean sc:
  rounding    half an fp16 step of the reference (the subnormal step below 2^-14)
  evaluation  u (2 |x sc| + 2 |mean sc| + |beta - mean sc| + |pre|): sc carries one rounding, mean sc and x sc two each,
              sh and the last add one each; through SiLU times max |silu'| < 1.1, plus u (8 + |pre|) |y| for
              v_exp_f32 / v_rcp_f32 and the rounding of the exponent's argument.  LayerNorm evaluates
              ((x - mean) rstd) gamma + beta: u (3 |pre - beta| + |pre|).
  statistics  |sc| dm + |x - mean| |sc| rho with dm = STAT_A u (|mean| + std), rho = u (STAT_R + STAT_RM |mean| / std):
              the statistics' own error (the last term: Chan merges of summaries whose means carry u |mean| each).  The
              three constants are not derived; they are set from the worst error of the fp32 emulations below (each
              kernel's summation order, numpy float32) over every case and profile, with at least a factor of two:
              measured worst |mean error| = 4.05 u (|mean| + std) (fused, 49 x 5120), worst relative rstd error 14.3 u
              at randn (the same case) and 106 u = 0.21 u |mean| / std at offset 50 (gn_stats_kernel, 2 x 1000 x 32);
              test_norm_plan.test_statistics_constants_hold_twice_the_emulations_error asserts the factor per case.
Worst |error| / bound of the emulated OUTPUT is 0.995 .. 0.998 in every group of cases, as for any correct kernel: among
a million elements some fp32 value lies next to an fp16 rounding tie.  The share of the fp32 terms (bound minus the half
step) the emulation needs is the informative figure, worst per group (test_norm_plan prints them): fused 0.23, twopass
0.16, apply1 0.13, narrow 0.22, groups 0.14, large 0.12, defect 0.16, supplied 0.20, strided 0.16; LayerNorm 0.08.  The
mutations of test_norm_plan (each a plausible kernel bug) show the bound is tight enough to see a wrong kernel."""
import collections
import functools
import zlib

import numpy as np
import torch

U = 2.0 ** -24
STAT_A = 10.0
STAT_R = 32.0
STAT_RM = 0.5
f32 = np.float32

Case = collections.namedtuple("Case", "group N HW C G silu eps profile pre want layouts")
# group     the GPU test that runs it
# pre       0, or pixels per caller-supplied summary (S = ceil(HW / pre) of them per image)
# want      (statistics kernel, apply kernel, T, NV, finalize)
# layouts   operand layouts the GPU suite runs: "dense", "left", "right" (see test_norm_gpu.run)

GN_MAX_CB = 512


def cdiv(a, b):
    return (a + b - 1) // b


def case_id(c):
    s = "%s-%dx%dx%d-g%d-%s" % (c.group, c.N, c.HW, c.C, c.G, c.profile)
    s += ("-silu" if c.silu else "") + ("-eps%g" % c.eps if c.eps != 1e-5 else "") + ("-pre%d" % c.pre if c.pre else "")
    return s


def block_channels(C, G):
    """Channels per statistics / apply2 block (gn_block_channels)."""
    cpg = C // G
    unit = cpg
    while unit % 8:
        unit += cpg
    cb = unit
    while cb + unit <= GN_MAX_CB and cb + unit <= C:
        cb += unit
    return min(cb, C)


def parent_slabs(N, HW, C, G):
    """gn_slabs before it dropped the empty slabs: about 1024 blocks, at least 64 pixels per slab, at most 256."""
    cblocks = cdiv(C, block_channels(C, G))
    s = max(1024 // (N * cblocks), 1)
    s = min(s, max(HW // 64, 1), 256)
    return s


def apply2_paths(c, plan):
    """What gn_apply2_kernel's prologue does per channel-block width, from the plan: [(width, groups in the block, LW,
    parts1, extra summary loop)], and whether the summaries are of equal size.  Restates the kernel (device code)."""
    stats, apply, T, NV, fin, S, rows, CB = plan[:8]
    assert apply == 2
    if c.pre:
        rows = c.pre
    if fin:
        S, rows = 1, c.HW
    cpg = c.C // c.G
    equal = c.HW % rows == 0
    out = []
    for cw in sorted({CB, c.C - (c.C - 1) // CB * CB}):
        ng = cw // cpg
        LW = 1 if (equal and S * ng <= 128 and ng <= 64) else 4
        parts1 = 64 * LW // ng
        out.append((cw, ng, LW, parts1, equal and S > 4 * parts1))
    return equal, out


def _build():
    cases = []

    def add(group, N, HW, C, G, want, silu=1, eps=1e-5, profiles=("randn",), pre=0, layouts=("dense",)):
        for p in profiles:
            cases.append(Case(group, N, HW, C, G, silu, eps, p, pre, want, layouts))

    ALL = ("randn", "p50", "m30")
    F4, F16, F1K = (0, 0, 256, 4, 0), (0, 0, 256, 16, 0), (0, 0, 1024, 16, 0)
    # fused: every HW edge of the three forms at cpg 10 (chunks straddle groups); the widths of the UNets
    for hw, w in ((1, F4), (63, F4), (64, F4), (65, F16), (255, F16), (256, F16), (257, F1K), (510, F1K), (512, F1K)):
        add("fused", 2, hw, 320, 32, w, profiles=ALL if hw in (63, 255, 510) else ("randn",), silu=hw % 2)
    for C in (384, 512, 1920, 2560):
        add("fused", 1, 61, C, 32, F4)
        add("fused", 1, 250, C, 32, F16, silu=0)
        add("fused", 1, 500, C, 32, F1K, profiles=("randn", "p50") if C == 1920 else ("randn",))
    add("fused", 1, 48, 5120, 32, F4)
    add("fused", 1, 49, 5120, 32, (2, 2, 0, 1, 0))          # the fall-off: 49 pixels need more than 4 x 12 planes
    add("fused", 1, 200, 5120, 32, (2, 2, 0, 1, 0), profiles=("randn", "m30"))
    for g in (1, 8, 16):
        add("groups", 1, 300, 320, g, F1K)
    # two-pass, small groups: cpg 1, 2, 3, 6 run gn_stats_kernel, cpg 4 gn_stats2_kernel
    for C, st in ((32, 1), (64, 1), (96, 1), (192, 1), (128, 2)):
        for hw in (513, 1000, 1600):
            add("twopass", 2, hw, C, 32, (st, 2, 0, 1, 0), profiles=ALL if hw == 1000 else ("randn",), silu=int(hw != 513))
    # gn_apply_kernel: more than 128 groups per channel block
    add("apply1", 1, 600, 512, 256, (1, 1, 0, 0, 0), profiles=ALL)
    add("apply1", 2, 513, 256, 256, (1, 1, 0, 0, 0), silu=0)
    add("apply1", 1, 520, 768, 256, (1, 1, 0, 0, 0))
    # a last channel block narrower than the others (768: CB = 504)
    for C, nv in ((640, 1), (1280, 1), (768, 1), (1536, 2)):
        add("narrow", 1, 1030, C, 32, (2, 2, 0, nv, 0), profiles=ALL if C == 768 else ("randn",))
    for g in (1, 8, 16):
        add("groups", 1, 1030, 320, g, (2, 2, 0, 1, 0), profiles=("randn", "p50") if g == 8 else ("randn",))
    add("groups", 1, 1024, 320, 8, (2, 2, 0, 1, 0))          # 16 equal summaries x 8 groups: one wave fetches (LW = 1)
    # large maps: NV = 8, 4, 2 and S = 256
    add("large", 1, 16400, 512, 32, (2, 2, 0, 8, 0))
    add("large", 2, 65600, 64, 32, (1, 2, 0, 8, 0), eps=1e-6)
    add("large", 1, 2750, 1280, 32, (2, 2, 0, 4, 0))
    add("large", 1, 16900, 128, 32, (2, 2, 0, 2, 0), profiles=("randn", "p50"), eps=1e-6)
    add("large", 1, 16448, 128, 32, (2, 2, 0, 2, 0))         # S = 256 with a ragged last slab (the cap itself)
    # the shapes whose last slabs were empty (or started past HW) before gn_slabs dropped them
    add("defect", 1, 4225, 128, 32, (2, 2, 0, 1, 0), profiles=ALL, eps=1e-6)
    add("defect", 2, 4225, 320, 32, (2, 2, 0, 2, 0))
    add("defect", 1, 8385, 128, 32, (2, 2, 0, 1, 0), profiles=("randn", "m30"))
    add("defect", 1, 4289, 128, 32, (2, 2, 0, 1, 0), profiles=("randn", "p50"))
    add("defect", 1, 16900, 512, 32, (2, 2, 0, 8, 0), eps=1e-6)
    # caller-supplied summaries: tiles of 128 and 256 rows, S <= 64 and S > 64 (finalize), ragged last tiles, and a small
    # map where the fused kernel ignores them
    add("supplied", 1, 4096, 320, 32, (0, 2, 0, 1, 0), pre=128, profiles=ALL)
    add("supplied", 1, 4096, 320, 32, (0, 2, 0, 1, 0), pre=256)
    add("supplied", 2, 4000, 320, 32, (0, 2, 0, 2, 0), pre=128, profiles=("randn", "p50"))          # ragged: 32 rows left
    add("supplied", 1, 16384, 128, 32, (0, 2, 0, 2, 1), pre=128)
    add("supplied", 1, 16641, 128, 32, (0, 2, 0, 2, 1), pre=256, profiles=("randn", "m30"))         # 66 tiles, the last one row
    add("supplied", 1, 8320, 640, 32, (0, 2, 0, 8, 1), pre=128, silu=0)
    add("supplied", 2, 1024, 320, 32, (0, 2, 0, 1, 0), pre=128)
    add("supplied", 2, 256, 320, 32, F16, pre=128)
    # strided operands, a case per kernel form
    L3 = ("dense", "left", "right")
    add("strided", 2, 60, 320, 32, F4, layouts=L3)
    add("strided", 1, 200, 640, 32, F16, layouts=L3)
    add("strided", 1, 300, 1280, 32, F1K, layouts=L3)
    add("strided", 2, 700, 96, 32, (1, 2, 0, 1, 0), layouts=L3)
    add("strided", 1, 1100, 640, 32, (2, 2, 0, 1, 0), layouts=L3, profiles=("randn", "p50"))
    add("strided", 1, 4289, 320, 32, (2, 2, 0, 1, 0), layouts=L3)
    add("strided", 1, 530, 512, 256, (1, 1, 0, 0, 0), layouts=L3)
    add("strided", 1, 8500, 128, 32, (0, 2, 0, 1, 1), pre=128, layouts=L3)
    return cases


CASES = _build()

# LayerNorm / row statistics: (rows, C, profile, strided)
LN_CASES = [(rows, C, p, st) for C in (8, 64, 320, 1280, 2048) for rows in (1, 5, 77, 1001)
            for p, st in (("randn", False), ("randn", True), ("p50", True), ("m30", False))
            if p == "randn" or rows in (5, 1001)]
ROW_STATS_CASES = [(rows, C, p) for C in (8, 320, 2056, 5120) for rows, p in ((1, "randn"), (77, "p50"), (1001, "randn"), (1001, "m30"))]


def ln_id(t):
    return "%dx%d-%s" % (t[0], t[1], t[2]) + ("-strided" if len(t) > 3 and t[3] else "")


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _profile(shape, profile, g):
    r = torch.randn(shape, generator=g)
    if profile == "randn":
        return (r * 1.5 + 0.7).half()
    off = 50.0 if profile == "p50" else -30.0
    return (r * 0.1 + off).half()


def make_inputs(c):
    """x [N, HW, C] fp16, gamma, beta [C] fp32."""
    g = _gen("%d-%d-%d-%d-%s" % (c.N, c.HW, c.C, c.G, c.profile))
    x = _profile((c.N, c.HW, c.C), c.profile, g)
    if c.profile != "randn" and c.G > 1:
        cpg = c.C // c.G
        x[0, :, cpg:2 * cpg] = 50.0 if c.profile == "p50" else -30.0
    gamma = 1.0 + 0.3 * torch.randn(c.C, generator=g)
    beta = 0.3 * torch.randn(c.C, generator=g)
    return x, gamma, beta


def constant_group(c):
    """Channel range of the constant group of image 0, or None."""
    if c.profile == "randn" or c.G == 1:
        return None
    cpg = c.C // c.G
    return cpg, 2 * cpg


def group_stats(x, G):
    """float64 (mean, biased variance) [N, G] of x [N, HW, C]."""
    N, HW, C = x.shape
    xg = x.double().view(N, HW, G, C // G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, var


def half_step(r):
    """Half the fp16 spacing at |r| (the subnormal spacing below 2^-14)."""
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 11)


def _act_and_bound(pre, e_pre, silu):
    if not silu:
        return pre, half_step(pre) + e_pre
    y = pre * torch.sigmoid(pre)
    return y, half_step(y) + 1.1 * e_pre + U * (8.0 + pre.abs()) * y.abs()


def reference(c, x, gamma, beta):
    """(y, bound), float64 [N, HW, C]."""
    mean, var = group_stats(x, c.G)
    cpg = c.C // c.G
    rstd = 1.0 / torch.sqrt(var + c.eps)
    mean_c = mean.repeat_interleave(cpg, dim=1)[:, None, :]
    std_c = var.sqrt().repeat_interleave(cpg, dim=1)[:, None, :]
    sc = (rstd.repeat_interleave(cpg, dim=1) * gamma.double())[:, None, :]
    xd = x.double()
    b = beta.double()
    pre = (xd - mean_c) * sc + b
    e_eval = U * (2 * (xd * sc).abs() + 2 * (mean_c * sc).abs() + (b - mean_c * sc).abs() + pre.abs())
    rho = U * (STAT_R + STAT_RM * mean_c.abs() / std_c.clamp_min(1e-30))
    e_stat = sc.abs() * (STAT_A * U * (mean_c.abs() + std_c)) + (xd - mean_c).abs() * sc.abs() * rho
    return _act_and_bound(pre, e_eval + e_stat, c.silu)


@functools.lru_cache(maxsize=3)
def inputs_and_reference(c):
    x, gamma, beta = make_inputs(c)
    y, bound = reference(c, x, gamma, beta)
    return x, gamma, beta, y, bound


def tile_summaries(x, G, rows):
    """float64 (mean, M2) of every tile of `rows` pixels x group, rounded to fp32: [N, S, G, 2] (what a convolution's
    epilogue leaves), and the float64 values."""
    N, HW, C = x.shape
    S = cdiv(HW, rows)
    out = torch.zeros(N, S, G, 2, dtype=torch.float64)
    for s in range(S):
        t = x[:, s * rows:min(HW, (s + 1) * rows)].double().view(N, -1, G, C // G)
        m = t.mean(dim=(1, 3))
        out[:, s, :, 0] = m
        out[:, s, :, 1] = ((t - m[:, None, :, None]) ** 2).sum(dim=(1, 3))
    return out.float(), out


def error_ratios(got, r, bound):
    """(worst |err| / bound, worst share of the bound's fp32 terms used beyond the fp16 rounding).  The first is close to 1
    for any correct kernel -- among a million elements some fp32 value lies next to a rounding tie -- so the second is
    the informative one: how much of the evaluation and statistics terms the result needed."""
    err = (got.double() - r).abs()
    hs = half_step(r)
    return (err / bound).max().item(), ((err - hs).clamp_min(0) / (bound - hs)).max().item()


SLAB = 4.0


def summary_errors(got, want, n):
    """Worst error of (mean, M2) summaries `got` [..., 2] against their float64 values `want` over n elements each, as
    fractions of SLAB times the bound's statistics terms: the mean within STAT_A u (|mean| + std); M2 = n var within
    twice the relative error granted to rstd, plus n dm^2 for being taken about the rounded mean (all a constant tile
    gets).  SLAB: a single slab's pivot can lie four standard deviations from the slab's mean and nothing averages over
    slabs as in a group's statistics; the emulated statistics kernels reach 1.06 (mean) and 0.91 (M2) of the group
    terms on one slab in 8096 (test_norm_plan asserts half of SLAB times the terms)."""
    got = got.double()
    mean, m2 = want[..., 0], want[..., 1]
    std = (m2 / n).sqrt()
    dm = (got[..., 0] - mean).abs() / (SLAB * STAT_A * U * (mean.abs() + std)).clamp_min(1e-300)
    tol = SLAB * 2 * U * (STAT_R + STAT_RM * mean.abs() / std.clamp_min(1e-30)) * m2 + n * (STAT_A * U * mean.abs()) ** 2
    dq = (got[..., 1] - m2).abs() / tol.clamp_min(1e-300)
    dq = torch.where((m2 == 0) & (got[..., 1] == 0), torch.zeros_like(dq), dq)
    return dm.max().item(), dq.max().item()


def slab_counts(HW, S, rows, cpg):
    return torch.tensor([min(rows, HW - s * rows) * cpg for s in range(S)], dtype=torch.float64)[None, :, None]


def ln_inputs_and_reference(rows, C, profile):
    """x [rows, C] fp16, gamma, beta fp32, float64 y and bound (eps = 1e-5), float64 (mean, M2) per row."""
    g = _gen("ln-%d-%d-%s" % (rows, C, profile))
    x = _profile((rows, C), profile, g)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=1, keepdim=True)
    sc = gamma.double() / torch.sqrt(var + 1e-5)
    pre = (xd - mean) * sc + beta.double()
    e_eval = U * (3 * (pre - beta.double()).abs() + pre.abs())
    # x - mean is formed from the ROUNDED mean: dm enters as with the GroupNorm
    rho = U * (STAT_R + STAT_RM * mean.abs() / var.sqrt().clamp_min(1e-30))
    e_stat = sc.abs() * (STAT_A * U * (mean.abs() + var.sqrt())) + (xd - mean).abs() * sc.abs() * rho
    y, bound = _act_and_bound(pre, e_eval + e_stat, 0)
    return x, gamma, beta, y, bound, torch.cat([mean, var * C], dim=1)


# ---------------------------------------------------------------------------------------- fp32 emulation of the kernels
def _merge(nA, mA, qA, nB, mB, qB):
    """stat_merge (common.h) on float32 arrays; summaries with nB <= 0 count nothing."""
    nB = np.broadcast_to(np.asarray(nB, f32), mA.shape)
    ok = nB > 0
    n = (nA + nB).astype(f32)
    d = (mB - mA).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (nB / n).astype(f32)
    m2 = (mA + d * f).astype(f32)
    q2 = (qA + (qB + ((d * d).astype(f32) * nA).astype(f32) * f).astype(f32)).astype(f32)
    return np.where(ok, n, nA).astype(f32), np.where(ok, m2, mA).astype(f32), np.where(ok, q2, qA).astype(f32)


def _rsqrt(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(f32)


def _butterfly(t):
    """__shfl_xor tree over waves of 64 along the last axis, then the waves added in order: [..., T] -> [...]."""
    T = t.shape[-1]
    t = t.reshape(t.shape[:-1] + (T // 64, 64))
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        t = (t + t[..., idx ^ off]).astype(f32)
    w = t[..., 0]
    acc = np.zeros(w.shape[:-1], f32)
    for i in range(w.shape[-1]):
        acc = (acc + w[..., i]).astype(f32)
    return acc


def _slabs(x, S, rows, rows_par):
    """x [N, HW, cw] -> [N, S, steps, rows_par, cw] (zero padded) and the validity mask [S, steps, rows_par]."""
    N, HW, cw = x.shape
    steps = cdiv(rows, rows_par)
    buf = np.zeros((N, S, steps * rows_par, cw), f32)
    ok = np.zeros((S, steps * rows_par), bool)
    for s in range(S):
        n = min(HW, (s + 1) * rows) - s * rows
        buf[:, s, :n] = x[:, s * rows:s * rows + n]
        ok[s, :n] = True
    return buf.reshape(N, S, steps, rows_par, cw), ok.reshape(S, steps, rows_par)


def emu_stats2(x, S, rows, CB, G):
    """gn_stats2_kernel: part [N, S, G, 2] float32 from x [N, HW, C] float32."""
    N, HW, C = x.shape
    cpg = C // G
    part = np.zeros((N, S, G, 2), f32)
    cnt = np.array([min(HW, (s + 1) * rows) - s * rows for s in range(S)], f32) * f32(cpg)
    for c0 in range(0, C, CB):
        cw = min(CB, C - c0)
        CCB = cw // 8
        rows_par = 256 // CCB
        v, ok = _slabs(x[:, :, c0:c0 + cw], S, rows, rows_par)
        steps = v.shape[2]
        ch = np.arange(cw)
        piv = v[:, :, 0, 0, (ch // cpg) * cpg]                             # [N, S, cw]: the group's first channel at the slab's first pixel
        f = (v - piv[:, :, None, None, :]).astype(f32) * ok[None, :, :, :, None]
        f = f.reshape(N, S, steps, rows_par, CCB, 8)
        gA = (np.arange(CCB) * 8) // cpg
        split = (gA + 1) * cpg - np.arange(CCB) * 8
        acc = np.zeros((4, N, S, rows_par, CCB), f32)                       # sa, qa, sb, qb
        for st in range(steps):
            for e in range(8):
                fe = f[:, :, st, :, :, e]
                first = (e < split)[None, None, None, :]
                acc[0] = (acc[0] + np.where(first, fe, 0)).astype(f32)
                acc[1] = (acc[1] + np.where(first, fe * fe, 0).astype(f32)).astype(f32)
                acc[2] = (acc[2] + np.where(first, 0, fe)).astype(f32)
                acc[3] = (acc[3] + np.where(first, 0, fe * fe).astype(f32)).astype(f32)
        for g in range(cw // cpg):
            sm = np.zeros((N, S), f32)
            sq = np.zeros((N, S), f32)
            for c8 in range((g * cpg) // 8, ((g + 1) * cpg - 1) // 8 + 1):
                off = 0 if (c8 * 8) // cpg == g else 2
                for r in range(rows_par):
                    sm = (sm + acc[off, :, :, r, c8]).astype(f32)
                    sq = (sq + acc[off + 1, :, :, r, c8]).astype(f32)
            d = (sm / cnt[None, :]).astype(f32)
            part[:, :, c0 // cpg + g, 0] = (piv[:, :, g * cpg] + d).astype(f32)
            part[:, :, c0 // cpg + g, 1] = (sq - (sm * d).astype(f32)).astype(f32)
    return part


def emu_stats1(x, S, rows, CB, G):
    """gn_stats_kernel: a pivot per (thread, channel), then Chan merges over pixel rows and the group's channels."""
    N, HW, C = x.shape
    cpg = C // G
    part = np.zeros((N, S, G, 2), f32)
    per = np.array([min(HW, (s + 1) * rows) - s * rows for s in range(S)], f32)
    for c0 in range(0, C, CB):
        cw = min(CB, C - c0)
        rows_par = 256 // (cw // 8)
        v, ok = _slabs(x[:, :, c0:c0 + cw], S, rows, rows_par)
        steps = v.shape[2]
        piv = v[:, :, 0]                                                   # [N, S, rows_par, cw]
        sm = np.zeros_like(piv)
        sq = np.zeros_like(piv)
        for st in range(steps):
            f = (v[:, :, st] - piv).astype(f32) * ok[None, :, st, :, None]
            sm = (sm + f).astype(f32)
            sq = (sq + (f * f).astype(f32)).astype(f32)
        cnt = ok.sum(axis=1).astype(f32)                                   # [S, rows_par]
        icnt = np.where(cnt > 0, f32(1) / np.maximum(cnt, 1), 0).astype(f32)
        d = (sm * icnt[None, :, :, None]).astype(f32)
        m = (piv + d).astype(f32)
        q = (sq - (sm * d).astype(f32)).astype(f32)
        nA = np.broadcast_to(cnt[None, :, 0, None], m[:, :, 0].shape).astype(f32)
        mA, qA = m[:, :, 0], q[:, :, 0]
        for r in range(1, rows_par):
            nA, mA, qA = _merge(nA, mA, qA, np.broadcast_to(cnt[None, :, r, None], mA.shape), m[:, :, r], q[:, :, r])
        pc = np.broadcast_to(per[None, :, None], (N, S, cw // cpg)).astype(f32)
        mA = mA.reshape(N, S, cw // cpg, cpg)
        qA = qA.reshape(N, S, cw // cpg, cpg)
        n, mg, qg = pc, mA[..., 0], qA[..., 0]
        for k in range(1, cpg):
            n, mg, qg = _merge(n, mg, qg, pc, mA[..., k], qA[..., k])
        part[:, :, c0 // cpg:c0 // cpg + cw // cpg, 0] = mg
        part[:, :, c0 // cpg:c0 // cpg + cw // cpg, 1] = qg
    return part


def _tile_counts(S, rows, HW, cpg):
    return np.array([(min(rows, HW - k * rows)) * cpg for k in range(S)], f32)


def _merge_strided(part, counts, parts):
    """`parts` threads per group merge the summaries k = pi, pi + parts, ... in order, thread 0 then merges the threads':
    the prologue of gn_apply_kernel, of gn_apply2_kernel's ragged path, and gn_finalize_kernel.  part [N, S, g, 2]."""
    N, S, g, _ = part.shape
    J = cdiv(S, parts)
    pm = np.zeros((N, J * parts, g), f32)
    pq = np.zeros((N, J * parts, g), f32)
    pn = np.zeros((J * parts,), f32)
    pm[:, :S], pq[:, :S], pn[:S] = part[..., 0], part[..., 1], counts
    pm, pq, pn = pm.reshape(N, J, parts, g), pq.reshape(N, J, parts, g), pn.reshape(J, parts)
    nA = np.zeros((N, parts, g), f32)
    mA, qA = np.zeros_like(nA), np.zeros_like(nA)
    for j in range(J):
        nA, mA, qA = _merge(nA, mA, qA, np.broadcast_to(pn[None, j, :, None], nA.shape), pm[:, j], pq[:, j])
    n, m, q = nA[:, 0], mA[:, 0], qA[:, 0]
    for k in range(1, parts):
        n, m, q = _merge(n, m, q, nA[:, k], mA[:, k], qA[:, k])
    return m, q


def _finish(mean, m2, HW, cpg, eps, count_bug=False, rcp=False):
    n = f32((HW - 1 if count_bug else HW)) * f32(cpg)
    var = (m2 * (f32(1) / n)).astype(f32) if rcp else (m2 / n).astype(f32)
    return mean, _rsqrt((np.maximum(var, 0) + f32(eps)).astype(f32))


def emu_merge(part, S, rows, HW, C, G, CB, apply, eps, mutation=None):
    """The apply kernels' prologue: summaries -> (mean, rstd) [N, G] float32."""
    cpg = C // G
    if mutation == "drop" and S >= 2:
        keep = [k for k in range(S) if k != 1]
    else:
        keep = list(range(S))
    counts = _tile_counts(S, rows, HW, cpg)
    cb = mutation == "count"
    if apply == 1:
        m, q = _merge_strided(part[:, keep], counts[keep], 256 // G)
        return _finish(m, q, HW, cpg, eps, cb)
    N = part.shape[0]
    mean = np.zeros((N, G), f32)
    rstd = np.zeros((N, G), f32)
    equal = HW % rows == 0
    for c0 in range(0, C, CB):
        cw = min(CB, C - c0)
        ng, g0 = cw // cpg, c0 // cpg
        p = part[:, :, g0:g0 + ng]
        if not equal:
            m, q = _merge_strided(p[:, keep], counts[keep], 256 // ng)
            mean[:, g0:g0 + ng], rstd[:, g0:g0 + ng] = _finish(m, q, HW, cpg, eps, cb)
            continue
        pk = p[:, keep]
        Sm = len(keep)
        if mutation == "empty":                      # one more summary, of no rows (zeros), merged like the others
            pk = np.concatenate([pk, np.zeros_like(pk[:, :1])], axis=1)
            Sm += 1
        LW = 1 if (Sm * ng <= 128 and ng <= 64) else 4
        parts1 = 64 * LW // ng
        J = cdiv(Sm, parts1)
        pivot = pk[:, 0, :, 0]
        d = np.zeros((N, J * parts1, ng), f32)
        qq = np.zeros((N, J * parts1, ng), f32)
        d[:, :Sm] = (pk[..., 0] - pivot[:, None, :]).astype(f32)
        qq[:, :Sm] = pk[..., 1]
        d, qq = d.reshape(N, J, parts1, ng), qq.reshape(N, J, parts1, ng)
        sa = np.zeros((N, parts1, ng), f32)
        sb, sq = np.zeros_like(sa), np.zeros_like(sa)
        for j in range(J):
            sa = (sa + d[:, j]).astype(f32)
            sb = (sb + (d[:, j] * d[:, j]).astype(f32)).astype(f32)
            sq = (sq + qq[:, j]).astype(f32)
        ta = np.zeros((N, ng), f32)
        tb, tq = np.zeros_like(ta), np.zeros_like(ta)
        for k in range(parts1):
            ta = (ta + sa[:, k]).astype(f32)
            tb = (tb + sb[:, k]).astype(f32)
            tq = (tq + sq[:, k]).astype(f32)
        dm = (ta * (f32(1) / f32(Sm))).astype(f32)
        cnt = f32(rows) * f32(cpg)
        m2 = (tq + (cnt * (tb - (ta * dm).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        mean[:, g0:g0 + ng], rstd[:, g0:g0 + ng] = _finish((pivot + dm).astype(f32), m2, HW, cpg, eps, cb, rcp=True)
    return mean, rstd


def emu_finalize(part, S, rows, HW, cpg):
    """gn_finalize_kernel: [N, S, G, 2] -> [N, 1, G, 2]."""
    m, q = _merge_strided(part, _tile_counts(S, rows, HW, cpg), 256)
    return np.stack([m, q], axis=-1)[:, None]


def fused_unit(C, G):
    cpg = C // G
    unit = cpg
    while unit % 8:
        unit += cpg
    return unit


def emu_fused(x, G, T, NV, eps, count_bug=False):
    """gn_fused_kernel<T, NV>: (mean, rstd) [N, G] float32; the panel in registers, two reductions."""
    N, HW, C = x.shape
    cpg = C // G
    Un = fused_unit(C, G)
    UC, B = Un // 8, C // Un
    PL = T // UC
    tid = np.arange(T)
    cchunk, plane = tid % UC, tid // UC
    active = plane < PL
    gA = (cchunk * 8) // cpg
    split = (gA + 1) * cpg - cchunk * 8
    pix = plane[:, None] + np.arange(NV)[None, :] * PL                    # [T, NV]
    ok = active[:, None] & (pix < HW)
    chan = cchunk[:, None] * 8 + np.arange(8)[None, :]                     # [T, 8]
    xb = x.reshape(N, HW, B, Un)
    v = xb[:, np.minimum(pix, HW - 1)[:, :, None], :, chan[:, None, :]]    # [T, NV, 8, N, B] (advanced indices first)
    v = np.moveaxis(v, (3, 4), (0, 1)) * ok[None, None, :, :, None]        # [N, B, T, NV, 8]
    v = v.astype(f32)
    first = np.arange(8)[None, :] < split[:, None]                         # [T, 8]
    s2 = np.zeros((N, B, T, 4), f32)
    for k in range(NV):
        pr = (v[:, :, :, k, 0::2] + v[:, :, :, k, 1::2]).astype(f32)
        s2 = (s2 + pr).astype(f32)
    a = np.zeros((N, B, T), f32)
    b = np.zeros((N, B, T), f32)
    for j in range(4):
        fj = first[:, 2 * j][None, None, :]
        a = (a + np.where(fj, s2[..., j], 0)).astype(f32)
        b = (b + np.where(fj, 0, s2[..., j])).astype(f32)
    cnt = f32(HW) * f32(cpg)

    def reduce4(a, b):
        out = np.zeros((N, B, 4), f32)
        for g in range(4):
            t = (np.where(gA == g, a, 0) + np.where(gA + 1 == g, b, 0)).astype(f32)
            out[..., g] = _butterfly(t)
        return out

    mean4 = (reduce4(a, b) / cnt).astype(f32)                             # [N, B, 4]
    mA = mean4[:, :, gA & 3]                                               # [N, B, T]
    mB = mean4[:, :, (gA + 1) & 3]
    qa = np.zeros((N, B, T), f32)
    qb = np.zeros((N, B, T), f32)
    for k in range(NV):
        for e in range(8):
            fe = first[:, e][None, None, :]
            dl = (v[:, :, :, k, e] - np.where(fe, mA, mB)).astype(f32)
            dd = (dl * dl).astype(f32) * ok[None, None, :, k]
            qa = (qa + np.where(fe, dd, 0)).astype(f32)
            qb = (qb + np.where(fe, 0, dd)).astype(f32)
    n2 = f32(HW - 1 if count_bug else HW) * f32(cpg)
    var4 = (reduce4(qa, qb) / n2).astype(f32)
    gpu = Un // cpg
    mean = mean4[:, :, :gpu].reshape(N, G)
    rstd = _rsqrt((var4[:, :, :gpu] + f32(eps)).astype(f32)).reshape(N, G)
    return mean, rstd


def emu_apply(x, mean, rstd, gamma, beta, silu, G, mutation=None, CB=0):
    """y = act(x sc + sh) in float32, rounded to fp16: [N, HW, C] torch.float16."""
    N, HW, C = x.shape
    cpg = C // G
    grp = np.arange(C) // cpg
    if mutation == "group":                         # a chunk that straddles two groups takes its first group's statistics
        grp = ((np.arange(C) // 8) * 8) // cpg
    ga, be = gamma.numpy().astype(f32), beta.numpy().astype(f32)
    if mutation == "gb":                            # the affine of the neighbouring channel block
        ga, be = np.roll(ga, CB), np.roll(be, CB)
    sc = (rstd[:, grp] * ga[None, :]).astype(f32)
    sh = (be[None, :] - (mean[:, grp] * sc).astype(f32)).astype(f32)
    f = ((x * sc[:, None, :]).astype(f32) + sh[:, None, :]).astype(f32)
    if silu:
        with np.errstate(over="ignore"):
            f = (f * (f32(1) / (f32(1) + np.exp2((f32(-1.4426950408889634) * f).astype(f32)).astype(f32)))).astype(f32)
    return torch.from_numpy(f).half()


def emulate_stats(c, plan, x, mutation=None):
    """(mean, rstd) [N, G] float32 as the kernels of `plan` (sd_norm_plan's out) compute them."""
    stats, apply, T, NV, fin, S, rows, CB = plan[:8]
    xf = x.numpy().astype(f32)
    cpg = c.C // c.G
    if mutation == "ex2":                           # variance as E[x^2] - mean^2 in float32
        xg = xf.reshape(c.N, c.HW, c.G, cpg)
        m = xg.mean(axis=(1, 3), dtype=f32)
        var = ((xg * xg).astype(f32).mean(axis=(1, 3), dtype=f32) - (m * m).astype(f32)).astype(f32)
        return m, _rsqrt((np.maximum(var, 0) + f32(c.eps)).astype(f32))
    if apply == 0:
        return emu_fused(xf, c.G, T, NV, c.eps, count_bug=mutation == "count")
    if stats == 0:
        part, rows = tile_summaries(x, c.G, c.pre)[0].numpy(), c.pre
    else:
        part = (emu_stats2 if stats == 2 else emu_stats1)(xf, S, rows, CB, c.G)
    if fin:
        part, S, rows = emu_finalize(part, S, rows, c.HW, cpg), 1, c.HW
    return emu_merge(part, S, rows, c.HW, c.C, c.G, CB, apply, c.eps, mutation)


def mutation_applies(c, plan, mutation):
    stats, apply, T, NV, fin, S, rows, CB = plan[:8]
    if c.pre and apply:
        rows = c.pre
    if mutation == "drop":
        return apply != 0 and not fin and S >= 2
    if mutation == "empty":
        return apply == 2 and not fin and c.HW % rows == 0
    if mutation == "group":
        return (c.C // c.G) % 8 != 0
    if mutation == "ex2":
        return c.profile == "p50"
    if mutation == "gb":
        return CB < c.C
    return mutation == "count"


def emulate(c, plan, x, gamma, beta, mutation=None):
    mean, rstd = emulate_stats(c, plan, x, mutation)
    return emu_apply(x.numpy().astype(f32), mean, rstd, gamma, beta, c.silu, c.G, mutation, plan[7])


def emulate_layernorm(x, gamma, beta, eps=1e-5):
    """layernorm_kernel: one wave per row, lane sums in chunk order, xor tree; ((x - mean) rstd) gamma + beta."""
    xf = x.numpy().astype(f32)
    rows, C = xf.shape
    CC = C // 8
    NI = cdiv(CC, 64)                               # chunks per lane (layernorm_kernel: at most four; row_stats_kernel: any)
    lanes = np.zeros((rows, 64, NI, 8), f32)
    ok = np.zeros((64, NI), bool)
    for i in range(NI):
        for lane in range(64):
            cc = lane + 64 * i
            if cc < CC:
                lanes[:, lane, i] = xf[:, cc * 8:cc * 8 + 8]
                ok[lane, i] = True
    sm = np.zeros((rows, 64), f32)
    for i in range(NI):
        for e in range(8):
            sm = (sm + lanes[:, :, i, e]).astype(f32)
    mean = (_butterfly(sm) / f32(C)).astype(f32)
    sq = np.zeros((rows, 64), f32)
    for i in range(NI):
        for e in range(8):
            d = (lanes[:, :, i, e] - mean[:, None]).astype(f32) * ok[None, :, i]
            sq = (sq + (d * d).astype(f32)).astype(f32)
    m2 = _butterfly(sq)
    rstd = _rsqrt(((m2 / f32(C)).astype(f32) + f32(eps)).astype(f32))
    f = (((xf - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32) * gamma.numpy()[None, :]).astype(f32)
    f = (f + beta.numpy()[None, :]).astype(f32)
    return torch.from_numpy(f).half(), mean, m2
