"""Cases, operands, float64 reference and element-wise bound shared by tests/test_ln_plan.py (CPU) and
tests/test_ln_gpu.py (GPU) for the folded-LayerNorm chain: a GEMM leaves per-row (mean, M2) parts of what it stores
(IGemmParams::rowstat_out), ln_row_stats (csrc/common.h) merges them, and the next GEMM's epilogue applies
(acc - mean * wsum) * rstd + b' on weights that carry the norm's affine (IGemmParams::ln_stat).  Nothing here touches a
device; the reference helpers run on whatever device their operands live on.

Consumers (sd_op_ln_linear, sd_op_ln_ffn_geglu) take the statistics and their layout (parts, part_w) from the caller, so
the cases hand them float64 statistics of the fp16 input rounded to fp32, in layouts no producer emits today.  A case
names the kernel it was written for; the CPU suite checks that sd_igemm_plan agrees.

Profiles of the consumer input x [M, C] (all fp16 numbers)
  rows       row r has its own level and spread: mean_r = -4 + 8 ((37 r) mod 101) / 100, std_r = 0.25 * 16 ^ (((29 r) mod
             53) / 52), so neighbours and rows 16 / 32 / 64 / 128 apart differ; each block of 16 columns is shifted by
             std_r * N(0, 1), so every statistics part sits at a level of its own and the n_k weights of the merge matter
  offset:50  rows 50 +- 0.1 (the 16-column blocks shifted by 0.05 N(0, 1))
  spikes     N(0, 1) rows with four channels at +-300

The bound, per output (m, n) ahead of any rounding to fp16, from the reference alone.  The pack-time fold is W_f =
fp16(W gamma s) (s = row_scale on the first rows_scaled outputs), wsum = sum_k W_f, b' = s (b + W beta); with S_n =
sum_k |W_f[n, k]|, A = sum_k |W_f[n, k]| |x[m, k]|, u32 = 2^-23 (one bit wider than round-to-nearest, as in conv_cases):
  rstd_m (K + 3) u32 (A + |mean_m| S_n)        K fp32 accumulations of exact products, no partial sum above A; the
                                               product mean * wsum, the subtraction and the multiplication by rstd
                                               (where rows of large offset lose digits: both terms are ~ |mean| S)
  rstd_m K u32 |mean_m| S_n                    wsum: an fp32 sum of K fp16 values in any order
  rstd_m e_mean S_n                            the merged mean: e_mean = (parts + 3) u32 max_k |mean_k| (the supplied part
                                               means rounded to fp32, n_k mean_k, parts - 1 additions, the factor 1 / C)
  |v - b'| rel_rstd                            rstd: the merged M2 is off by at most sum_k n_k (2 |d_k| e_d + e_d^2) +
                                               (parts + 4) u32 M2, d_k = mean_k - mean, e_d = e_mean + u32 max_k |mean_k|;
                                               rel_rstd = half the relative error of M2 / C + eps (its two roundings
                                               included) + 3 u32 for rsqrtf
  rstd_m (u16 + 2 u32) sum_k |W gamma s| |x - mean|     the fold's one rounding to fp16 (after two in fp32), and
  rstd_m 2^-25 sum_k |x - mean|                         its absolute form for folded weights in the subnormal range
  (K + 3) u32 s (|b| + sum_k |W| |beta|)       b' in fp32: K products, their sum in any order, + b, * s
  u32 |v|                                      the final addition of b'
plain outputs add u16 |v| + 2^-25 for the stored fp16; GEGLU takes the two halves through conv_cases.geglu_reference;
ffn_fused_kernel's extension is at reference_ffn.  tests/test_ln_plan.py holds an fp32 emulation of the kernels against
this bound and shows that it is tight enough to see the defects it is for."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import conv_cases as cc

U16, U32 = cc.U16, cc.U32
EPS = 1e-5
MAX_PARTS = 20                  # kMaxLnParts (igemm2.hip), kG3MaxLnParts, kPgMaxLnParts, kFfMaxLnParts
WS_MAX_PARTS = 4                # kWsStatParts (wsgemm.hip)
PROFILES = ("rows", "offset:50", "spikes")
OVER_CAPACITY = ((1344, 21, 64), (320, 40, 8))          # (C, parts, part_w) the consumers must refuse

L320 = ((1, 320), (2, 160), (4, 80), (5, 64), (20, 16), (3, 128), (7, 48))      # (3, 128): 128 | 128 | 64; (7, 48): .. | 32
L640 = ((1, 640), (2, 320), (4, 160), (10, 64), (20, 32), (3, 256), (7, 96))    # (3, 256): .. | 128; (7, 96): .. | 64
L1280 = ((20, 64), (1, 1280), (7, 192))                                         # exactly the capacity; (7, 192): .. | 128
LWS = ((1, 320), (2, 160), (3, 128), (4, 80))

Consumer = collections.namedtuple("Consumer", "family entry M C O geglu force want avoid runs")
# family   the kernel family the case is written for (the summary's list)
# entry    "linear": sd_op_ln_linear, "ffn": sd_op_ln_ffn_geglu (O unused: the hidden width is 4 C)
# O        stored output columns (the GEMM has 2 O under geglu)
# force    (variant, splits) for sd_igemm_force, or None
# want     the `consumer` id the entry must report (ffn: the `fused` flag), None where only `avoid` is asserted
# avoid    ids the entry must not report: the layout is beyond that kernel's capacity and the launch has to land elsewhere
# runs     ((parts, part_w), profile) pairs the GPU suite runs

Producer = collections.namedtuple("Producer", "family M K C res force want parts part_w")
# want     the `producer` id sd_op_linear_rowstats must report (-1: row_stats_kernel), parts / part_w the layout

Chain = collections.namedtuple("Chain", "name prod O geglu force want")
# a producer feeding a consumer of another family; force / want are the consumer's


def _runs(layouts, extra=(), extra_profiles=("offset:50", "spikes")):
    return tuple((lay, "rows") for lay in layouts) + tuple((lay, p) for lay in extra for p in extra_profiles)


def _build_consumers():
    cs = []

    def add(family, entry, M, C, O, geglu, force, want, runs, avoid=()):
        cs.append(Consumer(family, entry, M, C, O, geglu, force, want, tuple(avoid), tuple(runs)))

    # ---- igemm2 streamed tiles, forced: a 64-, a 128- and a 160-column tile (variants 3, 1, 2); igemm2_supported asks
    #      K % 64 == 0 and Cout % 8 == 0 only, so M = 130 and 257 put rows m >= M of the last 128-row tile on the
    #      clamped-index path; O = 192 leaves the 160-column tile a ragged second column tile, O = 320 the 128-column one
    for v, O in ((3, 192), (1, 320), (2, 192)):
        add("tile", "linear", 130, 320, O, 0, (v, 1), v, _runs(L320, (L320[3], L320[6])))
        add("tile", "linear", 257, 640, O, 0, (v, 1), v, _runs(L640, (L640[3], L640[6])))
        add("tile", "linear", 130, 1280, O, 0, (v, 1), v, _runs(L1280, (L1280[0],)))
    # ---- their GEGLU epilogue: the 128 x 128 and the 256 x 128 tile (variants 1, 0; Cout % 128 == 0)
    for v in (1, 0):
        add("tile-geglu", "linear", 130, 320, 192, 1, (v, 1), v, _runs(L320, (L320[3], L320[6])))
        add("tile-geglu", "linear", 257, 640, 192, 1, (v, 1), v, _runs(L640, (L640[3], L640[6])))
    add("tile-geglu", "linear", 130, 1280, 192, 1, (1, 1), 1, _runs(L1280, (L1280[0],)))
    # ---- igemm3 (force 18; igemm3_supported: pointwise, K >= 64 * G3_STAGES = 256, no GEGLU): C = 320 = 64 * G3_STAGES +
    #      64, one slab past the ring, and 1280; 192 columns = 80 | 80 | 32
    add("igemm3", "linear", 130, 320, 192, 0, (cc.REG, 1), cc.REG, _runs(L320, (L320[3], L320[6])))
    add("igemm3", "linear", 1000, 1280, 192, 0, (cc.REG, 1), cc.REG, _runs(L1280, (L1280[0],)))
    # ---- wsgemm with the LayerNorm (wsgemm_supported: K = 320, M % 128 == 0, M / 128 >= 8, parts <= 4; plain Cout % 160
    #      == 0 -> 13, GEGLU Cout % 128 == 0 -> 14), unforced as the UNet reaches it.  The launcher starts 32 blocks per
    #      XCD; XCD i owns M tiles [8 i tiles_m / 8 ..), its blocks cut the (n tile, m tile) list of L = tiles_n * nm
    #      entries into 32 contiguous runs, and a run walks consecutive M tiles of one N tile.
    #        M = 1024: the minimum, nm = 1, one tile per run
    #        M = 4096: nm = 4 and tiles_n = 24, L = 96: every block owns three entries, the runs starting at m tile 0 and 1
    #                  of an N tile walk three tiles, so both LDS statistics buffers are used again
    #        M = 1152: nine M tiles over eight XCDs (one owns two), L = 2 .. 6 over 32 blocks: most blocks idle
    #      The entry wants O % 64 == 0: the narrowest plain output is 320 columns (two N tiles), the narrowest GEGLU one
    #      128 (one N tile of [64 hidden | 64 gate]).
    for geglu, o_min, o_run3, o_uneven, want in ((0, 320, 3840, 320, 13), (1, 128, 1536, 192, 14)):
        add("wsgemm", "linear", 1024, 320, o_min, geglu, None, want, _runs(LWS, (LWS[2], LWS[3])))
        add("wsgemm", "linear", 4096, 320, o_run3, geglu, None, want, _runs(LWS))
        add("wsgemm", "linear", 1152, 320, o_uneven, geglu, None, want, _runs((LWS[1], LWS[2])))
        # five parts: beyond kWsStatParts, the kernel has to decline and the result still be right
        add("wsgemm-declines", "linear", 1024, 320, o_min, geglu, None, None, _runs((L320[3],)), avoid=(13, 14))
    # ---- geglu_persist_kernel (pgemm_geglu_supported: M % 256 == 0, Cout % 128 == 0, K >= 128, (M / 256) * (2 O / 128) >=
    #      512), unforced, O = 4 C: C = 640 -> 40 N tiles, M = 13 * 256 (12 * 40 = 480 is short); C = 1280 -> 80 N tiles,
    #      M = 7 * 256.  The launcher gives an M tile 256 / tiles_m blocks: 19 over 40 N tiles, 36 over 80 -- both ragged.
    #      At C = 320 the plan sends up to four parts to wsgemm, so only longer layouts reach this kernel there
    #      (20 N tiles, M = 26 * 256, 9 blocks over 20 N tiles).
    add("pgemm", "linear", 3328, 640, 2560, 1, None, 100, _runs(L640, (L640[3],)))
    add("pgemm", "linear", 1792, 1280, 5120, 1, None, 100, _runs(L1280[:2], (L1280[0],), ("offset:50",)))
    add("pgemm", "linear", 6656, 320, 1280, 1, None, 100, _runs((L320[3], L320[4], L320[6])))
    # ---- ffn_fused_kernel (ffn_fused_supported: C = 320, M % 128 == 0, M / 128 >= 64, parts <= 20): 64 and 65 blocks
    add("ffn", "ffn", 8192, 320, 0, 1, None, 1, _runs(L320, (L320[3], L320[6])))
    add("ffn", "ffn", 8320, 320, 0, 1, None, 1, _runs((L320[1], L320[6])))
    return cs


CONSUMERS = _build_consumers()
CONSUMER_FAMILIES = {"tile", "tile-geglu", "igemm3", "wsgemm", "wsgemm-declines", "pgemm", "ffn"}


def _build_producers():
    ps = []
    for res in (False, True):
        # igemm2 tile epilogue, one part per column tile; C = 200 leaves 64-column tiles an 8-column and 160-column
        # tiles a 40-column last part, C = 320 leaves 128-column tiles a 64-column one; M ragged
        ps.append(Producer("tile", 130, 128, 200, res, (3, 1), 3, 4, 64))
        ps.append(Producer("tile", 257, 128, 320, res, (1, 1), 1, 3, 128))
        ps.append(Producer("tile", 130, 128, 200, res, (2, 1), 2, 2, 160))
        # wsgemm (K = 320, M % 128 == 0, M / 128 >= 8, Cout % 160 == 0): one part per 80 columns
        ps.append(Producer("wsgemm", 1024, 320, 320, res, (13, 1), 13, 4, 80))
        # igemm3 (K >= 256): 80-column tiles, C = 200 -> 80 | 80 | 40
        ps.append(Producer("igemm3", 130, 320, 200, res, (cc.REG, 1), cc.REG, 3, 80))
        # a split-K launch leaves no statistics: row_stats_kernel over the stored y1, one part
        ps.append(Producer("row_stats", 130, 256, 200, res, (3, 2), -1, 1, 200))
    return ps


PRODUCERS = _build_producers()
PRODUCER_PROFILES = ("normal", "offset:50")

# one chain per producer family into a consumer of another family (M = 1024 and K = C = 320 so that wsgemm takes either side)
CHAINS = [
    Chain("wsgemm->igemm3", Producer("wsgemm", 1024, 320, 320, False, (13, 1), 13, 4, 80), 192, 0, (cc.REG, 1), cc.REG),
    Chain("tile->wsgemm", Producer("tile", 1024, 320, 320, True, (1, 1), 1, 3, 128), 320, 0, None, 13),
    Chain("igemm3->tile-geglu", Producer("igemm3", 1024, 320, 320, True, (cc.REG, 1), cc.REG, 4, 80), 192, 1, (1, 1), 1),
    Chain("row_stats->wsgemm-geglu", Producer("row_stats", 1024, 320, 320, True, (3, 2), -1, 1, 320), 128, 1, None, 14),
]


def consumer_id(c):
    s = "%s-%s-m%d-c%d-o%d%s" % (c.family, c.entry, c.M, c.C, c.O, "-geglu" if c.geglu else "")
    return s + ("-f%d,%d" % c.force if c.force else "-auto")


def run_id(c, lay, profile):
    return "%s-%dx%d-%s" % (consumer_id(c), lay[0], lay[1], profile)


def producer_id(p):
    return "%s-m%d-k%d-c%d%s-f%d,%d" % (p.family, p.M, p.K, p.C, "-res" if p.res else "", p.force[0], p.force[1])


def consumer_plan_args(c, parts):
    """geom[9], flags[10] of sd_igemm_plan for a consumer launch with `parts` statistics parts."""
    return (1, c.M, 1, c.C, (2 if c.geglu else 1) * c.O, 1, 1, 0, -1), (c.geglu, 0, 0, 0, 1, parts, 0, 0, 0, 0)


def producer_plan_args(p):
    return (1, p.M, 1, p.K, p.C, 1, 1, 0, -1), (0, 0, int(p.res), 0, 1, 0, 1, 0, 0, 0)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def row_scaling(c):
    """(rows_scaled, row_scale) of a consumer case: the q of q|k|v on the plain linears."""
    return (0, 1.0) if c.geglu or c.entry == "ffn" else (64, float(torch.tensor((c.C // 8) ** -0.5, dtype=torch.float32)))


def make_x(M, C, profile, g):
    r = torch.arange(M)
    lvl = torch.randn(C // 16, generator=g).repeat_interleave(16)
    noise = torch.randn(M, C, generator=g)
    if profile == "rows":
        mean = -4.0 + 8.0 * ((37 * r) % 101).float() / 100.0
        std = 0.25 * 16.0 ** (((29 * r) % 53).float() / 52.0)
        x = mean[:, None] + std[:, None] * (lvl[None, :] + noise)
    elif profile == "offset:50":
        x = 50.0 + 0.1 * (0.5 * lvl[None, :] + noise)
    else:
        assert profile == "spikes", profile
        x = noise
        for i, ch in enumerate((3, C // 3, C // 2 + 5, C - 2)):
            x[:, ch] = 300.0 if i % 2 == 0 else -300.0
    return x.half()


Operands = collections.namedtuple("Operands", "x gamma beta w1 b1 w2 b2 rows_scaled row_scale")


@functools.lru_cache(maxsize=2)
def consumer_operands(c, profile):
    """The operands of a consumer case on the CPU (x fp16 [M, C], gamma / beta fp32, w1 fp16 [cols, C], b1 fp32; ffn: w1
    [8 C, C], w2 [C, 4 C] scaled up so that the branch stands above the fp16 step of the residual stream); not to be
    modified."""
    g = torch.Generator().manual_seed(_seed(c.entry, c.M, c.C, c.O, c.geglu, profile))
    x = make_x(c.M, c.C, profile, g)
    gamma = 1.0 + 0.2 * torch.randn(c.C, generator=g)
    beta = 0.2 * torch.randn(c.C, generator=g) + 0.05
    cols = 8 * c.C if c.entry == "ffn" else (2 if c.geglu else 1) * c.O
    w1 = (torch.randn(cols, c.C, generator=g) / c.C ** 0.5).half()
    b1 = 0.2 * torch.randn(cols, generator=g)
    w2 = b2 = None
    if c.entry == "ffn":
        w2 = (30.0 * torch.randn(c.C, 4 * c.C, generator=g) / (4 * c.C) ** 0.5).half()
        b2 = 0.2 * torch.randn(c.C, generator=g)
    return Operands(x, gamma, beta, w1, b1, w2, b2, *row_scaling(c))


def part_widths(C, lay):
    parts, w = lay
    assert parts * w >= C > (parts - 1) * w, (C, lay)
    return [min(w, C - k * w) for k in range(parts)]


def part_stats(x, lay):
    """float64 (mean_k, M2_k) of each part of each row: two [M, parts] tensors on x's device."""
    xd = x.double()
    means, m2s = [], []
    for k, n in enumerate(part_widths(x.shape[1], lay)):
        seg = xd[:, k * lay[1]:k * lay[1] + n]
        m = seg.mean(1)
        means.append(m)
        m2s.append(((seg - m[:, None]) ** 2).sum(1))
    return torch.stack(means, 1), torch.stack(m2s, 1)


def supplied_stats(x, lay):
    """What the host hands a consumer: the float64 part statistics rounded to fp32, [M, parts, 2]."""
    mk, qk = part_stats(x, lay)
    return torch.stack((mk, qk), 2).float().contiguous()


def folded_weight(w, gamma, scale):
    """ln_fold_kernel's weight: fp16(w * gamma * s) with the two products in fp32."""
    return (w.float() * gamma.float()[None, :] * scale.float()[:, None]).half()


def _scale_vector(cols, rows_scaled, row_scale, device):
    s = torch.ones(cols, dtype=torch.float32, device=device)
    s[:rows_scaled] = row_scale
    return s


def linear_terms(x, gamma, beta, w, b, rows_scaled, row_scale):
    """float64, on x's device: the exact projection v = s (LayerNorm(x) W^T + b) [M, cols] and the parts of the bound that
    do not depend on the statistics layout: (v, base, P = |v - b'|, rstd [M], S [cols])."""
    dev = x.device
    xd, wd, gd, bed, bd = x.double(), w.to(dev).double(), gamma.to(dev).double(), beta.to(dev).double(), b.to(dev).double()
    K = xd.shape[1]
    s32 = _scale_vector(wd.shape[0], rows_scaled, row_scale, dev)
    s = s32.double()
    mean = xd.mean(1)
    xc = xd - mean[:, None]
    rstd = ((xc ** 2).mean(1) + EPS).rsqrt()
    v = (F.linear(xc * rstd[:, None] * gd + bed, wd) + bd) * s
    wg = wd * gd[None, :] * s[:, None]
    wf = folded_weight(w.to(dev), gamma.to(dev), s32).double()
    S = wf.abs().sum(1)
    A = xd.abs() @ wf.abs().t()
    fold = xc.abs() @ wg.abs().t()
    mS = mean.abs()[:, None] * S[None, :]
    base = rstd[:, None] * ((K + 3) * U32 * (A + mS) + K * U32 * mS + (U16 + 2 * U32) * fold
                            + 2.0 ** -25 * xc.abs().sum(1)[:, None])
    base = base + (K + 3) * U32 * (s * (bd.abs() + wd.abs() @ bed.abs()))[None, :] + U32 * v.abs()
    P = (v - (s * (bd + wd @ bed))[None, :]).abs()
    return v, base, P, rstd, S


def stat_errors(x, lay, produced=False):
    """float64 [M] each: e_mean, what the merged mean may be off by, and rel_rstd, the relative error of rstd (module
    docstring), from the exact part statistics of x.  produced: the parts are not the exact ones rounded to fp32 but a
    producer's one-pass fp32 summaries of n_k fp16 values (any order): each part mean is off by up to n_k u32 max |x| more,
    each M2_k by (n_k + 4) u32 of itself more."""
    parts = lay[0]
    C = x.shape[1]
    mk, qk = part_stats(x, lay)
    nk = torch.tensor(part_widths(C, lay), dtype=torch.float64, device=x.device)
    mean = (nk * mk).sum(1) / C
    mmax = mk.abs().max(1).values
    e_mean = (parts + 3) * U32 * mmax
    if produced:
        e_mean = e_mean + nk.max() * U32 * x.double().abs().max(1).values
    d = (mk - mean[:, None]).abs()
    e_d = (e_mean + U32 * mmax)[:, None]
    q = (qk + nk * d * d).sum(1)
    dq = (nk * (2 * d * e_d + e_d ** 2)).sum(1) + (parts + 4) * U32 * q
    if produced:
        dq = dq + ((nk + 4) * U32 * qk).sum(1)
    var = q / C + EPS
    return e_mean, 0.5 * (dq / C + 2 * U32 * var) / var + 3 * U32


def preactivation(x, ops, lay, produced=False):
    """(v, delta) of the projection on statistics in layout `lay`: the exact value and what the kernels' value ahead of
    the activation / the rounding to fp16 may be off by."""
    v, base, P, rstd, S = linear_terms(x, ops.gamma, ops.beta, ops.w1, ops.b1, ops.rows_scaled, ops.row_scale)
    e_mean, rel = stat_errors(x, lay, produced)
    return v, base + P * rel[:, None] + (rstd * e_mean)[:, None] * S[None, :]


def reference_linear(x, ops, lay, geglu, produced=False):
    """(r, bound) float64 [M, O] of sd_op_ln_linear on x's device."""
    v, delta = preactivation(x, ops, lay, produced)
    if geglu:
        h, gt = v.chunk(2, dim=-1)
        dh, dg = delta.chunk(2, dim=-1)
        return cc.geglu_reference(h, gt, dh, dg)
    return v, U16 * v.abs() + delta + 2.0 ** -25


def reference_ffn(x, ops, lay):
    """(y, branch, bound) float64 [M, C] of sd_op_ln_ffn_geglu: y = x + branch, branch = GEGLU(LN(x) W1^T + b1) W2^T + b2.
    ffn.hip rounds the hidden tensor to fp16 once (e1: the GEGLU bound, its u16 term is that rounding), accumulates the
    second GEMM in fp32 (K2 + 1 roundings: K2 accumulations and b2), rounds the branch to fp16 ahead of the residual
    add, adds x in fp32 (one rounding: u32 |y|) and rounds the sum to fp16:
      d = e1 |W2|^T + (K2 + 1) u32 ((|hid| + e1) |W2|^T + |b2|)
      |err| <= d + u16 (|branch| + d) + (u16 + u32) |y| + u16 (d + u16 |branch|) + 2^-24"""
    dev = x.device
    v, delta = preactivation(x, ops, lay)
    h, gt = v.chunk(2, dim=-1)
    dh, dg = delta.chunk(2, dim=-1)
    hid, e1 = cc.geglu_reference(h, gt, dh, dg)
    w2, b2 = ops.w2.to(dev).double(), ops.b2.to(dev).double()
    K2 = w2.shape[1]
    branch = F.linear(hid, w2, b2)
    d = e1 @ w2.abs().t() + (K2 + 1) * U32 * ((hid.abs() + e1) @ w2.abs().t() + b2.abs())
    y = x.double() + branch
    bound = d + U16 * (branch.abs() + d) + (U16 + U32) * y.abs() + U16 * (d + U16 * branch.abs()) + 2.0 ** -24
    return y, branch, bound


@functools.lru_cache(maxsize=2)
def _cached_terms(c, profile, device):
    ops = consumer_operands(c, profile)
    x = ops.x.to(device)
    return (x,) + linear_terms(x, ops.gamma, ops.beta, ops.w1, ops.b1, ops.rows_scaled, ops.row_scale)


def consumer_reference(c, profile, lay, device="cpu"):
    """The reference of one GPU run, the layout-independent part computed once per (case, profile): (r, bound) for the
    linear entry, (y, branch, bound) for the feed-forward; float64 on `device`, not to be modified."""
    ops = consumer_operands(c, profile)
    if c.entry == "ffn":
        return reference_ffn(ops.x.to(device), ops, lay)
    x, v, base, P, rstd, S = _cached_terms(c, profile, device)
    e_mean, rel = stat_errors(x, lay)
    delta = base + P * rel[:, None] + (rstd * e_mean)[:, None] * S[None, :]
    if c.geglu:
        h, gt = v.chunk(2, dim=-1)
        dh, dg = delta.chunk(2, dim=-1)
        return cc.geglu_reference(h, gt, dh, dg)
    return v, U16 * v.abs() + delta + 2.0 ** -25


# ------------------------------------------------------------------------------------------------ emulation (CPU, fp32)
ORDERS = ("slabs", "slabs-reversed", "chunks16")
DEFECTS = ("swap", "ragged-weight", "truncated", "no-wsum")


def _accumulate(a, b, order):
    """a b^T in fp32 with the partial sums of 64-deep K slabs added first to last, last to first, or 16 columns at a
    time (four times as many roundings of the running sum)."""
    K = a.shape[1]
    step = 16 if order == "chunks16" else 64
    starts = list(range(0, K, step))
    if order == "slabs-reversed":
        starts.reverse()
    acc = torch.zeros(a.shape[0], b.shape[0])
    for s0 in starts:
        acc = acc + a[:, s0:s0 + step] @ b[:, s0:s0 + step].t()
    return acc


def emulate_row_stats(stat, lay, C, defect=None):
    """ln_row_stats in fp32, in its order: (mean, rstd) [M] from the supplied [M, parts, 2].  Defects: "ragged-weight"
    weighs the last part with part_w, "truncated" merges the first MAX_PARTS parts only."""
    parts, w = lay
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(C), dtype=torch.float32)
    nks = [float(w) if defect == "ragged-weight" else float(n) for n in part_widths(C, lay)]
    used = min(parts, MAX_PARTS) if defect == "truncated" else parts
    s = torch.zeros(stat.shape[0])
    for k in range(used):
        s = s + torch.tensor(nks[k]) * stat[:, k, 0]
    mean = s * inv
    q = torch.zeros(stat.shape[0])
    for k in range(used):
        d = stat[:, k, 0] - mean
        q = q + (stat[:, k, 1] + torch.tensor(nks[k]) * d * d)
    return mean, torch.rsqrt(q * inv + torch.tensor(EPS, dtype=torch.float32))


def emulate_preactivation(x, ops, lay, order="slabs", defect=None):
    """The consumer kernels' arithmetic ahead of the activation, on the CPU in fp32: the pack-time fold, ln_row_stats on
    the supplied statistics, the accumulation, the epilogue.  Defects: those of emulate_row_stats, "swap" (row m uses the
    statistics of row m + 1), "no-wsum" (the mean correction dropped)."""
    C = x.shape[1]
    s = _scale_vector(ops.w1.shape[0], ops.rows_scaled, ops.row_scale, "cpu")
    wf = folded_weight(ops.w1, ops.gamma, s)
    wsum = wf.float().sum(1)
    bp = s * (ops.b1 + ops.w1.float() @ ops.beta)
    mean, rstd = emulate_row_stats(supplied_stats(x, lay), lay, C, defect)
    if defect == "swap":
        mean, rstd = mean.roll(-1), rstd.roll(-1)
    if defect == "no-wsum":
        wsum = torch.zeros_like(wsum)
    acc = _accumulate(x.float(), wf.float(), order)
    return (acc - mean[:, None] * wsum[None, :]) * rstd[:, None] + bp[None, :]


def emulate_linear(x, ops, lay, geglu, order="slabs", defect=None):
    v = emulate_preactivation(x, ops, lay, order, defect)
    if geglu:
        h, gt = v.chunk(2, dim=-1)
        return (h * F.gelu(gt)).half()
    return v.half()


def emulate_ffn(x, ops, lay, order="slabs", defect=None):
    hid = emulate_linear(x, ops, lay, 1, order, defect)
    branch = _accumulate(hid.float(), ops.w2.float(), order) + ops.b2[None, :]
    return (branch.half().float() + x.float()).half()


# ------------------------------------------------------------------------------------------------------------ producers
def producer_case(p):
    """The producer launch as a conv_cases.Case (its float64 reference and bound are conv_cases.reference)."""
    return cc.Case("lnprod", 1, p.M, 1, p.K, p.C, 1, 1, 0, -1, 0, 0, True, False, p.res, 1.0, 1.0, 0, p.force, None, "randn",
                   ("dense",))


@functools.lru_cache(maxsize=4)
def producer_operands(p, profile):
    """(x [M, K] fp16, w0 [C, K] fp16, b0 [C] fp32, res [M, C] fp16 | None) on the CPU.
      normal     randn operands; b0 carries a level per 16 columns so that the parts of a row differ
      rows       as normal with every row of x at a spread of its own and, with a residual, a level of its own (chains)
      offset:50  b0 = 50 exactly, small weights (and residual): rows 50 +- 0.1; rows 0 and M - 1 of x and res are zero, so
                 those rows of y1 are the constant 50 and their M2 must come out as exactly 0"""
    g = torch.Generator().manual_seed(_seed("producer", p.M, p.K, p.C, p.res, profile))
    x = torch.randn(p.M, p.K, generator=g)
    res = None
    if profile == "offset:50":
        w0 = 0.07 * torch.randn(p.C, p.K, generator=g) / p.K ** 0.5
        b0 = torch.full((p.C,), 50.0)
        if p.res:
            res = 0.07 * torch.randn(p.M, p.C, generator=g)
            res[0] = 0.0
            res[-1] = 0.0
        x[0] = 0.0
        x[-1] = 0.0
    else:
        w0 = torch.randn(p.C, p.K, generator=g) / p.K ** 0.5
        b0 = 0.2 * torch.randn(p.C, generator=g) + torch.randn((p.C + 15) // 16, generator=g).repeat_interleave(16)[:p.C]
        if p.res:
            res = torch.randn(p.M, p.C, generator=g)
        if profile == "rows":
            r = torch.arange(p.M)
            x = x * (0.25 * 16.0 ** (((29 * r) % 53).float() / 52.0))[:, None]
            if p.res:
                res = res + (-4.0 + 8.0 * ((37 * r) % 101).float() / 100.0)[:, None]
        else:
            assert profile == "normal", profile
    return x.half(), w0.half(), b0, res.half() if res is not None else None


def producer_reference(p, profile):
    """(r, bound) float64 [M, C] of y1, from conv_cases."""
    x, w0, b0, res = producer_operands(p, profile)
    c = producer_case(p)
    r, bound = cc.reference(c, x.view(1, p.M, 1, p.K), w0.view(p.C, p.K, 1, 1), b0, None,
                            res.view(1, p.M, 1, p.C) if res is not None else None)
    return r.view(p.M, p.C), bound.view(p.M, p.C)


def chain_consumer(ch):
    """The consumer half of a chain as a Consumer case (its x is the producer's stored y1)."""
    p = ch.prod
    return Consumer("chain", "linear", p.M, p.C, ch.O, ch.geglu, ch.force, ch.want, (), ())


@functools.lru_cache(maxsize=2)
def chain_operands(ch):
    """Operands of a chain's consumer (x = None: it is the producer's output)."""
    c = chain_consumer(ch)
    g = torch.Generator().manual_seed(_seed("chain", ch.name))
    gamma = 1.0 + 0.2 * torch.randn(c.C, generator=g)
    beta = 0.2 * torch.randn(c.C, generator=g) + 0.05
    cols = (2 if c.geglu else 1) * c.O
    w1 = (torch.randn(cols, c.C, generator=g) / c.C ** 0.5).half()
    b1 = 0.2 * torch.randn(cols, generator=g)
    return Operands(None, gamma, beta, w1, b1, None, None, *row_scaling(c))
