"""Cases, inputs, float64 references, element bounds and fp32 emulations shared by tests/test_edge_plan.py (CPU) and
tests/test_edge_gpu.py (GPU) for the three hand-written kernels at the UNet's edges: conv_head_kernel (conv_in),
conv_tail_kernel (conv_norm_out -> SiLU -> conv_out) of csrc/edge.hip and skinny_linear_kernel / small_linear_kernel
(the time-embedding linears) of csrc/misc.hip.  Nothing here touches a device.

conv_in (sd_op_unet_conv_in, Cout = 320; every case is one or a few 128-pixel tiles)
  grid    as conv_cases: x integers in [-2, 2], w in {-1, 0, 1} / 16, bias multiples of 1/16: bit for bit.
  tap     one-hot weights: output channel co copies input channel co % Cin at tap (co // Cin) % 9, bias 0, random fp16 x:
          bit for bit, and exactly +0 where the tap leaves the image.
  randn   inside conv_cases.reference's bound u16 |v| + (K + 3) u32 A + 2^-25, K = 9 Cin (the zero columns up to 64 add
          nothing); profile p50: bias near 50, weights scaled by 0.1 (the summaries' hard case).
  Summaries (groups > 0): (mean, M2) of every (image, 128-pixel tile, group) of the STORED fp16 output against float64
  through norm_cases.summary_errors.  head_epilogue's order (16 lanes x 8 rows x cpg sequential fp32 adds, four
  butterfly adds, one divide, second pass about the rounded mean) emulated over every case reaches at most 0.041 of
  SLAB times the mean's term (STAT_A holds many times over) and, of SLAB times the M2 term, 0.081 at groups 32, 0.409 at
  groups 5 and 1.28 at groups 1 (all three on grid cases; 0.058 / 0.318 / 0.976 on tap cases, at most 0.065 on randn and
  p50): norm_cases' constants hold with test_norm_plan's factor of two for chains of up to 512 adds and not for the
  2560 of groups 1, which gets HEAD_CHAIN (head_summary_errors; test_edge_plan asserts the factor per case).

conv_out (sd_op_unet_conv_out_ex, C = 320)
  tap     one-hot weights, bias 0: output channel j of launch `tapset` copies the normalised, activated channel c at tap t
          (TAPSETS: all nine taps, channels in all five 64-channel slabs).  One non-zero product and two additions of
          accumulators are exact in fp32, so y is the fp16 value the kernel put into LDS: inside norm_cases' bound e_a of
          the GroupNorm(+SiLU) reference a, and exactly zero bits where the tap leaves the image (beta != 0: zero AFTER
          the norm).
  randn   profiles randn / p50 of norm_cases.  Bound, from the reference alone: the kernel convolves a' = fp16(a_kernel)
          with |a' - a| <= e_a (norm_cases.reference's bound, which includes the fp16 rounding into LDS); the K = 2880
          products are exact in fp32 and are added with the bias in some order, at most K + 3 roundings of partial sums
          none above sum |w| |a'| + |bias| <= sum |w| (|a| + e_a) + |bias|; one rounding to fp16:
            |err| <= sum |w| e_a + (K + 3) u32 (sum |w| (|a| + e_a) + |bias|) + u16 |y| + 2^-25
          with u32 = 2^-23 and 2^-25 as in conv_cases.reference.
  Summaries: the kernel's own statistics pass (S = 0), or supplied = norm_cases.tile_summaries rounded to fp32.

small_linear (sd_op_small_linear); a case names its kernel: 1 skinny_linear_kernel, 0 small_linear_kernel
  grid    x multiples of 1/8 in [-2, 2], w in {-1, 0, 1} / 16, bias multiples of 1/16: bit for bit in fp32.
  split   x = a + b 2^-12, a multiples of 1/8 (|a| >= 1 for at least half), b in {-1, 0, 1}: every product is a multiple
          of 2^-16 and K max |x| / 16 < 256 (|a| <= 1 from K = 2048 up), so every partial sum fits 24 bits: bit for bit,
          and different from the result on fp16(x) -- the proof that the low half of the activation is carried.
  randn   bound (K + 3) u32 A + 2^-22 A, A = sum |act(x)| |w| + |bias|: fp32 accumulation in any order, and what
          hi + lo drops (lo is rounded to fp16: 2^-11 of 2^-11 of |x|).  SiLU on the way in adds sum |w| e(x), on the way
          out 1.1 delta + e(v), with e(v) = (8 + 4 |v|) u32 |silu(v)| built as conv_cases._activation_error: the
          hardware's exp2 and reciprocal at one ulp each, the exponent's argument rounded once, a handful of fp32
          operations; 1.1 > sup |silu'|.

Worst |err| / bound of the emulations and the share of the fp32 terms they use are printed by test_edge_plan."""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as cc
import norm_cases as nc

f32 = np.float32
U16, U32 = cc.U16, cc.U32
COUT_IN = 320
C_OUT = 320


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()) & 0x7fffffff)


# =================================================================================================== conv_in
Head = collections.namedtuple("Head", "N Cin H W kind G profile")
HEAD_SHAPES = [(1, 128), (128, 1), (2, 64), (8, 16), (16, 8), (3, 128), (16, 24), (32, 12)]
HEAD_GROUPS = (0, 1, 5, 32)


def _build_head():
    cases, i = [], 0
    for kind in ("grid", "tap"):
        for H, W in HEAD_SHAPES:
            for N in (1, 3):
                for Cin in (1, 4, 7):
                    cases.append(Head(N, Cin, H, W, kind, HEAD_GROUPS[i % 4], "randn"))
                    i += 5                      # (5 is odd: every group count meets every shape, batch and width)
    i = 1
    for H, W in ((8, 16), (16, 24)):
        for N in (1, 3):
            for Cin in (1, 4, 7):
                cases.append(Head(N, Cin, H, W, "randn", HEAD_GROUPS[1 + i % 3], "randn"))
                i += 1
    for G in (1, 5, 32):
        cases.append(Head(3, 4, 16, 24, "randn", G, "p50"))
    cases.append(Head(1, 7, 8, 16, "randn", 32, "p50"))
    return cases


HEAD_CASES = _build_head()


def head_id(c):
    return "in-%dx%dx%dx%d-%s-g%d%s" % (c.N, c.Cin, c.H, c.W, c.kind, c.G, "-p50" if c.profile == "p50" else "")


def head_conv_case(c):
    """The conv_cases.Case whose reference and bound a conv_in case uses."""
    return cc.Case("head", c.N, c.H, c.W, c.Cin, COUT_IN, 3, 1, 0, -1, 0, 0, True, False, False, 1.0, 1.0, 0, None, None,
                   c.kind, ("dense",))


def head_tap_weights(Cin):
    w = torch.zeros(COUT_IN, Cin, 3, 3)
    for co in range(COUT_IN):
        t = (co // Cin) % 9
        w[co, co % Cin, t // 3, t % 3] = 1.0
    return w.half()


def head_inputs(c):
    """x [N, Cin, H, W] fp16 (NCHW, as the latents), w [320, Cin, 3, 3] fp16, bias [320] fp32."""
    g = _gen(head_id(c))
    shape = (c.N, c.Cin, c.H, c.W)
    if c.kind == "grid":
        x = torch.randint(-2, 3, shape, generator=g).half()
        w = (torch.randint(-1, 2, (COUT_IN, c.Cin, 3, 3), generator=g).float() / 16.0).half()
        return x, w, cc._grid16((COUT_IN,), 0.5, g)
    x = torch.randn(shape, generator=g).half()
    if c.kind == "tap":
        return x, head_tap_weights(c.Cin), torch.zeros(COUT_IN)
    w = torch.randn(COUT_IN, c.Cin, 3, 3, generator=g) / (9 * c.Cin) ** 0.5
    bias = torch.randn(COUT_IN, generator=g) * 0.5
    if c.profile == "p50":
        w, bias = 0.1 * w, 50.0 + 0.05 * torch.randn(COUT_IN, generator=g)
    return x, w.half(), bias


def head_tap_gather(c, x):
    """What a tap case stores, by slicing the zero-padded input: [N, H, W, 320] fp16, +0 outside the image."""
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(c.N, c.H, c.W, COUT_IN, dtype=torch.float16)
    for co in range(COUT_IN):
        t = (co // c.Cin) % 9
        out[..., co] = xp[:, co % c.Cin, t // 3:t // 3 + c.H, t % 3:t % 3 + c.W]
    return out


@functools.lru_cache(maxsize=4)
def head_inputs_and_reference(c):
    """(x, w, bias, r, bound): r, bound [N, H, W, 320] float64 (conv_cases.reference); not to be modified."""
    x, w, bias = head_inputs(c)
    r, bound = cc.reference(head_conv_case(c), x.permute(0, 2, 3, 1).contiguous(), w, bias, None, None)
    return x, w, bias, r, bound


def head_summary_reference(c, y):
    """float64 (mean, M2) [N, S, G, 2] of the stored output y [N, H, W, 320] fp16 per 128-pixel tile and group."""
    return nc.tile_summaries(y.reshape(c.N, c.H * c.W, COUT_IN), c.G, 128)[1]


HEAD_CHAIN = 640.0


def head_summary_errors(c, summ, want):
    """norm_cases.summary_errors for conv_in's summaries [N, S, G, 2] against their float64 values `want`, the M2 fraction
    divided by max(1, 8 cpg / HEAD_CHAIN).  head_epilogue adds 8 cpg squares in sequence per lane; SLAB's terms were
    set for kernels whose chains are a few dozen adds long and hold for 8 cpg = 80 and 512 (groups 32 and 5), but a
    sequential fp32 sum of L same-signed terms drifts by up to L u / 2 when the addends repeat, as the squares do in
    the grid and tap cases (a third of a tap case's values are the same zero): the emulation reaches 1.28 of the
    terms at 8 cpg = 2560 (groups 1), so from HEAD_CHAIN adds on the tolerance grows with the chain."""
    cpg = COUT_IN // c.G
    dm, dq = nc.summary_errors(torch.as_tensor(summ), want, 128.0 * cpg)
    return dm, dq / max(1.0, 8 * cpg / HEAD_CHAIN)


def _fma(acc, a, b):
    """fp32 fused multiply-add (a, b fp32: the product is exact in float64)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(f32)


def emulate_head(c, x, w, bias, mutation=None):
    """conv_head_kernel in numpy float32: the im2col tile k = (kh * 3 + kw) * Cin + ci, zero from 9 Cin up, one 64-deep
    slab, + bias, fp16; then head_epilogue's summaries of the stored values.  -> (y [N, H, W, 320] fp16, summaries
    [N, S, G, 2] float32 | None).  Mutations: "kwmajor" taps read kw-major; "pad63" column 63 of a K = 63 problem
    treated as a tenth tap with the weight rows 9 Cin apart; "image" the summaries stored one image on."""
    N, Cin, H, W = x.shape
    xp = F.pad(x.float(), (1, 1, 3, 3)).numpy()                 # (rows padded by 3: the tenth tap of "pad63" reads row y + 2)
    A = np.zeros((N, H, W, 64), f32)
    for t in range(9):
        kh, kw = (t % 3, t // 3) if mutation == "kwmajor" else (t // 3, t % 3)
        A[..., t * Cin:(t + 1) * Cin] = np.moveaxis(xp[:, :, kh + 2:kh + 2 + H, kw:kw + W], 1, 3)
    B = np.zeros((COUT_IN, 64), f32)
    B[:, :9 * Cin] = w.float().permute(0, 2, 3, 1).reshape(COUT_IN, 9 * Cin).numpy()
    if mutation == "pad63":
        assert 9 * Cin == 63
        A[..., 63] = xp[:, 0, 5:5 + H, 0:W]
        B[:-1, 63] = B[1:, 0]
    acc = A.reshape(-1, 64) @ B.T
    y = torch.from_numpy((acc + bias.numpy()[None, :]).astype(f32)).half().reshape(N, H, W, COUT_IN)
    if not c.G:
        return y, None
    cpg, S = COUT_IN // c.G, H * W // 128
    v = y.float().numpy().reshape(N, S, 16, 8, c.G, cpg)        # [image, tile, lane, row, group, channel]
    sm = np.zeros((N, S, 16, c.G), f32)
    for r in range(8):
        for ch in range(cpg):
            sm = (sm + v[:, :, :, r, :, ch]).astype(f32)
    idx = np.arange(16)

    def tree(t):
        for off in (1, 2, 4, 8):
            t = (t + t[:, :, idx ^ off]).astype(f32)
        return t[:, :, 0]

    mean = (tree(sm) / f32(128 * cpg)).astype(f32)
    q = np.zeros_like(sm)
    for r in range(8):
        for ch in range(cpg):
            d = (v[:, :, :, r, :, ch] - mean[:, :, None, :]).astype(f32)
            q = _fma(q, d, d)
    summ = np.stack([mean, tree(q)], axis=-1)
    if mutation == "image":
        summ = np.roll(summ, 1, axis=0)
    return y, summ


# =================================================================================================== conv_out
Tail = collections.namedtuple("Tail", "N H W Cout silu G layout S rows kind profile tapset")
TAPSETS = (((0, 0), (63, 1), (64, 2), (191, 3)), ((319, 4), (127, 5), (128, 6), (192, 7)), ((255, 8), (256, 0), (10, 4), (300, 2)))
TAIL_SUPPLIED = ((1, 512), (4, 128), (16, 32), (17, 31), (32, 16), (35, 15))       # (S, rows) at H W = 512


def _build_tail():
    cases = []

    def add(N=3, H=16, W=16, Cout=4, silu=1, G=32, layout="dense", S=0, rows=0, kind="randn", profile="randn", tapset=0):
        c = Tail(N, H, W, Cout, silu, G, layout, S, rows, kind, profile, tapset)
        if c not in cases:
            cases.append(c)

    for H, W in ((8, 16), (16, 16), (8, 32), (24, 48)):
        add(H=H, W=W)
    add(N=1)
    for Cout in (1, 2, 3):
        add(Cout=Cout)
    add(silu=0)
    for G in (1, 5, 20):
        add(G=G)
    add(layout="ld328")
    add(profile="p50")
    add(profile="p50", silu=0, layout="ld328")
    for S, rows in TAIL_SUPPLIED:
        add(H=16, W=32, S=S, rows=rows)
    add(H=16, W=32, S=35, rows=15, profile="p50")
    add(H=16, W=32, S=17, rows=31, G=5, layout="ld328")
    add(H=16, W=32, S=32, rows=16, G=20, silu=0)
    add(H=16, W=32, S=4, rows=128, G=1, N=1)
    add(H=24, W=48, S=9, rows=128)                    # the UNet's own tile size
    for ts in range(3):
        add(kind="tap", tapset=ts)
        add(kind="tap", tapset=ts, H=8, W=16, N=1, silu=0)          # one tile: all four borders in one block
        add(kind="tap", tapset=ts, H=16, W=32, S=35, rows=15, layout="ld328")
    add(kind="tap", tapset=0, Cout=1)
    add(kind="tap", tapset=2, Cout=3, G=5)
    return cases


TAIL_CASES = _build_tail()


def tail_id(c):
    s = "out-%dx%dx%d-o%d-g%d-%s-%s" % (c.N, c.H, c.W, c.Cout, c.G, c.kind, c.profile)
    s += ("-silu" if c.silu else "") + ("-" + c.layout if c.layout != "dense" else "")
    s += ("-S%dx%d" % (c.S, c.rows) if c.S else "-own") + ("-t%d" % c.tapset if c.kind == "tap" else "")
    return s


def tail_norm_case(c):
    """The norm_cases.Case whose inputs, reference and bound a conv_out case uses."""
    return nc.Case("tail", c.N, c.H * c.W, C_OUT, c.G, c.silu, 1e-5, c.profile, c.rows if c.S else 0, None, (c.layout,))


def tail_weights(c):
    g = _gen(tail_id(c))
    if c.kind == "tap":
        w = torch.zeros(c.Cout, C_OUT, 3, 3)
        for j, (ch, t) in enumerate(TAPSETS[c.tapset][:c.Cout]):
            w[j, ch, t // 3, t % 3] = 1.0
        return w.half(), torch.zeros(c.Cout)
    w = (torch.randn(c.Cout, C_OUT, 3, 3, generator=g) / (9 * C_OUT) ** 0.5).half()
    return w, torch.randn(c.Cout, generator=g) * 0.5


def _nchw(t, c):
    return t.reshape(c.N, c.H, c.W, C_OUT).permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=4)
def tail_inputs_and_reference(c):
    """(x [N, HW, 320] fp16, gamma, beta, w, bias, r, bound, outside): r, bound [N, Cout, H, W] float64; outside: where a
    tap case's tap leaves the image (None otherwise).  Not to be modified."""
    n = tail_norm_case(c)
    x, gamma, beta = nc.make_inputs(n)
    a, e_a = nc.reference(n, x, gamma, beta)
    w, bias = tail_weights(c)
    wd = w.double()
    A, E = _nchw(a, c), _nchw(e_a, c)
    y = F.conv2d(A, wd, bias.double(), padding=1)
    sw_e = F.conv2d(E, wd.abs(), None, padding=1)
    if c.kind == "tap":
        outside = F.conv2d(torch.ones_like(A), wd, None, padding=1) == 0
        return x, gamma, beta, w, bias, y, sw_e, outside
    K = 9 * C_OUT
    mag = F.conv2d(A.abs() + E, wd.abs(), None, padding=1) + bias.double().abs()[None, :, None, None]
    return x, gamma, beta, w, bias, y, sw_e + (K + 3) * U32 * mag + U16 * y.abs() + 2.0 ** -25, None


def tail_supplied(c, x):
    """The summaries a producing convolution would leave: [N, S, G, 2] fp32."""
    part = nc.tile_summaries(x, c.G, c.rows)[0]
    assert part.shape[1] == c.S
    return part


def emulate_tail(c, x, gamma, beta, w, bias, part, S, rows, mutation=None):
    """conv_tail_kernel in numpy float32.  part [N, S, G, 2] float32: the supplied summaries, or what the statistics pass
    leaves (norm_cases.emu_stats2 at sd_norm_plan's S, rows, CB).  16 threads per group merge the summaries
    k = pi, pi + 16, ... (stat_merge), thread 0 the sixteen; y = fp16(act(x sc + sh)), zero outside the image; one fp32
    accumulator per kernel row over (kw, slab); their sum + bias, fp16.  -> [N, Cout, H, W] fp16.
    Mutations: "ragged" the last summary counted as a full one; "prepad" the halo zero BEFORE the norm; "kwmajor"."""
    HW, cpg = c.H * c.W, C_OUT // c.G
    counts = nc._tile_counts(S, rows, HW, cpg)
    if mutation == "ragged":
        counts[:] = f32(rows * cpg)
    m, q = nc._merge_strided(part, counts, 16)
    mean, rstd = nc._finish(m, q, HW, cpg, 1e-5)
    xf = x.numpy().astype(f32)
    a16 = nc.emu_apply(xf, mean, rstd, gamma, beta, c.silu, c.G)                    # [N, HW, C] fp16
    ap = F.pad(_nchw(a16.float(), c), (1, 1, 1, 1)).numpy()
    if mutation == "prepad":
        z = nc.emu_apply(np.zeros((c.N, 1, C_OUT), f32), mean, rstd, gamma, beta, c.silu, c.G).float().numpy()
        inside = np.zeros((c.H + 2, c.W + 2), bool)
        inside[1:-1, 1:-1] = True
        ap = np.where(inside[None, None], ap, z[:, 0, :, None, None])
    wf = w.float().numpy()
    acc = np.zeros((3, c.N, c.Cout, c.H, c.W), f32)
    for kh in range(3):
        for kw in range(3):
            wk = wf[:, :, kw, kh] if mutation == "kwmajor" else wf[:, :, kh, kw]
            for sl in range(C_OUT // 64):
                t = np.einsum("nchw,oc->nohw", ap[:, sl * 64:(sl + 1) * 64, kh:kh + c.H, kw:kw + c.W], wk[:, sl * 64:(sl + 1) * 64])
                acc[kh] = (acc[kh] + t.astype(f32)).astype(f32)
    v = ((acc[0] + acc[1]).astype(f32) + acc[2]).astype(f32)
    return torch.from_numpy((v + bias.numpy()[None, :, None, None]).astype(f32)).half()


# =================================================================================================== small_linear
Lin = collections.namedtuple("Lin", "B K n_out kind silu_in silu_out bias want")
SK_K, SK_N, SK_B = (32, 64, 128, 160, 1280), (16, 48, 8208), (1, 8, 16)
GV_K, GV_N, GV_B = (8, 40, 1312, 2816), (5, 6, 7, 20, 40), (1, 8, 9, 17)
# one case on each side of every clause of the predicate (B <= 16, K % 32 == 0, K <= 1280, n_out % 16 == 0)
THRESHOLDS = [((16, 64, 48), 1), ((17, 64, 48), 0), ((8, 32, 16), 1), ((8, 40, 16), 0), ((8, 1280, 16), 1), ((8, 1312, 16), 0),
              ((8, 64, 16), 1), ((8, 64, 20), 0), ((8, 64, 32), 1), ((8, 64, 24), 0)]


def _build_lin():
    cases = []

    def add(B, K, n, kind, want, si=0, so=0, bias=True):
        c = Lin(B, K, n, kind, si, so, bias, want)
        if c not in cases:
            cases.append(c)

    big = {(32, 1), (160, 8), (1280, 16), (1280, 1)}           # (K, B) run at n_out = 8208 = 16 x 513
    for kind in ("grid", "split"):
        for K in SK_K:
            for n in SK_N:
                for B in SK_B:
                    if n < 8208 or (K, B) in big:
                        add(B, K, n, kind, 1)
        for K in GV_K:
            for n in GV_N:
                for B in GV_B:
                    add(B, K, n, kind, 0)
        for (B, K, n), want in THRESHOLDS:
            add(B, K, n, kind, want)
    add(8, 160, 48, "grid", 1, bias=False)
    add(9, 40, 7, "grid", 0, bias=False)
    add(16, 1280, 48, "split", 1, bias=False)
    add(17, 1312, 6, "split", 0, bias=False)
    for si, so in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for B, K, n in ((1, 32, 16), (16, 160, 48), (8, 1280, 48), (16, 1280, 8208), (2, 320, 1280)):
            add(B, K, n, "randn", 1, si, so)
        for B, K, n in ((1, 8, 5), (9, 40, 7), (17, 1312, 20), (8, 2816, 40), (17, 1280, 48)):
            add(B, K, n, "randn", 0, si, so)
    add(8, 1280, 48, "randn", 1, 1, 1, bias=False)
    add(9, 1312, 6, "randn", 0, 1, 1, bias=False)
    return cases


LIN_CASES = _build_lin()


def lin_id(c):
    return "lin-%dx%dx%d-%s-%d%d%s-k%d" % (c.B, c.K, c.n_out, c.kind, c.silu_in, c.silu_out, "" if c.bias else "-nobias", c.want)


def lin_inputs(c):
    """x [B, K] fp32, w [n_out, K] fp16, bias [n_out] fp32 | None."""
    g = _gen(lin_id(c))
    if c.kind == "randn":
        x = torch.randn(c.B, c.K, generator=g) * 1.5
        w = (torch.randn(c.n_out, c.K, generator=g) / c.K ** 0.5).half()
        return x, w, (torch.randn(c.n_out, generator=g) * 0.5 if c.bias else None)
    w = (torch.randint(-1, 2, (c.n_out, c.K), generator=g).float() / 16.0).half()
    bias = cc._grid16((c.n_out,), 0.5, g) if c.bias else None
    if c.kind == "grid":
        return torch.randint(-16, 17, (c.B, c.K), generator=g).float() / 8.0, w, bias
    lim = 16 if c.K < 2048 else 8
    a = torch.randint(-lim, lim + 1, (c.B, c.K), generator=g).float() / 8.0
    one = torch.where(torch.rand(c.B, c.K, generator=g) < 0.5, 1.0, -1.0)
    a = torch.where((torch.arange(c.K) % 2 == 0)[None, :] | (a == 0), one, a)      # |a| = 1 at every other k at least
    b = torch.randint(-1, 2, (c.B, c.K), generator=g).float()
    return a + b * 2.0 ** -12, w, bias


def _silu64(v):
    return v * torch.sigmoid(v)


def silu_error(v):
    """What evaluating SiLU in fp32 may add at argument v (float64): conv_cases._activation_error's terms."""
    return (8.0 + 4.0 * v.abs()) * U32 * _silu64(v).abs()


def lin_reference(c, x, w, bias):
    """(r, bound) [B, n_out] float64 from the fp32 / fp16 operands."""
    xd, wd = x.double(), w.double()
    e_in = torch.zeros_like(xd)
    if c.silu_in:
        e_in, xd = silu_error(xd), _silu64(xd)
    v = xd @ wd.t()
    A = xd.abs() @ wd.abs().t()
    if bias is not None:
        v, A = v + bias.double(), A + bias.double().abs()
    delta = e_in @ wd.abs().t() + (c.K + 3) * U32 * A + 2.0 ** -22 * A
    if c.silu_out:
        return _silu64(v), 1.1 * delta + silu_error(v)
    return v, delta


@functools.lru_cache(maxsize=4)
def lin_inputs_and_reference(c):
    x, w, bias = lin_inputs(c)
    return (x, w, bias) + lin_reference(c, x, w, bias)


def _silu32(v):
    with np.errstate(over="ignore"):
        return (v * (f32(1) / (f32(1) + np.exp2((f32(-1.4426950408889634) * v).astype(f32)).astype(f32))).astype(f32)).astype(f32)


GUARD = 16


def emulate_linear(c, x, w, bias, kernel, mutation=None):
    """The two kernels in numpy float32 -> the output buffer [B n_out + GUARD] float32, its last GUARD elements the
    guard (13.0) behind y.
    kernel 1, skinny_linear_kernel: x = hi + lo (fp16 each), wave wv of four accumulates the 32-wide K steps
      wv, wv + 4, ... (hi then lo per step), the four partials are added in wave order, + bias, SiLU.  A block runs the
      tiles t, t + 512, ...  Mutations: "lo" dropped; "alias" one reduction buffer: the tile's wave-0 partial is that
      of tile t + 512 when the block has one.
    kernel 0, small_linear_kernel: lane l accumulates k = 8 l + 512 i + e in order (fused multiply-adds), a butterfly
      over the 64 lanes, + bias, SiLU.  Mutation "clamp": the columns a wave clamps are written too, at their own
      index."""
    B, K, n = c.B, c.K, c.n_out
    xs = x.numpy().astype(f32)
    if c.silu_in:
        xs = _silu32(xs)
    wf = w.float().numpy()
    out = np.full(B * n + GUARD, 13.0, f32)
    if kernel == 1:
        hi = torch.from_numpy(xs).half().float().numpy()
        lo = torch.from_numpy((xs - hi).astype(f32)).half().float().numpy()
        parts = np.zeros((4, B, n), f32)
        for ks in range(K // 32):
            s = slice(ks * 32, ks * 32 + 32)
            p = parts[ks % 4]
            p = (p + hi[:, s] @ wf[:, s].T).astype(f32)
            if mutation != "lo":
                p = (p + lo[:, s] @ wf[:, s].T).astype(f32)
            parts[ks % 4] = p
        if mutation == "alias":
            tiles = n // 16
            for t in range(tiles - 512):
                parts[0][:, t * 16:t * 16 + 16] = parts[0][:, (t + 512) * 16:(t + 512) * 16 + 16]
        v = (((parts[0] + parts[1]).astype(f32) + parts[2]).astype(f32) + parts[3]).astype(f32)
    else:
        steps = nc.cdiv(K, 512)
        xpad = np.zeros((B, steps * 512), f32)
        wpad = np.zeros((n, steps * 512), f32)
        xpad[:, :K], wpad[:, :K] = xs, wf
        xl = xpad.reshape(B, 1, steps, 64, 8)
        wl = wpad.reshape(1, n, steps, 64, 8)
        acc = np.zeros((B, n, 64), f32)
        for i in range(steps):
            for e in range(8):
                acc = _fma(acc, np.broadcast_to(xl[:, :, i, :, e], acc.shape), np.broadcast_to(wl[:, :, i, :, e], acc.shape))
        v = nc._butterfly(acc)
    if bias is not None:
        v = (v + bias.numpy()[None, :]).astype(f32)
    if c.silu_out:
        v = _silu32(v)
    if kernel == 0 and mutation == "clamp":
        for b in range(B):
            for col in range(n, nc.cdiv(n, 4) * 4):
                out[b * n + col] = v[b, n - 1]
    out[:B * n] = v.reshape(-1)
    return out


def worst_ratio(got, r, bound):
    """Worst |err| / bound (a bound of zero asks for the exact value)."""
    err = (got.double() - r).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item()
