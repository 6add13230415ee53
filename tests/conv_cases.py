"""Cases, inputs, float64 reference and error bound shared by tests/test_conv_plan.py (CPU) and tests/test_conv_gpu.py
(GPU) for the convolution / linear kernels igemm2_plan chooses among.  Nothing here touches a device.

A case names the kernel it was written for as (kind, split-K slices launched, reduction kernel): the CPU suite checks
that sd_igemm_plan gives that kind for every case and that the cases reach every kind and both reducers, the GPU suite
runs them through sd_op_conv2d_ex and compares what ran.

Input kinds
  grid   x integers in [-2, 2], w in {-1, 0, 1} / 16, bias / rowadd multiples of 1/16 in [-0.5, 0.5], res multiples of
         1/16 in [-2, 2], scales powers of two: every product and partial sum is a small multiple of 1/16 (1/128 under
         the smallest scale), so fp32 accumulation is exact in any order, tile or split, and the output is
         representable in fp16 (test_conv_plan proves that per case): the kernel must match the reference bit for bit.
  tap    w one-hot: output channel co copies input channel perm(co % Cin) at tap (co // Cin) % 9 (3x3) -- all nine taps
         in one launch, Cout = 9 Cin; x random fp16.  A pure gather: bit for bit.
  sat    GEGLU with the gate saturated: hidden half as grid, gate half zero weights and a bias of 16; gelu(16) == 16
         exactly in fp32, so y = 16 * hidden bit for bit (the 64-row interleave and the register permutation).
  randn  random operands, element-wise bound below."""
import collections
import functools
import math
import zlib

import torch
import torch.nn.functional as F

U16 = 2.0 ** -11
U32 = 2.0 ** -23

# igemm2.hip's variant table as far as the cases need it: id -> (BM, BN, ring depth); Tile family, and igemm3 (18)
TILE = {0: (256, 128, 3), 1: (128, 128, 2), 2: (128, 160, 2), 3: (128, 64, 2), 4: (64, 64, 2), 5: (256, 160, 3),
        6: (256, 128, 3), 7: (256, 160, 3), 8: (128, 64, 3), 9: (128, 160, 3), 11: (128, 80, 2), 12: (128, 80, 3),
        16: (128, 80, 4), 17: (128, 80, 5)}
REG = 18
REG_TILE = (128, 80, 4)         # igemm3.hip: G3_BM, G3_BN, G3_STAGES
HALO = {10: 160, 15: 128}       # id -> BN; 256 output pixels per tile
GEGLU_TILES = (0, 1, 6)         # Tile variants with the GEGLU epilogue (14 and kind 100 are the other GEGLU kernels)
ALL_KINDS = set(range(19)) | {100, -1}

_FIELDS = ("group N H W Cin Cout ks stride up pad geglu act bias rowadd res acc_scale bias_scale gn_groups force want "
           "kind layouts")
Case = collections.namedtuple("Case", _FIELDS)
# group      the GPU test that runs it
# N H W Cin  input geometry (before the optional 2x upsample), Cout GEMM columns (2x the stored width under geglu)
# pad        -1: the kernel size's default; 0 with stride 2: the VAE encoder's downsample
# bias rowadd res   which epilogue operands are present
# gn_groups  > 0: GroupNorm summaries asked of the launch (selects splitk_epilogue_gs_kernel behind a split)
# force      (variant, splits) for sd_igemm_force, or None
# want       (kind, split-K slices launched, reducer 0 / 1 / 2)
# layouts    operand layouts the GPU suite runs: "dense", "left", "right" (see test_conv_gpu.run)


def case_id(c):
    s = "%s-%dx%dx%dx%d-o%d-k%ds%d" % (c.group, c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride)
    s += ("u" if c.up else "") + ("p%d" % c.pad if c.pad >= 0 else "") + ("-geglu" if c.geglu else "")
    s += ("-act%d" % c.act if c.act else "") + "-" + "".join(k for k, on in zip("bar", (c.bias, c.rowadd, c.res)) if on)
    if c.acc_scale != 1.0 or c.bias_scale != 1.0:
        s += "-s%g,%g" % (c.acc_scale, c.bias_scale)
    s += ("-gn%d" % c.gn_groups if c.gn_groups else "")
    s += ("-f%d,%d" % c.force if c.force else "-auto") + "-%s" % c.kind
    return s


def cdiv(a, b):
    return (a + b - 1) // b


def out_size(c):
    """(OH, OW) as op_conv / sd_igemm_plan derive them."""
    IH, IW = c.H << c.up, c.W << c.up
    pad = c.pad if c.pad >= 0 else (1 if c.ks == 3 else 0)
    if c.stride == 1:
        return IH, IW
    if pad == 0:
        return (IH + 1 - c.ks) // c.stride + 1, (IW + 1 - c.ks) // c.stride + 1
    return (IH + 2 * pad - c.ks) // c.stride + 1, (IW + 2 * pad - c.ks) // c.stride + 1


def gemm_dims(c):
    OH, OW = out_size(c)
    return c.N * OH * OW, c.ks * c.ks * c.Cin           # M, K


def out_cols(c):
    return c.Cout // 2 if c.geglu else c.Cout


def halo_patch_width(OH, OW):
    for wt in (64, 32, 16):
        if OW % wt == 0 and OH % (256 // wt) == 0:
            return wt
    return 0


def launched(slabs, splits, gn):
    """(slices, reducer) a launcher starts for `splits` planned slices over `slabs` K slabs."""
    eff = cdiv(slabs, cdiv(slabs, splits))
    return eff, (0 if eff == 1 else (2 if gn else 1))


def plan_args(c):
    """geom[9], flags[10] of sd_igemm_plan for a case."""
    geom = (c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.up, c.pad)
    scaled = int(c.acc_scale != 1.0 or c.bias_scale != 1.0)
    flags = (c.geglu, c.act, int(c.res), int(c.rowadd), int(c.bias), 0, 0, c.gn_groups, 0, scaled)
    return geom, flags


def _build():
    cases = []

    def add(group, N, H, W, Cin, Cout, ks=1, stride=1, up=0, pad=-1, geglu=0, act=0, ops="b", scales=(1.0, 1.0), gn=0,
            force=None, want=None, kind="grid", layouts=("dense",)):
        c = Case(group, N, H, W, Cin, Cout, ks, stride, up, pad, geglu, act, "b" in ops, "a" in ops, "r" in ops,
                 float(scales[0]), float(scales[1]), gn, force, None, kind, tuple(layouts))
        if want is None:                # a forced streamed tile or halo tile runs as itself
            v, sp = force
            M, K = gemm_dims(c)
            want = (v,) + launched(Cin // 64 if v in HALO else K // 64, sp, gn)
        cases.append(c._replace(want=tuple(want)))

    # ---- ring: every streamed tile and igemm3 against K = 1, 2, STAGES-1, STAGES, STAGES+1 slabs, pointwise, two ragged
    #      128-row tiles (one 256-row tile), 88 columns; and a split whose last slice is shorter than the ring ----
    for v, (bm, bn, st) in sorted(TILE.items()):
        for slabs in sorted({1, 2, st - 1, st, st + 1}):
            add("ring", 1, 130, 1, 64 * slabs, 88, ops="br", force=(v, 1))
        add("ring", 1, 130, 1, 64 * (st + 1), 88, ops="br", force=(v, 2))
    for slabs in (REG_TILE[2], REG_TILE[2] + 1):            # igemm3 takes K >= 64 * G3_STAGES only
        add("ring", 1, 130, 1, 64 * slabs, 88, ops="br", force=(REG, 1), want=(REG, 1, 0))

    # ---- edges: row and column counts around one tile; 3x3 on odd images, three of them inside one tile ----
    for v, (bm, bn, st) in sorted(TILE.items()):
        for M in (1, bm - 1, bm, bm + 1):
            for Cout in (8, bn - 8, bn, bn + 8):
                add("edges", 1, M, 1, 128, Cout, ops="b", force=(v, 1))
        for H, W in ((7, 9), (9, 7)):
            add("edges", 3, H, W, 64, 72, ks=3, ops="ba", force=(v, 1))

    # ---- gather: all nine taps as a pure copy; stride 1, stride 2 with pad 1 / pad 0, upsample; one streamed tile and
    #      both halo tiles (stride 1 and upsample only: halo_supported), patch widths 16 / 32 / 64, N = 2 so that an
    #      image boundary falls inside a tile; every split the halo launcher can make of three slabs ----
    for H, W in ((16, 16), (8, 32), (4, 64)):
        add("gather", 2, H, W, 128, 9 * 128, ks=3, ops="", force=(3, 1), kind="tap")
        add("gather", 2, H, W, 128, 9 * 128, ks=3, stride=2, ops="", force=(3, 1), kind="tap")
        add("gather", 2, H, W, 128, 9 * 128, ks=3, stride=2, pad=0, ops="", force=(3, 1), kind="tap")
        add("gather", 2, H // 2, W // 2, 128, 9 * 128, ks=3, up=1, ops="", force=(3, 1), kind="tap")
        for v in sorted(HALO):
            for sp in (1, 2, 3):
                add("gather", 2, H, W, 192, 9 * 192, ks=3, ops="", force=(v, sp), kind="tap")
                add("gather", 2, H // 2, W // 2, 192, 9 * 192, ks=3, up=1, ops="", force=(v, sp), kind="tap")
    add("gather", 2, 7, 9, 64, 9 * 64, ks=3, ops="", force=(4, 1), kind="tap")          # odd image, ragged tiles
    add("gather", 2, 7, 9, 64, 9 * 64, ks=3, stride=2, pad=0, ops="", force=(4, 1), kind="tap")
    add("gather", 2, 7, 9, 64, 9 * 64, ks=3, stride=2, ops="", force=(4, 1), kind="tap")
    add("gather", 2, 7, 9, 64, 9 * 64, ks=3, up=1, ops="", force=(4, 1), kind="tap")

    # ---- epilogue: operand sets and the scaled form on a fused launch, behind each reducer, on a halo tile, on
    #      wsgemm 13 and igemm3 (the sets those take); the two activations on the tiles the planner gives them ----
    sets = [("b", (1, 1)), ("ba", (1, 1)), ("br", (1, 1)), ("bar", (1, 1)), ("bar", (2.0 ** -3, 2.0 ** 3)),
            ("bar", (2.0 ** 3, 2.0 ** -3)), ("b", (2.0 ** -3, 2.0 ** -3)), ("b", (2.0 ** 3, 2.0 ** 3))]
    for ops, sc in sets:
        add("epilogue", 2, 8, 8, 128, 72, ks=3, ops=ops, scales=sc, force=(3, 1))                   # fused
        add("epilogue", 2, 8, 8, 128, 72, ks=3, ops=ops, scales=sc, force=(3, 2))                   # reducer 1
        add("epilogue", 2, 8, 8, 128, 64, ks=3, ops=ops, scales=sc, gn=8, force=(3, 2))             # reducer 2
        add("epilogue", 2, 16, 16, 64, 72, ks=3, ops=ops, scales=sc, force=(10, 1))                 # halo, fused
        add("epilogue", 2, 16, 16, 128, 72, ks=3, ops=ops, scales=sc, force=(15, 2))                # halo, reducer 1
    for ops in ("b", "br", ""):
        add("epilogue", 1, 1024, 1, 320, 160, ops=ops, force=(13, 1), want=(13, 1, 0))
        add("epilogue", 1, 130, 1, 256, 88, ops=ops, force=(REG, 1), want=(REG, 1, 0))
    for act in (1, 2):
        add("epilogue", 1, 130, 1, 128, 88, act=act, ops="b", want=(4, 1, 0), kind="randn")
        add("epilogue", 1, 130, 1, 128, 88, act=act, ops="br", want=(4, 1, 0), kind="randn")
        add("epilogue", 1, 4096, 1, 64, 512, act=act, ops="b", want=(3, 1, 0), kind="randn")
        add("epilogue", 1, 2048, 1, 64, 2048, act=act, ops="b", want=(1, 1, 0), kind="randn")

    # ---- strided: the engine's layouts (x a column slice, y / res the left or the right columns of a concatenation
    #      buffer), one case per family; bit-identical to the dense run ----
    lay = ("dense", "left", "right")
    add("strided", 2, 7, 9, 128, 72, ks=3, ops="bar", force=(3, 1), layouts=lay)                    # Tile 3x3
    add("strided", 1, 130, 1, 128, 200, ops="br", force=(2, 1), layouts=lay)                        # Tile pointwise
    add("strided", 2, 16, 16, 64, 200, ks=3, ops="bar", force=(10, 1), layouts=lay)                 # Halo
    add("strided", 2, 4, 16, 64, 136, ks=3, up=1, ops="bar", force=(15, 1), layouts=lay)            # Halo + upsample
    add("strided", 2, 8, 8, 128, 72, ks=3, ops="bar", force=(3, 2), layouts=lay)                    # reducer 1
    add("strided", 2, 8, 8, 128, 64, ks=3, ops="bar", gn=8, force=(3, 2), layouts=lay)              # reducer 2
    add("strided", 2, 16, 16, 128, 72, ks=3, ops="bar", force=(10, 2), layouts=lay)                 # Halo, reducer 1
    add("strided", 1, 1024, 1, 320, 160, ops="br", force=(13, 1), want=(13, 1, 0), layouts=lay)     # wsgemm plain
    add("strided", 1, 1024, 1, 320, 256, geglu=1, ops="b", force=(14, 1), want=(14, 1, 0), kind="sat", layouts=lay)
    add("strided", 1, 130, 1, 256, 88, ops="br", force=(REG, 1), want=(REG, 1, 0), layouts=lay)     # igemm3
    add("strided", 1, 2048, 1, 128, 8192, geglu=1, ops="b", want=(100, 1, 0), kind="sat", layouts=lay)     # pgemm
    add("strided", 2, 7, 9, 64, 12, ks=3, ops="bar", want=(-1, 1, 0), layouts=lay)                  # igemm1
    add("strided", 1, 130, 1, 128, 256, geglu=1, ops="b", force=(1, 1), want=(1, 1, 0), kind="sat", layouts=lay)

    # ---- routes: the smallest problems the planner sends, unforced, to wsgemm 13 / 14, the persistent GEGLU and the
    #      old igemm kernel, and igemm3 under force; GEGLU tiles with the saturated gate; one randn case each ----
    for kind in ("grid", "randn"):
        add("routes", 1, 1024, 1, 320, 160, ops="b", want=(13, 1, 0), kind=kind)
        add("routes", 1, 256, 1, 256, 80, ops="br", force=(REG, 1), want=(REG, 1, 0), kind=kind)
        for Cout in (3, 4, 12):
            add("routes", 1, 5, 7, 64, Cout, ks=3, ops="bar", want=(-1, 1, 0), kind=kind)
    for kind in ("sat", "randn"):
        add("routes", 1, 1024, 1, 320, 128, geglu=1, ops="b", want=(14, 1, 0), kind=kind)
        add("routes", 1, 2048, 1, 128, 8192, geglu=1, ops="b", want=(100, 1, 0), kind=kind)
        for v in GEGLU_TILES:
            add("routes", 1, 258, 1, 192, 384, geglu=1, ops="b", force=(v, 1), want=(v, 1, 0), kind=kind)
    add("routes", 2, 7, 9, 64, 12, ks=3, stride=2, ops="b", want=(-1, 1, 0))
    add("routes", 2, 4, 5, 64, 12, ks=3, up=1, ops="b", want=(-1, 1, 0))
    # randn on the families the groups above run with exact inputs only: streamed tile (fused and split), halo
    add("routes", 2, 7, 9, 128, 72, ks=3, ops="bar", force=(3, 1), kind="randn")
    add("routes", 2, 8, 8, 128, 72, ks=3, ops="bar", force=(3, 2), kind="randn")
    add("routes", 2, 8, 8, 128, 64, ks=3, ops="bar", gn=8, force=(3, 2), kind="randn")
    add("routes", 2, 16, 16, 128, 200, ks=3, ops="bar", force=(10, 1), kind="randn")
    add("routes", 2, 4, 16, 128, 136, ks=3, up=1, ops="bar", force=(15, 2), kind="randn")
    add("routes", 2, 9, 7, 64, 72, ks=3, stride=2, pad=0, ops="b", scales=(2.0 ** -3, 2.0 ** 3), force=(4, 1), kind="randn")
    return cases


CASES = _build()

# sd_op_conv3x3_small_cout (conv_out, NCHW output): (N, H, W, Cin, Cout, kind)
SMALL_COUT_CASES = [(2, H, W, 64, Cout, kind) for (H, W) in ((13, 37), (8, 8)) for Cout in (1, 3, 4)
                    for kind in ("grid", "tap")]


def small_cout_id(sc):
    return "smallcout-%dx%dx%dx%d-o%d-%s" % sc


def small_cout_case(sc):
    N, H, W, Cin, Cout, kind = sc
    return Case("smallcout", N, H, W, Cin, Cout, 3, 1, 0, -1, 0, 0, True, False, False, 1.0, 1.0, 0, None, None, kind,
                ("dense",))


def seed_of(c):
    return zlib.crc32(case_id(c).encode()) & 0x7fffffff


def tap_of(c, co):
    """The tap (kh * 3 + kw) output channel co copies under kind "tap"; the small-Cout cases start theirs at an offset
    by (Cout, H) chosen so that between them they use all nine (test_conv_plan checks that)."""
    if c.Cout >= 9 * c.Cin:
        return (co // c.Cin) % 9
    return (5 * (c.Cout - 1) + 4 * (c.H % 2 == 0) + co) % 9


def _grid16(shape, lim, g):
    """Multiples of 1/16 in [-lim, lim]."""
    n = int(lim * 16)
    return torch.randint(-n, n + 1, shape, generator=g).float() / 16.0


def make_inputs(c):
    """x [N, H, W, Cin] fp16 (NHWC), w [Cout, Cin, ks, ks] fp16, bias [Cout] fp32 | None, rowadd [N, Cout] fp32 | None,
    res [N, OH, OW, out_cols] fp16 | None."""
    g = torch.Generator().manual_seed(seed_of(c))
    OH, OW = out_size(c)
    M, K = gemm_dims(c)
    oc = out_cols(c)
    wshape = (c.Cout, c.Cin, c.ks, c.ks)
    bias = rowadd = res = None
    if c.kind == "randn":
        x = torch.randn(c.N, c.H, c.W, c.Cin, generator=g).half()
        w = (torch.randn(wshape, generator=g) / math.sqrt(K)).half()
        if c.bias:
            bias = torch.randn(c.Cout, generator=g) * 0.5
        if c.rowadd:
            rowadd = torch.randn(c.N, c.Cout, generator=g) * 0.5
        if c.res:
            res = torch.randn(c.N, OH, OW, oc, generator=g).half()
        return x, w, bias, rowadd, res
    if c.kind == "tap":
        assert c.ks == 3 and not (c.rowadd or c.res)
        x = torch.randn(c.N, c.H, c.W, c.Cin, generator=g).half()
        perm = torch.randperm(c.Cin, generator=g)
        w = torch.zeros(wshape)
        for co in range(c.Cout):
            t = tap_of(c, co)
            w[co, perm[co % c.Cin], t // 3, t % 3] = 1.0
        if c.bias:                       # (small-Cout entry: the bias is not optional there)
            bias = torch.zeros(c.Cout)
        return x, w.half(), bias, None, None
    x = torch.randint(-2, 3, (c.N, c.H, c.W, c.Cin), generator=g).half()
    w = torch.randint(-1, 2, wshape, generator=g).float() / 16.0
    if c.acc_scale > c.bias_scale:
        # the accumulator scaled up next to a bias scaled down: multiples of 1/128 are fp16 numbers only below 16, so
        # the sums are kept small with sparse weights (one in 128 non-zero); still on the grid
        w = w * (torch.rand(wshape, generator=g) < 1.0 / 128).float()
    if c.bias:
        bias = _grid16((c.Cout,), 0.5, g)
    if c.rowadd:
        rowadd = _grid16((c.N, c.Cout), 0.5, g)
    if c.res:
        res = _grid16((c.N, OH, OW, oc), 2.0, g).half()
    if c.kind == "sat":
        assert c.geglu and c.bias and not c.act
        w[c.Cout // 2:] = 0.0
        bias[c.Cout // 2:] = 16.0
    else:
        assert c.kind == "grid"
    return x, w.half(), bias, rowadd, res


def _conv(c, x_nchw, w):
    if c.up:
        x_nchw = F.interpolate(x_nchw, scale_factor=2.0, mode="nearest")
    pad = c.pad if c.pad >= 0 else (1 if c.ks == 3 else 0)
    if c.stride > 1 and pad == 0 and c.ks == 3:
        x_nchw = F.pad(x_nchw, (0, 1, 0, 1))            # the VAE encoder's downsample: a zero column right and below
    return F.conv2d(x_nchw, w, None, stride=c.stride, padding=pad)


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def _activation_error(act, v):
    """What evaluating the activation in fp32 may add at argument v, from the published accuracy of what the kernels
    evaluate, not from their output: erf by Abramowitz-Stegun 7.1.26 (absolute error of erf below 1.5e-7, hence
    0.5 |v| 1.5e-7 on gelu), the hardware's exp2 and reciprocal at one ulp each, the exponent's argument (at most
    1.702 log2(e) |v| < 2.5 |v|) rounded once, and a handful of fp32 multiplications and additions."""
    a = (_gelu(v) if act == 2 else _quick_gelu(v)).abs()
    e = (8.0 + 4.0 * v.abs()) * U32 * a
    if act == 2:
        e = e + 0.5 * v.abs() * (1.5e-7 + 4.0 * U32)
    return e


def geglu_reference(h, gt, dh, dg):
    """(h gelu(g), bound) of the GEGLU rounding point below, from the two halves ahead of any rounding to fp16 and what
    each may be off by (shared with tests/ln_cases.py)."""
    dg = 1.13 * dg + _activation_error(2, gt)
    r = h * _gelu(gt)
    return r, dh * _gelu(gt).abs() + h.abs() * dg + dh * dg + U16 * r.abs() + 2.0 ** -25


def reference(c, x, w, bias, rowadd, res):
    """float64 on the CPU of the fp16 / fp32 operands: (r, bound), both [N, OH, OW, out_cols] float64.

    The bound, derived from the reference alone.  Let v = acc_scale * conv + bias_scale * bias + rowadd be the value
    ahead of any rounding to fp16 and A the same expression on absolute values.  The kernels accumulate the K products
    (exact in fp32: fp16 x fp16) and the epilogue terms in fp32 in some order: at most K + 3 roundings of partial sums
    none of which exceeds A in magnitude, so |v_kernel - v| <= delta = (K + 3) u32 A + 2^-25 with u32 = 2^-23, one bit
    wider than round-to-nearest fp32 because the MFMA's internal rounding is not documented as RNE; the scales are
    powers of two and add nothing.  Any order is covered, hence any tile, ring depth and split-K reduction.  2^-25 is
    half the smallest fp16 subnormal step.
      plain       y = fp16(v):               |err| <= u16 |v| + delta
      activation  p = act(v), L = sup |act'| (1.13 for gelu, 1.1 for quick_gelu):
                                             |p_kernel - p| <= L delta + activation_error(v) =: d
      residual    y = fp16(fp16(p) + res) (rounded before the add) or fp16(p + res): either way
                                             |err| <= u16 (|p| + |p + res|) + d
      GEGLU       y = fp16(h gelu(g)) with h, g the two halves of v, each within its own delta:
                  |err| <= dh |gelu(g)| + |h| dg' + dh dg' + u16 |y| + 2^-25,   dg' = 1.13 dg + activation_error(g)"""
    xd = x.double().permute(0, 3, 1, 2)
    wd = w.double()
    M, K = gemm_dims(c)
    conv = _conv(c, xd, wd)
    A = c.acc_scale * _conv(c, xd.abs(), wd.abs())
    v = c.acc_scale * conv
    if bias is not None:
        v = v + c.bias_scale * bias.double()[None, :, None, None]
        A = A + c.bias_scale * bias.double().abs()[None, :, None, None]
    if rowadd is not None:
        v = v + rowadd.double()[:, :, None, None]
        A = A + rowadd.double().abs()[:, :, None, None]
    v = v.permute(0, 2, 3, 1).contiguous()
    delta = (K + 3) * U32 * A.permute(0, 2, 3, 1).contiguous() + 2.0 ** -25
    if c.geglu:
        assert not c.act and res is None
        h, gt = v.chunk(2, dim=-1)
        dh, dg = delta.chunk(2, dim=-1)
        return geglu_reference(h, gt, dh, dg)
    p, d = v, delta
    if c.act:
        p = _gelu(v) if c.act == 2 else _quick_gelu(v)
        d = (1.13 if c.act == 2 else 1.1) * delta + _activation_error(c.act, v)
    if res is None:
        return p, U16 * p.abs() + d
    r = p + res.double()
    return r, U16 * (p.abs() + r.abs()) + d


@functools.lru_cache(maxsize=4)
def inputs_and_reference(c):
    """(x, w, bias, rowadd, res, r, bound) of a case, computed once for the tests that run it; not to be modified."""
    ins = make_inputs(c)
    return ins + reference(c, *ins)


def emulate(c, x, w, bias, rowadd, res, nsplit):
    """The kernels' arithmetic in torch on the CPU: fp32 accumulation over 64-deep K slabs in K order (nsplit == 1), or
    as `nsplit` partial sums over runs of slabs added afterwards; the epilogue in fp32; fp16 where the kernels round
    (the stored value, and ahead of the residual add).  [N, OH, OW, out_cols] fp16."""
    xf = x.float().permute(0, 3, 1, 2)
    if c.up:
        xf = F.interpolate(xf, scale_factor=2.0, mode="nearest")
    pad = c.pad if c.pad >= 0 else (1 if c.ks == 3 else 0)
    if c.stride > 1 and pad == 0 and c.ks == 3:
        xf = F.pad(xf, (0, 1, 0, 1))
    OH, OW = out_size(c)
    M, K = gemm_dims(c)
    cols = F.unfold(xf, c.ks, padding=pad, stride=c.stride)             # [N, K, OH * OW]
    a = cols.transpose(1, 2).reshape(M, K)
    b = w.float().reshape(c.Cout, K)
    slabs = K // 64
    per = cdiv(slabs, nsplit)
    parts = []
    for s0 in range(0, slabs, per):
        acc = torch.zeros(M, c.Cout)
        for s in range(s0, min(s0 + per, slabs)):
            acc = acc + a[:, s * 64:(s + 1) * 64] @ b[:, s * 64:(s + 1) * 64].t()
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    v = acc * torch.tensor(c.acc_scale)
    if bias is not None:
        v = v + bias * torch.tensor(c.bias_scale)
    v = v.view(c.N, OH * OW, c.Cout)
    if rowadd is not None:
        v = v + rowadd[:, None, :]
    v = v.view(c.N, OH, OW, c.Cout)
    if c.geglu:
        h, gt = v.chunk(2, dim=-1)
        return (h * F.gelu(gt)).half()
    if c.act:
        v = F.gelu(v) if c.act == 2 else v * torch.sigmoid(1.702 * v)
    y = v.half()
    if res is not None:
        y = (y.float() + res.float()).half()
    return y
