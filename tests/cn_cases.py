"""Cases, inputs, float64 reference, error bound and an emulation of cn_cond_conv_kernel's arithmetic (one layer of the
ControlNet conditioning embedding: 3x3 conv, pad 1, stride 1 or 2, bias, SiLU), and the problem tables and the bound of
the grouped zero-conv launch; shared by tests/test_cn_cases.py (CPU) and tests/test_controlnet_gpu.py (GPU).  Nothing
here touches a device."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

U16, U32 = 2.0 ** -11, 2.0 ** -23       # fp16 unit roundoff; one fp32 ulp (twice the unit roundoff), as tests/test_multi_controlnet_gpu.py
LOG2E = 1.4426950408889634
SILU_SLOPE = 1.1                        # max |silu'| = 1.0998...

# Cin = 3 reads the NCHW control image, the others NHWC; Cout / 16 block rows (blockIdx.y); N * OH * OW output pixels,
# 256 per block
Case = collections.namedtuple("Case", "Cin Cout stride N IH IW silu")
CASES = [
    Case(3, 16, 1, 1, 16, 16, 1),       # 256 pixels: exactly one block
    Case(3, 32, 2, 3, 9, 13, 1),        # odd sizes at stride 2: 9 x 13 -> 5 x 7, 105 pixels
    Case(3, 16, 1, 1, 1, 1, 1),         # a 1 x 1 image: every tap but the centre is outside
    Case(3, 96, 2, 1, 40, 36, 0),       # 360 pixels, six block rows, no activation
    Case(16, 32, 1, 3, 10, 11, 1),      # 330 pixels: a second block with a tail
    Case(16, 96, 2, 1, 33, 31, 1),      # 17 x 16 = 272
    Case(16, 16, 2, 3, 1, 20, 1),       # 1 x W at stride 2
    Case(32, 32, 1, 1, 1, 37, 1),       # 1 x W
    Case(32, 96, 2, 3, 9, 13, 1),
    Case(32, 16, 1, 1, 16, 32, 1),      # 512 pixels: two whole blocks
    Case(96, 96, 1, 1, 7, 9, 1),        # 63 pixels: less than one block
    Case(96, 16, 2, 3, 21, 19, 1),      # 11 x 10 x 3 = 330
    Case(96, 32, 2, 1, 1, 1, 1),
]


def case_id(c):
    return "cin%d-cout%d-s%d-N%d-%dx%d%s" % (c.Cin, c.Cout, c.stride, c.N, c.IH, c.IW, "" if c.silu else "-linear")


def out_hw(c):
    return (c.IH - 1) // c.stride + 1, (c.IW - 1) // c.stride + 1


def make_inputs(c):
    """fp16 x [N, Cin, IH, IW] (NCHW whatever the kernel's layout; the GPU test permutes), w [Cout, Cin, 3, 3], bias
    [Cout]; scaled so that the pre-activation has a standard deviation of about 2 and both signs."""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) & 0x7fffffff)
    if c.Cin == 3:
        x = torch.rand(c.N, 3, c.IH, c.IW, generator=g)                     # an image in [0, 1)
        w = torch.randn(c.Cout, 3, 3, 3, generator=g) * (2.0 / (27 / 3.0) ** 0.5)
    else:
        x = torch.randn(c.N, c.Cin, c.IH, c.IW, generator=g)
        w = torch.randn(c.Cout, c.Cin, 3, 3, generator=g) * (2.0 / (9 * c.Cin) ** 0.5)
    b = 0.3 * torch.randn(c.Cout, generator=g)
    return x.half(), w.half(), b.half()


def reference(c, x, w, b):
    """float64 on the fp16 operands: (silu(y) or y, y, A = |b| + sum |x| |w|), each [N, OH, OW, Cout]."""
    y = F.conv2d(x.double(), w.double(), b.double(), stride=c.stride, padding=1).permute(0, 2, 3, 1)
    A = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride=c.stride, padding=1).permute(0, 2, 3, 1)
    return (F.silu(y) if c.silu else y), y, A


@functools.lru_cache(maxsize=None)
def inputs_and_reference(c):
    """(x, w, b, out, y, A), computed once; callers must not modify them."""
    ins = make_inputs(c)
    return ins + reference(c, *ins)


def bound(c, out, y, A):
    """|kernel - out| may not exceed this.  From cn_cond_conv_kernel's arithmetic:
      * acc starts at the bias and takes 9 Cin fp32 FMAs in sequence (a tap outside the image multiplies by zero and
        changes nothing); every partial sum is at most A in magnitude, each FMA rounds once:  9 Cin u32 A on y;
      * silu_f (common.h) is y * rcp(1 + exp2(-log2(e) * y)): the product in exp2's argument (one rounding, which moves
        the exponential by |y| u32 relative), exp2 (an ulp), the addition, rcp (an ulp), the final product: six roundings
        relative to |silu(y)| <= A, plus |y| u32 |silu(y)|; the error of y passes through silu with slope <= 1.1:
        1.1 (9 Cin + 6) u32 A + u32 |y| |silu(y)|  (without the activation the same expression is merely generous);
      * one fp16 store, u16 |out|, and 2^-25 for an output in fp16's subnormal range."""
    return U16 * out.abs() + SILU_SLOPE * (9 * c.Cin + 6) * U32 * A + U32 * y.abs() * out.abs() + 2.0 ** -25


def border_ring(c):
    """[OH, OW] bool: the output pixels with a tap outside the image on at least one side."""
    OH, OW = out_hw(c)
    ring = torch.zeros(OH, OW, dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    return ring


def _fma(a, w, acc):
    """fp32 fma: the product of two fp32 values is exact in float64."""
    return (a.double() * w.double() + acc.double()).float()


def emulate(c, x, w, b, mutant=None):
    """The kernel's arithmetic in torch on the CPU: fp32 accumulators started at the bias, one FMA per (ky, kx, channel)
    in that order, silu_f's operations in fp32, one rounding to fp16.  Returns [N, OH, OW, Cout] fp16.
    mutant "no_pad": the clamped pixel of a tap outside the image is added instead of zero."""
    OH, OW = out_hw(c)
    xf, wf = x.float(), w.float()
    assert mutant in (None, "no_pad")
    xp = F.pad(xf, (1, 1, 1, 1), mode="replicate" if mutant == "no_pad" else "constant")
    acc = b.float().expand(c.N, OH, OW, c.Cout).clone()
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + c.stride * (OH - 1) + 1:c.stride, kx:kx + c.stride * (OW - 1) + 1:c.stride]
            for ci in range(c.Cin):
                acc = _fma(xs[:, ci, :, :, None], wf[:, ci, ky, kx], acc)
    if c.silu:
        t = torch.tensor(-LOG2E, dtype=torch.float32) * acc
        acc = acc * (1.0 / (1.0 + torch.exp2(t)))
    return acc.half()


# ---------------------------------------------------------------------------------------- grouped zero-convs
# One table of 16 problems (the most a launch takes), every M twice and every C four times, and a table of one.
RES_M = (1, 31, 32, 33, 127, 128, 129, 257)         # around the 32-row wave slab and the 128-row tile
RES_C = (64, 128, 320, 1280)
RES_TABLES = {
    "sixteen": [(M, RES_C[(i + i // 8) % 4]) for i, M in enumerate(RES_M + RES_M)],
    "one": [(129, 320)],
}
RES_SCALE = 0.8


def residual_problem(M, C_, seed):
    """fp16 x [M, C], w [C, C], fp32 bias [C], fp16 y0 [M, C]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C_, generator=g).half()
    w = (torch.randn(C_, C_, generator=g) / C_ ** 0.5).half()
    b = 0.1 * torch.randn(C_, generator=g)
    y0 = torch.randn(M, C_, generator=g).half()
    return x, w, b, y0


def residual_reference(x, w, b, y0, s):
    """float64: (y0 + t, bound) with t = s (x w^T + b).  The bound is the n = 1 form of bound (c) of
    tests/test_multi_controlnet_gpu.py::test_residual_op_element_by_element: u16 (|t| + |y0 + t|) + (C + 5) u32 A + 2^-25,
    A = |s| (|x| |w|^T + |b|)."""
    t = s * (x.double() @ w.double().t() + b.double()[None, :])
    A = abs(s) * (x.double().abs() @ w.double().abs().t() + b.double().abs()[None, :])
    want = y0.double() + t
    return want, U16 * (t.abs() + want.abs()) + (x.shape[1] + 5) * U32 * A + 2.0 ** -25
