"""Shared by tests/test_upconv_fold.py (CPU) and tests/test_upconv_fold_gpu.py: the fold of "nearest-2x upsample, then
3x3 conv" into four 2x2 convolutions on the input map, restated in numpy / torch, its float64 reference and the
element-wise bound of the folded kernel.

The identity, for output pixel (2i + dy, 2j + dx), dy, dx in {0, 1} (x = 0 outside the image):
    y[2i+dy, 2j+dx] = bias + sum_{a,b in {0,1}} W'_{dy,dx}[a, b] . x[i + a - 1 + dy, j + b - 1 + dx]
    rows     dy = 0: W'[a=0] = W[kh=0],           W'[a=1] = W[kh=1] + W[kh=2]
             dy = 1: W'[a=0] = W[kh=0] + W[kh=1], W'[a=1] = W[kh=2]            columns likewise with dx / kw
"""
import numpy as np
import torch
import torch.nn.functional as F

U16 = 2.0 ** -11
TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}       # TAPS[d][a] = kernel rows (columns) summed into tap a of parity d


def fold64(w):
    """w [O, I, 3, 3] -> {(dy, dx): [O, I, 2, 2]} in w's dtype by plain sums (exact in float64 for fp16 inputs)."""
    out = {}
    for dy in (0, 1):
        for dx in (0, 1):
            f = torch.zeros(w.shape[0], w.shape[1], 2, 2, dtype=w.dtype)
            for a in (0, 1):
                for b in (0, 1):
                    for kh in TAPS[dy][a]:
                        for kw in TAPS[dx][b]:
                            f[:, :, a, b] += w[:, :, kh, kw]
            out[(dy, dx)] = f
    return out


def fold_np(w16):
    """The engine's folded pack of fp16 w [O, I, 3, 3]: [4][O][4 I] fp16, panel dy * 2 + dx, K order [I/64][a][b][64];
    the taps summed in fp32 from 0, kernel rows outside and columns inside, then rounded to fp16 once (numpy: RNE)."""
    w = w16.numpy().astype(np.float32)
    O, I = w.shape[:2]
    out = np.zeros((4, O, I // 64, 2, 2, 64), dtype=np.float16)
    for dy in (0, 1):
        for dx in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    s = np.zeros((O, I), dtype=np.float32)
                    for kh in TAPS[dy][a]:
                        for kw in TAPS[dx][b]:
                            s = s + w[:, :, kh, kw]
                    out[dy * 2 + dx, :, :, a, b, :] = s.astype(np.float16).reshape(O, I // 64, 64)
    return torch.from_numpy(out.reshape(4, O, 4 * I))


def unpack_fold(panels, O, I):
    """[4][O][4 I] in the engine's K order -> {(dy, dx): [O, I, 2, 2]}."""
    p = panels.reshape(4, O, I // 64, 2, 2, 64).permute(0, 1, 2, 5, 3, 4).reshape(4, O, I, 2, 2)
    return {(dy, dx): p[dy * 2 + dx] for dy in (0, 1) for dx in (0, 1)}


def parity_conv(x_nchw, wf, bias=None):
    """The four 2x2 convolutions: x [N, C, H, W], wf {(dy, dx): [O, C, 2, 2]} -> [N, O, 2H, 2W] (dtype of x)."""
    N, _, H, W = x_nchw.shape
    O = wf[(0, 0)].shape[0]
    y = torch.zeros(N, O, 2 * H, 2 * W, dtype=x_nchw.dtype)
    for (dy, dx), w2 in wf.items():
        xp = F.pad(x_nchw, (1 - dx, dx, 1 - dy, dy))
        y[:, :, dy::2, dx::2] = F.conv2d(xp, w2.to(x_nchw.dtype), bias)
    return y


def upconv_ref64(x_nhwc, w, bias, acc_scale=1.0, bias_scale=1.0):
    """float64 acc_scale * conv3x3(nearest_up(x)) + bias_scale * bias on the ORIGINAL weights -> [N, 2H, 2W, O]."""
    xd = F.interpolate(x_nhwc.permute(0, 3, 1, 2).double(), scale_factor=2, mode="nearest")
    r = acc_scale * F.conv2d(xd, w.double(), None, padding=1)
    if bias is not None:
        r = r + bias_scale * bias.double()[None, :, None, None]
    return r.permute(0, 2, 3, 1).contiguous()


def upconv_bound(x_nhwc, w, ref, acc_scale=1.0):
    """Element-wise bound of the folded kernel against upconv_ref64, from the arithmetic alone.

    The kernel stores fp16(v), v = acc_scale * sum_k W16'_k x_k + bias_scale * bias, where W16' = fp16(fp32 sum of the
    taps) and the 4 Cin products (exact in fp32: fp16 x fp16) are accumulated in fp32.  With S = acc_scale * sum |W'| |x|
    on the exactly folded weights W':
      * the store rounds once:                                      2^-11 |ref| (+ second order)
      * a folded weight is rounded to fp16 once, |W16' - W'| <= 2^-11 |W'| (the <= 3 fp32 roundings of its sum are
        2^-24 each and go into the next term); a subnormal one is off by at most 2^-25:   2^-11 S + 2^-25 acc sum |x|
      * 4 Cin accumulations, each rounding a partial sum no larger than S:                 4 Cin 2^-24 S
      * 2^-25: half the smallest fp16 step, for a result that lands among the subnormals."""
    Cin = x_nhwc.shape[-1]
    xa = x_nhwc.permute(0, 3, 1, 2).double().abs()
    wf = {k: v.abs() for k, v in fold64(w.double()).items()}
    S = acc_scale * parity_conv(xa, wf).permute(0, 2, 3, 1)
    sx = acc_scale * parity_conv(xa, {k: torch.ones(1, Cin, 2, 2, dtype=torch.float64) for k in wf}).permute(0, 2, 3, 1)
    return U16 * ref.abs() + (U16 + 4 * Cin * 2.0 ** -24) * S + 2.0 ** -25 * sx + 2.0 ** -25


def emulate(x_nhwc, w, bias, acc_scale=1.0, bias_scale=1.0):
    """The folded kernel's arithmetic in torch on the CPU: fp16 folded weights (fold_np), fp32 accumulation, fp32
    epilogue, one rounding to fp16 -> [N, 2H, 2W, O] fp16."""
    O, I = w.shape[:2]
    wf = {k: v.float() for k, v in unpack_fold(fold_np(w), O, I).items()}
    v = acc_scale * parity_conv(x_nhwc.permute(0, 3, 1, 2).float(), wf)
    if bias is not None:
        v = v + bias_scale * bias.float()[None, :, None, None]
    return v.permute(0, 2, 3, 1).contiguous().half()


def exact_operands(N, H, W, Cin, Cout, seed):
    """x in {-2..2} / 8, weights in {-1, 0, 1}, integer bias: every product, every folded weight (|W'| <= 4) and every
    partial sum (a multiple of 1/8 below 9 * 2 * Cin / 8 < 2^12) is exact in fp16 / fp32, so the 9-tap and the folded
    kernel round the same fp32 value to fp16 and must agree bit for bit."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-2, 3, (N, H, W, Cin), generator=g).float() / 8).half()
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).half()
    b = torch.randint(-4, 5, (Cout,), generator=g).float()
    return x, w, b


def randn_operands(N, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    b = torch.randn(Cout, generator=g)
    return x, w, b


# (N, H, W, Cin, Cout) of the random-input cases: every patch width, two patches per image, both column tiles (160
# where Cout % 160 == 0), a ragged last tile and more than two tiles
RANDN_CASES = [(1, 16, 16, 64, 8), (2, 8, 32, 128, 136), (1, 4, 64, 192, 128), (2, 32, 16, 64, 328), (1, 16, 48, 128, 320)]
