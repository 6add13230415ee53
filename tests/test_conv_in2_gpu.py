"""conv_head2_kernel through sd_op_unet_conv_in2: conv_in from two NCHW sources in one launch,
    y[n] = conv3x3(cat(fp16(a[n % Na] * in_scale), n < zero_from ? b[n % Nb] : 0)) + bias,
exact cases bit for bit against torch on the CPU, random cases per element against float64, the GroupNorm summaries
against the stored values, guards, and the refused shapes."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pix2pix import call_conv_in2, conv_in2_refusals  # noqa: E402

pytestmark = pytest.mark.gpu

COUT, G = 320, 32
GUARD_ROWS = 3
SENTINEL = 777.0
HW = [(8, 16), (16, 16), (16, 24)]                     # one tile per image, two tiles, tiles that start mid-row
BATCH = [(1, 1, 1, 1), (3, 1, 1, 2), (6, 2, 2, 4), (2, 2, 2, 2)]       # (N, Na, Nb, zero_from)
CHANNELS = [(4, 4), (4, 5), (7, 7), (4, 1)]            # K = 72, 81, 126 (two chunks), 45 (one)
IRRATIONAL = torch.tensor(1.0 / math.sqrt(14.6 ** 2 + 1.0), dtype=torch.float32).item()
SCALES = [1.0, 0.5, IRRATIONAL]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def sample_of(a, b, N, zero_from, scale):
    """The concatenated sample the kernel never builds, fp16: scaled latents rounded once, zeros from zero_from on."""
    Na, Nb = a.shape[0], b.shape[0]
    rows = []
    for n in range(N):
        lat = (a[n % Na].float() * scale).half()
        img = b[n % Nb] if n < zero_from else torch.zeros_like(b[0])
        rows.append(torch.cat([lat, img], dim=0))
    return torch.stack(rows)


def launch(lib, a, b, w, bias, N, zero_from, scale, ldy=COUT, groups=G):
    """-> (y [N, H, W, 320] fp16 on the CPU, summaries [N, S, groups, 2]); asserts that every guard is untouched."""
    H, W = a.shape[-2:]
    M, S = N * H * W, H * W // 128
    ybuf = torch.full((M + 2 * GUARD_ROWS, ldy), SENTINEL, dtype=torch.float16, device="cuda")
    sbuf = torch.full((N * S * groups * 2 + 32,), SENTINEL, dtype=torch.float32, device="cuda")
    y, summ = ybuf[GUARD_ROWS:], sbuf[16:]
    ad, bd, wd, biasd = a.cuda().contiguous(), b.cuda().contiguous(), w.cuda().contiguous(), bias.cuda().contiguous()
    rc = lib.sd_op_unet_conv_in2(P(ad), a.shape[0], a.shape[1], scale, P(bd), b.shape[0], b.shape[1], zero_from, P(wd),
                                 P(biasd), P(y), ldy, P(summ) if groups else None, groups, N, H, W, COUT, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    assert (ybuf[:GUARD_ROWS] == SENTINEL).all() and (ybuf[GUARD_ROWS + M:] == SENTINEL).all()
    assert (ybuf[:, COUT:] == SENTINEL).all()
    n_s = N * S * groups * 2
    assert (sbuf[:16] == SENTINEL).all() and (sbuf[16 + n_s:] == SENTINEL).all()
    assert torch.equal(ad.cpu(), a) and (torch.equal(bd.cpu(), b) or torch.isnan(b).any())
    return ybuf[GUARD_ROWS:GUARD_ROWS + M, :COUT].cpu().reshape(N, H, W, COUT), summ[:n_s].cpu().reshape(N, S, groups, 2)


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16))


def tap_weights(Cin):
    """Output channel co copies input channel co % Cin at tap (co // Cin) % 9: with 320 >= 9 Cin every (tap, channel)."""
    w = torch.zeros(COUT, Cin, 3, 3)
    for co in range(COUT):
        t = (co // Cin) % 9
        w[co, co % Cin, t // 3, t % 3] = 1.0
    return w.half()


@pytest.mark.parametrize("N,Na,Nb,zero_from", BATCH)
@pytest.mark.parametrize("H,W", HW)
def test_exact_cases_are_bit_for_bit(engine_lib, H, W, N, Na, Nb, zero_from):
    """One-hot weights and small-integer inputs: a pure gather, so the zero padding at all four borders, the source
    split, the n % Na mapping, the zero group and the rounding of the scaled latents show bit for bit.  The output of
    the one non-zero product plus a bias that is a multiple of 1/16 is one fp32 addition and one fp16 rounding in the
    kernel and in torch alike.  Also: images that read the same (a, b) pair are bit-identical, a row stride wider than
    320 leaves its extra columns alone, and with zero_from = 0 a second source full of NaNs is never read."""
    for Ca, Cb in CHANNELS:
        Cin = Ca + Cb
        g = torch.Generator().manual_seed(1000 * H + 100 * W + 10 * N + Cin)
        a = torch.randint(-8, 9, (Na, Ca, H, W), generator=g).half()
        b = torch.randint(-8, 9, (Nb, Cb, H, W), generator=g).half()
        w = tap_weights(Cin)
        bias = torch.randint(-8, 9, (COUT,), generator=g).float() / 16.0
        for scale in SCALES:
            x = sample_of(a, b, N, zero_from, scale)
            if scale == IRRATIONAL:
                assert not torch.equal(x[:, :Ca].float(), a[torch.arange(N) % Na].float() * scale)     # (it does round)
            want = F.conv2d(x.float(), w.float(), bias, padding=1).half().permute(0, 2, 3, 1)
            got, _ = launch(engine_lib, a, b, w, bias, N, zero_from, scale)
            assert same_bits(got, want), (Ca, Cb, scale)
            pairs = {}
            for n in range(N):
                key = (n % Na, n % Nb if n < zero_from else -1)
                first = pairs.setdefault(key, n)
                assert same_bits(got[n], got[first]), (n, first)
        want_half = F.conv2d(sample_of(a, b, N, zero_from, 0.5).float(), w.float(), bias, padding=1).half().permute(0, 2, 3, 1)
        wide, _ = launch(engine_lib, a, b, w, bias, N, zero_from, 0.5, ldy=COUT + 8)
        assert same_bits(wide, want_half), (Ca, Cb)
        nan_b = torch.full_like(b, float("nan"))
        got0, _ = launch(engine_lib, a, nan_b, w, bias, N, 0, 1.0)
        want0 = F.conv2d(sample_of(a, b, N, 0, 1.0).float(), w.float(), bias, padding=1).half().permute(0, 2, 3, 1)
        assert torch.isfinite(got0.float()).all() and same_bits(got0, want0), (Ca, Cb)


def _random_case(lib, H, W, N, Na, Nb, zero_from, Ca, Cb, offset, scale):
    Cin = Ca + Cb
    g = torch.Generator().manual_seed(7 * H + 3 * W + N + 13 * Cin + (1 if offset else 0))
    a = (torch.randn(Na, Ca, H, W, generator=g) * 3).half()
    b = torch.randn(Nb, Cb, H, W, generator=g).half()
    w = (torch.randn(COUT, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    bias = torch.randn(COUT, generator=g) * 0.3
    if offset is not None:
        w = (0.1 * w.float()).half()
        bias = offset + 0.05 * torch.randn(COUT, generator=g)
    x = sample_of(a, b, N, zero_from, scale)
    Y = F.conv2d(x.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), None, padding=1).permute(0, 2, 3, 1)
    got, summ = launch(lib, a, b, w, bias, N, zero_from, scale)
    # fp32 accumulation of K = 9 Cin terms and one fp16 rounding
    bound = 2.0 ** -11 * Y.abs() + 9 * Cin * 2.0 ** -23 * mag + 2.0 ** -24
    worst = ((got.double() - Y).abs() / bound).max().item()
    print(f"conv_in2 {H}x{W} N={N} Ca={Ca} Cb={Cb} offset={offset}: worst error / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all()
    assert worst <= 1.0, (H, W, N, Ca, Cb, offset, worst)
    # summaries of the stored values, tile = 128 consecutive pixels of one image (test_ops_gpu._conv_in_case's tolerances)
    S = H * W // 128
    t = got.float().reshape(N, S, 128, G, COUT // G)
    if offset is not None:
        t = t.double()
    mean = t.mean(dim=(2, 4))
    m2 = ((t - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    assert torch.allclose(summ[..., 0], mean.float(), atol=2e-5, rtol=1e-4)
    assert torch.allclose(summ[..., 1], m2.float(), atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("N,Na,Nb,zero_from", BATCH)
@pytest.mark.parametrize("H,W", HW)
def test_random_cases_stay_inside_the_rounding_bound(engine_lib, H, W, N, Na, Nb, zero_from):
    for Ca, Cb in CHANNELS:
        _random_case(engine_lib, H, W, N, Na, Nb, zero_from, Ca, Cb, None, IRRATIONAL)


@pytest.mark.parametrize("H,W,N,Na,Nb,zero_from,Ca,Cb", [(16, 24, 3, 1, 1, 2, 4, 4), (16, 16, 6, 2, 2, 4, 7, 7)])
def test_random_cases_at_a_large_offset(engine_lib, H, W, N, Na, Nb, zero_from, Ca, Cb):
    """Outputs 50 +- 0.1, as test_ops_gpu's conv_in case: the summaries are checked against float64."""
    _random_case(engine_lib, H, W, N, Na, Nb, zero_from, Ca, Cb, 50.0, 1.0)


@pytest.mark.parametrize("H,W", HW)
def test_second_source_is_not_read_from_zero_from_on(engine_lib, H, W):
    """One launch in which some images read b and others are zeroed: N = 4, Nb = 4, zero_from = 2, so images 0 and 1 read
    b[0] and b[1] and nothing may read b[2] and b[3] -- NaNs planted there do not reach the output, bit for bit."""
    N, Na, Nb, zero_from = 4, 2, 4, 2
    for Ca, Cb in CHANNELS:
        g = torch.Generator().manual_seed(31 * H + W + Ca + Cb)
        a = torch.randint(-8, 9, (Na, Ca, H, W), generator=g).half()
        b = torch.randint(-8, 9, (Nb, Cb, H, W), generator=g).half()
        b[zero_from:] = float("nan")
        w, bias = tap_weights(Ca + Cb), torch.randint(-8, 9, (COUT,), generator=g).float() / 16.0
        got, summ = launch(engine_lib, a, b, w, bias, N, zero_from, 0.5)
        want = F.conv2d(sample_of(a, b, N, zero_from, 0.5).float(), w.float(), bias, padding=1).half().permute(0, 2, 3, 1)
        assert torch.isfinite(got.float()).all() and torch.isfinite(summ).all(), (Ca, Cb)
        assert same_bits(got, want), (Ca, Cb)
        assert not same_bits(got[0], got[2])             # (images 0 and 2 share a[0]: the second source is live)


def test_without_summaries_nothing_is_written_to_them(engine_lib):
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(1, 4, 8, 16, generator=g).half(), torch.randn(1, 4, 8, 16, generator=g).half()
    w, bias = (torch.randn(COUT, 8, 3, 3, generator=g) / 8).half(), torch.zeros(COUT)
    with_s, _ = launch(engine_lib, a, b, w, bias, 1, 1, 1.0)
    without, _ = launch(engine_lib, a, b, w, bias, 1, 1, 1.0, groups=0)
    assert same_bits(with_s, without)


def test_other_shapes_are_refused_with_a_message(engine_lib):
    buf = torch.zeros(64, dtype=torch.float16, device="cuda")
    for label, shape in conv_in2_refusals():
        assert call_conv_in2(engine_lib, shape, buf.data_ptr(), stream()) == 1, label
        assert b"sd_op_unet_conv_in2" in engine_lib.sd_last_error(), label
    torch.cuda.synchronize()
    assert not buf.any()
