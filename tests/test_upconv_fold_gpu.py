"""The folded upsample convolution on the GPU (conv3x3_halo_up2x2_kernel, fold_upconv_kernel), at the
smallest shapes at which each mechanism can go wrong: every patch width (input maps 16x16, 8x32, 4x64), two patches per
image, one to three 64-channel slabs (the three-stage weight ring wraps inside a slab and across slabs), both column
tiles (160 where Cout % 160 == 0, else 128), a ragged last column tile and more than two of them.

tests/upconv_cases.py holds the numpy fold, the float64 reference and the bound; tests/test_upconv_fold.py proves the
bound on an emulation of the kernel's arithmetic on the CPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import upconv_cases as uc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
GUARD = 256                    # guard rows in front of and behind x and y
MAPS = [(16, 16), (8, 32), (4, 64), (32, 16), (16, 48)]


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def upconv(lib, x, w, b, N, H, W, Cin, Cout, y=None, ldx=None, ldy=None, scales=(1.0, 1.0), groups=0, summ=None):
    """sd_op_upconv2x_ex on device operands -> (y [N * 4HW, Cout] view, ran)."""
    M = N * 4 * H * W
    if y is None:
        y = torch.zeros(M, Cout, dtype=torch.float16, device="cuda")
    ran = (C.c_int * 4)()
    rc = lib.sd_op_upconv2x_ex(P(x), P(w), P(b), None, None, P(y), N, H, W, Cin, Cout, ldx or Cin, Cout, ldy or Cout,
                               scales[0], scales[1], groups, P(summ), ran, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return y, tuple(ran)


def ninetap(lib, x, w, b, N, H, W, Cin, Cout, scales=(1.0, 1.0)):
    """sd_op_conv2d_ex(up = 1): the 9-tap kernels, which build their own params and never see the fold."""
    y = torch.zeros(N * 4 * H * W, Cout, dtype=torch.float16, device="cuda")
    ran = (C.c_int * 4)()
    rc = lib.sd_op_conv2d_ex(P(x), P(w), P(b), None, None, P(y), N, H, W, Cin, Cout, 3, 1, 1, 0, Cin, Cout, Cout, -1, 0,
                             scales[0], scales[1], 0, ran, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("Cin", [64, 192])
@pytest.mark.parametrize("Cout", [8, 136])
def test_fold_kernel_bits(engine_lib, Cin, Cout):
    """sd_op_fold_upconv against the numpy fold (fp32 sums in the kernel's order, RNE to fp16), bit for bit."""
    _, w, _ = uc.randn_operands(1, 1, 1, Cin, Cout, seed=Cin + Cout)
    out = torch.full((4, Cout, 4 * Cin), float("nan"), dtype=torch.float16, device="cuda")
    assert engine_lib.sd_op_fold_upconv(P(w.cuda()), P(out), Cout, Cin, stream()) == 0, engine_lib.sd_last_error()
    assert torch.equal(out.cpu().view(torch.int16), uc.fold_np(w).view(torch.int16))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", MAPS)
def test_exact_inputs_equal_ninetap(engine_lib, N, H, W):
    """Inputs on which every product, folded weight and sum is exact: the folded kernel equals the 9-tap kernel bit for
    bit (and the float64 reference), for 1..3 slabs and one ragged / several column tiles."""
    for Cin in (64, 128, 192):
        for Cout in (8, 128, 136, 328):
            x, w, b = uc.exact_operands(N, H, W, Cin, Cout, seed=H * W + Cin + Cout)
            xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
            y, ran = upconv(engine_lib, xd, wd, bd, N, H, W, Cin, Cout)
            assert ran[0] == 1, "the folded kernel did not run"
            y9 = ninetap(engine_lib, xd, wd, bd, N, H, W, Cin, Cout)
            assert torch.equal(y.view(torch.int16), y9.view(torch.int16)), (Cin, Cout, int((y != y9).sum()))
            if Cin == 64 and Cout == 136:
                ref = uc.upconv_ref64(x, w, b).reshape(-1, Cout).half()
                assert torch.equal(y.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("case", uc.RANDN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_random_inputs_against_float64(engine_lib, case):
    """Element by element against float64 conv3x3(nearest_up(x)) on the ORIGINAL fp16 weights, inside
    upconv_cases.upconv_bound.
    Measured on MI355X: profiles/upconv_fold.txt."""
    N, H, W, Cin, Cout = case
    x, w, b = uc.randn_operands(N, H, W, Cin, Cout, seed=Cin + Cout)
    ref = uc.upconv_ref64(x, w, b)
    bound = uc.upconv_bound(x, w, ref)
    y, ran = upconv(engine_lib, x.cuda(), w.cuda(), b.cuda(), N, H, W, Cin, Cout)
    assert ran[0] == 1
    got = y.cpu().reshape(ref.shape)
    assert torch.isfinite(got.float()).all()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print("upconv fold %s: rel-L2 %.2e, worst |err| / bound %.3f" % (case, rel_l2(got, ref), ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("scales", [(1.0, 1.0), (2.0 ** -3, 2.0 ** -3)])
@pytest.mark.parametrize("H,W,Cin,Cout", [(16, 16, 128, 136), (8, 32, 64, 320)])
def test_operands_as_the_engine_passes_them(engine_lib, scales, H, W, Cin, Cout):
    """x a column slice of a wider NaN-filled buffer (ldx > Cin) with NaN rows in front of the first and behind the last
    image; y a column slice of a wider sentinel-filled buffer (ldy > Cout) with guard rows: the result equals the dense
    run bit for bit and nothing outside the slice is written.  Both with the VAE's output scales."""
    N = 2
    x, w, b = uc.randn_operands(N, H, W, Cin, Cout, seed=7)
    wd, bd = w.cuda(), b.cuda()
    dense, ran = upconv(engine_lib, x.cuda(), wd, bd, N, H, W, Cin, Cout, scales=scales)
    assert ran[0] == 1
    ref = uc.upconv_ref64(x, w, b, *scales)
    assert ((dense.cpu().reshape(ref.shape).double() - ref).abs() / uc.upconv_bound(x, w, ref, scales[0])).max().item() <= 1.0
    rows_x, M = N * H * W, N * 4 * H * W
    xw, xo, yw, yo = Cin + 24, 16, Cout + 24, 16
    xbuf = torch.full((GUARD + rows_x + GUARD, xw), float("nan"), dtype=torch.float16, device="cuda")
    xv = xbuf[GUARD:GUARD + rows_x, xo:xo + Cin]
    xv.copy_(x.reshape(rows_x, Cin))
    ybuf = torch.full((GUARD + M + GUARD, yw), SENTINEL, dtype=torch.int16, device="cuda")
    yv = ybuf[GUARD:GUARD + M, yo:yo + Cout]
    _, ran = upconv(engine_lib, xv, wd, bd, N, H, W, Cin, Cout, y=yv, ldx=xw, ldy=yw, scales=scales)
    assert ran[0] == 1
    yb = ybuf.cpu()
    out = yb[GUARD:GUARD + M, yo:yo + Cout].clone()
    yb[GUARD:GUARD + M, yo:yo + Cout] = SENTINEL
    assert (yb == SENTINEL).all(), "rows or columns outside the output slice were written"
    assert torch.equal(out, dense.cpu().view(torch.int16)), "the strided run differs from the dense one"


@pytest.mark.parametrize("H,W,Cin,Cout,G", [(16, 16, 64, 128, 32), (8, 32, 128, 256, 32), (32, 16, 64, 320, 16), (16, 16, 64, 320, 32)])
def test_summaries(engine_lib, H, W, Cin, Cout, G):
    """The GroupNorm summaries of the epilogue, one per (patch, parity): with 32 groups, and with the sub-group widths
    the UNet's concatenation asks of its upsample convs (gn_cat_unit: 20 channels at 1280 | 640, 10 at 640 | 320; here
    on a 160-column tile).  Every (mean, M2) part against the float64 statistics of the fp16 values stored at its 256
    pixels, to the tolerance tests/test_pout_fold_gpu.py and tests/test_ops_gpu.py hold epilogue summaries to; the parts
    merged per image (Chan) against the image's statistics, which is all a consumer computes from them; then a
    GroupNorm run on them against one that makes its own statistics pass."""
    N = 2
    x, w, b = uc.randn_operands(N, H, W, Cin, Cout, seed=G + Cout)
    b = b + 3.0                                                         # a mean well away from zero
    OHW = 4 * H * W
    summ = torch.full((N * max(64, OHW // 64) * G * 2,), float("nan"), device="cuda")
    y, ran = upconv(engine_lib, x.cuda(), w.cuda(), b.cuda(), N, H, W, Cin, Cout, groups=G, summ=summ)
    assert ran[0] == 1 and ran[1] == OHW // 256 and ran[2] == 256, ran
    S, cpg = ran[1], Cout // G
    parts = summ[:N * S * G * 2].cpu().reshape(N, S, G, 2)
    assert torch.isfinite(parts).all()
    # summary (patch, parity) of an image covers output pixels (2i + dy, 2j + dx), (i, j) in the patch's R x Wt input pixels
    Wt = next(wt for wt in (64, 32, 16) if W % wt == 0 and H % (256 // wt) == 0)
    R = 256 // Wt
    t = y.cpu().double().reshape(N, H // R, R, 2, W // Wt, Wt, 2, G, cpg).permute(0, 1, 4, 3, 6, 2, 5, 7, 8)
    t = t.reshape(N, S, 256, G, cpg)
    mean_ref = t.mean(dim=(2, 4))
    m2_ref = ((t - mean_ref[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    assert torch.allclose(parts[..., 0], mean_ref.float(), atol=2e-5, rtol=1e-4)
    assert torch.allclose(parts[..., 1], m2_ref.float(), atol=1e-3, rtol=1e-4)
    # ... and merged per image (Chan; equal counts, so the merged mean is the average) they are the image's statistics
    pd = parts.double()
    mean = pd[..., 0].mean(dim=1)
    m2 = pd[..., 1].sum(dim=1) + 256.0 * cpg * ((pd[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    ti = y.cpu().double().reshape(N, OHW, G, cpg)
    mi = ti.mean(dim=(1, 3))
    assert torch.allclose(mean, mi, atol=2e-5, rtol=1e-4)
    assert torch.allclose(m2, ((ti - mi[:, None, :, None]) ** 2).sum(dim=(1, 3)), atol=1e-3 * S, rtol=1e-4)
    gamma = torch.linspace(0.5, 1.5, Cout, device="cuda")
    beta = torch.linspace(-1.0, 1.0, Cout, device="cuda")
    outs = []
    for pre in (summ, None):
        o = torch.zeros_like(y)
        info = (C.c_int64 * 10)()
        rc = engine_lib.sd_op_groupnorm_ex(P(y), Cout, P(gamma), P(beta), P(o), Cout, N, OHW, Cout, G, 1e-5, 1, P(pre),
                                           S if pre is not None else 0, 256 if pre is not None else 0, info, stream())
        assert rc == 0, engine_lib.sd_last_error()
        assert info[9] == (1 if pre is not None else 0), "the GroupNorm did not take the summaries"
        outs.append(o.float().cpu())
    # the two differ by the statistics' rounding (<= ~1e-4 relative in mean and rstd) and then by at most one fp16 step
    tol = 2.0 ** -10 * outs[1].abs() + 4e-4 * (1.0 + outs[1].abs())
    assert ((outs[0] - outs[1]).abs() <= tol).all(), ((outs[0] - outs[1]).abs() / tol).max().item()


@pytest.mark.parametrize("H,W,Cin,Cout", [(8, 8, 64, 64), (12, 20, 64, 64), (16, 16, 64, 12)])
def test_fallback_is_the_parent_path(engine_lib, H, W, Cin, Cout):
    """Where the predicate is false the entry reports the 9-tap path, bit-identical to sd_op_conv2d_ex(up = 1)."""
    N = 2
    assert engine_lib.sd_upconv_fold_supported(N, H, W, Cin, Cout) == 0
    x, w, b = uc.randn_operands(N, H, W, Cin, Cout, seed=11)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y, ran = upconv(engine_lib, xd, wd, bd, N, H, W, Cin, Cout)
    assert ran[0] == 0
    y9 = ninetap(engine_lib, xd, wd, bd, N, H, W, Cin, Cout)
    assert torch.equal(y.view(torch.int16), y9.view(torch.int16))


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from stablediffusion_amd import config, weights
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), 1, perturb=0.1).items()}
vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), 2, perturb=0.1).items()}
unet = HipUNet2DConditionModel(ucfg, "cuda:0").load_state_dict(usd)
vae = HipAutoencoderKL(vcfg, "cuda:0").load_state_dict(vsd)
g = torch.Generator().manual_seed(0)
x = torch.randn(2, 4, 64, 64, generator=g).half()
ehs = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g).half()
z = torch.randn(1, 4, 16, 16, generator=g).half()
y = unet(x.cuda(), torch.tensor(981.0), ehs.cuda())[0].float().cpu()
img = vae.decode(z.cuda())[0].float().cpu()
torch.save({"unet": y, "vae": img}, sys.argv[2])
"""


def test_models_with_and_without_the_fold(engine_lib, tmp_path):
    """The tiny UNet on 64 x 64 latents (its 16 -> 32 and 32 -> 64 upsamples fold, 8 -> 16 has no patch) and the tiny
    VAE decoding 16 x 16 latents (all three fold), each in a fresh process with and without SD_NO_UPCONV_FOLD=1 (the
    switch is read once): rel-L2 between the two <= 1e-2, the project's bar."""
    outs = {}
    for tag, switch in (("fold", None), ("ninetap", "1")):
        env = {k: v for k, v in os.environ.items() if k != "SD_NO_UPCONV_FOLD"}
        if switch:
            env["SD_NO_UPCONV_FOLD"] = switch
        path = str(tmp_path / (tag + ".pt"))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag] = torch.load(path)
    for k in ("unet", "vae"):
        a, b = outs["fold"][k], outs["ninetap"][k]
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        err = rel_l2(a, b)
        print("tiny %s, folded against 9-tap upsample convs: rel-L2 %.3e" % (k, err))
        assert err <= 1e-2
        assert not torch.equal(a, b), "the switch changed nothing: did the folded kernel run?"
