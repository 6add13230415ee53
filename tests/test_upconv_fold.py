"""Nearest-2x upsample + 3x3 conv folded into four 2x2 parity convolutions: what needs no GPU.

The dispatch predicate over a grid of shapes, the C-ABI symbols, the identity itself in float64 on odd, non-square
maps, and the element-wise bound of tests/test_upconv_fold_gpu.py held against a torch emulation of the folded
kernel's arithmetic (fp16 folded weights, fp32 accumulation, one rounding of the result)."""
import pytest
import torch

import upconv_cases as uc


@pytest.mark.parametrize("H,W,Cin,Cout,want", [
    (16, 16, 64, 64, 1), (8, 32, 64, 64, 1), (4, 64, 64, 64, 1), (32, 16, 64, 64, 1), (64, 64, 64, 64, 1),
    (16, 16, 1280, 1280, 1), (64, 64, 512, 512, 1), (16, 48, 128, 8, 1),
    (8, 8, 64, 64, 0), (12, 20, 64, 64, 0), (16, 16, 32, 64, 0), (16, 16, 64, 12, 0), (16, 16, 96, 64, 0),
])
def test_predicate(engine_lib, H, W, Cin, Cout, want):
    """True where a 256-pixel patch (64 / 32 / 16 columns wide) tiles the INPUT map and Cin % 64 == 0, Cout % 8 == 0."""
    for N in (1, 3):
        assert engine_lib.sd_upconv_fold_supported(N, H, W, Cin, Cout) == want


def test_predicate_rejects_operands_past_2gb(engine_lib):
    """The kernel addresses x through a 32-bit buffer descriptor."""
    assert engine_lib.sd_upconv_fold_supported(8, 256, 256, 1280, 1280) == 1        # 1.34 GB
    assert engine_lib.sd_upconv_fold_supported(16, 256, 256, 1280, 1280) == 0       # 2.7 GB
    assert engine_lib.sd_upconv_fold_supported(0, 16, 16, 64, 64) == 0


def test_symbols(engine_lib):
    for name in ("sd_upconv_fold_supported", "sd_op_fold_upconv", "sd_op_upconv2x_ex"):
        assert hasattr(engine_lib, name)


@pytest.mark.parametrize("N,C,O,H,W", [(2, 64, 24, 16, 16), (1, 64, 16, 8, 24), (2, 128, 32, 5, 7), (1, 64, 8, 1, 3)])
def test_identity_float64(N, C, O, H, W):
    """The four parity convolutions on exactly folded weights equal conv3x3(nearest_up(x)) in float64, borders included,
    on odd and non-square maps: fp16 operands make every product and sum exact, so the difference is 0."""
    x, w, b = uc.randn_operands(N, H, W, C, O, seed=H * 31 + W)
    ref = uc.upconv_ref64(x, w, b)
    y = uc.parity_conv(x.permute(0, 3, 1, 2).double(), uc.fold64(w.double()), b.double()).permute(0, 2, 3, 1)
    assert (y - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_fold_np_layout():
    """fold_np (the engine's pack order) unpacks to the float64 fold rounded to fp16 once."""
    _, w, _ = uc.randn_operands(1, 1, 1, 128, 24, seed=3)
    got = uc.unpack_fold(uc.fold_np(w), 24, 128)
    want = uc.fold64(w.double())
    for k in want:
        assert torch.equal(got[k], want[k].half()), k        # (fp32 sums of <= 4 fp16 values of like size are exact here)


@pytest.mark.parametrize("case", uc.RANDN_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("scales", [(1.0, 1.0), (2.0 ** -3, 2.0 ** -3)])
def test_emulation_within_bound(case, scales):
    """The kernel's arithmetic, emulated, stays inside the bound the GPU test uses (and uses a visible part of it:
    the once-rounded folded weights alone take about a fifth)."""
    N, H, W, Cin, Cout = case
    x, w, b = uc.randn_operands(N, H, W, Cin, Cout, seed=Cin + Cout)
    ref = uc.upconv_ref64(x, w, b, *scales)
    bound = uc.upconv_bound(x, w, ref, scales[0])
    err = (uc.emulate(x, w, b, *scales).double() - ref).abs()
    ratio = (err / bound).max().item()
    print("emulation %s scales %s: worst |err| / bound %.3f" % (case, scales, ratio))
    assert ratio <= 1.0
