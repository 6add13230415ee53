"""The single-operator entries run through the engine's own packers and op wrappers (WeightStore's pointer-level cores,
conv_prepare / conv_launch, op_ffn_fused).  Three properties that the move must keep:

(a) an entry's fp32 bias reaches the kernel as fp32 (the packers take it as an fp32 host array; WeightStore::set would
    round it to fp16),
(b) the folded-upsample pack of pack_conv(fold_up2x) is, byte for byte, what it was before the packers were split,
(c) the planning and the live pass of the fused feed-forward decide alike, on both sides of its 64-block threshold and
    for one and several statistics parts per row.
"""
import ctypes as C
import hashlib

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ (a) the bias stays fp32
TINY = 2.0 ** -12
BIAS = 0.5 + TINY              # exact in fp32, a round-to-even tie in fp16 (the step in [0.5, 1) is 2^-11)
WANT = 0.5 + 2.0 ** -11        # 1 * 2^-12 + BIAS, exact in fp32 and representable in fp16


def test_the_expected_values_on_the_cpu():
    """fp32 bias: 2^-12 + (0.5 + 2^-12) = 0.5 + 2^-11 exactly, stored in fp16 as it is.  A bias rounded to fp16 on the way
    is 0.5 (tie to even), and the sum 0.5 + 2^-12 rounds to 0.5 again (the second tie)."""
    acc = torch.tensor(TINY, dtype=torch.float16).float()
    assert acc.item() == TINY
    bias = torch.tensor(BIAS, dtype=torch.float32)
    assert bias.item() == BIAS
    assert (acc + bias).half().item() == WANT
    assert bias.half().item() == 0.5
    assert (acc + bias.half().float()).half().item() == 0.5


def _exact_operands(rows, K, Cout):
    x = torch.zeros(rows, K, dtype=torch.float16)
    x[:, 0] = 1.0
    w = torch.zeros(Cout, K, dtype=torch.float16)
    w[:, 0] = TINY
    b = torch.full((Cout,), BIAS, dtype=torch.float32)
    return x.cuda(), w.cuda(), b.cuda()


def test_conv2d_bias_stays_fp32(engine_lib):
    N, H, W, Cin, Cout = 1, 8, 8, 64, 64
    x, w, b = _exact_operands(N * H * W, Cin, Cout)            # NHWC: x[:, 0] = 1 is channel 0 of every pixel
    y = torch.zeros(N * H * W, Cout, dtype=torch.float16, device="cuda")
    rc = engine_lib.sd_op_conv2d(P(x), P(w), P(b), None, None, P(y), N, H, W, Cin, Cout, 1, 1, 0, 0, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    got = y.float().cpu()
    print("sd_op_conv2d: distinct outputs", sorted(set(got.flatten().tolist())))
    assert torch.equal(got, torch.full_like(got, WANT))


def test_linear_rowstats_bias_stays_fp32(engine_lib):
    M, K, Cc = 64, 64, 64
    x, w, b = _exact_operands(M, K, Cc)
    y1 = torch.zeros(M, Cc, dtype=torch.float16, device="cuda")
    stat = torch.zeros(M * 2, dtype=torch.float32, device="cuda")
    parts, part_w, prod = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    rc = engine_lib.sd_op_linear_rowstats(P(x), P(w), P(b), None, P(y1), P(stat), M, K, Cc, C.byref(parts), C.byref(part_w),
                                          C.byref(prod), stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    got = y1.float().cpu()
    print("sd_op_linear_rowstats: distinct outputs", sorted(set(got.flatten().tolist())), "producer", prod.value)
    assert torch.equal(got, torch.full_like(got, WANT))


# ------------------------------------------------------------------------------------------- (b) the folded pack's bytes
# SHA-256 of sd_op_fold_upconv's output [4][Cout][4 Cin] fp16 at the commit before the packers were split, for
# w = (randn(Cout, Cin, 3, 3; seed) / sqrt(9 Cin)).half()
FOLD_SHA256 = {
    (8, 64, 72): "5a6bc15374dc7c411e1551abeadf90e46204fe101bf7cb43c2aff3bfc02f2eab",
    (72, 128, 200): "13729cce3ab62f3d6989d6e40b35a7d9a1c659436def4cd34a170da3694f900a",
}


@pytest.mark.parametrize("Cout,Cin,seed", sorted(FOLD_SHA256))
def test_fold_upconv_bytes(engine_lib, Cout, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    out = torch.full((4, Cout, 4 * Cin), float("nan"), dtype=torch.float16, device="cuda")
    assert engine_lib.sd_op_fold_upconv(P(w.cuda()), P(out), Cout, Cin, stream()) == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    sha = hashlib.sha256(out.cpu().contiguous().view(torch.int16).numpy().tobytes()).hexdigest()
    print("sd_op_fold_upconv [%d][%d][3][3] seed %d sha256 %s" % (Cout, Cin, seed, sha))
    assert sha == FOLD_SHA256[(Cout, Cin, seed)]


# -------------------------------------------------------------------- (c) the fused feed-forward: planning = live pass
FFN_C = 320
_ffn = {}


def _ffn_case(lib, M):
    """Operands of one M and sd_op_ffn_geglu's result on them (statistics from its own row_stats pass), computed once."""
    if M not in _ffn:
        g = torch.Generator().manual_seed(M)
        Cc = FFN_C
        x = (torch.randn(M, Cc, generator=g) + 0.2 * torch.randn(1, Cc, generator=g)).half().cuda()
        w1 = (torch.randn(8 * Cc, Cc, generator=g) / Cc ** 0.5).half().cuda()
        b1 = (torch.randn(8 * Cc, generator=g) * 0.2).cuda()
        w2 = (torch.randn(Cc, 4 * Cc, generator=g) / (4 * Cc) ** 0.5).half().cuda()
        b2 = (torch.randn(Cc, generator=g) * 0.2).cuda()
        gamma = (1 + 0.2 * torch.randn(Cc, generator=g)).cuda()
        beta = (0.2 * torch.randn(Cc, generator=g)).cuda()
        ref = torch.zeros(M, Cc, dtype=torch.float16, device="cuda")
        ref_fused = C.c_int(-1)
        rc = lib.sd_op_ffn_geglu(P(x), P(gamma), P(beta), 1e-5, P(w1), P(b1), P(w2), P(b2), P(ref), M, Cc, 0, None,
                                 C.byref(ref_fused), stream())
        assert rc == 0, lib.sd_last_error()
        torch.cuda.synchronize()
        _ffn[M] = (x, w1, b1, w2, b2, gamma, beta, ref, ref_fused.value)
    return _ffn[M]


def _row_stats(x, parts, part_w):
    """(mean, M2) of every row of x over `parts` column ranges of part_w columns: [M][parts][2] fp32, from the fp16 values."""
    xs = x.double().view(x.shape[0], parts, part_w)
    mean = xs.mean(-1)
    m2 = ((xs - mean[..., None]) ** 2).sum(-1)
    return torch.stack([mean, m2], -1).float().contiguous()


@pytest.mark.parametrize("parts,part_w", [(1, 320), (5, 64)])
@pytest.mark.parametrize("M,want_fused", [(8192, 1), (8064, 0)])
def test_ln_ffn_geglu_plans_as_it_runs(engine_lib, M, want_fused, parts, part_w):
    """sd_op_ln_ffn_geglu at C = 320 with 64 blocks of 128 rows (ffn_fused_kernel) and with 63 (the two GEMMs, whose M x 4C
    hidden tensor the planning pass must have provided for), on one part per row (of 320 columns: a single part has to
    cover the row) and on five of 64: rc 0, the expected path, and the result of sd_op_ffn_geglu on the same operands to the
    3e-3 rel-L2 that test_ops_gpu.test_ffn_geglu_fused holds that entry to."""
    Cc = FFN_C
    x, w1, b1, w2, b2, gamma, beta, ref, ref_fused = _ffn_case(engine_lib, M)
    stat = _row_stats(x, parts, part_w)
    y = torch.zeros(M, Cc, dtype=torch.float16, device="cuda")
    fused = C.c_int(-1)
    rc = engine_lib.sd_op_ln_ffn_geglu(P(x), P(stat), parts, part_w, P(gamma), P(beta), 1e-5, P(w1), P(b1), P(w2), P(b2),
                                       P(y), M, Cc, C.byref(fused), stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    err = rel_l2(y, ref)
    print("sd_op_ln_ffn_geglu M %d parts %d x %d: fused %d (sd_op_ffn_geglu %d), rel-L2 to it %.3e"
          % (M, parts, part_w, fused.value, ref_fused, err))
    assert fused.value == want_fused and ref_fused == want_fused
    assert torch.isfinite(y.float()).all()
    assert err < 3e-3, err
