"""proj_out folded over the last ff.net.2 of a transformer ("proj_out folded into the last
feed-forward GEMM"): the pack-time fold against a float64 product, the end of a transformer through the functions the
UNet runs against the unfolded chain in fp32, and the tiny UNet with and without the fold (SD_NO_POUT_FOLD=1) in two
fresh processes."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def h(t):
    return t.half().cuda().contiguous()


def f16(t):
    """fp32 values an fp16 tensor can hold: the entries round their fp32 arguments to fp16, as a model's weights are"""
    return t.half().float()


@pytest.mark.parametrize("Cc,K", [(64, 256), (320, 1280)])
def test_fold_linear_against_float64(engine_lib, Cc, K):
    """W' = [W_o W_i | W_o], b' = W_o b_i + b_o.  Every element within one fp16 rounding of the exact value plus the slack
    of an fp32 accumulation: |got - exact| <= 2^-11 |exact| + 2^-22 sum |terms|, both from the float64 product."""
    g = torch.Generator().manual_seed(Cc + K)
    wo = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).half()
    wi = (torch.randn(Cc, K, generator=g) / K ** 0.5).half()
    bo = f16(torch.randn(Cc, generator=g) * 0.2)
    bi = f16(torch.randn(Cc, generator=g) * 0.2)
    wf = torch.zeros(Cc, K + Cc, dtype=torch.float16, device="cuda")
    bf = torch.zeros(Cc, dtype=torch.float32, device="cuda")
    wod, wid, bod, bid = h(wo), h(wi), bo.cuda(), bi.cuda()
    rc = engine_lib.sd_op_fold_linear(P(wod), P(bod), P(wid), P(bid), P(wf), P(bf), Cc, Cc, K, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    wo64, wi64 = wo.double(), wi.double()
    exact = wo64 @ wi64
    terms = wo64.abs() @ wi64.abs()
    got = wf.cpu().double()
    err = (got[:, :K] - exact).abs()
    bound = 2.0 ** -11 * exact.abs() + 2.0 ** -22 * terms
    worst = (err / bound).max().item()
    print(f"fold_linear ({Cc}, {K}): worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0, worst
    assert torch.equal(got[:, K:], wo64)                      # the residual's columns are W_o itself
    b_exact = wo64 @ bi.double() + bo.double()
    b_terms = wo64.abs() @ bi.double().abs() + bo.double().abs()
    b_err = (bf.cpu().double() - b_exact).abs()
    assert (b_err <= 2.0 ** -11 * b_exact.abs() + 2.0 ** -22 * b_terms).all(), b_err.max().item()


def test_fold_linear_refuses_ragged_k(engine_lib):
    z = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    b = torch.zeros(64, device="cuda")
    assert engine_lib.sd_op_fold_linear(P(z), P(b), P(z), P(b), P(z), P(b), 64, 64, 40, stream()) != 0


TAIL_CASES = [
    # M, C, imgs, summaries asked for (0 no, 1 checked where the launch leaves them, 2 and it must leave them), fused
    (300, 64, 1, 0, 0),            # ragged M, narrow tiles
    (1024, 640, 1, 2, 0),          # no tuned row: the rule splits K, the summaries come from the split-K reduction
    (512, 1280, 1, 0, 0),          # the split-K route of the mid block (the hint carries the tuned row's split)
    (8192, 320, 2, 1, 1),          # ffn.hip takes the feed-forward: 64 blocks, the smallest M it accepts; proj_out behind it
    (8320, 320, 1, 0, 1),          # 65 blocks; the last block alone on its CU
    (8192, 640, 8, 2, 0),          # the 32 x 32 level of the batch-8 UNet: the hinted 128 x 80 tile, summaries from its epilogue
]


@pytest.mark.parametrize("M,Cc,imgs,summaries,want_fused", TAIL_CASES)
def test_ffn_geglu_proj_out(engine_lib, M, Cc, imgs, summaries, want_fused):
    """x_in + proj_out(t3 + FF(LN(t3))) through run_xformer_tail against the unfolded chain in fp32 torch: rel-L2 < 3e-3
    (the bound of test_ffn_geglu_fused, this operator family's), bit-equal on a second call, and the GroupNorm summaries
    against float64 (mean, M2) of the STORED fp16 output.
    Measured on MI355X (rel-L2): see profiles/proj_out_fold.txt."""
    G = 32
    g = torch.Generator().manual_seed(M + Cc)
    t3 = (torch.randn(M, Cc, generator=g) + 0.2 * torch.randn(1, Cc, generator=g)).half()
    x_in = torch.randn(M, Cc, generator=g).half()
    w1 = (torch.randn(8 * Cc, Cc, generator=g) / Cc ** 0.5).half()
    b1 = f16(torch.randn(8 * Cc, generator=g) * 0.2)
    w2 = (torch.randn(Cc, 4 * Cc, generator=g) / (4 * Cc) ** 0.5).half()
    b2 = f16(torch.randn(Cc, generator=g) * 0.2)
    wpo = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).half()
    bpo = f16(torch.randn(Cc, generator=g) * 0.2)
    gamma = f16(1 + 0.2 * torch.randn(Cc, generator=g))
    beta = f16(0.2 * torch.randn(Cc, generator=g))
    xd, td, w1d, w2d, wpd = h(x_in), h(t3), h(w1), h(w2), h(wpo)
    b1d, b2d, bpd, gd, bd = b1.cuda(), b2.cuda(), bpo.cuda(), gamma.cuda(), beta.cuda()
    with torch.no_grad():
        tf = td.float()
        proj = F.linear(F.layer_norm(tf, (Cc,), gd, bd, 1e-5), w1d.float(), b1d)
        hid, gate = proj.chunk(2, dim=-1)
        ref = xd.float() + F.linear(tf + F.linear(hid * F.gelu(gate), w2d.float(), b2d), wpd.float(), bpd)
    HW = M // imgs
    slots = imgs * max(64, (HW + 63) // 64) * G * 2

    def run():
        y = torch.zeros(M, Cc, dtype=torch.float16, device="cuda")
        summ = torch.zeros(slots, dtype=torch.float32, device="cuda") if summaries else None
        fused, rows = C.c_int(-1), C.c_int(-1)
        rc = engine_lib.sd_op_ffn_geglu_proj_out(P(xd), P(td), P(gd), P(bd), 1e-5, P(w1d), P(b1d), P(w2d), P(b2d), P(wpd), P(bpd),
                                                 P(y), P(summ), C.byref(rows), M, Cc, imgs, C.byref(fused), stream())
        assert rc == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        return y, summ, fused.value, rows.value

    y, summ, fused, rows = run()
    err = rel_l2(y, ref)
    print(f"ffn_geglu_proj_out M={M} C={Cc}: rel-L2 {err:.3e}, fused {fused}, gn_rows {rows}")
    assert fused == want_fused
    assert torch.isfinite(y.float()).all()
    assert err < 3e-3, err
    y2, summ2, _, _ = run()
    assert torch.equal(y, y2)
    if summaries == 2:
        assert rows > 0, "the launch left no summaries"
    if rows > 0:
        assert HW % rows == 0, rows
        S = HW // rows
        t = y.cpu().double().reshape(imgs, S, rows, G, Cc // G)
        mean = t.mean(dim=(2, 4))
        m2 = ((t - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
        got = summ[:imgs * S * G * 2].cpu().reshape(imgs, S, G, 2)
        assert torch.allclose(got[..., 0], mean.float(), atol=2e-5, rtol=1e-4)
        assert torch.allclose(got[..., 1], m2.float(), atol=1e-3, rtol=1e-4)
        assert torch.equal(summ, summ2)


_CHILD = r"""
import importlib.util, os, sys
import numpy as np, torch
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root)
from stablediffusion_amd.models import HipUNet2DConditionModel
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(root, "tests", "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)
ucfg, vcfg, uw, vw = mg.golden_weights()
d = np.load(os.path.join(root, "tests", "golden", "tiny_sd.npz"))
unet = HipUNet2DConditionModel(ucfg).load_state_dict(uw)
y = unet(torch.from_numpy(d["unet_x"]).cuda(), torch.from_numpy(d["unet_t"]), torch.from_numpy(d["unet_ehs"]).cuda())[0]
np.save(out, y.float().cpu().numpy())
"""


def test_tiny_unet_with_and_without_the_fold(engine_lib, tmp_path):
    """The golden tiny UNet in two fresh processes, the fold on and SD_NO_POUT_FOLD=1: both within the bound
    test_engine_against_golden_vectors asserts (rel-L2 < 1e-2 against the oracle's output), their mutual distance reported
    (of the order of one fp16 rounding of the activations: the fold drops one, of the block's output, and rounds the product
    of two weight matrices once)."""
    import numpy as np
    want = np.load(os.path.join(ROOT, "tests", "golden", "tiny_sd.npz"))["unet_y"]
    outs = {}
    for name, switch in (("fold", None), ("pair", "1")):
        env = {k: v for k, v in os.environ.items() if k != "SD_NO_POUT_FOLD"}
        if switch:
            env["SD_NO_POUT_FOLD"] = switch
        path = str(tmp_path / f"{name}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = torch.from_numpy(np.load(path))
    ref = torch.from_numpy(np.asarray(want)).float()
    e_fold, e_pair = rel_l2(outs["fold"], ref), rel_l2(outs["pair"], ref)
    mutual = rel_l2(outs["fold"], outs["pair"])
    msg = json.dumps({"fold_vs_oracle": e_fold, "pair_vs_oracle": e_pair, "fold_vs_pair": mutual})
    print(msg)
    assert e_fold < 1e-2 and e_pair < 1e-2, msg
    assert mutual > 0.0, "SD_NO_POUT_FOLD=1 changed nothing: " + msg
