"""FreeU on the GPU: sd_op_freeu against the fp32 torch.fft oracle (tests/freeu_oracle.py) on the same fp16 inputs, the
UNet with FreeU on against the oracle's restated forward (plain, shared-CFG, ControlNet, IP-Adapter, SD_GN_CAT=1 in a
child process), and "off means off".

Operator bound: rel-L2 of the skip half <= 2 x the rel-L2 of oracle.half() against oracle -- the rounding error of a
perfect result, computed here from the reference, times 2 for one extra half-ulp from the fp32 summation order.  Where
the filtered map is exactly zero (every frequency of a 2 x 2 map is inside the box and s = 0) a relative error has no
denominator: there each output is held to 2^-20 x the plane's sum of |x|, sixteen fp32 roundings of the moments' sums
(2^-24 each), which is what the cancellation x - (4 x) / 4 can leave."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402  (first: it puts the repository root on sys.path for the child process too)
import freeu_oracle  # noqa: E402
from cn_oracle import controlnet_forward, synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipControlNetModel, HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-2
GAP = 0.1
FACTORS = (0.9, 0.2, 1.5, 1.6)
PAIRS = [(1.5, 0.2), (1.0, 1.0), (1.2, 0.0), (1.0, 2.0)]
# (N, H, W, C1, C2).  After the issue's nine: both sides of the LDS-resident / re-read boundary of the vector form
# (66 x 66 fits 72 KB with its twiddles, 67 x 67 does not), 2 and 4 channel vectors per block with a ragged last group,
# and the scalar form (channel counts that are no multiple of 8) with a ragged group, LDS-resident and re-read.
OP_CASES = [(2, 2, 2, 256, 256), (3, 3, 3, 64, 40), (1, 1, 3, 32, 24), (1, 5, 1, 32, 8), (2, 8, 8, 1280, 1280),
            (1, 16, 16, 1280, 640), (2, 9, 16, 64, 72), (1, 32, 32, 128, 136), (1, 64, 64, 64, 72),
            (1, 66, 66, 32, 16), (1, 67, 67, 32, 16), (8, 4, 4, 1280, 1288), (16, 3, 3, 64, 1032),
            (2, 7, 6, 6, 5), (64, 2, 3, 2, 300), (1, 200, 190, 2, 3)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("N,H,W,C1,C2", OP_CASES)
def test_op_matches_fft_oracle(engine_lib, N, H, W, C1, C2):
    g = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    x = (torch.randn(N, H, W, C1 + C2, generator=g) + 0.5).half()
    worst = 0.0
    for b, s in PAIRS:
        ref = freeu_oracle.freeu_cat(x, C1, b, s)                       # fp32, NHWC
        buf = x.clone().cuda()
        rc = engine_lib.sd_op_freeu(buf.data_ptr(), N, H, W, C1, C2, b, s, stream())
        assert rc == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        got = buf.cpu()
        # backbone: the first C1 / 2 channels are fp16(x * b) bit for bit, the second half is untouched
        assert torch.equal(got[..., :C1 // 2], (x[..., :C1 // 2].float() * b).half()), (b, s)
        assert torch.equal(got[..., C1 // 2:C1], x[..., C1 // 2:C1]), (b, s)
        skip, want = got[..., C1:].float(), ref[..., C1:]
        if max(H, W) <= 2 and s == 0.0:
            assert torch.count_nonzero(want) == 0
            lim = 2.0 ** -20 * x[..., C1:].float().abs().sum(dim=(1, 2), keepdim=True)
            print(f"op {N}x{H}x{W} C1={C1} C2={C2} b={b} s={s}: zero reference, max |y| {skip.abs().max().item():.2e}")
            assert (skip.abs() <= lim).all(), (b, s)
            continue
        yard = rel_l2(want.half(), want)
        err = rel_l2(skip, want)
        worst = max(worst, err / yard if yard > 0 else (0.0 if err == 0 else float("inf")))
        print(f"op {N}x{H}x{W} C1={C1} C2={C2} b={b} s={s}: rel-L2 {err:.3e}, fp16 rounding of the oracle {yard:.3e}")
        assert err <= 2 * yard, (b, s, err, yard)
        if (b, s) == (1.0, 1.0):
            assert torch.equal(got[..., :C1], x[..., :C1])
    print(f"op {N}x{H}x{W} C1={C1} C2={C2}: worst error / yardstick {worst:.2f}")


# ---------------------------------------------------------------------------------------------------- UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = config.tiny_unet()
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


def _inputs(cfg, B, H, W, rows=None):
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(rows or B, 77, cfg.cross_attention_dim, generator=g).half()
    return x, ehs


def _check(got, on, off, what):
    e_on, e_off, gap = rel_l2(got, on), rel_l2(got, off), rel_l2(on, off)
    print(f"{what}: vs oracle with FreeU {e_on:.2e}, vs oracle without {e_off:.2e} (oracles apart {gap:.2f})")
    assert e_on < TOL
    assert e_off > GAP


@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 8, 24), (3, 24, 24)])
def test_unet_with_freeu_matches_oracle(engine_lib, tiny, B, H, W):
    cfg, sd, net = tiny
    x, ehs = _inputs(cfg, B, H, W)
    t = torch.tensor(501.0)
    with torch.no_grad():
        on = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), freeu=FACTORS)
        off = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float())
    net.enable_freeu(*FACTORS)
    try:
        got = net(x.cuda(), t, ehs.cuda())[0]
    finally:
        net.disable_freeu()
    _check(got, on, off, f"unet B={B} {H}x{W}")


def test_unet_linear_text_time_with_freeu_matches_oracle(engine_lib):
    cfg = config.tiny_unet(linear=True, sdxl_cond=True)
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd).enable_freeu(*FACTORS)
    x, ehs = _inputs(cfg, 2, 16, 16)
    g = torch.Generator().manual_seed(8)
    added = {"text_embeds": torch.randn(2, 64, generator=g).half(),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)}
    t = torch.tensor(501.0)
    ref_added = {k: v.float() for k, v in added.items()}
    with torch.no_grad():
        on = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), ref_added, freeu=FACTORS)
        off = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), ref_added)
    got = net(x.cuda(), t, ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0]
    _check(got, on, off, "unet linear + text_time")


@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 8, 24), (3, 24, 24)])
def test_forward_cfg_shared_with_freeu_matches_oracle(engine_lib, tiny, B, H, W):
    cfg, sd, net = tiny
    assert net.cfg_share_eligible
    x, ehs = _inputs(cfg, B, H, W, rows=2 * B)
    t = torch.tensor(501.0)
    x2 = torch.cat([x, x]).float()
    with torch.no_grad():
        on = freeu_oracle.unet_forward(cfg, sd, x2, t, ehs.float(), freeu=FACTORS)
        off = freeu_oracle.unet_forward(cfg, sd, x2, t, ehs.float())
    net.enable_freeu(*FACTORS)
    try:
        got = net.forward_cfg(x.cuda(), 501.0, ehs.cuda(), share=True)[0]
    finally:
        net.disable_freeu()
    _check(got, on, off, f"forward_cfg(share) B={B} {H}x{W}")


@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 8, 24), (3, 24, 24)])
def test_controlnet_then_freeu_matches_oracle(engine_lib, tiny, B, H, W):
    cfg, sd, net = tiny
    ccfg = controlnet.encoder_config(cfg)
    csd = synth_cn_state_dict(ccfg, seed=4)
    cn = HipControlNetModel(net, ccfg).load_state_dict(csd)
    x, ehs = _inputs(cfg, B, H, W)
    g = torch.Generator().manual_seed(B + H)
    img = torch.rand(1, 3, 8 * H, 8 * W, generator=g).half()
    t = torch.tensor(501.0)
    with torch.no_grad():
        down, mid = controlnet_forward(ccfg, csd, x.float(), t, ehs.float(), img, 0.8)
        on = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), freeu=FACTORS, down_res=down, mid_res=mid)
        off = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), down_res=down, mid_res=mid)
    net.attach_controlnet(cn)
    net.enable_freeu(*FACTORS)
    try:
        got = net(x.cuda(), t, ehs.cuda(), controlnet_cond=img.cuda(), controlnet_conditioning_scale=0.8)[0]
    finally:
        net.disable_freeu()
        net.attach_controlnet(None)
    _check(got, on, off, f"controlnet + freeu B={B} {H}x{W}")


def test_freeu_applies_with_an_ip_adapter_attached(engine_lib, tiny):
    """The image branch at scale 0 is the text attention alone (another attention kernel, the same up path)."""
    cfg, sd, net = tiny
    ad = HipIPAdapter(net, 128, 4).load_state_dict(synth_ip_state_dict(cfg, 128, 4, seed=3))
    x, ehs = _inputs(cfg, 2, 16, 16)
    g = torch.Generator().manual_seed(6)
    kw = {"added_cond_kwargs": {"image_embeds": [torch.randn(2, 1, 128, generator=g).half().cuda()]}}
    t = torch.tensor(501.0)
    with torch.no_grad():
        on = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), freeu=FACTORS)
        off = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float())
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.0)
    net.enable_freeu(*FACTORS)
    try:
        got = net(x.cuda(), t, ehs.cuda(), **kw)[0]
    finally:
        net.disable_freeu()
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    _check(got, on, off, "ip-adapter (scale 0) + freeu")


def _gn_cat_child():
    """Runs under SD_GN_CAT=1 (read once per process, the first time the up path runs)."""
    assert os.environ.get("SD_GN_CAT") == "1"
    cfg = config.tiny_unet()
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd).enable_freeu(*FACTORS)
    t = torch.tensor(501.0)
    for B, H, W in [(2, 16, 16), (1, 8, 24), (3, 24, 24)]:
        x, ehs = _inputs(cfg, B, H, W)
        with torch.no_grad():
            on = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), freeu=FACTORS)
            off = freeu_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float())
        _check(net(x.cuda(), t, ehs.cuda())[0], on, off, f"SD_GN_CAT=1 unet B={B} {H}x{W}")
    print("gn-cat-child-ok")


def test_unet_with_freeu_under_gn_cat(engine_lib):
    env = dict(os.environ, SD_GN_CAT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "gn_cat_child"], env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gn-cat-child-ok" in r.stdout


# ------------------------------------------------------------------------------------------ off means off
def _launches(lib, run):
    run()
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    try:
        run()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {e.kernel.decode(): e.launches for e in ents[: n.value]}


def test_off_means_off(engine_lib, tiny):
    cfg, sd, net = tiny
    x, ehs = _inputs(cfg, 2, 16, 16)
    xd, ed = x.cuda(), ehs.cuda()
    never = HipUNet2DConditionModel(cfg).load_state_dict(sd)(xd, 501.0, ed)[0]
    run = lambda: net(xd, 501.0, ed)[0]   # noqa: E731
    off = _launches(engine_lib, run)
    net.enable_freeu(*FACTORS)
    try:
        with_freeu = run()
        on = _launches(engine_lib, run)
        net.use_graph(True)
        with pytest.raises(_lib.EngineError, match="FreeU"):
            run()
    finally:
        net.use_graph(False)
        net.disable_freeu()
    after = run()
    assert torch.equal(after, never) and not torch.equal(with_freeu, never)
    assert not any("freeu" in k for k in off), off
    assert on.pop("freeu_kernel") == 2 * (cfg.layers_per_block + 1)
    # (SD_GN_CAT unset: norm1 of every concatenation runs its own statistics pass with FreeU off too)
    assert on == off
    assert _launches(engine_lib, run) == off


if __name__ == "__main__" and sys.argv[1:] == ["gn_cat_child"]:
    _gn_cat_child()
