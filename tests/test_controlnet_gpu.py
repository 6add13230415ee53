"""ControlNet on the GPU: the grouped zero-conv residual launch and the conditioning embedding against fp32 torch, and
the UNet with a ControlNet attached against the fp32 oracle composition (tests/cn_oracle.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import cn_cases as cc
from cn_oracle import cond_embedding, synth_cn_state_dict, unet_cn_forward
from conftest import rel_l2
from oracle import unet_ref
from stablediffusion_amd import _lib, config, controlnet, weights
from stablediffusion_amd.models import HipControlNetModel, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu
TOL = 1e-2


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------- grouped residual op
def _sites(cfg, B, h, w):
    """(M, C) of every residual site of a UNet configuration at latent h x w, mid block last."""
    out = []
    boc = cfg.block_out_channels
    out.append((B * h * w, boc[0]))
    for i, c in enumerate(boc):
        out += [(B * h * w, c)] * cfg.layers_per_block
        if i != len(boc) - 1:
            h, w = h // 2, w // 2
            out.append((B * h * w, c))
    out.append((B * h * w, boc[-1]))
    return out


def _problems(sites, seed, pad=24):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for M, Cc in sites:
        x = torch.randn(M, Cc, generator=g).half().cuda()
        w = (torch.randn(Cc, Cc, generator=g) / Cc ** 0.5).half().cuda()
        b = (0.1 * torch.randn(Cc, generator=g)).cuda()
        # y lives in the skip half of a wider concatenation row; the other columns hold sentinels
        buf = torch.randn(M, Cc + pad, generator=g).half().cuda()
        buf[:, Cc:] = float("nan")
        ps.append((x, w, b, buf))
    return ps


def _run(lib, ps, scale, mode, iters=0):
    arr = (_lib.SdCnProblem * len(ps))()
    for i, (x, w, b, buf) in enumerate(ps):
        arr[i] = _lib.SdCnProblem(x.data_ptr(), x.stride(0), w.data_ptr(), b.data_ptr(), buf.data_ptr(), buf.stride(0),
                                  x.shape[0], x.shape[1])
    ms = C.c_float()
    rc = lib.sd_op_controlnet_residuals(arr, len(ps), scale, mode, iters, C.byref(ms) if iters else None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return ms.value


@pytest.mark.parametrize("preset", ["sd15", "sdxl"])
@pytest.mark.parametrize("B,h,w", [(1, 64, 64), (2, 40, 56), (3, 24, 32), (8, 64, 64)])
def test_grouped_residuals_match_fp32(engine_lib, preset, B, h, w):
    cfg = config.sd15_unet() if preset == "sd15" else config.sdxl_unet()
    if preset == "sdxl":
        h, w = h * 2 if B <= 2 else h, w * 2 if B <= 2 else w
    sites = _sites(cfg, B, h, w)
    ps = _problems(sites, seed=B * 7 + h)
    before = [buf.clone() for *_, buf in ps]
    _run(engine_lib, ps, 0.8, 0)
    for (x, wt, b, buf), old, (M, Cc) in zip(ps, before, sites):
        ref = old[:, :Cc].float() + 0.8 * (x.float() @ wt.float().t() + b)
        assert rel_l2(buf[:, :Cc], ref) < 2e-3, (M, Cc)
        assert torch.isnan(buf[:, Cc:]).all()                # the hidden half is untouched (sentinels)


def test_grouped_residuals_odd_rows_and_zero_scale(engine_lib):
    sites = [(3 * 5 * 7, 1280), (105, 640), (2 * 35, 320), (1, 64), (17, 128), (129, 256)]
    ps = _problems(sites, seed=5)
    before = [buf.clone() for *_, buf in ps]
    _run(engine_lib, ps, 0.0, 0)
    for (*_, buf), old in zip(ps, before):
        assert torch.equal(buf[:, :-24], old[:, :-24])       # s = 0 leaves y bit-unchanged
    _run(engine_lib, ps, 1.5, 0)
    for (x, wt, b, buf), old, (M, Cc) in zip(ps, before, sites):
        ref = old[:, :Cc].float() + 1.5 * (x.float() @ wt.float().t() + b)
        assert rel_l2(buf[:, :Cc], ref) < 2e-3, (M, Cc)
        assert torch.isnan(buf[:, Cc:]).all()


def test_grouped_equals_unfused(engine_lib):
    sites = _sites(config.sd15_unet(), 2, 32, 48)
    ps = _problems(sites, seed=9)
    qs = [(x, wt, b, buf.clone()) for x, wt, b, buf in ps]
    _run(engine_lib, ps, 0.6, 0)
    _run(engine_lib, qs, 0.6, 1)
    for (*_, a), (*_, b), (M, Cc) in zip(ps, qs, sites):
        d = (a[:, :Cc].float() - b[:, :Cc].float()).abs()
        assert (d <= 2e-3 * (1 + b[:, :Cc].float().abs())).all(), (M, Cc, d.max().item())
        assert torch.isnan(b[:, Cc:]).all()


def test_residual_op_rejects(engine_lib):
    ps = _problems([(64, 96)], seed=1)
    arr = (_lib.SdCnProblem * 1)()
    x, w, b, buf = ps[0]
    arr[0] = _lib.SdCnProblem(x.data_ptr(), 96, w.data_ptr(), b.data_ptr(), buf.data_ptr(), buf.stride(0), 64, 96)
    assert engine_lib.sd_op_controlnet_residuals(arr, 1, 1.0, 0, 0, None, stream()) == 4
    assert engine_lib.sd_op_controlnet_residuals(arr, 17, 1.0, 0, 0, None, stream()) == 1


GUARD_ROWS, GUARD_COLS = 2, 24
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16


def _run_table(lib, table, mode, seed):
    """One sd_op_controlnet_residuals call on a table of (M, C) problems, every y inside an int16 sentinel buffer with
    guard rows around it and guard columns to its right.  Returns [(got float64 [M, C], want, bound)]."""
    probs = [cc.residual_problem(M, C_, seed + i) for i, (M, C_) in enumerate(table)]
    dev = []
    arr = (_lib.SdCnProblem * len(probs))()
    for i, (x, w, b, y0) in enumerate(probs):
        M, C_ = x.shape
        buf = torch.full((M + 2 * GUARD_ROWS, C_ + GUARD_COLS), SENTINEL, dtype=torch.int16, device="cuda")
        buf[GUARD_ROWS:GUARD_ROWS + M, :C_] = y0.view(torch.int16).cuda()
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        dev.append((xd, wd, bd, buf))
        arr[i] = _lib.SdCnProblem(xd.data_ptr(), C_, wd.data_ptr(), bd.data_ptr(), buf[GUARD_ROWS:].data_ptr(), buf.stride(0), M, C_)
    rc = lib.sd_op_controlnet_residuals(arr, len(probs), cc.RES_SCALE, mode, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    out = []
    for (x, w, b, y0), (*_, buf) in zip(probs, dev):
        M, C_ = x.shape
        hb = buf.cpu()
        assert (hb[:GUARD_ROWS] == SENTINEL).all() and (hb[GUARD_ROWS + M:] == SENTINEL).all(), "guard rows were written"
        assert (hb[:, C_:] == SENTINEL).all(), "guard columns were written"
        got = hb[GUARD_ROWS:GUARD_ROWS + M, :C_].contiguous().view(torch.float16).double()
        out.append((got,) + cc.residual_reference(x, w, b, y0, C.c_float(cc.RES_SCALE).value))
    return out


@pytest.mark.parametrize("mode", [0, 1], ids=["grouped", "unfused"])
@pytest.mark.parametrize("table", sorted(cc.RES_TABLES))
def test_residuals_element_by_element(engine_lib, table, mode):
    """cn_residual_kernel (mode 0) on a full table of 16 problems -- M around the 32-row wave slab and the 128-row
    tile, C from 64 to 1280 -- and on a table of one, per element against float64 with the n = 1 form of the chained
    bound of tests/test_multi_controlnet_gpu.py; the per-problem GEMMs (mode 1) on the same data meet the same bound."""
    for (M, C_), (got, want, bound) in zip(cc.RES_TABLES[table], _run_table(engine_lib, cc.RES_TABLES[table], mode, seed=77)):
        assert torch.isfinite(got).all()
        err = (got - want).abs()
        print("residuals %s mode %d M %d C %d: rel_l2 %.2e, worst |err| / bound %.3f" % (table, mode, M, C_, rel_l2(got, want),
                                                                                        (err / bound).max()))
        worst = (err - bound).argmax()
        assert (err <= bound).all(), (M, C_, "element", int(worst), err.flatten()[worst].item(), bound.flatten()[worst].item())


# ------------------------------------------------------------------------- one conditioning layer, per element
def _run_cond_conv(lib, case, x, w, b):
    """sd_op_cn_cond_conv on CPU operands (x NCHW); returns (code, int16 bits [N, OH, OW, Cout]) after checking the
    guard rows in front of and behind y."""
    OH, OW = cc.out_hw(case)
    rows = case.N * OH * OW
    xd = (x if case.Cin == 3 else x.permute(0, 2, 3, 1)).contiguous().cuda()
    wd, bd = w.cuda(), b.cuda()
    G = 4
    ybuf = torch.full((G + rows + G, case.Cout), SENTINEL, dtype=torch.int16, device="cuda")
    code = lib.sd_op_cn_cond_conv(C.c_void_p(xd.data_ptr()), 1 if case.Cin == 3 else 0, C.c_void_p(wd.data_ptr()),
                                  C.c_void_p(bd.data_ptr()), case.N, case.IH, case.IW, case.Cin, case.Cout, case.stride,
                                  case.silu, C.c_void_p(ybuf[G:].data_ptr()), stream())
    torch.cuda.synchronize()
    hb = ybuf.cpu()
    assert (hb[:G] == SENTINEL).all() and (hb[G + rows:] == SENTINEL).all(), "guard rows around y were written"
    return code, hb[G:G + rows].contiguous().view(case.N, OH, OW, case.Cout)


@pytest.mark.parametrize("case", cc.CASES, ids=[cc.case_id(c) for c in cc.CASES])
def test_cond_conv_layer_element_by_element(engine_lib, case):
    """cn_cond_conv_kernel alone, every template variant at stride 1 and 2, against float64 conv2d + SiLU of the fp16
    operands with the bound of cn_cases.bound (tests/test_cn_cases.py proves it on an emulation); the border ring, where
    taps fall outside the image, is reported and asserted on its own."""
    x, w, b, out, y, A = cc.inputs_and_reference(case)
    code, bits = _run_cond_conv(engine_lib, case, x, w, b)
    assert code == 0, engine_lib.sd_last_error()
    got = bits.view(torch.float16).double()
    assert torch.isfinite(got).all()
    ratio = (got - out).abs() / cc.bound(case, out, y, A)
    ring = cc.border_ring(case)
    assert ring.any()
    print("%s: rel_l2 %.2e, worst |err| / bound %.3f, on the border ring %.3f" % (cc.case_id(case), rel_l2(got, out), ratio.max(),
                                                                               ratio[:, ring].max()))
    assert ratio[:, ring].max() <= 1.0, "a border pixel"
    assert ratio.max() <= 1.0


def test_cond_conv_layer_rejections_write_nothing(engine_lib):
    for case in [cc.Case(8, 16, 1, 1, 4, 4, 1), cc.Case(16, 24, 1, 1, 4, 4, 1), cc.Case(16, 16, 3, 1, 4, 4, 1),
                 cc.Case(16, 16, 1, 0, 4, 4, 1)]:
        x = torch.zeros(max(case.N, 1), case.Cin, 4, 4, dtype=torch.float16)
        w = torch.zeros(case.Cout, case.Cin, 3, 3, dtype=torch.float16)
        OH, OW = cc.out_hw(case)
        ybuf = torch.full((16 + max(case.N, 1) * OH * OW, case.Cout), SENTINEL, dtype=torch.int16, device="cuda")
        xd, wd, bd = x.cuda(), w.cuda(), torch.zeros(case.Cout, dtype=torch.float16, device="cuda")
        code = engine_lib.sd_op_cn_cond_conv(C.c_void_p(xd.data_ptr()), 0, C.c_void_p(wd.data_ptr()), C.c_void_p(bd.data_ptr()),
                                             case.N, 4, 4, case.Cin, case.Cout, case.stride, 1, C.c_void_p(ybuf.data_ptr()),
                                             stream())
        torch.cuda.synchronize()
        assert code == 4, case
        assert engine_lib.sd_last_error()
        assert (ybuf == SENTINEL).all()
    assert engine_lib.sd_op_cn_cond_conv(None, 0, None, None, 1, 4, 4, 16, 16, 1, 1, None, stream()) == 1


# ------------------------------------------------------------------------------------ conditioning embedding
@pytest.fixture(scope="module")
def tiny():
    ucfg = config.tiny_unet()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=21, perturb=0.1).items()}
    ccfg = controlnet.encoder_config(ucfg)
    csd = synth_cn_state_dict(ccfg, seed=4)
    net = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    cn = HipControlNetModel(net, ccfg).load_state_dict(csd)
    return ucfg, usd, ccfg, csd, net, cn


@pytest.mark.parametrize("n,H8,W8", [(1, 512, 512), (2, 512, 768), (3, 64, 64)])
def test_cond_embedding_matches_fp32(engine_lib, tiny, n, H8, W8):
    *_, csd, net, cn = tiny
    g = torch.Generator().manual_seed(n + H8)
    img = torch.rand(n, 3, H8, W8, generator=g).half()
    out = cn.cond_embedding(img.cuda())
    with torch.no_grad():
        ref = cond_embedding(csd, img.float())
    assert out.shape == ref.shape
    assert rel_l2(out, ref) < 3e-3


# ------------------------------------------------------------------------------------------ UNet + ControlNet
def _inputs(cfg, B, H, W, n_ctrl, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    img = torch.rand(n_ctrl, 3, 8 * H, 8 * W, generator=g).half()
    return x, ehs, img


def _sdxl_kwargs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    tdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    return {"text_embeds": torch.randn(B, tdim, generator=g).half(),
            "time_ids": torch.tensor([[64.0, 64.0, 0.0, 0.0, 64.0, 64.0]] * B)}


def _build(ucfg, seed):
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=seed, perturb=0.1).items()}
    ccfg = controlnet.encoder_config(ucfg)
    csd = synth_cn_state_dict(ccfg, seed=seed + 1)
    net = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    cn = HipControlNetModel(net, ccfg).load_state_dict(csd)
    return usd, ccfg, csd, net, cn


@pytest.mark.parametrize("variant", ["plain", "linear", "sdxl"])
@pytest.mark.parametrize("B,H,W,t,n_ctrl", [(2, 16, 16, 981.0, 1), (1, 8, 24, 1.0, 1), (3, 24, 16, 500.0, 3),
                                            (4, 16, 8, 301.0, 2)])
def test_unet_with_controlnet_matches_oracle(engine_lib, variant, B, H, W, t, n_ctrl):
    ucfg = config.tiny_unet(linear=variant == "linear", sdxl_cond=variant == "sdxl")
    usd, ccfg, csd, net, cn = _build(ucfg, seed=31)
    x, ehs, img = _inputs(ucfg, B, H, W, n_ctrl, B * 100 + H + n_ctrl)
    add = _sdxl_kwargs(ucfg, B, 3) if variant == "sdxl" else None
    add_dev = {k: v.cuda() for k, v in add.items()} if add else None
    with torch.no_grad():
        ref = unet_cn_forward(ucfg, usd, ccfg, csd, x, torch.tensor(t), ehs, img, 0.8,
                              {k: v.float() for k, v in add.items()} if add else None)
    net.attach_controlnet(cn)
    a = net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs=add_dev, controlnet_cond=img.cuda(),
            controlnet_conditioning_scale=0.8)[0]
    assert rel_l2(a, ref) < TOL
    with torch.no_grad():
        plain = unet_ref.unet_forward(ucfg, usd, x.float(), torch.tensor(t), ehs.float(),
                                      {k: v.float() for k, v in add.items()} if add else None)
    assert rel_l2(plain, ref) > 5 * TOL                       # the ControlNet really changes the result


def test_detach_scale_zero_and_rejections(engine_lib, tiny):
    ucfg, usd, ccfg, csd, net, cn = tiny
    fresh = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    x, ehs, img = _inputs(ucfg, 2, 16, 24, 1, 5)
    never = fresh(x.cuda(), 401.0, ehs.cuda())[0]
    net.attach_controlnet(cn)
    try:
        with_cn = net(x.cuda(), 401.0, ehs.cuda(), controlnet_cond=img.cuda(), controlnet_conditioning_scale=1.0)[0]
        zero = net(x.cuda(), 401.0, ehs.cuda(), controlnet_cond=img.cuda(), controlnet_conditioning_scale=0.0)[0]
        with pytest.raises(ValueError):
            net(x.cuda(), 401.0, ehs.cuda())                                 # attached: control image required
        with pytest.raises(ValueError):                                      # 3 images do not divide B = 2
            net(x.cuda(), 401.0, ehs.cuda(), controlnet_cond=img.repeat(3, 1, 1, 1).cuda(), controlnet_conditioning_scale=1.0)
        net.use_graph(True)
        with pytest.raises(_lib.EngineError):
            net(x.cuda(), 401.0, ehs.cuda(), controlnet_cond=img.cuda(), controlnet_conditioning_scale=1.0)
        net.use_graph(False)
    finally:
        net.use_graph(False)
        net.attach_controlnet(None)
    after = net(x.cuda(), 401.0, ehs.cuda())[0]
    assert torch.equal(zero, never) and torch.equal(after, never) and not torch.equal(with_cn, never)
    with pytest.raises(ValueError):
        net(x.cuda(), 401.0, ehs.cuda(), controlnet_cond=img.cuda(), controlnet_conditioning_scale=1.0)


def test_cache_reuse_and_invalidation(engine_lib, tiny):
    ucfg, usd, ccfg, csd, net, cn = tiny
    x, ehs, img = _inputs(ucfg, 2, 16, 16, 1, 8)
    img2 = torch.rand_like(img.float()).half().cuda()
    xd, ed, imd = x.cuda(), ehs.cuda(), img.cuda()
    net.attach_controlnet(cn)
    try:
        ref = net(xd, 900.0, ed, controlnet_cond=imd, controlnet_conditioning_scale=1.0)[0]
        ref2 = net(xd, 900.0, ed, controlnet_cond=img2, controlnet_conditioning_scale=1.0)[0]
        net.text_kv_cache(True)
        a = net(xd, 900.0, ed, controlnet_cond=imd, controlnet_conditioning_scale=1.0)[0]
        b = net(xd, 900.0, ed, controlnet_cond=imd, controlnet_conditioning_scale=1.0)[0]      # reuses the caches
        imd.copy_(img2)                        # same pointer, new contents: stale until the cache is toggled
        stale = net(xd, 900.0, ed, controlnet_cond=imd, controlnet_conditioning_scale=1.0)[0]
        net.text_kv_cache(True)
        fresh = net(xd, 900.0, ed, controlnet_cond=imd, controlnet_conditioning_scale=1.0)[0]
        other = torch.rand_like(img2.float()).half()
        c = net(xd, 900.0, ed, controlnet_cond=other, controlnet_conditioning_scale=1.0)[0]   # new pointer: recomputed
        net.text_kv_cache(False)
        c_ref = net(xd, 900.0, ed, controlnet_cond=other, controlnet_conditioning_scale=1.0)[0]
    finally:
        net.text_kv_cache(False)
        net.attach_controlnet(None)
    assert torch.equal(a, ref) and torch.equal(b, ref)
    assert torch.equal(stale, ref) and torch.equal(fresh, ref2)
    assert torch.equal(c, c_ref)


def test_controlnet_with_ip_adapter(engine_lib, monkeypatch, tiny):
    from ip_oracle import ip_attention, project, synth_ip_state_dict
    from stablediffusion_amd.models import HipIPAdapter
    ucfg, usd, ccfg, csd, net, cn = tiny
    ip_sd = synth_ip_state_dict(ucfg, 128, 4, seed=3)
    ad = HipIPAdapter(net, 128, 4).load_state_dict(ip_sd)
    x, ehs, img = _inputs(ucfg, 2, 16, 16, 1, 12)
    emb = torch.randn(2, 1, 128, generator=torch.Generator().manual_seed(2)).half()
    monkeypatch.setattr(unet_ref, "attention", ip_attention(ip_sd, 0.6))
    tok = project(ip_sd, emb.float(), 4)
    with torch.no_grad():
        ref = unet_cn_forward(ucfg, usd, ccfg, csd, x, torch.tensor(700.0), ehs, img, 0.9,
                              unet_ctx=(ehs.float(), tok))
    net.attach_controlnet(cn).attach_ip_adapter(ad).set_ip_adapter_scale(0.6)
    try:
        a = net(x.cuda(), 700.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [emb.cuda()]}, controlnet_cond=img.cuda(),
                controlnet_conditioning_scale=0.9)[0]
    finally:
        net.attach_controlnet(None).attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    assert rel_l2(a, ref) < TOL


def test_create_rejects_mismatched_configs(engine_lib, tiny):
    ucfg, usd, ccfg, csd, net, cn = tiny
    bad = [controlnet.encoder_config(ucfg, block_out_channels=(64, 128, 256, 320)),
           controlnet.encoder_config(ucfg, cross_attention_dim=128),
           controlnet.encoder_config(ucfg, layers_per_block=1),
           controlnet.encoder_config(ucfg, in_channels=9)]
    for c in bad:
        with pytest.raises(_lib.EngineError):
            HipControlNetModel(net, c)
    with pytest.raises(_lib.EngineError):
        HipControlNetModel(net, ccfg, conditioning_channels=1)
    deeper = controlnet.encoder_config(ucfg, transformer_layers_per_block=(2, 1, 1, 1), attention_head_dim=(1, 2, 4, 4))
    HipControlNetModel(net, deeper)                               # heads and depth may differ


# ----------------------------------------------------------------------------------------------- full size
@pytest.mark.parametrize("preset", ["sd15", "sdxl"])
def test_fullsize_unet_with_controlnet(engine_lib, preset):
    ucfg = config.sd15_unet() if preset == "sd15" else config.sdxl_unet()
    B, H = (8, 64) if preset == "sd15" else (2, 128)
    usd, ccfg, csd, net, cn = _build(ucfg, seed=41)
    x, ehs, img = _inputs(ucfg, B, H, H, B // 2, 13)
    add = _sdxl_kwargs(ucfg, B, 5) if preset == "sdxl" else None
    net.attach_controlnet(cn)
    a = net(x.cuda(), 500.0, ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in add.items()} if add else None,
            controlnet_cond=img.cuda(), controlnet_conditioning_scale=1.0)[0].float().cpu()
    del net, cn
    torch.cuda.empty_cache()
    with torch.no_grad():
        ref = unet_cn_forward(ucfg, usd, ccfg, csd, x, torch.tensor(500.0), ehs, img, 1.0,
                              {k: v.float() for k, v in add.items()} if add else None)
    assert rel_l2(a, ref) < TOL


# ------------------------------------------------------------------------------------------------ pipeline
def test_tiny_txt2img_with_control_image_matches_oracle_loop(engine_lib, monkeypatch):
    """10-step DDIM through the pipeline (device-fused CFG step) with a ControlNet loaded from an original-format dict
    and a guidance window that switches it off for the last two steps, against pipeline_ref.denoise_ref with the
    oracle composition."""
    from oracle import pipeline_ref
    from stablediffusion_amd.models import HipAutoencoderKL
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    from test_controlnet import _to_original
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=11, perturb=0.1).items()}
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1).items()}
    ccfg = controlnet.encoder_config(ucfg)
    csd = synth_cn_state_dict(ccfg, seed=6)
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler("DDIM")
    model.load_controlnet(_to_original(csd, ccfg, "control_model."))
    g = torch.Generator().manual_seed(4)
    B = 2
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    ctrl = torch.rand(1, 3, 128, 128, generator=g)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    got = pipe(model, prompt_embeds=pos.cuda(), negative_prompt_embeds=neg.cuda(), latents=lat0.cuda(),
               num_inference_steps=10, guidance_scale=5.0, height=128, width=128, control_image=ctrl,
               controlnet_conditioning_scale=0.9, control_guidance_end=0.8)
    assert pipe._fused_step_available(model, lat0.cuda())
    step = [0]

    def cn_unet(cfg, w, x, t, ehs, added):
        scale = 0.9 if step[0] < 8 else 0.0
        step[0] += 1
        return unet_cn_forward(cfg, w, ccfg, csd, x, t, ehs, ctrl.half(), scale, added)

    ref_ctx = torch.cat([neg, pos]).float()
    plain = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), ref_ctx, steps=10, guidance_scale=5.0, scheduler="DDIM")
    monkeypatch.setattr(pipeline_ref, "unet_forward", cn_unet)
    ref = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), ref_ctx, steps=10, guidance_scale=5.0, scheduler="DDIM")
    assert step[0] == 10
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got, ref) < TOL
    assert rel_l2(plain, ref) > 5 * TOL
    model.unload_controlnet()
