"""IP-Adapter on the GPU: the fused decoupled cross-attention kernel against fp32 SDPA + lambda SDPA, and the UNet
with an adapter attached against the fp32 oracle with its attention patched the way diffusers'
IPAdapterAttnProcessor2_0 computes it (tests/ip_oracle.py)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sdpa(q, k, v, heads, scale=None):
    B, Tq, Cq = q.shape
    d = Cq // heads
    o = F.scaled_dot_product_attention(q.view(B, Tq, heads, d).transpose(1, 2),
                                       k.reshape(B, -1, heads, d).transpose(1, 2),
                                       v.reshape(B, -1, heads, d).transpose(1, 2), scale=scale)
    return o.transpose(1, 2).reshape(B, Tq, Cq)


def _run_op(lib, q, k, v, kip, vip, B, Tq, L, Tip, heads, d, lam, prescaled=0):
    """q, k, v, kip, vip: fp16 device views [B, T, width] with their own row strides (stride(1))."""
    out = torch.full((B, Tq, heads * d), float("nan"), dtype=torch.float16, device="cuda")
    rc = lib.sd_op_ip_cross_attention(P(q), P(k), P(v), P(kip), P(vip), P(out), B, Tq, L, Tip, heads, d,
                                      q.stride(1), k.stride(1), v.stride(1), kip.stride(1), vip.stride(1),
                                      out.stride(1), lam, prescaled, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return out


def _case(B, Tq, L, Tip, heads, d, seed, kscale=1.0, kipscale=1.0, strided=True):
    g = torch.Generator().manual_seed(seed)
    C_ = heads * d
    q = torch.randn(B, Tq, C_, generator=g).half()
    # text K / V as the UNet holds them: slices of one stacked [K | V] row (and IP K / V of another)
    kv = torch.randn(B, L, 2 * C_ + (24 if strided else 0), generator=g)
    kv[..., :C_] *= kscale
    kv = kv.half()
    kvi = torch.randn(B, Tip, 2 * C_ + (40 if strided else 0), generator=g)
    kvi[..., :C_] *= kipscale
    kvi = kvi.half()
    return q, kv, kvi


def _ref(q, kv, kvi, heads, d, lam):
    C_ = heads * d
    qf, kvf, kvif = q.float(), kv.float(), kvi.float()
    return (_sdpa(qf, kvf[..., :C_], kvf[..., C_:2 * C_], heads)
            + lam * _sdpa(qf, kvif[..., :C_], kvif[..., C_:2 * C_], heads))


def _check(engine_lib, B, Tq, L, Tip, heads, d, lam, seed, tol=3e-3, **kw):
    q, kv, kvi = _case(B, Tq, L, Tip, heads, d, seed, **kw)
    C_ = heads * d
    ref = _ref(q, kv, kvi, heads, d, lam)
    qd, kvd, kvid = q.cuda(), kv.cuda(), kvi.cuda()
    out = _run_op(engine_lib, qd, kvd[..., :C_], kvd[..., C_:2 * C_], kvid[..., :C_], kvid[..., C_:2 * C_],
                  B, Tq, L, Tip, heads, d, lam)
    assert torch.isfinite(out.float()).all()
    err = rel_l2(out, ref)
    assert err < tol, err
    return out, ref


@pytest.mark.parametrize("d", [32, 40, 64, 80, 160])
@pytest.mark.parametrize("L,Tip", [(1, 4), (77, 16), (154, 64), (77, 4)])
def test_ip_op_matches_sdpa(engine_lib, d, L, Tip):
    heads = 2 if d == 160 else 3
    _check(engine_lib, 2, 67, L, Tip, heads, d, 0.6, seed=d * 1000 + L * 10 + Tip)


@pytest.mark.parametrize("lam", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("d", [40, 64])
def test_ip_op_scales(engine_lib, d, lam):
    _check(engine_lib, 3, 301, 77, 4, 5, d, lam, seed=7 + d)


def test_ip_op_zero_scale_is_text_attention(engine_lib):
    """lambda = 0: the image keys take no part -- equal to the text-only attention within rounding."""
    B, Tq, L, Tip, heads, d = 2, 129, 77, 16, 4, 40
    q, kv, kvi = _case(B, Tq, L, Tip, heads, d, 5)
    C_ = heads * d
    ref = _sdpa(q.float(), kv.float()[..., :C_], kv.float()[..., C_:2 * C_], heads)
    qd, kvd, kvid = q.cuda(), kv.cuda(), kvi.cuda()
    kvid[..., :C_] = float("inf")                       # never read
    out = _run_op(engine_lib, qd, kvd[..., :C_], kvd[..., C_:2 * C_], kvid[..., :C_], kvid[..., C_:2 * C_],
                  B, Tq, L, Tip, heads, d, 0.0)
    assert rel_l2(out, ref) < 3e-3


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("seg", ["text", "ip"])
def test_ip_op_large_scores(engine_lib, d, seg):
    """Scores far outside exp2's fp32 range in one segment (std 60, extremes past +-200 in log2 units): only the exact
    max subtraction keeps them finite."""
    ks, kis = (60.0, 1.0) if seg == "text" else (1.0, 60.0)
    _check(engine_lib, 2, 97, 77, 16, 2, d, 1.0, seed=31 + d, kscale=ks, kipscale=kis, tol=5e-3)


@pytest.mark.parametrize("d", [40, 64, 80, 160])
@pytest.mark.parametrize("seg", ["text", "ip"])
def test_ip_op_very_negative_scores(engine_lib, d, seg):
    """Every score of one segment very negative (keys anti-aligned with the queries): nothing underflows to 0 / 0."""
    B, Tq, L, Tip, heads = 2, 50, 77, 8, 2
    C_ = heads * d
    g = torch.Generator().manual_seed(d + (1 if seg == "ip" else 0))
    q = (torch.rand(B, Tq, C_, generator=g) + 0.5).half()
    kv = torch.randn(B, L, 2 * C_, generator=g)
    kvi = torch.randn(B, Tip, 2 * C_, generator=g)
    tgt = kv if seg == "text" else kvi
    # scores about -150 (below -100 for every key): exp2 of them underflows fp32 unless the max is subtracted
    tgt[..., :C_] = -(torch.rand(tgt.shape[0], tgt.shape[1], C_, generator=g) + 2.0) * (60.0 / d ** 0.5)
    kv, kvi = kv.half(), kvi.half()
    ref = _ref(q, kv, kvi, heads, d, 0.8)
    qd, kvd, kvid = q.cuda(), kv.cuda(), kvi.cuda()
    out = _run_op(engine_lib, qd, kvd[..., :C_], kvd[..., C_:], kvid[..., :C_], kvid[..., C_:], B, Tq, L, Tip, heads, d,
                  0.8)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, ref) < 5e-3


def test_ip_op_prescaled(engine_lib):
    """The UNet's form: queries carry log2(e)/sqrt(d) from the folded projection."""
    B, Tq, L, Tip, heads, d = 2, 200, 77, 4, 8, 40
    q, kv, kvi = _case(B, Tq, L, Tip, heads, d, 9)
    c = 1.4426950408889634 / d ** 0.5
    qs = (q.float() * c).half()
    C_ = heads * d
    ref = _ref((qs.float() / c), kv, kvi, heads, d, 1.0)
    qd, kvd, kvid = qs.cuda(), kv.cuda(), kvi.cuda()
    out = torch.empty(B, Tq, C_, dtype=torch.float16, device="cuda")
    rc = engine_lib.sd_op_ip_cross_attention(P(qd), P(kvd[..., :C_]), P(kvd[..., C_:]), P(kvid[..., :C_]),
                                             P(kvid[..., C_:]), P(out), B, Tq, L, Tip, heads, d, C_, kvd.stride(1),
                                             kvd.stride(1), kvid.stride(1), kvid.stride(1), C_, 1.0, 1, 0, None,
                                             stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < 3e-3


def test_ip_op_rejects_unsupported(engine_lib):
    x = torch.zeros(1, 8, 512, dtype=torch.float16, device="cuda")
    for (L, Tip, d) in [(161, 4, 64), (77, 65, 64), (77, 0, 64), (77, 4, 128)]:
        rc = engine_lib.sd_op_ip_cross_attention(P(x), P(x), P(x), P(x), P(x), P(x), 1, 8, L, Tip, 512 // d, d,
                                                 512, 512, 512, 512, 512, 512, 1.0, 0, 0, None, stream())
        assert rc == 4, (L, Tip, d)


# ---------------------------------------------------------------------------------------------- UNet level
from ip_oracle import ip_attention, project, synth_ip_state_dict  # noqa: E402
from oracle import unet_ref  # noqa: E402
from stablediffusion_amd import config, weights  # noqa: E402
from stablediffusion_amd.models import HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

TOL = 1e-2
D_IMG, N_TOK = 128, 4


@pytest.fixture(scope="module")
def tiny():
    cfg = config.tiny_unet()
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1).items()}
    ip_sd = synth_ip_state_dict(cfg, D_IMG, N_TOK, seed=3)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    ad = HipIPAdapter(net, D_IMG, N_TOK).load_state_dict(ip_sd)
    return cfg, sd, ip_sd, net, ad


def _inputs(cfg, B, H, W, n_img, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(B, n_img, D_IMG, generator=g).half()
    return x, ehs, img


def _oracle(monkeypatch, cfg, sd, ip_sd, x, t, ehs, img, scale):
    monkeypatch.setattr(unet_ref, "attention", ip_attention(ip_sd, scale))
    tok = project(ip_sd, img.float(), N_TOK)
    with torch.no_grad():
        return unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), (ehs.float(), tok))


@pytest.mark.parametrize("B,H,W,t,n_img", [(2, 16, 16, 981.0, 1), (1, 8, 24, 1.0, 2), (3, 32, 32, 500.0, 1),
                                           (3, 16, 24, 301.0, 3)])
def test_unet_with_ip_adapter_matches_oracle(engine_lib, monkeypatch, tiny, B, H, W, t, n_img):
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, B, H, W, n_img, B * 100 + H + n_img)
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.7)
    try:
        ref = _oracle(monkeypatch, cfg, sd, ip_sd, x, t, ehs, img, 0.7)
        plain = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), ehs.float())
        a = net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})[0]
        b = net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})[0]
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    assert rel_l2(a, ref) < TOL
    assert rel_l2(plain, ref) > 5 * TOL          # the image branch really changes the result
    assert torch.equal(a, b)


def test_deprecated_2d_image_embeds(engine_lib, tiny):
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, 2, 16, 16, 1, 4)
    net.attach_ip_adapter(ad)
    try:
        a = net(x.cuda(), 11.0, ehs.cuda(), added_cond_kwargs={"image_embeds": img[:, 0].cuda()})[0]
        b = net(x.cuda(), 11.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})[0]
    finally:
        net.attach_ip_adapter(None)
    assert torch.equal(a, b)


def test_detach_restores_plain_forward_bitwise(engine_lib, tiny):
    cfg, sd, ip_sd, net, ad = tiny
    fresh = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    x, ehs, img = _inputs(cfg, 2, 16, 24, 1, 5)
    never = fresh(x.cuda(), 401.0, ehs.cuda())[0]
    net.attach_ip_adapter(ad)
    with_ip = net(x.cuda(), 401.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})[0]
    with pytest.raises(ValueError):
        net(x.cuda(), 401.0, ehs.cuda())                     # attached: image_embeds required
    net.attach_ip_adapter(None)
    after = net(x.cuda(), 401.0, ehs.cuda())[0]
    assert torch.equal(after, never) and not torch.equal(with_ip, never)
    with pytest.raises(ValueError):
        net(x.cuda(), 401.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})


def test_destroying_attached_adapter_detaches(engine_lib, tiny):
    """C-ABI contract: sd_ip_adapter_destroy on an attached adapter detaches it; the next forward is the plain one."""
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, 1, 16, 16, 1, 6)
    plain = net(x.cuda(), 7.0, ehs.cuda())[0]
    h = C.c_void_p()
    assert engine_lib.sd_ip_adapter_create(net._h, D_IMG, N_TOK, C.byref(h)) == 0
    from stablediffusion_amd.models import _load_weights
    _load_weights(engine_lib, h, "ip_adapter", ip_sd)
    assert engine_lib.sd_ip_adapter_finalize(h) == 0
    assert engine_lib.sd_unet_set_ip_adapter(net._h, h) == 0
    assert engine_lib.sd_ip_adapter_destroy(h) == 0
    assert torch.equal(net(x.cuda(), 7.0, ehs.cuda())[0], plain)


def test_zero_scale_matches_plain_forward(engine_lib, tiny):
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, 2, 16, 16, 2, 7)
    plain = net(x.cuda(), 600.0, ehs.cuda())[0]
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.0)
    try:
        z = net(x.cuda(), 600.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})[0]
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    assert rel_l2(z, plain) < 1e-3


def test_ip_kv_cache_reuses_and_invalidates(engine_lib, tiny):
    """The image K / V follow the text K / V cache: bitwise the uncached result inside a loop, recomputed after
    sd_unet_text_kv_cache re-arms it when the embedding contents behind the same pointer changed."""
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, 2, 16, 16, 1, 8)
    x, ehs, img = x.cuda(), ehs.cuda(), img.cuda()
    kw = {"image_embeds": [img]}
    net.attach_ip_adapter(ad)
    try:
        base = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
        net.text_kv_cache(True)
        a = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
        b = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
        assert torch.equal(a, base) and torch.equal(b, base)
        img.mul_(-1.0)                              # new contents, same pointer
        stale = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
        assert torch.equal(stale, base)             # (cached, as documented, until the cache is re-armed)
        net.text_kv_cache(True)
        c = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
    finally:
        net.text_kv_cache(False)
    fresh = net(x, 501.0, ehs, added_cond_kwargs=kw)[0]
    net.attach_ip_adapter(None)
    assert torch.equal(c, fresh) and not torch.equal(c, base)


def test_graph_mode_with_adapter_is_rejected(engine_lib, tiny):
    cfg, sd, ip_sd, net, ad = tiny
    x, ehs, img = _inputs(cfg, 1, 16, 16, 1, 9)
    net.attach_ip_adapter(ad).use_graph(True)
    try:
        with pytest.raises(RuntimeError, match="graph replay with an IP-Adapter"):
            net(x.cuda(), 5.0, ehs.cuda(), added_cond_kwargs={"image_embeds": [img.cuda()]})
    finally:
        net.use_graph(False).attach_ip_adapter(None)


def test_adapter_rejects_unsupported_configs(engine_lib, tiny):
    cfg, sd, ip_sd, net, ad = tiny
    for d_img, n_tok in [(128, 0), (128, 17), (100, 4)]:
        with pytest.raises(RuntimeError, match="error 4"):
            HipIPAdapter(net, d_img, n_tok)


@pytest.mark.parametrize("preset,B,hw,d_img", [("sd15", 8, 64, 1024), ("sdxl", 2, 128, 1280)])
def test_fullsize_unet_with_ip_adapter(engine_lib, monkeypatch, preset, B, hw, d_img):
    """Full-width UNet + synthetic adapter against the oracle run in fp32 on the GPU through PyTorch-ROCm."""
    cfg = config.PRESETS[preset][0]()
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=21).items()}
    ip_sd = synth_ip_state_dict(cfg, d_img, N_TOK, seed=22)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    ad = HipIPAdapter(net, d_img, N_TOK).load_state_dict(ip_sd)
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.8)
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 4, hw, hw, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    img = torch.randn(B, 1, d_img, generator=g).half()
    added = {"image_embeds": [img.cuda()]}
    ref_added = None
    if cfg.addition_embed_type == "text_time":
        te = torch.randn(B, 1280, generator=g).half()
        ids = torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B)
        added.update(text_embeds=te.cuda(), time_ids=ids.cuda())
        ref_added = {"text_embeds": te.float().cuda(), "time_ids": ids.cuda()}
    got = net(x.cuda(), 501.0, ehs.cuda(), added_cond_kwargs=added)[0]
    dsd = {k: v.cuda() for k, v in sd.items()}
    dip = {k: v.cuda() for k, v in ip_sd.items()}
    monkeypatch.setattr(unet_ref, "attention", ip_attention(dip, 0.8))
    orig = unet_ref.timestep_sinusoid                # (the sinusoid table is built on the host)
    monkeypatch.setattr(unet_ref, "timestep_sinusoid", lambda tt, *a, **k: orig(tt.cpu(), *a, **k).cuda())
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    tok = project(dip, img.float().cuda(), N_TOK)
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, dsd, x.float().cuda(), torch.tensor(501.0), (ehs.float().cuda(), tok),
                                    ref_added)
    assert rel_l2(got, ref) < TOL


def test_tiny_txt2img_with_ip_embeds_matches_oracle_loop(engine_lib, monkeypatch):
    """10-step DDIM through the pipeline (device-fused CFG step) with ip_adapter_image_embeds and an adapter loaded
    from an original-format dict, against pipeline_ref.denoise_ref with the IP-patched attention."""
    from oracle import pipeline_ref
    from stablediffusion_amd import ip_adapter
    from stablediffusion_amd.models import HipAutoencoderKL
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=11, perturb=0.1).items()}
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1).items()}
    ip_sd = synth_ip_state_dict(ucfg, D_IMG, N_TOK, seed=5)
    # the same weights in the original file layout (ids 2 i + 1 in diffusers' site order)
    orig = {"image_proj": {"proj.weight": ip_sd[f"{ip_adapter.PROJ}.image_embeds.weight"],
                           "proj.bias": ip_sd[f"{ip_adapter.PROJ}.image_embeds.bias"],
                           "norm.weight": ip_sd[f"{ip_adapter.PROJ}.norm.weight"],
                           "norm.bias": ip_sd[f"{ip_adapter.PROJ}.norm.bias"]}, "ip_adapter": {}}
    for i, site in ip_adapter.site_ids(ucfg).items():
        for n in ("to_k_ip", "to_v_ip"):
            orig["ip_adapter"][f"{i}.{n}.weight"] = ip_sd[f"{site}.attn2.processor.{n}.0.weight"]
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler("DDIM")
    model.load_ip_adapter(orig)
    model.set_ip_adapter_scale(0.8)
    g = torch.Generator().manual_seed(4)
    B = 2
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    ie = torch.randn(2 * B, 1, D_IMG, generator=g).half()
    ie[:B] = 0                                                  # what a zero negative image embedding looks like
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    got = pipe(model, prompt_embeds=pos.cuda(), negative_prompt_embeds=neg.cuda(), latents=lat0.cuda(),
               num_inference_steps=10, guidance_scale=5.0, height=128, width=128, ip_adapter_image_embeds=[ie.cuda()])
    assert pipe._fused_step_available(model, lat0.cuda())
    monkeypatch.setattr(unet_ref, "attention", ip_attention(ip_sd, 0.8))
    tok = project(ip_sd, ie.float(), N_TOK)
    ref = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), (torch.cat([neg, pos]).float(), tok), steps=10,
                                   guidance_scale=5.0, scheduler="DDIM")
    plain = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), torch.cat([neg, pos]).float(), steps=10,
                                     guidance_scale=5.0, scheduler="DDIM")
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got, ref) < TOL
    assert rel_l2(plain, ref) > 5 * TOL
