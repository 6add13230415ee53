"""IP-Adapter Plus on the GPU: resampler_attn_kernel through sd_op_resampler_attention against float64 SDPA over the
concatenated fp16 operands (tests/resampler_oracle.py holds the cases, the reference and the bound; the CPU suite proves
the bound on an emulation of the kernel's arithmetic), the Resampler graph against the float64 oracle, the UNet with a
Plus adapter against the fp32 oracle fed the oracle's tokens, the image K / V cache rules, and the txt2img loop with an
image prompt through the engine's CLIP vision tower."""
import ctypes as C

import pytest
import torch

import resampler_oracle as ro
from conftest import rel_l2
from ip_oracle import ip_attention, project, synth_ip_state_dict
from oracle import unet_ref
from stablediffusion_amd import _lib, config, ip_adapter, weights
from stablediffusion_amd.models import HipIPAdapter, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu

TAIL = 64                      # guard rows behind every operand and behind out
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
TOL = 1e-2                     # of tests/test_ip_adapter_gpu.py
TOK_TOL = 5e-3                 # of tests/test_clip_vision_gpu.py


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16, device="cuda")


def run_op(lib, q, kx, vx, kl, vl, heads, strided):
    """One launch; returns the [B, n_q, A] fp16 output on the CPU after checking that nothing around it was written.
    strided: the graph's layout -- k | v as column slices of one wide buffer per source, q and out in padded rows, NaN
    in every pad column and in 64 rows behind each last row; else dense operands (still NaN behind them)."""
    B, n_q, A = q.shape
    T = kx.shape[1]
    if strided:
        qb, xb, lb = _nan(B * n_q + TAIL, A + 8), _nan(B * T + TAIL, 2 * A + 24), _nan(B * n_q + TAIL, 2 * A + 40)
        qv = qb[:B * n_q, :A]
        kxv, vxv = xb[:B * T, 8:A + 8], xb[:B * T, A + 16:2 * A + 16]
        klv, vlv = lb[:B * n_q, 0:A], lb[:B * n_q, A + 32:2 * A + 32]
        ldo = A + 8
    else:
        bufs = [_nan(B * n + TAIL, A) for n in (n_q, T, T, n_q, n_q)]
        qv, kxv, vxv, klv, vlv = (b[:B * n] for b, n in zip(bufs, (n_q, T, T, n_q, n_q)))
        ldo = A
    for dst, src in ((qv, q), (kxv, kx), (vxv, vx), (klv, kl), (vlv, vl)):
        dst.copy_(src.reshape(-1, A).cuda())
    obuf = torch.full((B * n_q + TAIL, ldo), SENTINEL, dtype=torch.int16, device="cuda")
    rc = lib.sd_op_resampler_attention(P(qv), P(kxv), P(vxv), P(klv), P(vlv), P(obuf), B, n_q, T, heads, qv.stride(0),
                                       kxv.stride(0), vxv.stride(0), klv.stride(0), vlv.stride(0), ldo, 0, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    ob = obuf.cpu()
    assert (ob[B * n_q:] == SENTINEL).all(), "rows behind the output were written"
    assert (ob[:, A:] == SENTINEL).all(), "pad columns of the output were written"
    return ob[:B * n_q, :A].contiguous().view(torch.float16).view(B, n_q, A)


def check(tag, out, ops, heads, rel_tol=3e-3):
    O, A = ro.op_reference(*ops, heads)
    o = out.double()
    assert torch.isfinite(o).all(), tag
    Tk = ops[1].shape[1] + ops[3].shape[1]
    bound = ro.op_bound(O, A, Tk, torch.maximum(ops[2].abs().max(), ops[4].abs().max()).double())
    err = (o - O).abs()
    ratio, r = (err / bound).max().item(), rel_l2(out, O)
    print("%s: rel_l2 %.2e, worst |err| / bound %.3f" % (tag, r, ratio))
    assert r < rel_tol, (tag, r)
    assert ratio <= 1.0, (tag, ratio)
    return ratio


@pytest.mark.parametrize("n_q", ro.OP_N_Q)
@pytest.mark.parametrize("T", ro.OP_T_FEAT)
def test_op_against_float64(engine_lib, T, n_q):
    """Every key count at which the staging, the per-wave key split or the padding changes, operands as the graph
    passes them (bit-identical to the dense layout), out inside a sentinel-filled buffer."""
    for heads, B in ro.OP_HEADS_B:
        ops = ro.op_inputs(B, n_q, T, heads, seed=T * 100 + n_q)
        strided = run_op(engine_lib, *ops, heads, True)
        check(f"T{T} nq{n_q} h{heads} B{B}", strided, ops, heads)
        dense = run_op(engine_lib, *ops, heads, False)
        assert torch.equal(dense.view(torch.int16), strided.view(torch.int16))


@pytest.mark.parametrize("seg", ["features", "latents"])
def test_op_large_scores(engine_lib, seg):
    """Scores far outside exp2's fp32 range in one segment (std 60 per unit of q, extremes past +-200 in log2 units):
    either segment may dominate the joint softmax; only the exact max subtraction keeps it finite."""
    ks = (60.0, 1.0) if seg == "features" else (1.0, 60.0)
    for T, n_q in ((257, 16), (33, 4)):
        ops = ro.op_inputs(2, n_q, T, 3, seed=31 + T, kx_scale=ks[0], kl_scale=ks[1])
        check(f"large {seg} T{T}", run_op(engine_lib, *ops, 3, True), ops, 3, rel_tol=5e-3)


@pytest.mark.parametrize("seg", ["features", "latents"])
def test_op_very_negative_scores(engine_lib, seg):
    """Every score of one segment about -150 (keys anti-aligned with positive queries): that segment underflows to
    weight 0 entirely and the other carries the softmax; nothing becomes 0 / 0."""
    B, n_q, T, heads = 2, 16, 50, 3
    g = torch.Generator().manual_seed(5 if seg == "features" else 6)
    q, kx, vx, kl, vl = ro.op_inputs(B, n_q, T, heads, seed=77)
    q = (torch.rand(q.shape, generator=g) + 0.5).half()
    tgt = kx if seg == "features" else kl
    neg = (-(torch.rand(tgt.shape, generator=g) + 2.0) * (60.0 / 8.0)).half()
    ops = (q, neg if seg == "features" else kx, vx, neg if seg == "latents" else kl, vl)
    out = run_op(engine_lib, *ops, heads, True)
    check(f"negative {seg}", out, ops, heads, rel_tol=5e-3)
    # the surviving segment alone gives the same answer: the other one's weights are zero
    if seg == "features":
        alone = ro.op_reference(q, kx[:, :0], vx[:, :0], kl, vl, heads)[0]
    else:
        alone = ro.op_reference(q, kx, vx, kl[:, :0], vl[:, :0], heads)[0]
    assert rel_l2(out, alone) < 5e-3


def test_op_constant_v(engine_lib):
    """Every V row of both segments equal to c under random scores: the weights sum to one, so out = c within one
    fp16 step of c."""
    B, n_q, T, heads = 2, 16, 257, 3
    q, kx, vx, kl, vl = ro.op_inputs(B, n_q, T, heads, seed=12)
    g = torch.Generator().manual_seed(13)
    c = (torch.randn(heads * 64, generator=g) * torch.tensor([1.0, 8.0, 0.01, 100.0]).repeat(heads * 16)).half()
    for row in (torch.ones(heads * 64).half(), c):
        ops = (q, kx, row.expand_as(vx).contiguous(), kl, row.expand_as(vl).contiguous())
        out = run_op(engine_lib, *ops, heads, True)
        cd = row.double()
        step = torch.maximum(2.0 ** (torch.floor(torch.log2(cd.abs().clamp_min(2.0 ** -14))) - 10),
                             torch.tensor(2.0 ** -24, dtype=torch.float64))       # fp16 spacing at c
        dev = (out.double() - cd).abs()
        print("constant V: worst |out - c| / step %.3f" % (dev / step).max().item())
        assert (dev <= step).all(), (dev / step).max().item()


def test_op_prescaled_and_rejections(engine_lib):
    B, n_q, T, heads = 2, 16, 257, 2
    q, kx, vx, kl, vl = ro.op_inputs(B, n_q, T, heads, seed=3)
    c = ro.LOG2E / 8.0
    qs = (q.float() * c).half()
    O, _ = ro.op_reference(qs.float() / c, kx, vx, kl, vl, heads)
    A = heads * 64
    d = [t.reshape(-1, A).cuda() for t in (qs, kx, vx, kl, vl)]
    out = torch.empty(B * n_q, A, dtype=torch.float16, device="cuda")
    rc = engine_lib.sd_op_resampler_attention(*(P(t) for t in d), P(out), B, n_q, T, heads, A, A, A, A, A, A, 1, 0, None, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert rel_l2(out.view(B, n_q, A), O) < 3e-3
    for nq, t, ld in [(17, 16, A), (0, 16, A), (16, 305, A), (16, 0, A)]:
        assert engine_lib.sd_op_resampler_attention(*(P(x) for x in d), P(out), 1, nq, t, heads, ld, ld, ld, ld, ld, ld, 0, 0,
                                                    None, stream()) == 4, (nq, t)
    assert engine_lib.sd_op_resampler_attention(*(P(x) for x in d), P(out), 1, 16, 16, heads, A + 4, A, A, A, A, A, 0, 0, None,
                                                stream()) == 1         # a stride that is no multiple of 8


# ---------------------------------------------------------------------------------------------- graph level
D_EMB, DIM, HEADS, DEPTH = 128, 128, 2, 2


def _feat(rows, T, seed, d=D_EMB):
    return torch.randn(rows, T, d, generator=torch.Generator().manual_seed(seed)).half()


@pytest.fixture(scope="module")
def tiny():
    cfg = config.tiny_unet()
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1).items()}
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    ads = {}
    for n_q in (4, 16):
        ip_sd = ro.synth_resampler_state_dict(cfg, D_EMB, DIM, HEADS, DEPTH, n_q, seed=3 + n_q)
        ads[n_q] = (ip_sd, net.make_ip_adapter(ip_sd, D_EMB, n_q))
    return cfg, sd, net, ads


@pytest.mark.parametrize("n_img", [1, 2])
@pytest.mark.parametrize("n_q", [4, 16])
@pytest.mark.parametrize("T", [17, 50, 257])
def test_resampler_tokens_match_oracle(engine_lib, tiny, T, n_q, n_img):
    cfg, _, _, ads = tiny
    ip_sd, ad = ads[n_q]
    assert ad.kind == "resampler" and ad.resampler["depth"] == DEPTH
    ad.feature_tokens = T
    x = _feat(2 * n_img, T, seed=T + n_q + n_img)
    got = ad.project(x.cuda())
    want = ro.resampler_forward(ip_sd, x.float())
    e = rel_l2(got, want)
    print(f"resampler tokens T{T} nq{n_q} rows{2 * n_img}: rel-L2 {e:.2e}")
    assert got.shape == (2 * n_img, n_q, cfg.cross_attention_dim) and torch.isfinite(got.float()).all()
    assert e < TOK_TOL


def _oracle_forward(monkeypatch, cfg, sd, ip_sd, x, t, ehs, feats, scale):
    monkeypatch.setattr(unet_ref, "attention", ip_attention(ip_sd, scale))
    tok = ro.project_plus(ip_sd, feats.float())
    with torch.no_grad():
        return unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), (ehs.float(), tok))


def _inputs(cfg, B, H, W, n_img, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    return x, ehs, torch.randn(B, n_img, T, D_EMB, generator=g).half()


@pytest.mark.parametrize("B,H,W,t,n_img,T,n_q", [(2, 16, 16, 981.0, 1, 257, 16), (1, 8, 24, 1.0, 2, 50, 16),
                                                 (3, 16, 24, 301.0, 3, 17, 4)])
def test_unet_with_plus_adapter_matches_oracle(engine_lib, monkeypatch, tiny, B, H, W, t, n_img, T, n_q):
    cfg, sd, net, ads = tiny
    ip_sd, ad = ads[n_q]
    ad.feature_tokens = T
    x, ehs, feats = _inputs(cfg, B, H, W, n_img, T, B * 100 + H + n_img)
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.7)
    try:
        ref = _oracle_forward(monkeypatch, cfg, sd, ip_sd, x, t, ehs, feats, 0.7)
        plain = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), ehs.float())
        a = net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs={"image_embeds": [feats.cuda()]})[0]
        b = net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs={"image_embeds": [feats.cuda()]})[0]
        with pytest.raises(ValueError, match=f"{T}, {D_EMB}"):
            net(x.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs={"image_embeds": [feats[:, :, 0].cuda()]})
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    assert rel_l2(a, ref) < TOL
    assert rel_l2(plain, ref) > 5 * TOL          # the image branch really changes the result
    assert torch.equal(a, b)


def _launches(lib, run):
    lib.sd_prof_enable(1)
    try:
        out = run()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return out, {e.kernel.decode(): e.launches for e in ents[: n.value]}


def test_resampler_runs_once_per_loop(engine_lib, tiny):
    """Under the text K/V cache the Resampler runs with the first forward of a (pointer, B, n_img) and not again, until
    sd_unet_text_kv_cache or sd_ip_adapter_set_feature_tokens invalidates the image K / V."""
    cfg, sd, net, ads = tiny
    ip_sd, ad = ads[16]
    ad.feature_tokens = 50
    x, ehs, feats = (t.cuda() for t in _inputs(cfg, 2, 16, 16, 1, 50, 8))
    kw = {"image_embeds": [feats]}
    fwd = lambda: net(x, 501.0, ehs, added_cond_kwargs=kw)[0]  # noqa: E731
    net.attach_ip_adapter(ad)
    try:
        base = fwd()
        net.text_kv_cache(True)
        first, n1 = _launches(engine_lib, fwd)
        second, n2 = _launches(engine_lib, fwd)
        assert n1.get("resampler_attn_kernel") == DEPTH and "resampler_attn_kernel" not in n2
        assert sum(n1.values()) - sum(n2.values()) >= 10 * DEPTH + 4
        assert torch.equal(first, base) and torch.equal(second, base)
        net.text_kv_cache(True)
        third, n3 = _launches(engine_lib, fwd)
        assert n3.get("resampler_attn_kernel") == DEPTH and torch.equal(third, base)
        _, n4 = _launches(engine_lib, fwd)
        assert "resampler_attn_kernel" not in n4
        ad.feature_tokens = 50                      # the setter invalidates whatever the value
        fifth, n5 = _launches(engine_lib, fwd)
        assert n5.get("resampler_attn_kernel") == DEPTH and torch.equal(fifth, base)
    finally:
        net.text_kv_cache(False)
        net.attach_ip_adapter(None)


def test_detach_restores_plain_and_linear_adapter_is_unchanged(engine_lib, monkeypatch, tiny):
    cfg, sd, net, ads = tiny
    ip_sd, ad = ads[16]
    ad.feature_tokens = 17
    fresh = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    x, ehs, feats = (t.cuda() for t in _inputs(cfg, 2, 16, 24, 1, 17, 5))
    never = fresh(x, 401.0, ehs)[0]
    # a base (linear) adapter on a UNet that never saw a Resampler ...
    lin_sd = synth_ip_state_dict(cfg, 128, 4, seed=3)
    img = torch.randn(2, 1, 128, generator=torch.Generator().manual_seed(1)).half().cuda()
    lin_fresh = HipIPAdapter(fresh, 128, 4).load_state_dict(lin_sd)
    fresh.attach_ip_adapter(lin_fresh)
    lin_want = fresh(x, 401.0, ehs, added_cond_kwargs={"image_embeds": [img]})[0]
    fresh.attach_ip_adapter(None)
    net.attach_ip_adapter(ad)
    with_plus = net(x, 401.0, ehs, added_cond_kwargs={"image_embeds": [feats]})[0]
    net.attach_ip_adapter(None)
    after = net(x, 401.0, ehs)[0]
    assert torch.equal(after, never) and not torch.equal(with_plus, never)
    # ... and on the one that did: the same bits, and the oracle's result as before
    lin = net.make_ip_adapter(lin_sd, 128, 4)
    assert lin.kind == "linear"
    net.attach_ip_adapter(lin)
    try:
        lin_got = net(x, 401.0, ehs, added_cond_kwargs={"image_embeds": [img]})[0]
        tok = lin.project(img[:, 0])
    finally:
        net.attach_ip_adapter(None)
    assert torch.equal(lin_got, lin_want)
    assert rel_l2(tok, project(lin_sd, img.float().cpu(), 4)) < 2e-3
    monkeypatch.setattr(unet_ref, "attention", ip_attention(lin_sd, 1.0))
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, sd, x.float().cpu(), torch.tensor(401.0),
                                    (ehs.float().cpu(), project(lin_sd, img.float().cpu(), 4)))
    assert rel_l2(lin_got, ref) < TOL


@pytest.mark.parametrize("preset,dim,heads", [("sd15", 768, 12), ("sdxl", 1280, 20)])
def test_fullsize_resampler_tokens(engine_lib, preset, dim, heads):
    """The published sizes (D_emb 1280, depth 4, 16 queries, 257 feature rows), two images, against the float64 oracle."""
    cfg = config.PRESETS[preset][0]()
    net = HipUNet2DConditionModel(cfg)                     # configuration only: the adapter needs no UNet weights
    ip_sd = ro.synth_resampler_state_dict(cfg, 1280, dim, heads, 4, 16, seed=22)
    ad = net.make_ip_adapter(ip_sd, 1280, 16)
    assert ad.feature_tokens == 257
    x = _feat(2, 257, seed=dim, d=1280)
    got = ad.project(x.cuda())
    want = ro.resampler_forward(ip_sd, x.float())
    e = rel_l2(got, want)
    print(f"{preset} Plus resampler tokens: rel-L2 {e:.2e}")
    assert torch.isfinite(got.float()).all() and e < TOK_TOL


def test_tiny_txt2img_with_image_prompt_matches_oracle_loop(engine_lib, monkeypatch):
    """txt2img with ip_adapter_image= a pixel tensor through load_image_encoder's tower (two layers) and a Plus adapter
    loaded from an original-format dict: against the oracle loop fed hidden_states[-2] of the same tower (of the image,
    and of the zero image for the negative half), on the device-fused step."""
    from oracle import pipeline_ref
    from stablediffusion_amd.models import HipAutoencoderKL, HipCLIPVisionModelWithProjection
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=11, perturb=0.1).items()}
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1).items()}
    ip_sd = ro.synth_resampler_state_dict(ucfg, D_EMB, DIM, HEADS, DEPTH, 16, seed=5)
    orig = {"image_proj": {k[len(ip_adapter.PROJ) + 1:]: v for k, v in ip_sd.items() if k.startswith(ip_adapter.PROJ)},
            "ip_adapter": {}}
    for i, site in ip_adapter.site_ids(ucfg).items():
        for n in ("to_k_ip", "to_v_ip"):
            orig["ip_adapter"][f"{i}.{n}.weight"] = ip_sd[f"{site}.attn2.processor.{n}.0.weight"]
    ecfg = config.CLIPVisionConfig(hidden_size=D_EMB, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                   image_size=56, patch_size=14, hidden_act="quick_gelu", projection_dim=64)
    g = torch.Generator().manual_seed(4)
    esd = {}
    probe = HipCLIPVisionModelWithProjection(ecfg)
    for i in range(engine_lib.sd_clip_vision_num_weights(probe._h)):
        key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert engine_lib.sd_clip_vision_weight_info(probe._h, i, C.byref(key), shape, C.byref(nd)) == 0
        k, shp = key.value.decode(), tuple(shape[j] for j in range(nd.value))
        if "norm" in k and k.endswith("weight"):
            w = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            w = 0.05 * torch.randn(shp, generator=g)
        elif "embedding" in k:
            w = 0.5 * torch.randn(shp, generator=g)
        else:
            w = torch.randn(shp, generator=g) / (shp[-1] if len(shp) == 2 else shp[1] * shp[2] * shp[3]) ** 0.5
        esd[k] = w.half().float()
    del probe
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler("DDIM")
    model.load_ip_adapter(orig)
    model.set_ip_adapter_scale(0.8)
    assert model.base.ip_adapter.kind == "resampler" and model.base.ip_adapter.feature_tokens == 257
    model.load_image_encoder(ecfg, esd)
    assert model.base.ip_adapter.feature_tokens == 17        # (56 / 14)^2 + 1
    B = 2
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    px = torch.randn(1, 3, 56, 56, generator=g).half()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    got = pipe(model, prompt_embeds=pos.cuda(), negative_prompt_embeds=neg.cuda(), latents=lat0.cuda(),
               num_inference_steps=10, guidance_scale=5.0, height=128, width=128, ip_adapter_image=px.cuda())
    assert pipe._fused_step_available(model, lat0.cuda())
    enc = model.image_encoder
    hp = enc(px.cuda(), output_hidden_states=True).hidden_states[-2].float().cpu()
    hn = enc(torch.zeros_like(px).cuda(), output_hidden_states=True).hidden_states[-2].float().cpu()
    assert hp.shape == (1, 17, D_EMB) and not torch.equal(hp, hn)
    feats = torch.cat([hn[None].expand(B, 1, 17, D_EMB), hp[None].expand(B, 1, 17, D_EMB)])
    monkeypatch.setattr(unet_ref, "attention", ip_attention(ip_sd, 0.8))
    tok = ro.project_plus(ip_sd, feats)
    ref = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), (torch.cat([neg, pos]).float(), tok), steps=10,
                                   guidance_scale=5.0, scheduler="DDIM")
    plain = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), torch.cat([neg, pos]).float(), steps=10,
                                     guidance_scale=5.0, scheduler="DDIM")
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got, ref) < TOL
    assert rel_l2(plain, ref) > 5 * TOL
