"""CLIP vision encoder on the HIP engine: the patch-embedding operator element by element against float64, the whole
tower against transformers' CLIPVisionModelWithProjection run in fp32 on the CPU from the same fp16-rounded weights
(relative L2 < 5e-3 per tensor, the figure tests/test_clip_gpu.py holds this layer stack to), and `ip_adapter_image=`
end to end through the pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2
from stablediffusion_amd import config
from stablediffusion_amd.image_processor import ClipImageProcessor
from stablediffusion_amd.models import HipCLIPVisionModelWithProjection

transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

TOL = 5e-3
SENTINEL = -1234.0


# ------------------------------------------------------------------------------------ sd_op_vit_patch_embed
def _embed_ref(px, w, cls, pos, P):
    """float64: conv(stride P) -> [B, N, H], class row in front, + position embedding."""
    px, w, cls, pos = px.double(), w.double(), cls.double(), pos.double()
    B, _, S, _ = px.shape
    G = S // P
    patches = px.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * P * P)
    y = patches @ w.reshape(w.shape[0], -1).t()
    y = torch.cat([cls.expand(B, 1, -1), y], dim=1)
    return y + pos[None]


def _run_embed(lib, px, w, cls, pos, P, ld, lead=64, tail=64):
    """The operator into the middle of a sentinel-filled buffer with row stride ld; returns (output, whole buffer)."""
    B, _, S, _ = px.shape
    H = w.shape[0]
    T = 1 + (S // P) ** 2
    buf = torch.full((lead + B * T * ld + tail,), SENTINEL, dtype=torch.float16, device="cuda")
    out = buf[lead:lead + B * T * ld]
    d = [t.cuda().half().contiguous() for t in (px, w, cls, pos)]
    rc = lib.sd_op_vit_patch_embed(C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()),
                                   C.c_void_p(d[3].data_ptr()), C.c_void_p(out.data_ptr()), ld, B, S, P, H,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    rows = out.reshape(B * T, ld).cpu()
    return rows[:, :H].reshape(B, T, H), rows, buf.cpu(), lead


EMBED_SHAPES = [(14, 42, 72), (14, 112, 136), (16, 48, 64)]          # (P, S, H): K = 588, 588 (65 tokens, ragged tiles), 768


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P,S,H", EMBED_SHAPES)
def test_patch_embed_exact(engine_lib, P, S, H, B):
    """Integer operands small enough that every partial sum is an integer below 2048: the fp16 output equals the float64
    reference bit for bit, and nothing outside the [B, T, H] window of the padded buffer is written."""
    g = torch.Generator().manual_seed(P * 1000 + S + B)
    T = 1 + (S // P) ** 2
    px = torch.randint(-2, 3, (B, 3, S, S), generator=g).float()
    w = torch.randint(-1, 2, (H, 3, P, P), generator=g).float()
    cls = torch.randint(-8, 9, (H,), generator=g).float()
    pos = torch.randint(-8, 9, (T, H), generator=g).float()
    ref = _embed_ref(px, w, cls, pos, P)
    assert ref.abs().max() < 2048 and (2 * 3 * P * P + 16) < 2048        # every partial sum is exact in fp16 / fp32
    ld = H + 24
    got, rows, buf, lead = _run_embed(engine_lib, px, w, cls, pos, P, ld)
    assert torch.equal(got.double(), ref)
    assert (rows[:, H:] == SENTINEL).all()                               # the row padding
    assert (buf[:lead] == SENTINEL).all() and (buf[lead + B * T * ld:] == SENTINEL).all()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P,S,H", EMBED_SHAPES)
def test_patch_embed_random(engine_lib, P, S, H, B):
    """Random fp16 operands, element by element against float64:
    |err| <= 2^-10 |y| + K 2^-23 max|x| max|w| + 2^-24 (the fp16 store, the fp32 accumulation of K terms)."""
    g = torch.Generator().manual_seed(P * 77 + S + B)
    T = 1 + (S // P) ** 2
    K = 3 * P * P
    px = (2.0 * torch.randn(B, 3, S, S, generator=g)).half().float()
    w = (0.05 * torch.randn(H, 3, P, P, generator=g)).half().float()
    cls = torch.randn(H, generator=g).half().float()
    pos = (0.5 * torch.randn(T, H, generator=g)).half().float()
    ref = _embed_ref(px, w, cls, pos, P)
    got, rows, _, _ = _run_embed(engine_lib, px, w, cls, pos, P, H + 8)
    err = (got.double() - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + K * 2.0 ** -23 * px.abs().max().item() * w.abs().max().item() + 2.0 ** -24
    worst = (err / bound).max().item()
    print(f"patch_embed P={P} S={S} H={H} B={B}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all()
    assert (rows[:, H:] == SENTINEL).all()


def test_patch_embed_rejects_bad_arguments(engine_lib):
    t = torch.zeros(4096, dtype=torch.float16, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert engine_lib.sd_op_vit_patch_embed(p, p, p, p, p, 64, 1, 43, 14, 64, None) != 0      # S % P
    assert engine_lib.sd_op_vit_patch_embed(p, p, p, p, p, 60, 1, 28, 14, 64, None) != 0      # ld < H
    assert engine_lib.sd_op_vit_patch_embed(p, p, p, p, p, 68, 1, 28, 14, 64, None) != 0      # ld % 8
    assert engine_lib.sd_op_vit_patch_embed(p, p, p, p, None, 64, 1, 28, 14, 64, None) != 0


# ---------------------------------------------------------------------------------------- model vs transformers
def _hf(cfg: config.CLIPVisionConfig, seed: int):
    torch.manual_seed(seed)
    hf_cfg = transformers.CLIPVisionConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, image_size=cfg.image_size, patch_size=cfg.patch_size,
        hidden_act=cfg.hidden_act, projection_dim=cfg.projection_dim, layer_norm_eps=cfg.layer_norm_eps)
    m = transformers.CLIPVisionModelWithProjection(hf_cfg).eval()
    sd = {k: v.half().float() for k, v in m.state_dict().items()}       # both sides see fp16-representable weights
    # random-init norms are (1, 0) and biases 0: perturb them so every affine path is exercised
    g = torch.Generator().manual_seed(seed + 100)
    for k in sd:
        if "norm" in k:
            sd[k] = (sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)).half().float()
        elif k.endswith(".bias"):
            sd[k] = (0.05 * torch.randn(sd[k].shape, generator=g)).half().float()
    m.load_state_dict(sd)
    return m, sd


def _pixels(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    # normalised pixels span about [-1.8, 2.2]
    return (torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g) * 4.0 - 1.8).half()


def _check(cfg, B, seed, tag):
    hf, sd = _hf(cfg, seed)
    eng = HipCLIPVisionModelWithProjection.from_state_dict(cfg, sd)
    px = _pixels(cfg, B, seed)
    with torch.no_grad():
        ref = hf(px.float(), output_hidden_states=True)
        # CLIPVisionModelOutput carries no pooler_output: the tower's own output does
        ref_pooled = hf.vision_model(pixel_values=px.float()).pooler_output
    del hf
    out = eng(px.cuda(), output_hidden_states=True)
    L = cfg.num_hidden_layers
    assert len(out.hidden_states) == L + 1 == len(ref.hidden_states)
    errs = [rel_l2(a, b) for a, b in zip(out.hidden_states, ref.hidden_states)]
    e_last = rel_l2(out.last_hidden_state, ref.last_hidden_state)
    e_pool = rel_l2(out.pooler_output, ref_pooled)
    e_emb = rel_l2(out.image_embeds, ref.image_embeds)
    print(f"{tag}: hidden_states rel-L2 first {errs[0]:.2e} max {max(errs):.2e} last {errs[-1]:.2e}; "
          f"last_hidden {e_last:.2e} pooler {e_pool:.2e} image_embeds {e_emb:.2e}")
    for i, e in enumerate(errs):
        assert e < TOL, f"hidden_states[{i}]: {e}"
    assert e_last < TOL and e_pool < TOL and e_emb < TOL
    assert torch.equal(out.last_hidden_state, out.hidden_states[-1])      # no final norm on last_hidden_state
    assert out[0] is out.image_embeds and tuple(out.image_embeds.shape) == (B, cfg.projection_dim)
    # without the hidden states: the same image_embeds bit for bit (ping-pong residual buffers)
    out2 = eng(px.cuda())
    assert out2.hidden_states is None
    assert torch.equal(out2.image_embeds, out.image_embeds)
    assert torch.equal(out2.last_hidden_state, out.last_hidden_state)
    assert torch.equal(out2.pooler_output, out.pooler_output)
    return eng


def test_tower_d64_quick_gelu(engine_lib):
    """(a) H 128, 2 heads (d 64), 3 layers, quick_gelu, 56 / 14 (17 tokens)."""
    cfg = config.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                                  image_size=56, patch_size=14, hidden_act="quick_gelu", projection_dim=128)
    _check(cfg, B=2, seed=0, tag="a d64")


def test_tower_d80_gelu_65_tokens(engine_lib):
    """(b) H 160, 2 heads (d 80), gelu, 112 / 14: 65 tokens, one past the 64-key tile, ragged M; H is no multiple of 64."""
    cfg = config.CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2,
                                  image_size=112, patch_size=14, hidden_act="gelu", projection_dim=96)
    _check(cfg, B=3, seed=1, tag="b d80")


def test_tower_d104_padded_heads(engine_lib):
    """(c) H 208, 2 heads (d 104 -> padded to 128, pre-scaled queries), 42 / 14."""
    cfg = config.CLIPVisionConfig(hidden_size=208, intermediate_size=416, num_hidden_layers=2, num_attention_heads=2,
                                  image_size=42, patch_size=14, hidden_act="gelu", projection_dim=64)
    _check(cfg, B=2, seed=2, tag="c d104")


def test_tower_vit_h14_width(engine_lib):
    """(d) ViT-H/14 at its width, 2 layers: the real GEMM shapes, M = 514."""
    import dataclasses
    cfg = dataclasses.replace(config.clip_vit_h14(), num_hidden_layers=2)
    _check(cfg, B=2, seed=3, tag="d ViT-H/14 x2")


def test_tower_vit_bigg14_width(engine_lib):
    """ViT-bigG/14 at its width (1664, 16 heads of 104 padded to 128), 2 layers."""
    import dataclasses
    cfg = dataclasses.replace(config.clip_vit_bigg14(), num_hidden_layers=2)
    _check(cfg, B=2, seed=4, tag="ViT-bigG/14 x2")


def test_tower_vit_h14_full_depth(engine_lib):
    """ViT-H/14 at full depth, B = 2: error growth over 32 layers (the time is the host reference's)."""
    _check(config.clip_vit_h14(), B=2, seed=5, tag="ViT-H/14 x32")


# ------------------------------------------------------------------------------------------------- end to end
D_IMG, N_TOK = 128, 4


@pytest.fixture(scope="module")
def wrapper():
    from ip_oracle import synth_ip_state_dict
    from stablediffusion_amd import ip_adapter, weights
    from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
    from stablediffusion_amd.pipeline import SDModelWrapper
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), seed=11, perturb=0.1).items()}
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1).items()}
    ip_sd = synth_ip_state_dict(ucfg, D_IMG, N_TOK, seed=5)
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
    ecfg = config.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                                   image_size=56, patch_size=14, hidden_act="quick_gelu", projection_dim=D_IMG)
    hf, esd = _hf(ecfg, seed=0)
    return model, ucfg, ecfg, hf, esd


def _image(seed=9, wh=(90, 70)):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, size=(wh[1], wh[0], 3), dtype=np.uint8))


def test_pipeline_ip_adapter_image_runs_on_the_engine(engine_lib, wrapper):
    """pipeline(ip_adapter_image=<PIL image>) with load_image_encoder's tower gives latents bit-identical to the same
    call with ip_adapter_image_embeds built from the shim's own image_embeds; no torch module sits in either slot."""
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    model, ucfg, ecfg, _, esd = wrapper
    model.load_image_encoder(ecfg, esd)
    assert isinstance(model.image_encoder, HipCLIPVisionModelWithProjection)
    assert isinstance(model.feature_extractor, ClipImageProcessor) and model.feature_extractor.size == 56
    assert not isinstance(model.image_encoder, torch.nn.Module)
    img = _image()
    g = torch.Generator().manual_seed(4)
    B = 2
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half().cuda()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_inference_steps=4, guidance_scale=5.0, height=128,
              width=128)
    got = pipe(model, latents=lat0.clone(), ip_adapter_image=img, **kw)
    emb = model.image_encoder(model.feature_extractor(img, return_tensors="pt").pixel_values).image_embeds
    assert tuple(emb.shape) == (1, D_IMG)
    e = torch.cat([torch.zeros(B, 1, D_IMG, dtype=emb.dtype, device=emb.device), emb.expand(B, D_IMG)[:, None]])
    want = pipe(model, latents=lat0.clone(), ip_adapter_image_embeds=[e], **kw)
    plain_model_scale = model._ip_scale
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    # the image matters: another picture moves the latents
    other = pipe(model, latents=lat0.clone(), ip_adapter_image=_image(seed=10), **kw)
    assert not torch.equal(other, got)
    assert model._ip_scale == plain_model_scale
    model.unload_image_encoder()
    assert model.image_encoder is None and model.feature_extractor is None


def test_encode_image_with_a_torch_encoder_is_unchanged(engine_lib, wrapper):
    """A torch CLIPVisionModelWithProjection in the slot goes the way it always did: encode_image returns its
    image_embeds (host fp32 here), repeated per prompt image, and zeros for the negative -- and the engine's tower in
    the same slot agrees with it to the model tolerance."""
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    model, _, ecfg, hf, esd = wrapper
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    pipe.model = model
    img = _image()
    proc = ClipImageProcessor(size=ecfg.image_size)
    model.image_encoder, model.feature_extractor = hf, proc
    try:
        with torch.no_grad():
            pos, neg = pipe.encode_image(img, torch.device("cuda"), 2)
            want = hf(proc(img, return_tensors="pt").pixel_values).image_embeds.repeat_interleave(2, dim=0)
        assert pos.device.type == "cuda" and pos.dtype == torch.float32 and tuple(pos.shape) == (2, D_IMG)
        assert torch.equal(pos.cpu(), want) and torch.equal(neg, torch.zeros_like(pos))
        model.load_image_encoder(ecfg, esd)
        pos2, neg2 = pipe.encode_image(img, torch.device("cuda"), 2)
        assert pos2.dtype == torch.float16 and tuple(pos2.shape) == (2, D_IMG) and not neg2.any()
        e = rel_l2(pos2, want)
        print(f"encode_image engine vs torch encoder: rel-L2 {e:.2e}")
        assert e < TOL
    finally:
        model.unload_image_encoder()
