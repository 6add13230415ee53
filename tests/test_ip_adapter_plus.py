"""IP-Adapter Plus host side (no GPU): conversion of Resampler files, resampler_config, the engine's manifest and its
argument checks, the float64 Resampler oracle against a module-style restatement, and the pipeline on the CPU doubles."""
import ctypes as C

import pytest
import torch

from resampler_oracle import (PlusOracleUNet, project_plus, resampler_forward, resampler_modules,
                              synth_resampler_state_dict)
from stablediffusion_amd import _lib, config, ip_adapter, schedulers, weights
from stablediffusion_amd.models import HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

PROJ = ip_adapter.PROJ
TINY = dict(d_emb=128, dim=128, heads=2, depth=2, n_q=16)


def _original(cfg, nested=True, seed=0, **kw):
    """An original-format IP-Adapter Plus file's dict for `cfg`."""
    sizes = dict(TINY, **kw)
    sd = synth_resampler_state_dict(cfg, seed=seed, **sizes)
    proj = {k[len(PROJ) + 1:]: v for k, v in sd.items() if k.startswith(PROJ)}
    ids = {p: i for i, p in ip_adapter.site_ids(cfg).items()}
    ipw = {}
    for k, v in sd.items():
        if not k.startswith(PROJ):
            site, name = k.split(".attn2.processor.")
            ipw[f"{ids[site]}.{name.split('.')[0]}.weight"] = v
    if nested:
        return {"image_proj": proj, "ip_adapter": ipw}, sd
    return {**{f"image_proj.{k}": v for k, v in proj.items()}, **{f"ip_adapter.{k}": v for k, v in ipw.items()}}, sd


def _engine_manifest(lib, h):
    out = []
    for i in range(lib.sd_ip_adapter_num_weights(h)):
        key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert lib.sd_ip_adapter_weight_info(h, i, C.byref(key), shape, C.byref(nd)) == 0
        out.append((key.value.decode(), tuple(shape[j] for j in range(nd.value))))
    return out


def _pc(**kw):
    base = dict(kind=_lib.SD_IP_PROJ_RESAMPLER, image_embed_dim=128, num_tokens=16, dim=128, heads=2, depth=2, ff_mult=4)
    return _lib.SdIPProjectionConfig(**dict(base, **kw))


@pytest.mark.parametrize("nested", [True, False])
def test_plus_file_converts(nested):
    cfg = config.tiny_unet()
    orig, want = _original(cfg, nested=nested)
    sd, d_emb, n_q = ip_adapter.convert(orig, cfg)
    assert (d_emb, n_q) == (128, 16)
    rc = ip_adapter.resampler_config(sd, cfg)
    assert rc == dict(dim=128, heads=2, depth=2, num_tokens=16, image_embed_dim=128, ff_mult=4)
    assert list(sd) == list(ip_adapter.ip_adapter_manifest(cfg, d_emb, n_q, rc))
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(ip_adapter.ip_adapter_manifest(cfg, d_emb, n_q, rc))
    assert set(sd) == set(want) and all(torch.equal(sd[k], want[k]) for k in sd)
    assert ip_adapter.is_resampler(sd)
    assert f"{PROJ}.layers.1.0.to_kv.weight" in sd and f"{PROJ}.layers.1.1.3.weight" in sd     # suffixes unchanged


@pytest.mark.parametrize("preset,sizes", [("tiny", TINY), ("sd15", dict(d_emb=1280, dim=768, heads=12, depth=4, n_q=16)),
                                          ("sdxl", dict(d_emb=1280, dim=1280, heads=20, depth=4, n_q=16))])
def test_manifest_matches_engine(engine_lib, preset, sizes):
    cfg = config.PRESETS[preset][0]()
    net = HipUNet2DConditionModel(cfg)
    rc = dict(dim=sizes["dim"], heads=sizes["heads"], depth=sizes["depth"], ff_mult=4)
    pc = _pc(image_embed_dim=sizes["d_emb"], num_tokens=sizes["n_q"], **rc)
    h = C.c_void_p()
    _lib.check(engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(pc), C.byref(h)), "create_ex")
    try:
        want = ip_adapter.ip_adapter_manifest(cfg, sizes["d_emb"], sizes["n_q"], rc)
        assert _engine_manifest(engine_lib, h) == list(want.items())
    finally:
        engine_lib.sd_ip_adapter_destroy(h)


def test_projection_config_layout_matches_header():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sd_engine.h")).read()
    body = re.search(r"typedef struct sd_ip_projection_config \{(.*?)\} sd_ip_projection_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.SdIPProjectionConfig._fields_]
    assert all(f[1] is C.c_int32 for f in _lib.SdIPProjectionConfig._fields_)


def test_create_ex_rejections(engine_lib):
    """Argument checks that need no device work."""
    net = HipUNet2DConditionModel(config.tiny_unet())
    h = C.c_void_p()
    for bad in (_pc(heads=4), _pc(dim=192, heads=2), _pc(num_tokens=17), _pc(num_tokens=0), _pc(depth=0), _pc(ff_mult=0),
                _pc(image_embed_dim=100)):
        assert engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(bad), C.byref(h)) == 4
    assert b"dim_head" in (engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(_pc(heads=4)), C.byref(h)),
                           engine_lib.sd_last_error())[1]
    assert engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(_pc(kind=7)), C.byref(h)) == 1
    # the linear kind through _ex is sd_ip_adapter_create: same manifest, Resampler fields ignored
    lin = _lib.SdIPProjectionConfig(kind=_lib.SD_IP_PROJ_LINEAR, image_embed_dim=128, num_tokens=4, dim=5)
    _lib.check(engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(lin), C.byref(h)), "create_ex")
    try:
        assert _engine_manifest(engine_lib, h) == list(ip_adapter.ip_adapter_manifest(config.tiny_unet(), 128, 4).items())
        assert engine_lib.sd_ip_adapter_set_feature_tokens(h, 257) == 4          # a linear adapter has no feature rows
    finally:
        engine_lib.sd_ip_adapter_destroy(h)
    _lib.check(engine_lib.sd_ip_adapter_create_ex(net._h, C.byref(_pc()), C.byref(h)), "create_ex")
    try:
        assert engine_lib.sd_ip_adapter_set_feature_tokens(h, 0) == 1
        assert engine_lib.sd_ip_adapter_set_feature_tokens(h, 305) == 4          # 305 + 16 = 321 keys
        assert b"320" in engine_lib.sd_last_error()
        assert engine_lib.sd_ip_adapter_set_feature_tokens(h, 304) == 0
        assert engine_lib.sd_ip_adapter_set_feature_tokens(h, 257) == 0
    finally:
        engine_lib.sd_ip_adapter_destroy(h)


def _drop(orig, pred):
    orig["image_proj"] = {k: v for k, v in orig["image_proj"].items() if not pred(k)}
    return orig


def test_malformed_resampler_files_are_rejected():
    cfg = config.tiny_unet()
    cases = {}
    cases["missing key"] = _drop(_original(cfg)[0], lambda k: k == "layers.1.0.norm2.bias")
    cases["depth gap"] = _drop(_original(cfg, depth=3)[0], lambda k: k.startswith("layers.1."))
    o = _original(cfg)[0]
    o["image_proj"]["layers.0.0.to_kv.weight"] = torch.zeros(128, 128)
    cases["to_kv is not twice to_q"] = o
    o = _original(cfg)[0]
    for i in range(2):
        o["image_proj"][f"layers.{i}.0.to_q.weight"] = torch.zeros(96, 128)
        o["image_proj"][f"layers.{i}.0.to_kv.weight"] = torch.zeros(192, 128)
        o["image_proj"][f"layers.{i}.0.to_out.weight"] = torch.zeros(128, 96)
    cases["to_q rows 96"] = o
    o = _original(cfg)[0]
    o["image_proj"]["norm_out.weight"] = torch.ones(128)
    cases["ctx"] = o
    for name, orig in cases.items():
        with pytest.raises(ValueError, match="Resampler"):
            ip_adapter.convert(orig, cfg)


def test_faceid_file_is_rejected():
    cfg = config.tiny_unet()
    orig = _original(cfg)[0]
    orig["image_proj"] = {"proj.0.weight": torch.randn(128, 512), "proj.0.bias": torch.randn(128),
                          "proj.2.weight": torch.randn(4 * 64, 128), "proj.2.bias": torch.randn(4 * 64),
                          "norm.weight": torch.ones(64), "norm.bias": torch.zeros(64)}
    with pytest.raises(ValueError, match="FaceID"):
        ip_adapter.convert(orig, cfg)
    orig["image_proj"] = {"perceiver_resampler.latents": torch.randn(1, 4, 64), "proj.0.weight": torch.randn(128, 512)}
    with pytest.raises(ValueError, match="FaceID"):
        ip_adapter.convert(orig, cfg)


@pytest.mark.parametrize("T,n_q,R", [(17, 4, 2), (50, 16, 1), (257, 16, 2)])
def test_oracle_agrees_with_module_restatement(T, n_q, R):
    cfg = config.tiny_unet()
    sd = synth_resampler_state_dict(cfg, seed=3, **dict(TINY, n_q=n_q))
    x = torch.randn(R, T, 128, generator=torch.Generator().manual_seed(T)).half().float()
    a = resampler_forward(sd, x)
    b = resampler_modules(sd, x).double()
    assert a.shape == (R, n_q, cfg.cross_attention_dim)
    rel = float((a - b).norm() / a.norm())
    assert rel < 1e-5, rel
    other = torch.randn(R, T, 128, generator=torch.Generator().manual_seed(T + 1000)).half().float()
    assert float((resampler_forward(sd, other) - a).norm() / a.norm()) > 1e-2      # the tokens depend on the features


# ---------------------------------------------------------------------------------------------- pipeline surface
def _model(image_encoder=None, feature_extractor=None):
    from doubles import OracleVAE
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    return SDModelWrapper(base=PlusOracleUNet(ucfg, uw), vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(),
                          device="cpu", unet_state_dict=uw, image_encoder=image_encoder,
                          feature_extractor=feature_extractor)


def _inputs(total, n_img=1, T=17, d_emb=128, seed=9):
    g = torch.Generator().manual_seed(seed)
    ctx = config.tiny_unet().cross_attention_dim
    return (torch.randn(total, 4, 8, 8, generator=g), torch.randn(total, 77, ctx, generator=g),
            torch.randn(total, 77, ctx, generator=g), torch.randn(2 * total, n_img, T, d_emb, generator=g))


def test_load_plus_adapter_changes_the_result_and_needs_4d_embeds():
    cfg = config.tiny_unet()
    lat, pe, ne, ie = _inputs(2, n_img=2)
    m = _model()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64)
    plain = pipe(m, **kw)
    assert not m.ip_adapter_is_plus
    m.load_ip_adapter(_original(cfg, seed=1)[0])
    assert m.ip_adapter_is_plus and m.base.ip_adapter["n_tok"] == 16 and m.base.ip_adapter["d_img"] == 128
    with_ip = pipe(m, ip_adapter_image_embeds=[ie], **kw)
    assert not torch.allclose(with_ip, plain, atol=1e-4)
    emb = type(m.base).calls[-1]["added_cond_kwargs"]["image_embeds"]
    assert len(emb) == 1 and torch.equal(emb[0], ie)
    one = ie[[0, 2]]                                           # one row per half: repeated to the batch
    got = pipe.prepare_ip_adapter_image_embeds(None, [one], torch.device("cpu"), 2, True)[0]
    assert torch.equal(got, torch.cat([one[:1].repeat(2, 1, 1, 1), one[1:].repeat(2, 1, 1, 1)]))
    with pytest.raises(ValueError, match="T_feat"):
        pipe(m, ip_adapter_image_embeds=[ie[:, :, 0]], **kw)
    m.unload_ip_adapter()
    assert not m.ip_adapter_is_plus
    assert torch.equal(pipe(m, **kw), plain)


def test_image_prompt_uses_penultimate_hidden_states_and_a_zero_image_negative():
    """diffusers' encode_image for projection layers other than ImageProjection, restated."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(0)
    enc = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                                         num_attention_heads=2, image_size=32, patch_size=8,
                                                         projection_dim=64)).eval()
    cfg = config.tiny_unet()
    m = _model(image_encoder=enc)
    m.load_ip_adapter(_original(cfg, seed=1)[0])
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    pipe.model = m
    px = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        got = pipe.prepare_ip_adapter_image_embeds(px, None, torch.device("cpu"), 3, True)
        pos = enc(px, output_hidden_states=True).hidden_states[-2]
        neg = enc(torch.zeros_like(px), output_hidden_states=True).hidden_states[-2]
    assert len(got) == 1 and got[0].shape == (6, 1, 17, 128)
    assert torch.allclose(got[0], torch.cat([neg[None].expand(3, 1, 17, 128), pos[None].expand(3, 1, 17, 128)]), atol=1e-6)
    assert float(neg.abs().max()) > 0                          # the zero image's features, not zeros
    lat, pe, ne, _ = _inputs(1)
    with torch.no_grad():
        out = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64,
                   ip_adapter_image=px)
        want = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64,
                    width=64, ip_adapter_image_embeds=[torch.cat([neg[None], pos[None]])])
    assert torch.equal(out, want)
    tok = project_plus(m._ip[0], got[0])
    assert tok.shape == (6, 16, cfg.cross_attention_dim) and not torch.allclose(tok[0], tok[3], atol=1e-3)


def test_kernel_arithmetic_emulation_stays_inside_the_elementwise_bound():
    """The bound the GPU test applies to sd_op_resampler_attention holds for a torch emulation of the kernel's stated
    arithmetic on every operator case (prints the worst |err| / bound)."""
    import resampler_oracle as ro
    worst = 0.0
    for T in ro.OP_T_FEAT:
        for n_q in ro.OP_N_Q:
            for heads, B in ro.OP_HEADS_B:
                ops = ro.op_inputs(B, n_q, T, heads, seed=T * 100 + n_q)
                O, A = ro.op_reference(*ops, heads)
                err = (ro.op_emulate(*ops, heads).double() - O).abs()
                bound = ro.op_bound(O, A, T + n_q, torch.maximum(ops[2].abs().max(), ops[4].abs().max()).double())
                worst = max(worst, float((err / bound).max()))
    print("resampler attention emulation: worst |err| / bound %.3f" % worst)
    assert worst <= 1.0
