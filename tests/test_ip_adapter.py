"""IP-Adapter host side (no GPU): original-file key conversion, the id -> site order of diffusers 0.27.2, shape checks,
rejection of Resampler files, and the engine's adapter manifest."""
import ctypes as C

import numpy as np

import pytest
import torch

from ip_oracle import synth_ip_state_dict
from stablediffusion_amd import _lib, config, ip_adapter
from stablediffusion_amd.models import HipUNet2DConditionModel


def _original(cfg, d_img=64, n_tok=4, nested=True, sites=None):
    """An original-format file's dict for `cfg` (sites in diffusers' order unless given)."""
    ctx = cfg.cross_attention_dim
    proj = {"proj.weight": torch.randn(n_tok * ctx, d_img), "proj.bias": torch.randn(n_tok * ctx),
            "norm.weight": torch.ones(ctx), "norm.bias": torch.zeros(ctx)}
    ipw = {}
    for i, (_, c) in enumerate(sites if sites is not None else ip_adapter.xattn_sites(cfg)):
        ipw[f"{2 * i + 1}.to_k_ip.weight"] = torch.randn(c, ctx)
        ipw[f"{2 * i + 1}.to_v_ip.weight"] = torch.randn(c, ctx)
    if nested:
        return {"image_proj": proj, "ip_adapter": ipw}
    return {**{f"image_proj.{k}": v for k, v in proj.items()}, **{f"ip_adapter.{k}": v for k, v in ipw.items()}}


def test_site_ids_sd15():
    ids = ip_adapter.site_ids(config.sd15_unet())
    assert len(ids) == 16 and list(ids) == list(range(1, 32, 2))
    assert ids[1] == "down_blocks.0.attentions.0.transformer_blocks.0"
    assert ids[11] == "down_blocks.2.attentions.1.transformer_blocks.0"
    assert ids[13] == "up_blocks.1.attentions.0.transformer_blocks.0"
    assert ids[29] == "up_blocks.3.attentions.2.transformer_blocks.0"
    assert ids[31] == "mid_block.attentions.0.transformer_blocks.0"


def test_site_ids_sdxl():
    ids = ip_adapter.site_ids(config.sdxl_unet())
    assert len(ids) == 70 and max(ids) == 139
    assert ids[1] == "down_blocks.1.attentions.0.transformer_blocks.0"
    assert ids[49] == "up_blocks.0.attentions.0.transformer_blocks.0"
    assert [ids[i] for i in range(121, 140, 2)] == [f"mid_block.attentions.0.transformer_blocks.{k}" for k in range(10)]


def test_site_ids_tiny():
    cfg = config.tiny_unet()
    ids = ip_adapter.site_ids(cfg)
    assert len(ids) == 16 and ids[31].startswith("mid_block")
    assert [c for _, c in ip_adapter.xattn_sites(cfg)][:6] == [64, 64, 128, 128, 256, 256]


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("preset", ["sd15", "tiny"])
def test_convert(preset, nested):
    cfg = config.PRESETS[preset][0]()
    orig = _original(cfg, d_img=1024 if preset == "sd15" else 64, nested=nested)
    sd, d_img, n_tok = ip_adapter.convert(orig, cfg)
    assert (d_img, n_tok) == ((1024 if preset == "sd15" else 64), 4)
    assert list(sd) == list(ip_adapter.ip_adapter_manifest(cfg, d_img, n_tok))
    flat = orig if not nested else {f"{a}.{k}": v for a, d in orig.items() for k, v in d.items()}
    assert torch.equal(sd["up_blocks.1.attentions.0.transformer_blocks.0.attn2.processor.to_k_ip.0.weight"],
                       flat["ip_adapter.13.to_k_ip.weight"])
    assert torch.equal(sd[f"{ip_adapter.PROJ}.image_embeds.weight"], flat["image_proj.proj.weight"])


def test_convert_from_files(tmp_path):
    cfg = config.tiny_unet()
    orig = _original(cfg)
    torch.save(orig, tmp_path / "ip-adapter.bin")
    from safetensors.torch import save_file
    save_file(_original(cfg, nested=False), str(tmp_path / "ip-adapter.safetensors"))
    for f in ("ip-adapter.bin", "ip-adapter.safetensors"):
        sd, d_img, n_tok = ip_adapter.convert(str(tmp_path / f), cfg)
        assert len(sd) == 4 + 2 * 16 and (d_img, n_tok) == (64, 4)
    with pytest.raises(FileNotFoundError):
        ip_adapter.convert("h94/IP-Adapter", cfg)


def test_down_mid_up_order_fails_on_shape():
    cfg = config.sd15_unet()
    sites = ip_adapter.xattn_sites(cfg)
    permuted = sites[:6] + sites[-1:] + sites[6:-1]          # down, mid, up: id 19 gets a 640-wide site, 1280 expected
    with pytest.raises(ValueError, match="expected"):
        ip_adapter.convert(_original(cfg, d_img=1024, sites=permuted), cfg)


def test_missing_key_and_wrong_ctx():
    cfg = config.tiny_unet()
    orig = _original(cfg)
    del orig["ip_adapter"]["31.to_v_ip.weight"]
    with pytest.raises(KeyError, match="missing"):
        ip_adapter.convert(orig, cfg)
    bad = _original(config.tiny_unet())
    bad["image_proj"]["norm.weight"] = torch.ones(128)
    with pytest.raises(ValueError, match="cross_attention_dim"):
        ip_adapter.convert(bad, cfg)
    extra = _original(cfg)
    extra["ip_adapter"]["33.to_k_ip.weight"] = torch.randn(64, 64)
    with pytest.raises(KeyError):
        ip_adapter.convert(extra, cfg)


def test_resampler_file_is_rejected():
    cfg = config.tiny_unet()
    orig = _original(cfg)
    orig["image_proj"] = {"latents": torch.randn(1, 16, 64), "proj_in.weight": torch.randn(64, 64),
                          "proj_out.weight": torch.randn(64, 64), "norm_out.weight": torch.ones(64)}
    with pytest.raises(ValueError, match="Resampler"):
        ip_adapter.convert(orig, cfg)


def _engine_manifest(lib, h):
    out = []
    for i in range(lib.sd_ip_adapter_num_weights(h)):
        key, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert lib.sd_ip_adapter_weight_info(h, i, C.byref(key), shape, C.byref(nd)) == 0
        out.append((key.value.decode(), tuple(shape[j] for j in range(nd.value))))
    return out


@pytest.mark.parametrize("preset,d_img", [("sd15", 1024), ("sdxl", 1280), ("tiny", 128)])
def test_manifest_matches_engine(engine_lib, preset, d_img):
    cfg = config.PRESETS[preset][0]()
    net = HipUNet2DConditionModel(cfg)
    h = C.c_void_p()
    _lib.check(engine_lib.sd_ip_adapter_create(net._h, d_img, 4, C.byref(h)), "create")
    try:
        assert _engine_manifest(engine_lib, h) == list(ip_adapter.ip_adapter_manifest(cfg, d_img, 4).items())
    finally:
        engine_lib.sd_ip_adapter_destroy(h)
    for d, n in [(d_img, 0), (d_img, 17), (d_img + 8, 4)]:
        assert engine_lib.sd_ip_adapter_create(net._h, d, n, C.byref(h)) == 4


def test_synth_state_dict_round_trips():
    cfg = config.tiny_unet()
    sd = synth_ip_state_dict(cfg, 128, 4)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(ip_adapter.ip_adapter_manifest(cfg, 128, 4))


# ---------------------------------------------------------------------------------------------- pipeline surface
import os  # noqa: E402
import socket  # noqa: E402

import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from ip_oracle import IPOracleUNet  # noqa: E402
from stablediffusion_amd import distributed as sdd, schedulers, weights  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402


def _model(ip=True, image_encoder=None, feature_extractor=None):
    from doubles import OracleUNet, OracleVAE
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    base = IPOracleUNet(ucfg, uw) if ip else OracleUNet(ucfg, uw)
    return SDModelWrapper(base=base, vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(), device="cpu",
                          unet_state_dict=uw, image_encoder=image_encoder, feature_extractor=feature_extractor)


def _ip_file(cfg, d_img=64, seed=1):
    g = torch.manual_seed(seed)                          # (_original draws from the global generator)
    orig = _original(cfg, d_img=d_img)
    for part in orig.values():
        for k in part:
            part[k] = part[k] * (0.1 if k.endswith("bias") else 0.2) if not k.startswith("norm") else part[k]
    return orig, g


def _embeds(total, n_img=1, d_img=64, seed=9):
    g = torch.Generator().manual_seed(seed)
    ucfg = config.tiny_unet()
    return (torch.randn(total, 4, 8, 8, generator=g), torch.randn(total, 77, ucfg.cross_attention_dim, generator=g),
            torch.randn(total, 77, ucfg.cross_attention_dim, generator=g), torch.randn(2 * total, n_img, d_img, generator=g))


def _tiny_clip_vision():
    from transformers import CLIPImageProcessor, CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(0)
    enc = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                                         num_attention_heads=2, image_size=32, patch_size=8,
                                                         projection_dim=64)).eval()
    proc = CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    return enc, proc


def test_prepare_ip_adapter_image_embeds_from_an_image():
    """Restated diffusers 0.27.2: image_encoder(feature_extractor(img).pixel_values).image_embeds, a zero negative,
    repeated per image of the batch, [negative, positive] under CFG."""
    from PIL import Image
    enc, proc = _tiny_clip_vision()
    m = _model(image_encoder=enc, feature_extractor=proc)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    pipe.model = m
    img = Image.fromarray((np.random.default_rng(0).random((40, 48, 3)) * 255).astype("uint8"))
    got = pipe.prepare_ip_adapter_image_embeds(img, None, torch.device("cpu"), 3, True)
    with torch.no_grad():
        pos = enc(proc(img, return_tensors="pt").pixel_values).image_embeds            # [1, 64]
    want = torch.cat([torch.zeros(3, 1, 64), pos[None].expand(3, 1, 64)])
    assert len(got) == 1 and got[0].shape == (6, 1, 64)
    assert torch.allclose(got[0], want, atol=1e-6)
    no_cfg = StableDiffusionUnifiedPipeline(do_cfg=False, device="cpu")
    no_cfg.model = m
    assert torch.allclose(no_cfg.prepare_ip_adapter_image_embeds([img], None, torch.device("cpu"), 2, False)[0],
                          pos[None].expand(2, 1, 64), atol=1e-6)


def test_precomputed_image_embeds_pass_through():
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    e = torch.randn(6, 2, 64)
    assert pipe.prepare_ip_adapter_image_embeds(None, [e], torch.device("cpu"), 3, True)[0] is e or \
        torch.equal(pipe.prepare_ip_adapter_image_embeds(None, [e], torch.device("cpu"), 3, True)[0], e)
    one = torch.randn(2, 1, 64)                                # one row per half: repeated to the batch
    got = pipe.prepare_ip_adapter_image_embeds(None, [one], torch.device("cpu"), 3, True)[0]
    assert torch.equal(got, torch.cat([one[:1].repeat(3, 1, 1), one[1:].repeat(3, 1, 1)]))


def test_without_ip_kwargs_the_unet_call_is_unchanged():
    lat, pe, ne, _ = _embeds(2)
    from doubles import OracleUNet
    m_plain = _model(ip=False)
    m = _model()
    type(m.base).calls = []
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    a = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64)
    b = pipe(m_plain, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64,
             width=64)
    assert isinstance(m_plain.base, OracleUNet)
    assert all(c["added_cond_kwargs"] is None for c in type(m.base).calls) and len(type(m.base).calls) == 2
    assert torch.equal(a, b)


def test_load_ip_adapter_changes_the_result_and_unloads():
    cfg = config.tiny_unet()
    lat, pe, ne, ie = _embeds(2)
    m = _model()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64)
    plain = pipe(m, **kw)
    m.load_ip_adapter(_ip_file(cfg)[0])
    m.set_ip_adapter_scale(0.5)
    assert m.base.ip_adapter is not None and m.base.ip_scale == 0.5
    with_ip = pipe(m, ip_adapter_image_embeds=[ie], **kw)
    assert not torch.allclose(with_ip, plain, atol=1e-4)
    emb = type(m.base).calls[-1]["added_cond_kwargs"]["image_embeds"]
    assert len(emb) == 1 and torch.equal(emb[0], ie)           # [neg | pos] of the batch: passed unchanged
    m.unload_ip_adapter()
    assert m.base.ip_adapter is None
    assert torch.equal(pipe(m, **kw), plain)


def test_lora_refuse_keeps_the_ip_adapter():
    cfg = config.tiny_unet()
    m = _model()
    m.load_ip_adapter(_ip_file(cfg)[0])
    m.set_ip_adapter_scale(0.7)
    old = m.base
    g = torch.Generator().manual_seed(1)
    key = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    w = m._unet_sd[key + ".weight"]
    m.load_lora_weights({f"unet.{key}.lora.down.weight": torch.randn(4, w.shape[1], generator=g) * 0.05,
                         f"unet.{key}.lora.up.weight": torch.randn(w.shape[0], 4, generator=g) * 0.05}, "style")
    m.apply_adapters()
    assert m.base is not old
    assert m.base.ip_adapter is not None and m.base.ip_scale == 0.7
    assert m.base.ip_adapter["sd"] is m._ip[0]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, total, out_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    sdd.init("gloo")
    lat, pe, ne, ie = _embeds(total)
    if rank != 0:
        pe.zero_(); ne.zero_(); ie.zero_()           # must arrive through the broadcast
    m = _model()
    m.load_ip_adapter(_ip_file(config.tiny_unet())[0])
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    imgs = sdd.sharded_txt2img(pipe, m, lat, pe, ne, rank, world, num_inference_steps=2, height=64, width=64,
                               ip_adapter_image_embeds=[ie])
    if rank == 0:
        torch.save(imgs, out_path)
    sdd.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("total", [3])
def test_sharded_txt2img_with_ip_embeds_equals_unsharded(tmp_path, total):
    out = str(tmp_path / "imgs.pt")
    mp.spawn(_worker, args=(2, _free_port(), total, out), nprocs=2, join=True)
    sharded = torch.load(out, weights_only=True)
    torch.set_num_threads(2)
    lat, pe, ne, ie = _embeds(total)
    m = _model()
    m.load_ip_adapter(_ip_file(config.tiny_unet())[0])
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    full = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64,
                width=64, ip_adapter_image_embeds=[ie])
    assert sharded.shape == full.shape == (total, 3, 64, 64)
    assert torch.allclose(sharded, full, atol=1e-5)
