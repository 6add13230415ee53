"""SDXL refiner, host side: the five-id text_time configuration through config / C struct / checkpoint readers, the
wrapper's third UNet slot, and the pipeline's use_refiner / refiner_start paths on stand-in UNets.  CPU only."""
import ctypes as C
import json
from types import SimpleNamespace

import pytest
import torch

from refiner_doubles import RecordingUNet, StubTextEncoder, StubTokenizer
from stablediffusion_amd import _lib, checkpoints, config, weights
from stablediffusion_amd.models import _unet_config_struct
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


def tiny_sdxl_base():
    """tiny_unet's SDXL form reading two 64-wide encoders (the refiner reads the second alone)."""
    return config.UNetConfig(**dict(config.tiny_unet(linear=True, sdxl_cond=True).to_dict(), cross_attention_dim=128))


# ------------------------------------------------------------------------------------------------ configuration
def test_num_time_ids_property_and_presets():
    assert config.tiny_unet().num_time_ids == 0
    assert config.sdxl_unet().num_time_ids == 6 and config.sdxl_unet().pooled_projection_dim is None
    assert config.tiny_unet(linear=True, sdxl_cond=True).num_time_ids == 6
    r = config.sdxl_refiner_unet()
    assert r.num_time_ids == 5 and r.projection_class_embeddings_input_dim == 1280 + 5 * 256
    assert r.block_out_channels == (384, 768, 1536, 1536) and r.attention_head_dim == (6, 12, 24, 24)
    assert config.tiny_refiner_unet().num_time_ids == 5
    assert config.PRESETS["sdxl_refiner"][0]() == r
    assert sum(torch.Size(s).numel() for s in weights.unet_manifest(r).values()) == 2_259_526_660
    bad = config.UNetConfig(**dict(r.to_dict(), pooled_projection_dim=1000))
    with pytest.raises(ValueError):
        bad.num_time_ids


def _create(lib, c):
    h = C.c_void_p()
    rc = lib.sd_unet_create(C.byref(c), C.byref(h))
    if rc == 0:
        lib.sd_unet_destroy(h)
    return rc


def test_config_struct_round_trip(engine_lib):
    assert "num_time_ids" in [f[0] for f in _lib.SdUNetConfig._fields_]
    assert _unet_config_struct(config.tiny_refiner_unet()).num_time_ids == 5
    assert _unet_config_struct(config.tiny_unet(linear=True, sdxl_cond=True)).num_time_ids == 6
    assert _unet_config_struct(config.tiny_unet()).num_time_ids == 0
    # 0 means 6: a zero-initialised caller's SDXL-base configuration is accepted as before ...
    c = _unet_config_struct(config.tiny_unet(linear=True, sdxl_cond=True))
    c.num_time_ids = 0
    assert _create(engine_lib, c) == 0
    # ... and the refiner's widths are not: 224 - 6 * 32 = 32 > 0 passed the old check, 5 ids give the real pooled width
    c = _unet_config_struct(config.tiny_refiner_unet())
    assert _create(engine_lib, c) == 0
    for n in (-1, 9, 7):            # out of 1..8; 224 - 7 * 32 = 0 leaves no pooled columns
        c.num_time_ids = n
        assert _create(engine_lib, c) == 4, n
        assert b"num_time_ids" in engine_lib.sd_last_error()


def test_engine_manifest_of_the_refiner_topology(engine_lib):
    from stablediffusion_amd.models import HipUNet2DConditionModel
    cfg = config.tiny_refiner_unet()
    net = HipUNet2DConditionModel(cfg)
    got = {}
    for i in range(engine_lib.sd_unet_num_weights(net._h)):
        key, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert engine_lib.sd_unet_weight_info(net._h, i, C.byref(key), shape, C.byref(ndim)) == 0
        got[key.value.decode()] = tuple(shape[j] for j in range(ndim.value))
    assert got == dict(weights.unet_manifest(cfg))
    assert got["add_embedding.linear_1.weight"] == (256, 224)


def test_text_time_input_entry_rejects_bad_arguments(engine_lib):
    """sd_op_text_time_input validates before it launches: no device needed."""
    p = C.c_void_p(64)
    f = engine_lib.sd_op_text_time_input
    for B, P, ad, n in ((1, 64, 32, 0), (1, 64, 32, 9), (1, 64, 31, 5), (1, 0, 32, 5), (1, -4, 32, 5), (0, 64, 32, 5),
                        (1, 64, 0, 5)):
        assert f(p, p, p, B, P, ad, n, 1, 0.0, None) == 1, (B, P, ad, n)
        assert b"sd_op_text_time_input" in engine_lib.sd_last_error()
    assert f(None, p, p, 1, 64, 32, 5, 1, 0.0, None) == 1


# ------------------------------------------------------------------------------------------------ checkpoints
def _hub_json(cfg):
    d = cfg.to_dict()
    d.pop("pooled_projection_dim")              # diffusers' files do not carry it
    for k in ("attention_head_dim", "transformer_layers_per_block", "block_out_channels", "down_block_types",
              "up_block_types"):
        d[k] = list(d[k])
    return d


def test_unet_config_from_json_refiner_and_base():
    ref = config.sdxl_refiner_unet()
    got = checkpoints.unet_config_from_json(_hub_json(ref))
    assert got == ref and got.num_time_ids == 5                      # inferred from the signature
    assert checkpoints.unet_config_from_json(dict(_hub_json(ref), pooled_projection_dim=1280)) == ref
    base = config.sdxl_unet()
    got = checkpoints.unet_config_from_json(_hub_json(base))
    assert got == base and got.pooled_projection_dim is None and got.num_time_ids == 6
    assert checkpoints.unet_config_from_json(_hub_json(config.sd15_unet())) == config.sd15_unet()
    tiny = config.tiny_refiner_unet()                                # no signature: the explicit field decides
    assert checkpoints.unet_config_from_json(dict(_hub_json(tiny), pooled_projection_dim=64)) == tiny
    assert checkpoints.unet_config_from_json(_hub_json(tiny)).pooled_projection_dim is None


def test_load_unet_folder_both_layouts(tmp_path):
    from safetensors.torch import save_file
    cfg = config.tiny_refiner_unet()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=3, dtype=torch.float16)
    for folder in (tmp_path / "a" / "unet", tmp_path / "b"):
        folder.mkdir(parents=True)
        json.dump(dict(_hub_json(cfg), pooled_projection_dim=64), open(folder / "config.json", "w"))
        save_file(sd, str(folder / "diffusion_pytorch_model.fp16.safetensors"))
    for root in (tmp_path / "a", tmp_path / "b"):
        got_cfg, got_sd = checkpoints.load_unet_folder(str(root))
        assert got_cfg == cfg and set(got_sd) == set(sd)
        assert all(torch.equal(got_sd[k], sd[k]) for k in sd)


def test_ldm_key_map_covers_the_refiner():
    cfg = config.sdxl_refiner_unet()
    man = weights.unet_manifest(cfg)
    pmap = checkpoints.ldm_unet_key_map(cfg)
    targets = sorted(pmap.values(), key=len, reverse=True)
    assert len(set(pmap.values())) == len(pmap)                      # one-to-one
    used = set()
    for k in man:
        hit = next((t for t in targets if k.startswith(t + ".")), None)
        assert hit is not None, k
        used.add(hit)
    assert used == set(pmap.values())                                # nothing maps outside the manifest
    # and a single-file refiner round-trips: diffusers names -> LDM names (inverse map) -> ldm_to_diffusers_unet
    tiny = config.tiny_refiner_unet()
    tman = weights.unet_manifest(tiny)
    tmap = checkpoints.ldm_unet_key_map(tiny)
    inv = sorted(((v, k) for k, v in tmap.items()), key=lambda p: len(p[0]), reverse=True)
    renames = {new: old for old, new in checkpoints._RESNET_RENAMES}
    ldm = {}
    for i, k in enumerate(tman):
        new, old = next(p for p in inv if k.startswith(p[0] + "."))
        rest = k[len(new) + 1:]
        if ".resnets." in new:
            head = next((n for n in renames if rest.startswith(n)), None)
            if head:
                rest = renames[head] + rest[len(head):]
        ldm[checkpoints.UNET_PREFIX + old + "." + rest] = torch.full((1,), float(i))
    back = checkpoints.ldm_to_diffusers_unet(ldm, tiny)
    assert list(back) == list(tman) and all(back[k].item() == i for i, k in enumerate(tman))


# ------------------------------------------------------------------------------------------------ wrapper
def _vae_stub():
    moved = []
    return SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), moved=moved,
                           to=lambda d: moved.append(str(d)))


def _model(with_refiner=True, with_enc2=True):
    kw = dict(base=RecordingUNet(tiny_sdxl_base()), vae=_vae_stub(), text_encoder=StubTextEncoder(64, 64, 1),
              tokenizer=StubTokenizer(), device="cpu")
    if with_enc2:
        kw.update(text_encoder_2=StubTextEncoder(64, 64, 2), tokenizer_2=StubTokenizer(), model_type="sdxl")
    if with_refiner:
        kw.update(refiner=RecordingUNet(config.tiny_refiner_unet()))
    return SDModelWrapper(**kw)


def test_wrapper_refiner_slot():
    m = _model(with_refiner=False)
    assert m.refiner is None and not m.has_refiner
    with pytest.raises(ValueError, match="engine UNet or a local folder"):
        m.load_refiner(None)
    with pytest.raises(ValueError):
        m.load_refiner(3)
    with pytest.raises(ValueError):
        m.load_refiner("/nonexistent/refiner.safetensors")
    r = RecordingUNet(config.tiny_refiner_unet())
    m.load_refiner(r)
    assert m.refiner is r and m.has_refiner
    m.to("cpu")
    assert r.device == "cpu" and m.base.device == "cpu"
    r.device = None
    m.to("meta")
    assert r.device == "meta" and m.base.device == "meta"            # to() moves the refiner with the base
    m.unload_refiner()
    assert m.refiner is None and not m.has_refiner
    assert _model().has_refiner                                       # the constructor argument


# ------------------------------------------------------------------------------------------------ pipeline pieces
def test_get_add_time_ids_refiner_rows_and_messages():
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    pipe.model = _model()
    pipe._use_refiner = True
    ids, neg = pipe._get_add_time_ids((128, 96), (0, 8), None, torch.float32, aesthetic_score=6.0,
                                      negative_aesthetic_score=2.5)
    assert ids.tolist() == [[128.0, 96.0, 0.0, 8.0, 6.0]] and neg.tolist() == [[128.0, 96.0, 0.0, 8.0, 2.5]]
    # six base-style ids on the five-id refiner: the reference's first message (sd_unified_pipeline.py:999-1005)
    with pytest.raises(ValueError, match="requires_aesthetics_score"):
        pipe._get_add_time_ids((128, 128), (0, 0), (128, 128), torch.float32)
    # a configuration whose widths do not add up: the second (:1006-1009)
    pipe.model.refiner.add_embedding.linear_1.in_features = 999
    with pytest.raises(ValueError, match="incorrect config"):
        pipe._get_add_time_ids((128, 128), (0, 0), None, torch.float32, aesthetic_score=6.0, negative_aesthetic_score=2.5)
    # the base keeps its six ids, one tensor
    pipe._use_refiner = False
    assert pipe._get_add_time_ids((128, 128), (0, 0), (128, 128), torch.float16).tolist() == [[128, 128, 0, 0, 128, 128]]


def test_encode_prompt_second_encoder_only():
    m = _model()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    pipe.model = m
    pipe._use_refiner = True
    pe, ne, pooled, npooled = pipe.encode_prompt("a cat", negative_prompt="blurry", num_images_per_prompt=2)
    assert m.text_encoder.calls == 0 and m.text_encoder_2.calls == 2
    ids = m.tokenizer_2("a cat").input_ids
    o = m.text_encoder_2(ids, output_hidden_states=True)
    assert pe.shape == (2, 77, 64) and torch.equal(pe[0], o.hidden_states[-2][0]) and torch.equal(pe[1], pe[0])
    assert pooled.shape == (2, 64) and torch.equal(pooled[0], o[0][0])
    on = m.text_encoder_2(m.tokenizer_2("blurry").input_ids, output_hidden_states=True)
    assert torch.equal(ne[0], on.hidden_states[-2][0]) and torch.equal(npooled[1], on[0][0])
    pe2, *_ = pipe.encode_prompt("a cat", clip_skip=1)
    assert torch.equal(pe2[0], o.hidden_states[-3][0])
    pe3, *_ = pipe.encode_prompt("a cat", prompt_2="a dog")           # prompt_2 is the refiner's prompt
    od = m.text_encoder_2(m.tokenizer_2("a dog").input_ids, output_hidden_states=True)
    assert torch.equal(pe3[0], od.hidden_states[-2][0])
    pipe.model = _model(with_enc2=False)
    with pytest.raises(ValueError, match="text_encoder_2"):
        pipe.encode_prompt("a cat")


def test_refiner_argument_errors():
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    kw = dict(prompt="a cat", num_inference_steps=5, seed=1)
    for r in (0.0, 1.0, -0.2, 1.5, True):
        with pytest.raises(ValueError, match="refiner_start"):
            pipe(_model(), refiner_start=r, **kw)
    lat = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match="use_refiner"):
        pipe(_model(), refiner_start=0.6, use_refiner=True, image=lat, **kw)
    with pytest.raises(ValueError, match="denoising_end"):
        pipe(_model(), refiner_start=0.6, denoising_end=0.8, **kw)
    with pytest.raises(ValueError, match="no refiner"):
        pipe(_model(with_refiner=False), refiner_start=0.6, **kw)
    with pytest.raises(ValueError, match="no refiner"):
        pipe(_model(with_refiner=False), use_refiner=True, image=lat, **kw)
    with pytest.raises(ValueError, match="text_encoder_2"):
        pipe(_model(with_enc2=False), refiner_start=0.6, **kw)
    with pytest.raises(ValueError, match="text_encoder_2"):
        pipe(_model(with_enc2=False), use_refiner=True, image=lat, **kw)


@pytest.mark.parametrize("sched", ["euler", "DDIM"])
def test_refiner_start_splits_the_schedule_between_the_two_unets(sched):
    m = _model()
    m.set_scheduler(sched)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    kw = dict(prompt="a cat", negative_prompt="blurry", num_inference_steps=5, seed=7, guidance_scale=4.0)
    out = pipe(m, refiner_start=0.6, **kw)
    assert out.shape == (1, 4, 16, 16) and torch.isfinite(out).all()
    tb, tr = [c.t for c in m.base.calls], [c.t for c in m.refiner.calls]
    cutoff = 1000 - 0.6 * 1000
    assert tb and tr and all(t >= cutoff for t in tb) and all(t < cutoff for t in tr)
    m.scheduler.set_timesteps(5)
    assert tb + tr == [float(t) for t in m.scheduler.timesteps.tolist()]           # the whole schedule, once
    # the base: two encoders (128 wide), six ids, both halves alike
    for c in m.base.calls:
        assert c.sample == (2, 4, 16, 16) and c.ehs == (2, 77, 128)
        assert c.time_ids.tolist() == [[128.0, 128, 0, 0, 128, 128]] * 2
    # the refiner: encoder 2 alone (64 wide), five ids, the negative row first with its own score
    for c in m.refiner.calls:
        assert c.sample == (2, 4, 16, 16) and c.ehs == (2, 77, 64) and c.text_embeds.shape == (2, 64)
        assert c.time_ids.tolist() == [[128.0, 128, 0, 0, 2.5], [128.0, 128, 0, 0, 6.0]]
    # ... and it is the two-call composition
    m2 = _model()
    m2.set_scheduler(sched)
    a = pipe(m2, denoising_end=0.6, **kw)
    b = pipe(m2, use_refiner=True, image=a, denoising_start=0.6, **kw)
    assert torch.equal(out, b)
    assert [c.t for c in m2.base.calls] == tb and [c.t for c in m2.refiner.calls] == tr
    # scores are arguments
    m3 = _model()
    pipe(m3, use_refiner=True, image=a, denoising_start=0.6, aesthetic_score=7.0, negative_aesthetic_score=1.0, **kw)
    assert m3.refiner.calls[0].time_ids[:, 4].tolist() == [1.0, 7.0] and not m3.base.calls
    # the default call is untouched by all this
    m4 = _model()
    pipe(m4, **kw)
    assert len(m4.base.calls) == 5 and not m4.refiner.calls
