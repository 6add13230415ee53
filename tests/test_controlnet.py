"""ControlNet without a GPU: manifest names and shapes against the engine's declaration, configuration parsing and
rejections, and the original-format (lllyasviel) <-> diffusers key conversion."""
import ctypes as C

import pytest
import torch

from cn_oracle import synth_cn_state_dict
from stablediffusion_amd import _lib, checkpoints, config, controlnet
from stablediffusion_amd.models import HipControlNetModel, HipUNet2DConditionModel


def _count(m):
    n = 0
    for shp in m.values():
        k = 1
        for d in shp:
            k *= d
        n += k
    return n


def test_manifest_sd15_names_and_size():
    m = controlnet.controlnet_manifest(controlnet.encoder_config(config.sd15_unet()))
    # a diffusers SD1.5 ControlNet holds about 361 M parameters (sanity check only)
    assert 360e6 < _count(m) < 362e6
    assert m["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert m["controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
    assert m["controlnet_cond_embedding.conv_out.weight"] == (320, 256, 3, 3)
    assert [m[f"controlnet_down_blocks.{i}.weight"][0] for i in range(12)] == [320] * 4 + [640] * 3 + [1280] * 5
    assert m["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    assert "controlnet_down_blocks.12.weight" not in m
    assert not any(k.startswith(("up_blocks", "conv_out", "conv_norm_out")) for k in m)


def test_manifest_sdxl():
    m = controlnet.controlnet_manifest(controlnet.encoder_config(config.sdxl_unet()))
    assert [m[f"controlnet_down_blocks.{i}.weight"][0] for i in range(9)] == [320] * 4 + [640] * 3 + [1280] * 2
    assert "controlnet_down_blocks.9.weight" not in m
    assert m["add_embedding.linear_1.weight"] == (1280, 2816)
    assert "down_blocks.2.attentions.1.transformer_blocks.9.attn2.to_k.weight" in m


@pytest.mark.parametrize("preset", ["tiny", "sd15", "sdxl"])
def test_manifest_equals_engine_weight_info(engine_lib, preset):
    ucfg = {"tiny": config.tiny_unet, "sd15": config.sd15_unet, "sdxl": config.sdxl_unet}[preset]()
    ccfg = controlnet.encoder_config(ucfg)
    u = HipUNet2DConditionModel(ucfg)
    cn = HipControlNetModel(u, ccfg)
    got = []
    for i in range(engine_lib.sd_controlnet_num_weights(cn._h)):
        k, shp, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert engine_lib.sd_controlnet_weight_info(cn._h, i, C.byref(k), shp, C.byref(nd)) == 0
        got.append((k.value.decode(), tuple(shp[j] for j in range(nd.value))))
    assert got == list(controlnet.controlnet_manifest(ccfg).items())


def test_create_rejects_mismatches(engine_lib):
    ucfg = config.tiny_unet()
    u = HipUNet2DConditionModel(ucfg)
    for changes in ({"block_out_channels": (64, 128, 256, 320)}, {"cross_attention_dim": 128}, {"layers_per_block": 1},
                    {"in_channels": 9}):
        with pytest.raises(_lib.EngineError):
            HipControlNetModel(u, controlnet.encoder_config(ucfg, **changes))
    with pytest.raises(_lib.EngineError):                          # text_time conditioning must match
        HipControlNetModel(u, controlnet.encoder_config(config.tiny_unet(sdxl_cond=True)))
    with pytest.raises(_lib.EngineError):
        HipControlNetModel(u, controlnet.encoder_config(ucfg), conditioning_channels=1)
    with pytest.raises(_lib.EngineError):                          # 9-channel inpaint UNets take no ControlNet
        inp = config.UNetConfig(**dict(ucfg.to_dict(), in_channels=9))
        HipControlNetModel(HipUNet2DConditionModel(inp), controlnet.encoder_config(inp))
    # heads and transformer depth may differ from the UNet's
    HipControlNetModel(u, controlnet.encoder_config(ucfg, transformer_layers_per_block=(2, 1, 1, 1),
                                                     attention_head_dim=(1, 2, 4, 4)))


def _diffusers_json(**kw):
    d = {"_class_name": "ControlNetModel", "in_channels": 4, "block_out_channels": [320, 640, 1280, 1280],
         "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"], "layers_per_block": 2,
         "cross_attention_dim": 768, "attention_head_dim": 8, "conditioning_embedding_out_channels": [16, 32, 96, 256],
         "global_pool_conditions": False, "controlnet_conditioning_channel_order": "rgb"}
    d.update(kw)
    return d


def test_config_from_json():
    cfg = controlnet.config_from_json(_diffusers_json())
    assert cfg.block_out_channels == (320, 640, 1280, 1280)
    assert cfg.up_block_types == ("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D")
    assert controlnet.controlnet_manifest(cfg) == controlnet.controlnet_manifest(controlnet.encoder_config(config.sd15_unet()))


@pytest.mark.parametrize("bad", [{"global_pool_conditions": True}, {"conditioning_embedding_out_channels": [16, 32, 96, 128]},
                                 {"conditioning_channels": 1}, {"controlnet_conditioning_channel_order": "bgr"}])
def test_config_rejections(bad):
    with pytest.raises(ValueError):
        controlnet.config_from_json(_diffusers_json(**bad))


def _to_original(sd, cfg, prefix):
    """diffusers -> original naming by inverting the converter's prefix map (and the resnet member renames)."""
    inv = {v: k for k, v in controlnet.original_key_map(cfg).items()}
    out = {}
    for k, v in sd.items():
        best = max((p for p in inv if k == p or k.startswith(p + ".")), key=len)
        rest = k[len(best) + 1:]
        if ".resnets." in best:
            for old, new in checkpoints._RESNET_RENAMES:
                if rest.startswith(new + "."):
                    rest = old + rest[len(new):]
                    break
        out[prefix + inv[best] + ("." + rest if rest else "")] = v
    return out


@pytest.mark.parametrize("prefix", ["", "control_model."])
def test_original_round_trip(prefix):
    cfg = controlnet.encoder_config(config.tiny_unet())
    sd = synth_cn_state_dict(cfg, seed=1)
    orig = _to_original(sd, cfg, prefix)
    assert f"{prefix}input_hint_block.14.weight" in orig and f"{prefix}zero_convs.11.0.weight" in orig
    assert f"{prefix}middle_block_out.0.bias" in orig and f"{prefix}input_blocks.1.0.in_layers.0.weight" in orig
    assert controlnet.is_original(orig)
    back = controlnet.convert_original(orig, cfg)
    assert set(back) == set(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    cfg2, sd2 = controlnet.load(orig, config.tiny_unet())
    assert controlnet.controlnet_manifest(cfg2) == controlnet.controlnet_manifest(cfg)


def test_load_checks_shapes_and_keys():
    cfg = controlnet.encoder_config(config.tiny_unet())
    sd = synth_cn_state_dict(cfg, seed=2)
    bad = dict(sd)
    bad["controlnet_mid_block.weight"] = torch.zeros(256, 256, 3, 3)
    with pytest.raises(ValueError):
        controlnet.load(bad, config.tiny_unet())
    missing = dict(sd)
    del missing["controlnet_down_blocks.3.bias"]
    with pytest.raises(KeyError):
        controlnet.load(missing, config.tiny_unet())
    deeper = synth_cn_state_dict(controlnet.encoder_config(config.tiny_unet(), transformer_layers_per_block=(2, 1, 1, 1)))
    cfg_d, _ = controlnet.load(deeper, config.tiny_unet())
    assert cfg_d.transformer_layers_per_block == (2, 1, 1, 1)


def test_unet_call_refuses_control_kwargs_without_controlnet(engine_lib):
    u = HipUNet2DConditionModel(config.tiny_unet())
    with pytest.raises(ValueError):
        u._control(torch.zeros(1, 3, 64, 64), 1.0, 1, 8, 8, "cpu")
    assert u._control(None, None, 1, 8, 8, "cpu") == (None, 0.0)
