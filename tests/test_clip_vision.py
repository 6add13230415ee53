"""Host side of the CLIP vision encoder (no GPU): the weight manifest against transformers' state dict, the image
preprocessing against transformers' CLIPImageProcessor, the config and folder loaders, create-time rejections."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from stablediffusion_amd import _lib, checkpoints, config
from stablediffusion_amd.image_processor import ClipImageProcessor


def _tiny_hf_config(transformers, **over):
    kw = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56,
              patch_size=14, hidden_act="quick_gelu", projection_dim=48)
    kw.update(over)
    return transformers.CLIPVisionConfig(**kw)


def _manifest(lib, cfg: config.CLIPVisionConfig):
    from stablediffusion_amd.models import HipCLIPVisionModelWithProjection
    eng = HipCLIPVisionModelWithProjection(cfg)
    got = {}
    for i in range(lib.sd_clip_vision_num_weights(eng._h)):
        key, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert lib.sd_clip_vision_weight_info(eng._h, i, C.byref(key), shape, C.byref(ndim)) == 0
        got[key.value.decode()] = tuple(shape[j] for j in range(ndim.value))
    return got


@pytest.mark.parametrize("over", [dict(), dict(hidden_size=208, intermediate_size=320, image_size=42, hidden_act="gelu"),
                                  dict(patch_size=16, image_size=48, projection_dim=128)])
def test_manifest_matches_transformers_state_dict(engine_lib, over):
    """sd_clip_vision_weight_info reports exactly the state-dict entries of CLIPVisionModelWithProjection of the same
    config: names (`pre_layrnorm` included) and shapes; `position_ids` is a non-persistent buffer and in neither."""
    transformers = pytest.importorskip("transformers")
    hf_cfg = _tiny_hf_config(transformers, **over)
    want = {k: tuple(v.shape) for k, v in transformers.CLIPVisionModelWithProjection(hf_cfg).state_dict().items()}
    assert not any(k.endswith("position_ids") for k in want)
    got = _manifest(engine_lib, config.CLIPVisionConfig.from_hf(hf_cfg))
    assert got == want
    assert "vision_model.pre_layrnorm.weight" in got
    S, P, H = hf_cfg.image_size, hf_cfg.patch_size, hf_cfg.hidden_size
    assert got["vision_model.embeddings.patch_embedding.weight"] == (H, 3, P, P)
    assert got["vision_model.embeddings.position_embedding.weight"] == (1 + (S // P) ** 2, H)


@pytest.mark.parametrize("wh", [(224, 224), (301, 517), (640, 333), (97, 150), (225, 224)])
def test_image_processor_matches_transformers(wh):
    """Against transformers' CLIPImageProcessor on random PIL images: max abs difference <= 2e-6 (a plain PIL
    restatement measured 4.8e-7, two fp32 ulps at magnitude 2; the cap leaves room for operation order)."""
    transformers = pytest.importorskip("transformers")
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(wh[0] * 1000 + wh[1])
    img = Image.fromarray(rng.integers(0, 256, size=(wh[1], wh[0], 3), dtype=np.uint8))
    assert img.size == wh
    ref = transformers.CLIPImageProcessor()(img, return_tensors="pt").pixel_values
    proc = ClipImageProcessor()
    got = proc(img, return_tensors="pt").pixel_values
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 224, 224) == tuple(ref.shape)
    diff = (got - ref).abs().max().item()
    print(f"image {wh}: max abs diff {diff:.3e}")
    assert diff <= 2e-6
    # lists and arrays go the same way
    both = proc([img, np.asarray(img)], return_tensors="pt").pixel_values
    assert tuple(both.shape) == (2, 3, 224, 224)
    assert torch.equal(both[0], got[0]) and torch.equal(both[1], got[0])


def test_image_processor_other_size_and_errors():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, size=(70, 90, 3), dtype=np.uint8))
    px = ClipImageProcessor(size=56)(img).pixel_values
    assert tuple(px.shape) == (1, 3, 56, 56)
    assert isinstance(ClipImageProcessor(size=56)(img, return_tensors="np").pixel_values, np.ndarray)
    with pytest.raises(ValueError):
        ClipImageProcessor()(np.zeros((3, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        ClipImageProcessor()([])


def test_config_from_dict_round_trip():
    transformers = pytest.importorskip("transformers")
    for ctor in (config.clip_vit_l14, config.clip_vit_h14, config.clip_vit_bigg14):
        cfg = ctor()
        assert config.CLIPVisionConfig.from_dict(cfg.to_dict()) == cfg
        assert cfg.hidden_size % cfg.num_attention_heads == 0 and cfg.image_size % cfg.patch_size == 0
    assert config.clip_vit_bigg14().hidden_size // config.clip_vit_bigg14().num_attention_heads == 104
    # a transformers config.json: unknown keys are ignored, known ones carried
    hf = _tiny_hf_config(transformers, hidden_act="gelu", layer_norm_eps=1e-6)
    cfg = config.CLIPVisionConfig.from_dict(json.loads(hf.to_json_string()))
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads) == (128, 256, 2, 2)
    assert (cfg.image_size, cfg.patch_size, cfg.hidden_act, cfg.projection_dim, cfg.layer_norm_eps) == (56, 14, "gelu", 48, 1e-6)
    # a full CLIPConfig: the vision section, projection_dim from the top level
    full = {"projection_dim": 96, "vision_config": {"hidden_size": 64, "intermediate_size": 128, "num_hidden_layers": 1,
                                                    "num_attention_heads": 1, "image_size": 28, "patch_size": 14}}
    cfg = config.CLIPVisionConfig.from_dict(full)
    assert (cfg.hidden_size, cfg.projection_dim, cfg.image_size) == (64, 96, 28)


def test_load_image_encoder_folder(tmp_path):
    transformers = pytest.importorskip("transformers")
    st = pytest.importorskip("safetensors.torch")
    hf_cfg = _tiny_hf_config(transformers)
    model = transformers.CLIPVisionModelWithProjection(hf_cfg).half()
    folder = tmp_path / "image_encoder"
    os.makedirs(folder)
    with open(folder / "config.json", "w") as f:
        f.write(hf_cfg.to_json_string())
    want = {k: v.contiguous() for k, v in model.state_dict().items()}
    st.save_file(want, str(folder / "model.safetensors"))
    for path in (folder, tmp_path):                 # the folder itself, or the one above it
        cfg, sd = checkpoints.load_image_encoder_folder(str(path))
        assert cfg == config.CLIPVisionConfig.from_hf(hf_cfg)
        assert set(sd) == set(want) and all(torch.equal(sd[k], want[k]) for k in want)
    # model.fp16.safetensors wins when both are there
    marked = dict(want)
    marked["visual_projection.weight"] = torch.ones_like(want["visual_projection.weight"])
    st.save_file(marked, str(folder / "model.fp16.safetensors"))
    _, sd = checkpoints.load_image_encoder_folder(str(folder))
    assert torch.equal(sd["visual_projection.weight"], marked["visual_projection.weight"])
    with pytest.raises(FileNotFoundError):
        os.makedirs(tmp_path / "empty")
        with open(tmp_path / "empty" / "config.json", "w") as f:
            f.write(hf_cfg.to_json_string())
        checkpoints.load_image_encoder_folder(str(tmp_path / "empty"))


SD_ERR_UNSUPPORTED = 4      # include/sd_engine.h


def _create(lib, **over):
    kw = dict(hidden_size=128, intermediate_size=256, num_layers=1, num_heads=2, image_size=56, patch_size=14,
              hidden_act=0, projection_dim=32, layer_norm_eps=1e-5)
    kw.update(over)
    c = _lib.SdClipVisionConfig(**kw)
    h = C.c_void_p()
    rc = lib.sd_clip_vision_create(C.byref(c), C.byref(h))
    msg = lib.sd_last_error().decode()
    if rc == 0:
        lib.sd_clip_vision_destroy(h)
    return rc, msg


def test_create_rejections(engine_lib):
    assert _create(engine_lib)[0] == 0
    rc, msg = _create(engine_lib, image_size=57)                        # S % P != 0
    assert rc == SD_ERR_UNSUPPORTED and "57" in msg and "patch_size" in msg
    rc, msg = _create(engine_lib, hidden_size=136, num_heads=3)         # H % heads != 0
    assert rc == SD_ERR_UNSUPPORTED and "num_heads" in msg
    rc, msg = _create(engine_lib, hidden_size=132, num_heads=2)         # H % 8 != 0
    assert rc == SD_ERR_UNSUPPORTED and "multiples of 8" in msg
    rc, msg = _create(engine_lib, hidden_size=272, num_heads=2)         # d = 136: above every paddable head dim
    assert rc == SD_ERR_UNSUPPORTED and "136" in msg
    # head dims the attention kernels lack are padded, not rejected: 104 -> 128 (ViT-bigG/14), 48 -> 64
    assert _create(engine_lib, hidden_size=208, num_heads=2)[0] == 0
    assert _create(engine_lib, hidden_size=96, num_heads=2)[0] == 0
    assert _create(engine_lib, hidden_act=2)[0] == 1


def test_shim_rejects_what_it_does_not_do(engine_lib):
    from stablediffusion_amd.models import HipCLIPVisionModelWithProjection
    with pytest.raises(TypeError):
        HipCLIPVisionModelWithProjection(config.clip_l())
    with pytest.raises(_lib.EngineError):
        HipCLIPVisionModelWithProjection(config.CLIPVisionConfig(hidden_act="relu"))
    enc = HipCLIPVisionModelWithProjection(config.CLIPVisionConfig(hidden_size=128, intermediate_size=256,
                                                                   num_hidden_layers=1, num_attention_heads=2,
                                                                   image_size=56, projection_dim=32))
    with pytest.raises(_lib.EngineError):                               # weights not loaded
        enc(torch.zeros(1, 3, 56, 56))
    assert enc.dtype == torch.float16 and enc.config.image_size == 56
