"""ControlNet weights for the engine: configuration, manifest, file reading and key conversion.

The engine runs diffusers 0.27.2's `ControlNetModel`: an encoder copy of the UNet (conv_in, time / add embedding,
down_blocks, mid_block) whose conv_in output is offset by `controlnet_cond_embedding(control_image)`, and one 1x1
"zero conv" per skip (`controlnet_down_blocks.{i}`) plus `controlnet_mid_block`.  Its configuration is a `UNetConfig`
of the encoder fields (the up-path fields are mirrored from the down path and not used).

Accepted files: a diffusers folder (`config.json` + `diffusion_pytorch_model[.fp16].safetensors`), a diffusers state
dict, or an original (lllyasviel ControlNet 1.0 / 1.1) `.pth` / `.safetensors` state dict, with or without the
`control_model.` prefix:
  time_embed / label_emb / input_blocks / middle_block   -> as the UNet's (checkpoints.ldm_unet_key_map)
  input_hint_block.{0,2,4,6,8,10,12,14}                  -> controlnet_cond_embedding.{conv_in, blocks.0-5, conv_out}
  zero_convs.{i}.0                                       -> controlnet_down_blocks.{i}
  middle_block_out.0                                     -> controlnet_mid_block
Not supported (rejected with an error): shuffle-style `global_pool_conditions` (from config.json, or an original
file or folder whose name says shuffle: its keys are those of any other ControlNet), conditioning channels other than 3,
conditioning_embedding_out_channels other than (16, 32, 96, 256), MultiControlNet lists, Control-LoRA, T2I-Adapter.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Dict, Tuple, Union

import torch

from . import checkpoints
from .config import UNetConfig
from .weights import unet_manifest

COND = "controlnet_cond_embedding"
COND_OUT_CHANNELS = (16, 32, 96, 256)
_ORIG_PREFIX = "control_model."
_ENCODER_PREFIXES = ("conv_in.", "time_embedding.", "add_embedding.", "down_blocks.", "mid_block.")


def _up_types(down):
    return tuple(t.replace("Down", "Up") for t in reversed(down))


def encoder_config(cfg: UNetConfig, **changes) -> UNetConfig:
    """A ControlNet configuration for a UNet configuration (same encoder; `changes` override fields)."""
    d = cfg.to_dict()
    d["time_cond_proj_dim"] = None          # ControlNetModel has no cond_proj (and the engine's never declares one)
    d.update(changes)
    d["up_block_types"] = _up_types(d["down_block_types"])
    d["out_channels"] = d.get("out_channels", 4)
    return UNetConfig(**{k: tuple(v) if isinstance(v, list) else v for k, v in d.items()})


def num_sites(cfg: UNetConfig) -> int:
    """Residual sites: conv_in, every down resnet / transformer output, every downsampler (mid block excluded)."""
    nb = len(cfg.block_out_channels)
    return 1 + nb * cfg.layers_per_block + (nb - 1)


def site_channels(cfg: UNetConfig):
    boc = cfg.block_out_channels
    ch = [boc[0]]
    for i, c in enumerate(boc):
        ch += [c] * cfg.layers_per_block
        if i != len(boc) - 1:
            ch.append(c)
    return ch


def controlnet_manifest(cfg: UNetConfig, conditioning_channels: int = 3) -> "OrderedDict[str, Tuple[int, ...]]":
    """Every ControlNet weight in diffusers naming with its shape, in the engine's declaration order."""
    m: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict(
        (k, v) for k, v in unet_manifest(cfg).items() if k.startswith(_ENCODER_PREFIXES))
    cin = conditioning_channels
    outs = [COND_OUT_CHANNELS[0]]
    for i in range(len(COND_OUT_CHANNELS) - 1):
        outs += [COND_OUT_CHANNELS[i], COND_OUT_CHANNELS[i + 1]]
    for l, co in enumerate(outs):
        p = f"{COND}.conv_in" if l == 0 else f"{COND}.blocks.{l - 1}"
        m[p + ".weight"] = (co, cin, 3, 3)
        m[p + ".bias"] = (co,)
        cin = co
    c0 = cfg.block_out_channels[0]
    m[f"{COND}.conv_out.weight"] = (c0, cin, 3, 3)
    m[f"{COND}.conv_out.bias"] = (c0,)
    for i, c in enumerate(site_channels(cfg)):
        m[f"controlnet_down_blocks.{i}.weight"] = (c, c, 1, 1)
        m[f"controlnet_down_blocks.{i}.bias"] = (c,)
    mid = cfg.block_out_channels[-1]
    m["controlnet_mid_block.weight"] = (mid, mid, 1, 1)
    m["controlnet_mid_block.bias"] = (mid,)
    return m


def config_from_json(d: dict) -> UNetConfig:
    """A diffusers ControlNetModel `config.json` -> the engine's ControlNet configuration.  Raises ValueError for what
    the engine does not run."""
    if d.get("global_pool_conditions"):
        raise ValueError("ControlNet with global_pool_conditions (shuffle) is not supported")
    if tuple(d.get("conditioning_embedding_out_channels", COND_OUT_CHANNELS)) != COND_OUT_CHANNELS:
        raise ValueError("ControlNet conditioning_embedding_out_channels must be (16, 32, 96, 256)")
    if d.get("conditioning_channels", 3) != 3:
        raise ValueError("ControlNet conditioning_channels must be 3")
    if d.get("controlnet_conditioning_channel_order", "rgb") != "rgb":
        raise ValueError("ControlNet controlnet_conditioning_channel_order must be 'rgb'")
    d = dict(d)
    d.setdefault("out_channels", 4)
    d["up_block_types"] = list(_up_types(d["down_block_types"]))
    return checkpoints.unet_config_from_json(d)


def original_key_map(cfg: UNetConfig) -> Dict[str, str]:
    """Prefix map {original module prefix -> diffusers module prefix} of an original ControlNet."""
    m = {k: v for k, v in checkpoints.ldm_unet_key_map(cfg).items()
         if not k.startswith(("output_blocks.", "out."))}
    names = ["conv_in"] + [f"blocks.{i}" for i in range(6)] + ["conv_out"]
    for i, n in enumerate(names):
        m[f"input_hint_block.{2 * i}"] = f"{COND}.{n}"
    for i in range(num_sites(cfg)):
        m[f"zero_convs.{i}.0"] = f"controlnet_down_blocks.{i}"
    m["middle_block_out.0"] = "controlnet_mid_block"
    return m


def is_original(sd: Dict[str, torch.Tensor]) -> bool:
    return any(k.startswith(("input_hint_block.", _ORIG_PREFIX + "input_hint_block.")) for k in sd)


def convert_original(sd: Dict[str, torch.Tensor], cfg: UNetConfig) -> Dict[str, torch.Tensor]:
    """Original (lllyasviel) ControlNet state dict -> diffusers naming.  Raises KeyError for unmapped keys."""
    pmap = original_key_map(cfg)
    resnets = {v for v in pmap.values() if ".resnets." in v}
    out: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        if k.startswith(_ORIG_PREFIX):
            k = k[len(_ORIG_PREFIX):]
        if k in ("lvlb_weights", "betas") or k.startswith(("alphas", "sqrt_", "log_one", "posterior")):
            continue                        # (scheduler buffers some training checkpoints carry)
        nk = checkpoints._apply_prefix_map(k, pmap, resnets)
        if nk is None:
            raise KeyError(f"unmapped ControlNet key: {k}")
        out[nk] = v
    return out


def check_state_dict(sd: Dict[str, torch.Tensor], cfg: UNetConfig):
    """Every key and shape against the manifest (ValueError / KeyError with the first offenders)."""
    man = controlnet_manifest(cfg)
    missing = [k for k in man if k not in sd]
    extra = [k for k in sd if k not in man]
    if missing or extra:
        raise KeyError(f"ControlNet state dict: missing {missing[:3]}, unexpected {extra[:3]}")
    for k, shp in man.items():
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"ControlNet {k}: expected shape {shp}, got {tuple(sd[k].shape)}")


def infer_config(sd: Dict[str, torch.Tensor], unet_cfg: UNetConfig) -> UNetConfig:
    """The configuration of a diffusers-named ControlNet state dict that feeds a UNet of `unet_cfg`: the UNet's
    encoder, with the transformer depth per block read from the weights (heads cannot be read and are the UNet's)."""
    depth = []
    for i, t in enumerate(unet_cfg.down_block_types):
        pre = f"down_blocks.{i}.attentions.0.transformer_blocks."
        n = len({k[len(pre):].split(".")[0] for k in sd if k.startswith(pre)})
        depth.append(n if n else unet_cfg.transformer_layers_per_block[i])
    return encoder_config(unet_cfg, transformer_layers_per_block=tuple(depth))


def load(path_or_dict: Union[str, os.PathLike, Dict], unet_cfg: UNetConfig) -> Tuple[UNetConfig, Dict[str, torch.Tensor]]:
    """A ControlNet folder, file or state dict -> (configuration, diffusers-named state dict), checked."""
    cfg = None
    if isinstance(path_or_dict, dict):
        sd = path_or_dict
    else:
        path = os.fspath(path_or_dict)
        if "shuffle" in os.path.basename(os.path.normpath(path)).lower():
            # an original shuffle file has the keys of any other ControlNet; only its name tells it apart
            raise ValueError("ControlNet shuffle (global_pool_conditions) is not supported")
        if os.path.isdir(path):
            cj = os.path.join(path, "config.json")
            if os.path.isfile(cj):
                with open(cj) as f:
                    cfg = config_from_json(json.load(f))
            path = checkpoints._find_weights(path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"ControlNet weights: no such file {path!r} (hub names are not resolved)")
        if path.endswith(".safetensors"):
            sd = checkpoints.load_safetensors(path)
        elif path.endswith((".pth", ".bin", ".ckpt")):
            sd = torch.load(path, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd)
        else:
            raise ValueError(f"ControlNet weights: expected .safetensors / .pth / .bin, got {path!r}")
    if is_original(sd):
        sd = convert_original(sd, encoder_config(unet_cfg))
    if cfg is None:
        cfg = infer_config(sd, unet_cfg)
    check_state_dict(sd, cfg)
    return cfg, sd


def _per_net(v, n, name):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} ControlNet{'s' if n != 1 else ''}")
        return [float(x) for x in v]
    return [float(v)] * n


def keep_schedule(n_steps, scales, starts=0.0, ends=1.0):
    """The conditioning scales of a denoising loop, one row of per-net scales per step (diffusers' controlnet_keep times
    the scale): scale_i * (1 - float(step / n < start_i or (step + 1) / n > end_i)).  Lists give one entry per net;
    floats broadcast to the net count (one net when all three are floats)."""
    n_nets = max([len(v) for v in (scales, starts, ends) if isinstance(v, (list, tuple))], default=1)
    sc, st, en = (_per_net(v, n_nets, k) for v, k in ((scales, "controlnet_conditioning_scale"),
                                                      (starts, "control_guidance_start"), (ends, "control_guidance_end")))
    n = int(n_steps)
    return [[s * (1.0 - float(i / n < a or (i + 1) / n > b)) for s, a, b in zip(sc, st, en)] for i in range(n)]


def list_arguments(n_nets, control_image, scales, starts, ends):
    """The argument checks of a call with `n_nets` ControlNets loaded as a list (ValueError, before anything runs):
    control_image a non-empty list with one entry per net; scale and guidance window floats or lists of the net count,
    every window 0 <= start < end <= 1.  Returns (scales, starts, ends) as lists of n_nets floats."""
    if not isinstance(control_image, (list, tuple)):
        raise ValueError(f"{n_nets} ControlNets are loaded: control_image must be a list with one entry per net")
    if len(control_image) == 0:
        raise ValueError("control_image is an empty list")
    if len(control_image) != n_nets:
        raise ValueError(f"control_image: {len(control_image)} entries for {n_nets} ControlNets")
    sc = _per_net(scales, n_nets, "controlnet_conditioning_scale")
    st = _per_net(starts, n_nets, "control_guidance_start")
    en = _per_net(ends, n_nets, "control_guidance_end")
    for a, b in zip(st, en):
        if not 0.0 <= a < b <= 1.0:
            raise ValueError("need 0 <= control_guidance_start < control_guidance_end <= 1")
    return sc, st, en
