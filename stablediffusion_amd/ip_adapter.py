"""IP-Adapter (image prompt) weights for the engine: file reading, key conversion and checks.

The original IP-Adapter files (`ip-adapter_sd15.bin`, `ip-adapter_sdxl.safetensors`, ...) hold
  image_proj.proj.{weight,bias}   [n_tok * ctx, D_img], [n_tok * ctx]   (ImageProjection.image_embeds)
  image_proj.norm.{weight,bias}   [ctx]
  ip_adapter.{id}.to_{k,v}_ip.weight   [C, ctx]   (no bias)
nested as {"image_proj": {...}, "ip_adapter": {...}} in a `.bin`, flat in a `.safetensors`.  diffusers 0.27.2
(`_convert_ip_adapter_attn_to_diffusers`) maps id = 2 i + 1 onto the i-th cross-attention processor in
`unet.attn_processors` order: down_blocks, then up_blocks, then mid_block (UNet2DConditionModel registers the up
blocks before the mid block), inside a block attentions.j before transformer_blocks.k.  The engine takes the
converted keys in diffusers' post-load naming (`ip_adapter_manifest`):
  encoder_hid_proj.image_projection_layers.0.{image_embeds,norm}.{weight,bias}
  <site>.attn2.processor.to_{k,v}_ip.0.weight
Only the base adapters' linear + LayerNorm projection is supported; IP-Adapter Plus / FaceID files (Resampler or MLP
projections) are rejected.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, List, Tuple, Union

import torch

from .config import UNetConfig

PROJ = "encoder_hid_proj.image_projection_layers.0"
_BASE_PROJ_KEYS = {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}


def xattn_sites(cfg: UNetConfig) -> List[Tuple[str, int]]:
    """(transformer block prefix, channels) of every attn2, in diffusers' attn_processors order."""
    nb = len(cfg.block_out_channels)
    boc = cfg.block_out_channels
    depth = cfg.transformer_layers_per_block
    sites = []
    for i, bt in enumerate(cfg.down_block_types):
        if bt == "CrossAttnDownBlock2D":
            for j in range(cfg.layers_per_block):
                for k in range(depth[i]):
                    sites.append((f"down_blocks.{i}.attentions.{j}.transformer_blocks.{k}", boc[i]))
    for i, bt in enumerate(cfg.up_block_types):
        if bt == "CrossAttnUpBlock2D":
            for j in range(cfg.layers_per_block + 1):
                for k in range(depth[nb - 1 - i]):
                    sites.append((f"up_blocks.{i}.attentions.{j}.transformer_blocks.{k}", boc[nb - 1 - i]))
    for k in range(depth[-1]):
        sites.append((f"mid_block.attentions.0.transformer_blocks.{k}", boc[-1]))
    return sites


def site_ids(cfg: UNetConfig) -> "OrderedDict[int, str]":
    """Original-file id -> transformer block prefix (id = 2 i + 1)."""
    return OrderedDict((2 * i + 1, p) for i, (p, _) in enumerate(xattn_sites(cfg)))


def ip_adapter_manifest(cfg: UNetConfig, image_embed_dim: int, num_tokens: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """Diffusers-named keys and shapes the engine's adapter expects, in its order (sd_ip_adapter_weight_info)."""
    ctx = cfg.cross_attention_dim
    m = OrderedDict()
    m[f"{PROJ}.image_embeds.weight"] = (num_tokens * ctx, image_embed_dim)
    m[f"{PROJ}.image_embeds.bias"] = (num_tokens * ctx,)
    m[f"{PROJ}.norm.weight"] = (ctx,)
    m[f"{PROJ}.norm.bias"] = (ctx,)
    for p, c in xattn_sites(cfg):
        m[f"{p}.attn2.processor.to_k_ip.0.weight"] = (c, ctx)
        m[f"{p}.attn2.processor.to_v_ip.0.weight"] = (c, ctx)
    return m


def read(path_or_dict: Union[str, os.PathLike, Dict]) -> Dict[str, torch.Tensor]:
    """An original IP-Adapter state dict, flattened to `image_proj.*` / `ip_adapter.*` keys.  Files: `.safetensors`,
    or a `.bin` read with torch.load(weights_only=True) (tensors and dicts only).  No hub names: a local file."""
    if isinstance(path_or_dict, dict):
        sd = path_or_dict
    else:
        path = os.fspath(path_or_dict)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"IP-Adapter weights: no such file {path!r} (hub names are not resolved)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path)
        elif path.endswith(".bin"):
            sd = torch.load(path, map_location="cpu", weights_only=True)
        else:
            raise ValueError(f"IP-Adapter weights: expected a .bin or .safetensors file, got {path!r}")
    flat = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            for k2, v2 in v.items():
                flat[f"{k}.{k2}"] = v2
        else:
            flat[k] = v
    return flat


def convert(path_or_dict, cfg: UNetConfig) -> Tuple[Dict[str, torch.Tensor], int, int]:
    """Original file -> (diffusers-named state dict, image_embed_dim, num_tokens), every shape checked against the
    UNet configuration.  Raises ValueError (unsupported projection, wrong shapes), KeyError (missing / extra keys)."""
    sd = read(path_or_dict)
    proj = {k[len("image_proj."):]: v for k, v in sd.items() if k.startswith("image_proj.")}
    if set(proj) != _BASE_PROJ_KEYS:
        if any(k.startswith(("latents", "proj_in", "proj_out", "layers", "proj.0", "perceiver")) for k in proj):
            raise ValueError("IP-Adapter Plus / FaceID files (Resampler or MLP image projection) are not supported: "
                             "only the base adapters' linear + LayerNorm projection")
        raise KeyError(f"image_proj: expected keys {sorted(_BASE_PROJ_KEYS)}, got {sorted(proj)}")
    ctx = cfg.cross_attention_dim
    pw, pb = proj["proj.weight"], proj["proj.bias"]
    if tuple(proj["norm.weight"].shape) != (ctx,) or tuple(proj["norm.bias"].shape) != (ctx,):
        raise ValueError(f"image_proj.norm: expected [{ctx}] (cross_attention_dim), got {tuple(proj['norm.weight'].shape)}")
    if pw.ndim != 2 or pw.shape[0] % ctx != 0 or tuple(pb.shape) != (pw.shape[0],):
        raise ValueError(f"image_proj.proj: expected [n_tok * {ctx}, D_img], got {tuple(pw.shape)}")
    n_tok, d_img = pw.shape[0] // ctx, pw.shape[1]
    out = OrderedDict()
    out[f"{PROJ}.image_embeds.weight"] = pw
    out[f"{PROJ}.image_embeds.bias"] = pb
    out[f"{PROJ}.norm.weight"] = proj["norm.weight"]
    out[f"{PROJ}.norm.bias"] = proj["norm.bias"]
    sites = xattn_sites(cfg)
    ids = {2 * i + 1: site for i, site in enumerate(sites)}
    seen = set()
    for k in (k for k in sd if k.startswith("ip_adapter.")):
        parts = k.split(".")
        if len(parts) != 4 or parts[3] != "weight" or parts[2] not in ("to_k_ip", "to_v_ip") or not parts[1].isdigit():
            raise KeyError(f"unexpected IP-Adapter key {k!r}")
        i = int(parts[1])
        if i not in ids:
            raise KeyError(f"{k}: id {i} names no cross-attention of this UNet (ids 1, 3, ..., {2 * len(sites) - 1})")
        prefix, c = ids[i]
        w = sd[k]
        if tuple(w.shape) != (c, ctx):
            raise ValueError(f"{k} -> {prefix}: expected [{c}, {ctx}], got {tuple(w.shape)} "
                             "(a file for another UNet, or its sites in another order)")
        out[f"{prefix}.attn2.processor.{parts[2]}.0.weight"] = w
        seen.add(k)
    missing = [f"ip_adapter.{i}.{n}.weight" for i in ids for n in ("to_k_ip", "to_v_ip")
               if f"ip_adapter.{i}.{n}.weight" not in seen]
    if missing:
        raise KeyError(f"IP-Adapter file is missing {len(missing)} keys, e.g. {missing[:3]}")
    return out, d_img, n_tok
