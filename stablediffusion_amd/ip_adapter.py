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

IP-Adapter Plus files (`ip-adapter-plus_sd15`, `ip-adapter-plus-face_sd15`, `ip-adapter-plus_sdxl_vit-h`) project the
image encoder's penultimate hidden states [T_feat, D_emb] through a perceiver Resampler instead.  Its `image_proj.` keys
  latents [1, n_q, dim]   proj_in.{weight,bias} [dim, D_emb]   proj_out.{weight,bias} [ctx, dim]   norm_out.{weight,bias}
  layers.{i}.0.{norm1,norm2}.{weight,bias}   layers.{i}.0.{to_q,to_kv,to_out}.weight   (to_q: [heads * 64, dim])
  layers.{i}.1.0.{weight,bias} (LayerNorm)   layers.{i}.1.1.weight [ff_mult dim, dim]   layers.{i}.1.3.weight
keep their suffixes UNCHANGED under the same prefix (diffusers renames them differently from release to release, and the
engine pins none of those namings).  `resampler_config` reads the sizes back from the shapes; `convert` returns
(state dict, D_emb, n_q) for such a file.  dim_head is 64 in every published file and is not recorded in the file, so
heads = to_q rows / 64, and the engine asks for dim = heads * 64.  The Resampler's semantics are restated from the
IP-Adapter repository as recalled, not pinned against an installed copy.

FaceID files (an MLP `proj.0.*` or a `perceiver_resampler.*` projection over face-recognition embeddings) are rejected.
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Dict, List, Tuple, Union

import torch

from .config import UNetConfig

PROJ = "encoder_hid_proj.image_projection_layers.0"
_BASE_PROJ_KEYS = {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
DIM_HEAD = 64          # of the Resampler's attention, in every published IP-Adapter Plus file


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


def resampler_manifest(ctx: int, rc: Dict[str, int]) -> "OrderedDict[str, Tuple[int, ...]]":
    """Suffixes (after `image_proj.` / PROJ + ".") and shapes of a Resampler projection for a cross_attention_dim of
    `ctx`, in the engine's order."""
    dim, d_emb, n_q = rc["dim"], rc["image_embed_dim"], rc["num_tokens"]
    inner, hidden = rc["heads"] * DIM_HEAD, rc["ff_mult"] * rc["dim"]
    m = OrderedDict()
    m["latents"] = (1, n_q, dim)
    m["proj_in.weight"] = (dim, d_emb)
    m["proj_in.bias"] = (dim,)
    m["proj_out.weight"] = (ctx, dim)
    m["proj_out.bias"] = (ctx,)
    m["norm_out.weight"] = (ctx,)
    m["norm_out.bias"] = (ctx,)
    for i in range(rc["depth"]):
        for n in ("norm1", "norm2"):
            m[f"layers.{i}.0.{n}.weight"] = (dim,)
            m[f"layers.{i}.0.{n}.bias"] = (dim,)
        m[f"layers.{i}.0.to_q.weight"] = (inner, dim)
        m[f"layers.{i}.0.to_kv.weight"] = (2 * inner, dim)
        m[f"layers.{i}.0.to_out.weight"] = (dim, inner)
        m[f"layers.{i}.1.0.weight"] = (dim,)
        m[f"layers.{i}.1.0.bias"] = (dim,)
        m[f"layers.{i}.1.1.weight"] = (hidden, dim)
        m[f"layers.{i}.1.3.weight"] = (dim, hidden)
    return m


def is_resampler(state_dict: Dict) -> bool:
    """Whether a converted (diffusers-prefixed) adapter state dict carries a Resampler projection."""
    return f"{PROJ}.latents" in state_dict


def resampler_config(state_dict: Dict[str, torch.Tensor], cfg: UNetConfig = None) -> Dict[str, int]:
    """dim, heads, depth, num_tokens (n_q), image_embed_dim (D_emb) and ff_mult of a Resampler projection, read from the
    shapes of its tensors: keys are the original suffixes, bare or under `image_proj.` / PROJ.  Every shape is checked
    against the others (and against cfg.cross_attention_dim when a configuration is given); anything missing, extra or
    inconsistent raises ValueError naming the Resampler."""
    proj = {}
    for k, v in state_dict.items():
        for pre in (PROJ + ".", "image_proj."):
            if k.startswith(pre):
                proj[k[len(pre):]] = v
                break
        else:
            if k.split(".")[0] in ("latents", "proj_in", "proj_out", "norm_out", "layers"):
                proj[k] = v

    def fail(msg):
        raise ValueError(f"IP-Adapter Plus Resampler projection: {msg}")

    for k in ("latents", "proj_in.weight", "layers.0.0.to_q.weight", "layers.0.1.1.weight"):
        if k not in proj:
            fail(f"incomplete, no {k!r}")
    lat, pin, q0, w1 = (proj[k] for k in ("latents", "proj_in.weight", "layers.0.0.to_q.weight", "layers.0.1.1.weight"))
    if lat.ndim != 3 or lat.shape[0] != 1:
        fail(f"latents: expected [1, n_q, dim], got {tuple(lat.shape)}")
    n_q, dim = int(lat.shape[1]), int(lat.shape[2])
    if pin.ndim != 2 or pin.shape[0] != dim:
        fail(f"proj_in.weight: expected [{dim}, D_emb], got {tuple(pin.shape)}")
    if q0.ndim != 2 or q0.shape[0] % DIM_HEAD != 0 or q0.shape[0] == 0:
        fail(f"to_q has {tuple(q0.shape)[0]} rows, not a multiple of dim_head = {DIM_HEAD}")
    if w1.ndim != 2 or w1.shape[0] % dim != 0 or w1.shape[0] == 0:
        fail(f"layers.0.1.1.weight: expected [ff_mult * {dim}, {dim}], got {tuple(w1.shape)}")
    idx = sorted({int(k.split(".")[1]) for k in proj if k.startswith("layers.") and k.split(".")[1].isdigit()})
    if idx != list(range(len(idx))):
        fail(f"layer indices {idx} are not contiguous from 0")
    rc = {"dim": dim, "heads": int(q0.shape[0]) // DIM_HEAD, "depth": len(idx), "num_tokens": n_q,
          "image_embed_dim": int(pin.shape[1]), "ff_mult": int(w1.shape[0]) // dim}
    ctx = cfg.cross_attention_dim if cfg is not None else int(proj["proj_out.weight"].shape[0]) if "proj_out.weight" in proj else 0
    want = resampler_manifest(ctx, rc)
    missing = [k for k in want if k not in proj]
    if missing:
        fail(f"incomplete, {len(missing)} keys missing, e.g. {missing[:3]}")
    extra = [k for k in proj if k not in want]
    if extra:
        fail(f"unexpected keys, e.g. {sorted(extra)[:3]}")
    for k, shp in want.items():
        if tuple(proj[k].shape) != shp:
            hint = " (to_kv must have twice to_q's rows)" if k.endswith("to_kv.weight") else \
                   " (cross_attention_dim of the UNet)" if k.startswith(("proj_out", "norm_out")) else ""
            fail(f"{k}: expected {list(shp)}, got {list(proj[k].shape)}{hint}")
    return rc


def ip_adapter_manifest(cfg: UNetConfig, image_embed_dim: int, num_tokens: int,
                        resampler: Dict[str, int] = None) -> "OrderedDict[str, Tuple[int, ...]]":
    """Diffusers-named keys and shapes the engine's adapter expects, in its order (sd_ip_adapter_weight_info).
    resampler: a resampler_config() for an IP-Adapter Plus projection (None: the base adapters' linear + LayerNorm)."""
    ctx = cfg.cross_attention_dim
    m = OrderedDict()
    if resampler is not None:
        rc = dict(resampler, image_embed_dim=image_embed_dim, num_tokens=num_tokens)
        for k, shp in resampler_manifest(ctx, rc).items():
            m[f"{PROJ}.{k}"] = shp
    else:
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
    UNet configuration.  An IP-Adapter Plus file gives its Resampler keys under PROJ, D_emb and n_q (the other sizes:
    resampler_config of the result).  Raises ValueError (FaceID files, an incomplete or inconsistent Resampler, wrong
    shapes), KeyError (missing / extra keys)."""
    sd = read(path_or_dict)
    proj = {k[len("image_proj."):]: v for k, v in sd.items() if k.startswith("image_proj.")}
    ctx = cfg.cross_attention_dim
    out = OrderedDict()
    if any(k.startswith(("proj.0", "proj.2", "proj.3", "perceiver_resampler")) for k in proj):
        raise ValueError("IP-Adapter FaceID files (an MLP or perceiver_resampler projection of face-recognition embeddings) "
                         "are not supported: the base adapters' linear + LayerNorm and the Plus files' Resampler are")
    if any(k.startswith(("latents", "proj_in", "proj_out", "norm_out", "layers")) for k in proj):
        rc = resampler_config({f"image_proj.{k}": v for k, v in proj.items()}, cfg)
        for k in resampler_manifest(ctx, rc):
            out[f"{PROJ}.{k}"] = proj[k]
        d_img, n_tok = rc["image_embed_dim"], rc["num_tokens"]
    else:
        if set(proj) != _BASE_PROJ_KEYS:
            raise KeyError(f"image_proj: expected keys {sorted(_BASE_PROJ_KEYS)}, got {sorted(proj)}")
        pw, pb = proj["proj.weight"], proj["proj.bias"]
        if tuple(proj["norm.weight"].shape) != (ctx,) or tuple(proj["norm.bias"].shape) != (ctx,):
            raise ValueError(f"image_proj.norm: expected [{ctx}] (cross_attention_dim), got {tuple(proj['norm.weight'].shape)}")
        if pw.ndim != 2 or pw.shape[0] % ctx != 0 or tuple(pb.shape) != (pw.shape[0],):
            raise ValueError(f"image_proj.proj: expected [n_tok * {ctx}, D_img], got {tuple(pw.shape)}")
        n_tok, d_img = pw.shape[0] // ctx, pw.shape[1]
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
