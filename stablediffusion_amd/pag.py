"""Perturbed-attention guidance (Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance",
2024) -- the host side: layer names, the per-step scale and the combine.

Semantics as in diffusers >= 0.30 (`StableDiffusionPAGPipeline`), recalled: diffusers is not installed here, so nothing
below is pinned against it.

  * batch order [uncond ; text ; perturbed] with CFG, [text ; perturbed] without; the perturbed group takes the text
    group's latents, timestep, prompt embeddings and added conditions;
  * in every BasicTransformerBlock of a selected Transformer2DModel, attn1 of the perturbed images is
    to_out(to_v(norm1(x))): an identity attention map;
  * eps = u + g (t - u) + s (t - p) with CFG, t + s (t - p) without;
  * s = max(0, pag_scale - pag_adaptive_scale * (1000 - timestep)).
"""
from __future__ import annotations

import re
from typing import Iterable, List, Sequence, Tuple, Union

DEFAULT_LAYERS = ("mid",)

_NAME = re.compile(r"^(down|up|mid)(?:\.block_(\d+))?(?:\.attentions_(\d+))?$")


def transformer_sites(cfg) -> List[str]:
    """The engine's site key of every Transformer2DModel of a UNet topology, in execution order (down, mid, up)."""
    keys = []
    nb = len(cfg.block_out_channels)
    for i, kind in enumerate(cfg.down_block_types):
        if kind == "CrossAttnDownBlock2D" and cfg.transformer_layers_per_block[i] > 0:
            keys += [f"down_blocks.{i}.attentions.{j}" for j in range(cfg.layers_per_block)]
    if cfg.transformer_layers_per_block[nb - 1] > 0:
        keys.append("mid_block.attentions.0")
    for i, kind in enumerate(cfg.up_block_types):
        if kind == "CrossAttnUpBlock2D" and cfg.transformer_layers_per_block[nb - 1 - i] > 0:
            keys += [f"up_blocks.{i}.attentions.{j}" for j in range(cfg.layers_per_block + 1)]
    return keys


def site_keys(cfg, layers: Union[str, Iterable[str]]) -> Tuple[str, ...]:
    """`pag_applied_layers` in diffusers' spellings -- "mid", "down.block_2", "down.block_2.attentions_1", "up.block_1",
    "up.block_1.attentions_0", or a list of them -- as the engine's site keys, in execution order and without
    repetitions.  A name that selects no transformer of this topology is a ValueError."""
    if isinstance(layers, str):
        layers = (layers,)
    layers = tuple(layers)
    if not layers:
        raise ValueError("pag_applied_layers is empty")
    sites = transformer_sites(cfg)
    picked = set()
    for name in layers:
        m = _NAME.match(name) if isinstance(name, str) else None
        if m is None:
            raise ValueError(f"pag_applied_layers: cannot parse {name!r} (expected 'mid', 'down.block_I', "
                             "'up.block_I' or one of those with '.attentions_J')")
        where, blk, att = m.group(1), m.group(2), m.group(3)
        if where == "mid":
            if (blk is not None and int(blk) != 0) or (att is not None and int(att) != 0):
                hit = []
            else:
                hit = [k for k in sites if k.startswith("mid_block.")]
        else:
            if blk is None:
                if att is not None:
                    raise ValueError(f"pag_applied_layers: {name!r} names an attention without its block")
                prefix = f"{where}_blocks."
                hit = [k for k in sites if k.startswith(prefix)]
            else:
                prefix = f"{where}_blocks.{int(blk)}.attentions."
                hit = [k for k in sites if k.startswith(prefix) and (att is None or k == prefix + str(int(att)))]
        if not hit:
            raise ValueError(f"pag_applied_layers: {name!r} selects no transformer of this UNet "
                             f"(its transformers: {', '.join(sites)})")
        picked.update(hit)
    return tuple(k for k in sites if k in picked)


def step_scale(pag_scale: float, pag_adaptive_scale: float, timestep: float) -> float:
    """The scale of one step: max(0, pag_scale - pag_adaptive_scale * (1000 - timestep))."""
    return max(0.0, float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(timestep)))


def combine(noise_pred, guidance_scale: float, s: float, do_cfg: bool):
    """The guided prediction from a model output in PAG's batch order (any tensor library's chunk / arithmetic)."""
    if do_cfg:
        u, t, p = noise_pred.chunk(3)
        return u + guidance_scale * (t - u) + s * (t - p)
    t, p = noise_pred.chunk(2)
    return t + s * (t - p)
