"""Regional prompts ("attention couple"): this prompt here, that prompt there, in one UNet forward.

Region 0 is the call's own prompt; regions 1..R-1 each have a prompt and a mask in [0, 1].  Only `attn2` changes: a
latent pixel's cross-attention output is the weighted sum of separate cross-attentions against each region's prompt,

    out[n, t] = sum_r W_l[n, t, r] softmax(s q[n, t] K[n, rL:(r+1)L]^T) V[n, rL:(r+1)L]

with the R prompts riding in one encoder_hidden_states of R L tokens (the engine's region_xattn_kernel, one launch per
attn2).  The semantics are this project's own (the form is not in diffusers 0.27.2):

  m_r = clamp(interpolate(mask_r, (h, w), "nearest"), 0, 1)             r >= 1, at the latent size
  m_0 = clamp(1 - sum_{r>=1} m_r, 0, 1) + base_weight                  base_weight >= 0
  w_r = m_r / sum_r m_r                                                (the denominator is at least 1)

and a transformer on an (h / 2^l, w / 2^l) map reads the 2x2 mean of the level above, l times over.  Under CFG the
uncond rows weigh region 0 alone; their other segments repeat the negative embedding and are never attended.
This module holds the host side: the weights, the argument checks of the pipeline call and the token layout."""
from __future__ import annotations

import torch
import torch.nn.functional as F

MAX_REGIONS = 8


def region_weights(masks: torch.Tensor, h: int, w: int, base_weight: float = 0.0) -> torch.Tensor:
    """masks [R-1, H, W] or [R-1, 1, H, W] in any float / bool dtype -> weights [R, h, w] fp32 that sum to 1 per pixel."""
    if not isinstance(masks, torch.Tensor) or masks.ndim not in (3, 4) or (masks.ndim == 4 and masks.shape[1] != 1):
        raise ValueError("region_masks: expected a tensor [R-1, H, W] or [R-1, 1, H, W]")
    if masks.shape[0] < 1 or masks.shape[0] > MAX_REGIONS - 1:
        raise ValueError(f"region_masks: between 1 and {MAX_REGIONS - 1} regions besides the base prompt, got {masks.shape[0]}")
    base_weight = float(base_weight)
    if not base_weight >= 0.0 or base_weight == float("inf"):
        raise ValueError(f"region_base_weight must be finite and >= 0, got {base_weight}")
    m = masks.to(torch.float32).reshape(masks.shape[0], 1, masks.shape[-2], masks.shape[-1])
    m = F.interpolate(m, size=(int(h), int(w)), mode="nearest")[:, 0].clamp(0.0, 1.0)
    m0 = (1.0 - m.sum(0, keepdim=True)).clamp(0.0, 1.0) + base_weight
    m = torch.cat([m0, m], dim=0)
    return m / m.sum(0, keepdim=True)


def level_weights(weights: torch.Tensor, level: int) -> torch.Tensor:
    """[..., h, w] -> the weights a transformer `level` halvings down reads: the 2x2 mean, `level` times over (what the
    engine's region_pyramid_kernel writes, there as [Bw, T_l, R])."""
    for _ in range(int(level)):
        weights = F.avg_pool2d(weights, 2)
    return weights


def batch_weights(weights: torch.Tensor, batch: int, cfg: bool) -> torch.Tensor:
    """[R, h, w] -> the forward's [2 batch, R, h, w] (CFG: the uncond rows, first, one-hot on region 0) or [batch, ...]."""
    pos = weights[None].expand(batch, *weights.shape)
    if not cfg:
        return pos.contiguous()
    neg = torch.zeros_like(pos)
    neg[:, 0] = 1.0
    return torch.cat([neg, pos], dim=0).contiguous()


def join_embeds(base: torch.Tensor, regions, negative=None) -> tuple:
    """base [B, L, D] and R-1 region embeddings [B, L, D] -> positive [B, R L, D]; negative [B, L, D] -> [B, R L, D]
    (repeated per segment) or None."""
    for e in regions:
        if tuple(e.shape) != tuple(base.shape):
            raise ValueError(f"region prompt embeddings must match the prompt's {tuple(base.shape)}, got {tuple(e.shape)}")
    pos = torch.cat([base] + [e.to(base.device, base.dtype) for e in regions], dim=1)
    neg = None if negative is None else torch.cat([negative] * (len(regions) + 1), dim=1)
    return pos, neg


def masks_tensor(model, region_masks, height: int, width: int) -> torch.Tensor:
    """region_masks as given (a tensor, a PIL image or a list of PIL images / arrays) -> [R-1, H, W] fp32."""
    if isinstance(region_masks, torch.Tensor):
        return region_masks
    items = list(region_masks) if isinstance(region_masks, (list, tuple)) else [region_masks]
    out = [model.mask_processor.preprocess(m, height=height, width=width).to(torch.float32) for m in items]
    return torch.cat([m.reshape(-1, m.shape[-2], m.shape[-1])[:1] for m in out], dim=0)


def _count(region_masks) -> int:
    if isinstance(region_masks, torch.Tensor):
        return int(region_masks.shape[0]) if region_masks.ndim >= 3 else -1
    return len(region_masks) if isinstance(region_masks, (list, tuple)) else 1


def check_call(prompts, masks, embeds, base_weight, prompt_embeds) -> int:
    """The pipeline call's regional arguments, checked before anything runs; returns R.  (What regional prompts do not
    run with: combos.REFUSALS.)"""
    if masks is None or (prompts is None and embeds is None):
        raise ValueError("regional prompts need region_masks and region_prompts (or region_prompt_embeds)")
    if isinstance(prompts, str):
        raise ValueError("region_prompts is a list: one prompt (or one list of per-image prompts) per region")
    n = len(prompts) if prompts is not None else len(embeds)
    if n > MAX_REGIONS - 1:
        raise ValueError(f"at most {MAX_REGIONS - 1} region prompts ({MAX_REGIONS} regions with the base prompt), got {n}")
    if n < 1:
        raise ValueError("region_prompts is empty")
    nm = _count(masks)
    if nm != n:
        raise ValueError(f"{n} region prompts but {nm} region masks")
    if isinstance(masks, torch.Tensor) and (masks.ndim not in (3, 4) or (masks.ndim == 4 and masks.shape[1] != 1)):
        raise ValueError("region_masks: expected a tensor [R-1, H, W] or [R-1, 1, H, W]")
    bw = float(base_weight)
    if not bw >= 0.0 or bw == float("inf"):
        raise ValueError(f"region_base_weight must be finite and >= 0, got {bw}")
    if prompt_embeds is not None and embeds is None:
        raise NotImplementedError("prompt_embeds= with regional prompts needs region_prompt_embeds= (one [B, L, D] per region)")
    if prompt_embeds is None and embeds is not None:
        raise NotImplementedError("region_prompt_embeds= goes with prompt_embeds= (region_prompts= with prompt=)")
    return n + 1
