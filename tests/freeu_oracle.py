"""fp32 restatement of diffusers 0.27.2's FreeU (utils/torch_utils.py `fourier_filter` / `apply_freeu`, called by the
first two up blocks of UNet2DConditionModel when `enable_freeu` was called), for the tests (not a test module).  Built
from oracle.unet_ref's pieces the way cn_oracle is; nothing under oracle/ is edited.  Recalled, not pinned: diffusers is
not installed where this was written."""
import math

import torch
import torch.nn.functional as F

from cn_oracle import _emb, _encoder
from oracle.unet_ref import _conv, resnet_block, transformer_2d


def fourier_filter(x, threshold=1, scale=1.0):
    """fourier_filter: the centre box of the shifted spectrum over (H, W) times `scale`, back, real part.  x [B,C,H,W];
    computed in the dtype of x (fp32 or fp64)."""
    B, C, H, W = x.shape
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    xf = xf * mask
    return torch.fft.ifftn(torch.fft.ifftshift(xf, dim=(-2, -1)), dim=(-2, -1)).real


def closed_form_filter(x, scale):
    """The same filter without a transform (the form the engine's kernel computes), in the dtype of x:
    y = x + (s-1)/(HW) sum x' [(1 + cos t)(1 + cos f) - sin t sin f]; an axis of length 1 contributes the factor 1."""
    B, C, H, W = x.shape
    dh = torch.arange(H, dtype=x.dtype)[:, None] - torch.arange(H, dtype=x.dtype)[None, :]        # h - h'
    dw = torch.arange(W, dtype=x.dtype)[:, None] - torch.arange(W, dtype=x.dtype)[None, :]
    th, ph = 2 * math.pi * dh / H, 2 * math.pi * dw / W
    ch, sh = (1 + torch.cos(th), torch.sin(th)) if H > 1 else (torch.ones_like(th), torch.zeros_like(th))
    cw, sw = (1 + torch.cos(ph), torch.sin(ph)) if W > 1 else (torch.ones_like(ph), torch.zeros_like(ph))
    corr = torch.einsum("bcij,hi,wj->bchw", x, ch, cw) - torch.einsum("bcij,hi,wj->bchw", x, sh, sw)
    return x + (scale - 1.0) / (H * W) * corr


def apply_freeu(resolution_idx, hidden, skip, freeu):
    """apply_freeu: freeu = (s1, s2, b1, b2); up block 0 uses (b1, s1), up block 1 (b2, s2), later blocks nothing."""
    if freeu is None or resolution_idx > 1:
        return hidden, skip
    s1, s2, b1, b2 = freeu
    b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
    half = hidden.shape[1] // 2
    hidden = torch.cat([hidden[:, :half] * b, hidden[:, half:]], dim=1)
    return hidden, fourier_filter(skip, threshold=1, scale=s)


def unet_forward(cfg, w, sample, timestep, ehs, added_cond_kwargs=None, freeu=None, down_res=None, mid_res=None):
    """UNet2DConditionModel.forward with FreeU (freeu = (s1, s2, b1, b2) or None) and optional ControlNet residuals,
    which are added to the skips before FreeU sees them."""
    emb = _emb(cfg, w, sample, timestep, added_cond_kwargs)
    ctx = ehs
    skips, x = _encoder(cfg, w, _conv(sample, w, "conv_in"), emb, ctx)
    if down_res is not None:
        skips = [s + r for s, r in zip(skips, down_res)]
    if mid_res is not None:
        x = x + mid_res
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    nblk = len(cfg.block_out_channels)
    rev_heads = list(reversed(cfg.attention_head_dim))
    rev_depth = list(reversed(cfg.transformer_layers_per_block))
    for i, btype in enumerate(cfg.up_block_types):
        for j in range(cfg.layers_per_block + 1):
            x, skip = apply_freeu(i, x, skips.pop(), freeu)
            x = torch.cat([x, skip], dim=1)
            x = resnet_block(x, emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnUpBlock2D":
                x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g)
        if i != nblk - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv(x, w, f"up_blocks.{i}.upsamplers.0.conv")
    x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
    return _conv(F.silu(x), w, "conv_out")


def freeu_cat(cat_nhwc, C1, b, s):
    """The operator on one concatenation [N, H, W, C1 + C2] (any float dtype): its fp32 result, NHWC."""
    x = cat_nhwc.float().permute(0, 3, 1, 2)
    hidden, skip = apply_freeu(0, x[:, :C1], x[:, C1:], (s, s, b, b))
    return torch.cat([hidden, skip], dim=1).permute(0, 2, 3, 1).contiguous()
