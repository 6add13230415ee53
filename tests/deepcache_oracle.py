"""fp32 restatement of the UNet forward with DeepCache (Ma, Fang, Wang, CVPR 2024), for the tests (not a test module).
Built from oracle.unet_ref's pieces the way cn_oracle and freeu_oracle are; nothing under oracle/ is edited.

The semantics are the engine's own, stated in the model's wiring (not pinned to the DeepCache package).
With L = layers_per_block, s_0 = conv_in's output and s_j = the output of layer j - 1 of down_blocks.0, layer j of the
last up block reads cat([hidden, s_{L-j}]).  For a depth d in 1..L the cached feature F_d is the hidden input of layer
L - d of the last up block.  The full form computes everything and returns F_d beside the output; the reuse form
(`cached` given) runs conv_in, layers 0..d-1 of down_blocks.0, layers L-d..L of the last up block on cat([F_d, s_d]) and
the tail, and nothing else."""
import torch
import torch.nn.functional as F

from cn_oracle import _emb
from oracle.unet_ref import _conv, resnet_block, transformer_2d


def _down_layer(cfg, w, x, emb, ctx, i, j):
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
    if cfg.down_block_types[i] == "CrossAttnDownBlock2D":
        x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i],
                           cfg.transformer_layers_per_block[i], lin, g)
    return x


def _up_layer(cfg, w, x, skip, emb, ctx, i, j):
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    x = resnet_block(torch.cat([x, skip], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
    if cfg.up_block_types[i] == "CrossAttnUpBlock2D":
        x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", list(reversed(cfg.attention_head_dim))[i],
                           list(reversed(cfg.transformer_layers_per_block))[i], lin, g)
    return x


def _tail(cfg, w, x):
    x = F.group_norm(x, cfg.norm_num_groups, w["conv_norm_out.weight"], w["conv_norm_out.bias"], cfg.norm_eps)
    return _conv(F.silu(x), w, "conv_out")


def forward(cfg, w, x, t, ctx, added, depth, cached=None):
    """(out, F_depth).  `cached` None: the full forward (out equals oracle.unet_ref.unet_forward's bit for bit).
    `cached` = an F_depth: the reuse forward on it, which returns the same tensor as its second value."""
    L, nblk = cfg.layers_per_block, len(cfg.block_out_channels)
    assert 1 <= depth <= L
    emb = _emb(cfg, w, x, t, added)
    x = _conv(x, w, "conv_in")
    skips = [x]
    if cached is not None:
        for j in range(depth):
            x = _down_layer(cfg, w, x, emb, ctx, 0, j)
            skips.append(x)
        x = cached
        for j in range(L - depth, L + 1):
            x = _up_layer(cfg, w, x, skips.pop(), emb, ctx, nblk - 1, j)
        assert not skips
        return _tail(cfg, w, x), cached
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    for i in range(nblk):
        for j in range(L):
            x = _down_layer(cfg, w, x, emb, ctx, i, j)
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = transformer_2d(x, ctx, w, "mid_block.attentions.0", cfg.attention_head_dim[-1],
                       cfg.transformer_layers_per_block[-1], lin, g)
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    feat = None
    for i in range(nblk):
        for j in range(L + 1):
            if i == nblk - 1 and j == L - depth:
                feat = x
            x = _up_layer(cfg, w, x, skips.pop(), emb, ctx, i, j)
        if i != nblk - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv(x, w, f"up_blocks.{i}.upsamplers.0.conv")
    return _tail(cfg, w, x), feat
