"""Float restatement of the UNet forward with an AnimateDiff motion adapter, for the tests (not a test module).  Built from
oracle.unet_ref's pieces the way deepcache_oracle is; nothing under oracle/ is edited.

Recalled from diffusers 0.27.2 MotionAdapter / UNetMotionModel / TransformerTemporalModel (not pinned, the
library is not installed where this was written).  The UNet's batch is V videos of F consecutive frames.  One motion
module follows every (resnet, transformer) pair of the down and up blocks (the resnet in a block without attention) and,
when the adapter has one, the mid block's transformer, before its second resnet; a skip holds the module's output.

A module on x [V F, C, H, W]: GroupNorm(32, eps 1e-6) with statistics over a group's channels and all F H W positions of
one video, proj_in (Linear), h += to_out(attn(LN1(h) + pe)), h += to_out2(attn(LN2(h) + pe)), h += FF_geglu(LN3(h)),
proj_out, + x; both attentions over the F frames of one pixel, pe the sinusoidal rows of stablediffusion_amd.motion."""
import torch
import torch.nn.functional as F

from cn_oracle import _emb
from deepcache_oracle import _tail
from oracle.unet_ref import _conv, _lin, resnet_block, transformer_2d
from stablediffusion_amd.motion import position_table


def _temporal_attention(h, w, p, heads, pe):
    """h [V HW, F, C]: softmax(q k^T / sqrt(d)) v over the F rows, q / k / v projected from h + pe without bias."""
    B, Fr, C = h.shape
    x = h + pe[:Fr].to(h.dtype)
    d = C // heads
    q, k, v = (_lin(x, w, f"{p}.{n}", bias=False).view(B, Fr, heads, d).transpose(1, 2) for n in ("to_q", "to_k", "to_v"))
    o = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, dim=-1) @ v
    return _lin(o.transpose(1, 2).reshape(B, Fr, C), w, p + ".to_out.0")


def motion_module(x, mw, p, heads, frames, groups=32):
    """One module; mw = the adapter's weights (diffusers names)."""
    N, C, H, W = x.shape
    V = N // frames
    assert V * frames == N
    # [V F, C, H, W] -> [V, C, F, H, W]: the norm's statistics run over a video
    h = x.reshape(V, frames, C, H, W).permute(0, 2, 1, 3, 4)
    h = F.group_norm(h, groups, mw[p + ".norm.weight"], mw[p + ".norm.bias"], 1e-6)
    h = h.permute(0, 3, 4, 2, 1).reshape(V * H * W, frames, C)          # [V HW, F, C]
    h = _lin(h, mw, p + ".proj_in")
    b = p + ".transformer_blocks.0"
    pe = position_table(32, C)
    for n, a in (("norm1", "attn1"), ("norm2", "attn2")):
        y = F.layer_norm(h, (C,), mw[f"{b}.{n}.weight"], mw[f"{b}.{n}.bias"], 1e-5)
        h = h + _temporal_attention(y, mw, f"{b}.{a}", heads, pe)
    y = F.layer_norm(h, (C,), mw[b + ".norm3.weight"], mw[b + ".norm3.bias"], 1e-5)
    hidden, gate = _lin(y, mw, b + ".ff.net.0.proj").chunk(2, dim=-1)
    h = h + _lin(hidden * F.gelu(gate), mw, b + ".ff.net.2")
    h = _lin(h, mw, p + ".proj_out")
    h = h.reshape(V, H, W, frames, C).permute(0, 3, 4, 1, 2).reshape(N, C, H, W)
    return h + x


def forward(cfg, w, mcfg, mw, x, t, ctx, frames, taps=None):
    """The UNet forward on V videos of `frames` frames with the adapter (mcfg, mw).  x [V F, C, H, W], ctx [V F, L, D]
    (a video's text embedding repeated per frame).  taps (a dict): the input of every module, by its prefix."""
    L, nblk = cfg.layers_per_block, len(cfg.block_out_channels)
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    mh = mcfg.motion_num_attention_heads

    def mm(x, p, heads):
        if taps is not None:
            taps[p] = x
        return motion_module(x, mw, p, heads, frames, mcfg.motion_norm_num_groups)

    emb = _emb(cfg, w, x, t, None)
    x = _conv(x, w, "conv_in")
    skips = [x]
    for i in range(nblk):
        for j in range(L):
            x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
            if cfg.down_block_types[i] == "CrossAttnDownBlock2D":
                x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i],
                                   cfg.transformer_layers_per_block[i], lin, g)
            x = mm(x, f"down_blocks.{i}.motion_modules.{j}", mh[i])
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = transformer_2d(x, ctx, w, "mid_block.attentions.0", cfg.attention_head_dim[-1], cfg.transformer_layers_per_block[-1],
                       lin, g)
    if mcfg.use_motion_mid_block:
        x = mm(x, "mid_block.motion_modules.0", mh[-1])
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    for i in range(nblk):
        for j in range(L + 1):
            x = resnet_block(torch.cat([x, skips.pop()], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if cfg.up_block_types[i] == "CrossAttnUpBlock2D":
                x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", list(reversed(cfg.attention_head_dim))[i],
                                   list(reversed(cfg.transformer_layers_per_block))[i], lin, g)
            x = mm(x, f"up_blocks.{i}.motion_modules.{j}", mh[nblk - 1 - i])
        if i != nblk - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv(x, w, f"up_blocks.{i}.upsamplers.0.conv")
    assert not skips
    return _tail(cfg, w, x)
