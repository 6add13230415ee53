"""fp32 restatement of diffusers 0.27.2's ControlNetModel.forward and of UNet2DConditionModel.forward with
down_block_additional_residuals / mid_block_additional_residual, for the tests (not a test module).  Built from
oracle.unet_ref's pieces; nothing under oracle/ is edited."""
import torch
import torch.nn.functional as F

from oracle.unet_ref import _conv, _lin, resnet_block, timestep_sinusoid, transformer_2d
from stablediffusion_amd import controlnet


COND = controlnet.COND


def synth_cn_state_dict(cfg, seed=0, zero_scale=1.0):
    """Random ControlNet weights in diffusers naming, fp16-rounded.  The zero convs are NOT zero (a trained
    ControlNet's are not): scaled like trained 1x1 convs times `zero_scale`."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in controlnet.controlnet_manifest(cfg).items():
        if k.endswith("norm.weight") or ".norm1.weight" in k or ".norm2.weight" in k or ".norm3.weight" in k:
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            t = 0.05 * torch.randn(shp, generator=g)
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            t = torch.randn(shp, generator=g) / fan_in ** 0.5
            if k.startswith(("controlnet_down_blocks", "controlnet_mid_block")):
                t = t * zero_scale
        sd[k] = t.half().float()
    return sd


def cond_embedding(w, image):
    """ControlNetConditioningEmbedding: conv_in + SiLU, six 3x3 blocks (every second one stride 2) + SiLU, conv_out."""
    x = F.silu(_conv(image, w, f"{COND}.conv_in"))
    for i in range(6):
        x = F.silu(_conv(x, w, f"{COND}.blocks.{i}", stride=2 if i % 2 else 1))
    return _conv(x, w, f"{COND}.conv_out")


def _emb(cfg, w, sample, timestep, added_cond_kwargs):
    B = sample.shape[0]
    t = torch.as_tensor(timestep)
    if t.ndim == 0:
        t = t[None]
    t = t.expand(B)
    boc = cfg.block_out_channels
    t_emb = timestep_sinusoid(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(sample.dtype)
    emb = _lin(F.silu(_lin(t_emb, w, "time_embedding.linear_1")), w, "time_embedding.linear_2")
    if cfg.addition_embed_type == "text_time":
        te = timestep_sinusoid(added_cond_kwargs["time_ids"].flatten(), cfg.addition_time_embed_dim,
                               cfg.flip_sin_to_cos, cfg.freq_shift).reshape(B, -1).to(sample.dtype)
        add = torch.cat([added_cond_kwargs["text_embeds"].to(sample.dtype), te], dim=-1)
        emb = emb + _lin(F.silu(_lin(add, w, "add_embedding.linear_1")), w, "add_embedding.linear_2")
    return emb


def _encoder(cfg, w, x, emb, ctx):
    """down path + mid block from conv_in's output x: (skips, mid)."""
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    skips = [x]
    nblk = len(cfg.block_out_channels)
    for i, btype in enumerate(cfg.down_block_types):
        for j in range(cfg.layers_per_block):
            x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnDownBlock2D":
                x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}",
                                   cfg.attention_head_dim[i], cfg.transformer_layers_per_block[i], lin, g)
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = transformer_2d(x, ctx, w, "mid_block.attentions.0", cfg.attention_head_dim[-1],
                       cfg.transformer_layers_per_block[-1], lin, g)
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    return skips, x


def controlnet_forward(cfg, w, sample, timestep, ehs, cond_image, scale, added_cond_kwargs=None):
    """ControlNetModel.forward (guess_mode False): the scaled down-block residuals and the scaled mid residual.
    cond_image [n, 3, 8h, 8w] with n dividing the batch: sample b uses image b mod n."""
    B = sample.shape[0]
    img = cond_image.float().repeat(B // cond_image.shape[0], 1, 1, 1)
    emb = _emb(cfg, w, sample, timestep, added_cond_kwargs)
    x = _conv(sample, w, "conv_in") + cond_embedding(w, img)
    skips, mid = _encoder(cfg, w, x, emb, ehs)
    down = [_conv(s, w, f"controlnet_down_blocks.{i}", padding=0) * scale for i, s in enumerate(skips)]
    return down, _conv(mid, w, "controlnet_mid_block", padding=0) * scale


def unet_forward_res(cfg, w, sample, timestep, ehs, added_cond_kwargs=None, down_res=None, mid_res=None):
    """UNet2DConditionModel.forward with down_block_additional_residuals / mid_block_additional_residual."""
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
            x = torch.cat([x, skips.pop()], dim=1)
            x = resnet_block(x, emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnUpBlock2D":
                x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g)
        if i != nblk - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv(x, w, f"up_blocks.{i}.upsamplers.0.conv")
    x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
    return _conv(F.silu(x), w, "conv_out")


def unet_cn_forward(ucfg, usd, ccfg, csd, sample, timestep, ehs, cond_image, scale, added_cond_kwargs=None,
                    unet_ctx=None):
    """The pipeline's composition: ControlNet residuals into the UNet.  unet_ctx: the UNet's cross-attention context
    when it differs from the ControlNet's (the IP-Adapter's (text, image tokens) tuple); the ControlNet sees ehs."""
    down, mid = controlnet_forward(ccfg, csd, sample.float(), timestep, ehs.float(), cond_image, scale, added_cond_kwargs)
    return unet_forward_res(ucfg, usd, sample.float(), timestep, unet_ctx if unet_ctx is not None else ehs.float(),
                            added_cond_kwargs, down, mid)
