"""fp32 restatement of perturbed-attention guidance (Ahn et al. 2024; diffusers >= 0.30 PAGIdentitySelfAttnProcessor2_0 and
StableDiffusionPAGPipeline) for the tests (not a test module).  Built from oracle.unet_ref's pieces the way freeu_oracle /
cn_oracle are; nothing under oracle/ is edited.  Recalled, not pinned: diffusers is not installed where this was written
(DESIGN.md section 8).

The forward takes the whole batch [uncond ; text ; perturbed] (or [text ; perturbed]) as a caller would hand it to
diffusers: the last `n_pert` images are the perturbed group, and in every BasicTransformerBlock of a transformer named in
`sites` (the engine's site keys) their attn1 is to_out(to_v(norm1(x))) -- the identity attention map."""
import torch
import torch.nn.functional as F

from cn_oracle import _emb
from freeu_oracle import apply_freeu
from oracle.unet_ref import _conv, _lin, attention, resnet_block


def _block(x, ctx, w, p, heads, n_pert):
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm1.weight"], w[p + ".norm1.bias"], 1e-5)
    if n_pert:
        nq = x.shape[0] - n_pert
        a = attention(h[:nq], h[:nq], w, p + ".attn1", heads)
        ident = _lin(_lin(h[nq:], w, p + ".attn1.to_v", False), w, p + ".attn1.to_out.0")
        x = x + torch.cat([a, ident])
    else:
        x = x + attention(h, h, w, p + ".attn1", heads)
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm2.weight"], w[p + ".norm2.bias"], 1e-5)
    x = x + attention(h, ctx, w, p + ".attn2", heads)
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm3.weight"], w[p + ".norm3.bias"], 1e-5)
    hidden, gate = _lin(h, w, p + ".ff.net.0.proj").chunk(2, dim=-1)
    return x + _lin(hidden * F.gelu(gate), w, p + ".ff.net.2")


def _transformer(x, ctx, w, p, heads, depth, linear, groups, n_pert):
    B, C, H, W = x.shape
    h = F.group_norm(x, groups, w[p + ".norm.weight"], w[p + ".norm.bias"], 1e-6)
    if not linear:
        h = _conv(h, w, p + ".proj_in", padding=0).permute(0, 2, 3, 1).reshape(B, H * W, C)
    else:
        h = _lin(h.permute(0, 2, 3, 1).reshape(B, H * W, C), w, p + ".proj_in")
    for d in range(depth):
        h = _block(h, ctx, w, f"{p}.transformer_blocks.{d}", heads, n_pert)
    if not linear:
        h = _conv(h.reshape(B, H, W, C).permute(0, 3, 1, 2), w, p + ".proj_out", padding=0)
    else:
        h = _lin(h, w, p + ".proj_out").reshape(B, H, W, C).permute(0, 3, 1, 2)
    return h + x


def unet_forward(cfg, w, sample, timestep, ehs, sites, n_pert, added_cond_kwargs=None, freeu=None):
    """UNet2DConditionModel.forward on the whole batch; the last n_pert images perturbed in the transformers `sites`."""
    sites = set(sites)
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    nblk = len(cfg.block_out_channels)

    def xf(x, p, heads, depth):
        return _transformer(x, ehs, w, p, heads, depth, lin, g, n_pert if p in sites else 0)

    emb = _emb(cfg, w, sample, timestep, added_cond_kwargs)
    x = _conv(sample, w, "conv_in")
    skips = [x]
    for i, btype in enumerate(cfg.down_block_types):
        for j in range(cfg.layers_per_block):
            x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnDownBlock2D":
                x = xf(x, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i], cfg.transformer_layers_per_block[i])
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = xf(x, "mid_block.attentions.0", cfg.attention_head_dim[-1], cfg.transformer_layers_per_block[-1])
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    rev_heads = list(reversed(cfg.attention_head_dim))
    rev_depth = list(reversed(cfg.transformer_layers_per_block))
    for i, btype in enumerate(cfg.up_block_types):
        for j in range(cfg.layers_per_block + 1):
            x, skip = apply_freeu(i, x, skips.pop(), freeu)
            x = resnet_block(torch.cat([x, skip], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnUpBlock2D":
                x = xf(x, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i])
        if i != nblk - 1:
            x = _conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, f"up_blocks.{i}.upsamplers.0.conv")
    x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
    return _conv(F.silu(x), w, "conv_out")


def pag_batch(x, ehs, cfg_on, added_cond_kwargs=None):
    """(sample, ehs, added) of the whole batch from B latents and the G B rows of the un-perturbed groups."""
    B = x.shape[0]
    G = 2 if cfg_on else 1
    dup = lambda v: torch.cat([v, v[(G - 1) * B:]])
    added = None if added_cond_kwargs is None else {k: dup(v) for k, v in added_cond_kwargs.items()}
    return torch.cat([x] * (G + 1)), dup(ehs), added


def forward_pag(cfg, w, x, timestep, ehs, sites, cfg_on, added_cond_kwargs=None, freeu=None):
    """What HipUNet2DConditionModel.forward_pag computes, in the dtype of x (already scaled): [(G + 1) B, ...]."""
    sample, ehs3, added = pag_batch(x, ehs, cfg_on, added_cond_kwargs)
    return unet_forward(cfg, w, sample, timestep, ehs3, sites, x.shape[0], added, freeu)


def pag_combine(model_out, rows, g, s):
    """float64: u + g (t - u) + s (t - p) of rows [u ; t ; p], t + s (t - p) of rows [t ; p]."""
    m = model_out.double().reshape(rows, -1)
    if rows == 3:
        u, t, p = m
        return u + g * (t - u) + s * (t - p)
    t, p = m
    return t + s * (t - p)


def linear_step(e, x, hist, c_x, c_eps, c_hist, h_x, h_eps):
    """float64: sd_cfg_linear_step's update on the guided prediction e -> (new x, new hist or None)."""
    e, x = e.double().reshape(-1), x.double().reshape(-1)
    out = c_x * x + c_eps * e
    if hist is None:
        return out, None
    return out + c_hist * hist.double().reshape(-1), h_x * x + h_eps * e
