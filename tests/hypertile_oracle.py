"""float64 restatement of HyperTile for the tests (not a test module): the division rule as include/sd_engine.h states it
(recalled from tfernd/HyperTile, not pinned), the tiled attention, and the UNet forward with tiled attn1,
built from oracle.unet_ref's pieces the way tome_oracle is.

One BasicTransformerBlock on an Hs x Ws map that draws nh x nw: q, k, v are rearranged "b (nh th nw tw) c ->
(b nh nw) (th tw) c", attention runs per tile, the output goes back through the inverse.  A forward takes its divisions
from the rule or from outside (`divisions`: site -> (nh, nw), what the engine reported)."""
import torch
import torch.nn.functional as F

from cn_oracle import _emb
from oracle.unet_ref import _conv, _lin, resnet_block
from tome_oracle import _heads, _xattn, mix32, site_table


def counts(n, tile_size, swap_size):
    m = min(tile_size, n)
    extents = [e for e in range(m, n + 1) if n % e == 0][:swap_size]
    return [n // e for e in extents]


def plan(Hs, Ws, tile_size, swap_size, seed, step, site):
    """(nh, nw, th, tw)."""
    ch, cw = counts(Hs, tile_size, swap_size), counts(Ws, tile_size, swap_size)
    nh = ch[mix32(seed, step, site, 0) % len(ch)]
    nw = cw[mix32(seed, step, site, 1) % len(cw)]
    return nh, nw, Hs // nh, Ws // nw


def to_tiles(t, Hs, Ws, nh, nw):
    """[B, Hs Ws, C] raster order -> [B nh nw, th tw, C]."""
    B, T, C = t.shape
    th, tw = Hs // nh, Ws // nw
    return t.view(B, nh, th, nw, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nh * nw, th * tw, C)


def from_tiles(t, Hs, Ws, nh, nw):
    """The inverse of to_tiles."""
    C = t.shape[-1]
    th, tw = Hs // nh, Ws // nw
    B = t.shape[0] // (nh * nw)
    return t.view(B, nh, nw, th, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hs * Ws, C)


def tiled_attention(q, k, v, heads, Hs, Ws, nh, nw):
    """softmax(q k^T / sqrt(d)) v within each tile; q, k, v [B, Hs Ws, heads d] -> [B, Hs Ws, heads d], in q's dtype
    (float64 for the reference)."""
    qt, kt, vt = (to_tiles(t, Hs, Ws, nh, nw) for t in (q, k, v))
    o = F.scaled_dot_product_attention(_heads(qt, heads), _heads(kt, heads), _heads(vt, heads))
    o = o.transpose(1, 2).reshape(qt.shape)
    return from_tiles(o, Hs, Ws, nh, nw)


class HyperTile:
    """Settings and state of one forward: which sites take part and the division each used (given or drawn)."""

    def __init__(self, tile_size, swap_size=2, max_depth=0, seed=0, step=0, divisions=None):
        self.tile_size, self.swap_size, self.max_depth, self.seed, self.step = tile_size, swap_size, max_depth, seed, step
        self.divisions = divisions      # site -> (nh, nw) (None: drawn here)
        self.site = 0
        self.sites = None               # transformer prefix -> first ordinal (a forward that skips blocks)
        self.sample_h = None
        self.used = {}                  # site -> (Hs, Ws, nh, nw, level)

    def division(self, Hs, Ws):
        """(nh, nw) of the block about to run ((1, 1): plain); advances the site counter."""
        site = self.site
        self.site += 1
        level = (self.sample_h // Hs).bit_length() - 1
        if self.tile_size <= 0 or level > self.max_depth:
            return 1, 1
        if self.divisions is not None:
            nh, nw = self.divisions[site]
        else:
            nh, nw = plan(Hs, Ws, self.tile_size, self.swap_size, self.seed, self.step, site)[:2]
        self.used[site] = (Hs, Ws, nh, nw, level)
        return nh, nw


def block(x, ctx, w, p, heads, Hs, Ws, ht):
    nh, nw = ht.division(Hs, Ws)
    C = x.shape[-1]
    h = F.layer_norm(x, (C,), w[p + ".norm1.weight"], w[p + ".norm1.bias"], 1e-5)
    q, k, v = (_lin(h, w, p + ".attn1" + n, False) for n in (".to_q", ".to_k", ".to_v"))
    x = x + _lin(tiled_attention(q, k, v, heads, Hs, Ws, nh, nw), w, p + ".attn1.to_out.0")
    h = F.layer_norm(x, (C,), w[p + ".norm2.weight"], w[p + ".norm2.bias"], 1e-5)
    x = x + _xattn(h, ctx, w, p + ".attn2", heads)
    h = F.layer_norm(x, (C,), w[p + ".norm3.weight"], w[p + ".norm3.bias"], 1e-5)
    hidden, gate = _lin(h, w, p + ".ff.net.0.proj").chunk(2, dim=-1)
    return x + _lin(hidden * F.gelu(gate), w, p + ".ff.net.2")


def transformer_2d(x, ctx, w, p, heads, depth, linear, groups, ht):
    B, C, H, W = x.shape
    ht.site = ht.sites[p]               # (a forward that skips blocks keeps the full forward's ordinals)
    res = x
    h = F.group_norm(x, groups, w[p + ".norm.weight"], w[p + ".norm.bias"], 1e-6)
    if not linear:
        h = _conv(h, w, p + ".proj_in", padding=0).permute(0, 2, 3, 1).reshape(B, H * W, C)
    else:
        h = _lin(h.permute(0, 2, 3, 1).reshape(B, H * W, C), w, p + ".proj_in")
    for d in range(depth):
        h = block(h, ctx, w, f"{p}.transformer_blocks.{d}", heads, H, W, ht)
    if not linear:
        h = _conv(h.reshape(B, H, W, C).permute(0, 3, 1, 2), w, p + ".proj_out", padding=0)
    else:
        h = _lin(h, w, p + ".proj_out").reshape(B, H, W, C).permute(0, 3, 1, 2)
    return h + res


def deepcache_forward(cfg, w, x, t, ctx, added, depth, ht, cached=None):
    """deepcache_oracle.forward with every BasicTransformerBlock going through `ht` (a HyperTile): (out, F_depth).  A
    block keeps the ordinal it has in the full forward, so a reuse step (`cached` given) draws what a store step would."""
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    L, nblk = cfg.layers_per_block, len(cfg.block_out_channels)
    ht.sites, ht.sample_h, ht.used = site_table(cfg), x.shape[2], {}
    rev_heads, rev_depth = list(reversed(cfg.attention_head_dim)), list(reversed(cfg.transformer_layers_per_block))

    def down(x, i, j):
        x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
        if cfg.down_block_types[i] == "CrossAttnDownBlock2D":
            x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i],
                               cfg.transformer_layers_per_block[i], lin, g, ht)
        return x

    def up(x, skip, i, j):
        x = resnet_block(torch.cat([x, skip], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
        if cfg.up_block_types[i] == "CrossAttnUpBlock2D":
            x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g, ht)
        return x

    def tail(x):
        x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
        return _conv(F.silu(x), w, "conv_out")

    emb = _emb(cfg, w, x, t, added)
    x = _conv(x, w, "conv_in")
    skips = [x]
    if cached is not None:
        for j in range(depth):
            x = down(x, 0, j)
            skips.append(x)
        x = cached
        for j in range(L - depth, L + 1):
            x = up(x, skips.pop(), nblk - 1, j)
        return tail(x), cached
    for i in range(nblk):
        for j in range(L):
            x = down(x, i, j)
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = transformer_2d(x, ctx, w, "mid_block.attentions.0", cfg.attention_head_dim[-1],
                       cfg.transformer_layers_per_block[-1], lin, g, ht)
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    feat = None
    for i in range(nblk):
        for j in range(L + 1):
            if i == nblk - 1 and j == L - depth:
                feat = x
            x = up(x, skips.pop(), i, j)
        if i != nblk - 1:
            x = _conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, f"up_blocks.{i}.upsamplers.0.conv")
    return tail(x), feat


def unet_forward(cfg, w, x, t, ctx, added, ht):
    """oracle.unet_ref.unet_forward with every BasicTransformerBlock going through `ht` (a HyperTile)."""
    return deepcache_forward(cfg, w, x, t, ctx, added, 1, ht)[0]
