"""float64 restatement of token merging for the tests (not a test module): tomesd 0.1.3's
bipartite_soft_matching_random2d as the engine states it (recalled, not pinned; include/sd_engine.h,
sd_op_tome_match), and the UNet forward with it, built from oracle.unet_ref's pieces the way deepcache_oracle is.

One BasicTransformerBlock on an H x W map: the tokens are matched on the block's input x (the residual stream norm1
reads), attn1 runs on the merged sequence and its output is unmerged:  x + u(attn1(m(norm1(x)))), tomesd's order
("pre": merge norm1(x), then project), or the engine's ("post": project every row, merge q / k / v).  The two agree to
rounding because the projections are linear.  A forward can take its maps from outside (`maps`: site -> [B, T])."""
import torch
import torch.nn.functional as F

from cn_oracle import _emb
from oracle.unet_ref import _conv, _lin, resnet_block

M32 = 0xFFFFFFFF


def mix32(seed, step, site, cell):
    h = (seed ^ (step * 0x9E3779B9) ^ (site * 0x85EBCA6B) ^ (cell * 0xC2B2AE35)) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def plan(H, W, sx, sy, ratio, use_rand, seed, step, site):
    """(Nd, Ns, r, T', dst tokens in rank order, src tokens in rank order)."""
    hsy, wsx = H // sy, W // sx
    dst = []
    for cy in range(hsy):
        for cx in range(wsx):
            k = mix32(seed, step, site, cy * wsx + cx) % (sx * sy) if use_rand else 0
            dst.append((cy * sy + k // sx) * W + cx * sx + k % sx)
    dst.sort()                          # ranks are raster order within each set
    T = H * W
    isdst = set(dst)
    src = [t for t in range(T) if t not in isdst]
    Nd, Ns = len(dst), len(src)
    assert Nd == len(isdst)
    r = min(Ns, int(T * ratio))
    return Nd, Ns, r, T - r, dst, src


def scores(x, src, dst):
    """x [T, C] float64 -> s [Ns, Nd]; a zero row has reciprocal norm 0."""
    x = x.double()
    n = x.norm(dim=-1)
    rn = torch.where(n > 0, 1.0 / n, torch.zeros_like(n))
    # (one reduction per score, the same for every score: identical rows give identical scores, which a BLAS need not)
    dots = (x[src][:, None, :] * x[dst][None, :, :]).sum(-1)
    return dots * rn[src][:, None] * rn[dst][None, :]


def match_from_scores(s, r, src, dst, T):
    """(map [T], node_max [Ns], node_idx [Ns], merged [Ns] bool) by the lower-rank tie rules."""
    Ns, Nd = s.shape
    node_max = s.max(dim=1).values
    node_idx = torch.tensor([int((s[i] == node_max[i]).nonzero()[0]) for i in range(Ns)], dtype=torch.long)
    order = sorted(range(Ns), key=lambda i: (-node_max[i].item(), i))
    merged = torch.zeros(Ns, dtype=torch.bool)
    merged[order[:r]] = True
    mp = torch.empty(T, dtype=torch.long)
    U = Ns - r
    p = 0
    for i in range(Ns):
        if merged[i]:
            mp[src[i]] = U + node_idx[i]
        else:
            mp[src[i]] = p
            p += 1
    for j in range(Nd):
        mp[dst[j]] = U + j
    return mp, node_max, node_idx, merged


def merge(rows, mp, Tm):
    """rows [T, K] -> [Tm, K]: the mean of every merged row's members."""
    out = torch.zeros(Tm, rows.shape[1], dtype=torch.float64)
    out.index_add_(0, mp, rows.double())
    cnt = torch.bincount(mp, minlength=Tm).double()
    return out / cnt[:, None]


class Tome:
    """Settings and state of one forward: which blocks merge, the maps used (given or computed) per site."""

    def __init__(self, ratio, max_downsample=1, sx=2, sy=2, use_rand=True, seed=0, step=0, maps=None, order="pre"):
        self.ratio, self.max_ds, self.sx, self.sy = ratio, max_downsample, sx, sy
        self.use_rand, self.seed, self.step = use_rand, seed, step
        self.maps = maps                # site -> LongTensor [B, T] (None: computed here)
        self.order = order
        self.site = 0
        self.sample_h = None
        self.used = {}                  # site -> dict(H, W, r, Tm, maps [B, T], x [B, T, C])

    def block_maps(self, x, H, W):
        """Maps [B, T] and T' of the block about to run (None: it does not merge); advances the site counter."""
        site = self.site
        self.site += 1
        if self.ratio <= 0 or self.sample_h // H > self.max_ds:
            return None
        Nd, Ns, r, Tm, dst, src = plan(H, W, self.sx, self.sy, self.ratio, self.use_rand, self.seed, self.step, site)
        if r < 1:
            return None
        if self.maps is not None:
            mp = self.maps[site].long()
        else:
            mp = torch.stack([match_from_scores(scores(x[b], src, dst), r, src, dst, H * W)[0] for b in range(x.shape[0])])
        self.used[site] = dict(H=H, W=W, r=r, Tm=Tm, maps=mp, x=x.detach().clone(), src=src, dst=dst)
        return mp, Tm


def _heads(t, heads):
    B, T, C = t.shape
    return t.view(B, T, heads, C // heads).transpose(1, 2)


def _attn1(h, w, p, heads, mp, Tm, order):
    """attn1 of norm1's output h [B, T, C] with token merging through mp [B, T] (None: plain)."""
    B, T, C = h.shape
    if mp is None:
        q, k, v = (_lin(h, w, p + n, False) for n in (".to_q", ".to_k", ".to_v"))
    elif order == "pre":
        hm = torch.stack([merge(h[b], mp[b], Tm) for b in range(B)]).to(h.dtype)
        q, k, v = (_lin(hm, w, p + n, False) for n in (".to_q", ".to_k", ".to_v"))
    else:
        q, k, v = (torch.stack([merge(_lin(h, w, p + n, False)[b], mp[b], Tm) for b in range(B)]).to(h.dtype)
                   for n in (".to_q", ".to_k", ".to_v"))
    o = F.scaled_dot_product_attention(_heads(q, heads), _heads(k, heads), _heads(v, heads))
    o = o.transpose(1, 2).reshape(B, -1, C)
    if mp is not None:
        o = torch.stack([o[b][mp[b]] for b in range(B)])
    return _lin(o, w, p + ".to_out.0")


def _xattn(x, ctx, w, p, heads):
    B, T, C = x.shape
    q, k, v = _lin(x, w, p + ".to_q", False), _lin(ctx, w, p + ".to_k", False), _lin(ctx, w, p + ".to_v", False)
    o = F.scaled_dot_product_attention(_heads(q, heads), _heads(k, heads), _heads(v, heads))
    return _lin(o.transpose(1, 2).reshape(B, T, C), w, p + ".to_out.0")


def block(x, ctx, w, p, heads, H, W, tome):
    got = tome.block_maps(x, H, W)
    mp, Tm = got if got is not None else (None, 0)
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm1.weight"], w[p + ".norm1.bias"], 1e-5)
    x = x + _attn1(h, w, p + ".attn1", heads, mp, Tm, tome.order)
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm2.weight"], w[p + ".norm2.bias"], 1e-5)
    x = x + _xattn(h, ctx, w, p + ".attn2", heads)
    h = F.layer_norm(x, (x.shape[-1],), w[p + ".norm3.weight"], w[p + ".norm3.bias"], 1e-5)
    hidden, gate = _lin(h, w, p + ".ff.net.0.proj").chunk(2, dim=-1)
    return x + _lin(hidden * F.gelu(gate), w, p + ".ff.net.2")


def site_table(cfg):
    """Transformer prefix -> ordinal of its first BasicTransformerBlock in execution order of the full forward."""
    L, out, n = cfg.layers_per_block, {}, 0
    rev_depth = list(reversed(cfg.transformer_layers_per_block))
    for i, btype in enumerate(cfg.down_block_types):
        if btype == "CrossAttnDownBlock2D":
            for j in range(L):
                out[f"down_blocks.{i}.attentions.{j}"] = n
                n += cfg.transformer_layers_per_block[i]
    out["mid_block.attentions.0"] = n
    n += cfg.transformer_layers_per_block[-1]
    for i, btype in enumerate(cfg.up_block_types):
        if btype == "CrossAttnUpBlock2D":
            for j in range(L + 1):
                out[f"up_blocks.{i}.attentions.{j}"] = n
                n += rev_depth[i]
    return out


def transformer_2d(x, ctx, w, p, heads, depth, linear, groups, tome):
    B, C, H, W = x.shape
    if getattr(tome, "sites", None) is not None:
        tome.site = tome.sites[p]       # (a forward that skips blocks keeps the full forward's ordinals)
    res = x
    h = F.group_norm(x, groups, w[p + ".norm.weight"], w[p + ".norm.bias"], 1e-6)
    if not linear:
        h = _conv(h, w, p + ".proj_in", padding=0).permute(0, 2, 3, 1).reshape(B, H * W, C)
    else:
        h = _lin(h.permute(0, 2, 3, 1).reshape(B, H * W, C), w, p + ".proj_in")
    for d in range(depth):
        h = block(h, ctx, w, f"{p}.transformer_blocks.{d}", heads, H, W, tome)
    if not linear:
        h = _conv(h.reshape(B, H, W, C).permute(0, 3, 1, 2), w, p + ".proj_out", padding=0)
    else:
        h = _lin(h, w, p + ".proj_out").reshape(B, H, W, C).permute(0, 3, 1, 2)
    return h + res


def unet_forward(cfg, w, x, t, ctx, added, tome):
    """oracle.unet_ref.unet_forward with every BasicTransformerBlock going through `tome` (a Tome)."""
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    L, nblk = cfg.layers_per_block, len(cfg.block_out_channels)
    tome.site, tome.sample_h, tome.used = 0, x.shape[2], {}
    emb = _emb(cfg, w, x, t, added)
    x = _conv(x, w, "conv_in")
    skips = [x]
    for i, btype in enumerate(cfg.down_block_types):
        for j in range(L):
            x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnDownBlock2D":
                x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i],
                                   cfg.transformer_layers_per_block[i], lin, g, tome)
            skips.append(x)
        if i != nblk - 1:
            x = _conv(x, w, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
            skips.append(x)
    x = resnet_block(x, emb, w, "mid_block.resnets.0", g, eps)
    x = transformer_2d(x, ctx, w, "mid_block.attentions.0", cfg.attention_head_dim[-1],
                       cfg.transformer_layers_per_block[-1], lin, g, tome)
    x = resnet_block(x, emb, w, "mid_block.resnets.1", g, eps)
    rev_heads, rev_depth = list(reversed(cfg.attention_head_dim)), list(reversed(cfg.transformer_layers_per_block))
    for i, btype in enumerate(cfg.up_block_types):
        for j in range(L + 1):
            x = resnet_block(torch.cat([x, skips.pop()], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnUpBlock2D":
                x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g, tome)
        if i != nblk - 1:
            x = _conv(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, f"up_blocks.{i}.upsamplers.0.conv")
    x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
    return _conv(F.silu(x), w, "conv_out")


def deepcache_forward(cfg, w, x, t, ctx, added, depth, tome, cached=None):
    """deepcache_oracle.forward with every BasicTransformerBlock going through `tome`: (out, F_depth).  A block keeps
    the ordinal it has in the full forward, so a reuse step (`cached` given) draws what a store step would."""
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    L, nblk = cfg.layers_per_block, len(cfg.block_out_channels)
    tome.sites, tome.sample_h, tome.used = site_table(cfg), x.shape[2], {}
    rev_heads, rev_depth = list(reversed(cfg.attention_head_dim)), list(reversed(cfg.transformer_layers_per_block))

    def down(x, i, j):
        x = resnet_block(x, emb, w, f"down_blocks.{i}.resnets.{j}", g, eps)
        if cfg.down_block_types[i] == "CrossAttnDownBlock2D":
            x = transformer_2d(x, ctx, w, f"down_blocks.{i}.attentions.{j}", cfg.attention_head_dim[i],
                               cfg.transformer_layers_per_block[i], lin, g, tome)
        return x

    def up(x, skip, i, j):
        x = resnet_block(torch.cat([x, skip], dim=1), emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
        if cfg.up_block_types[i] == "CrossAttnUpBlock2D":
            x = transformer_2d(x, ctx, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g, tome)
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
                       cfg.transformer_layers_per_block[-1], lin, g, tome)
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
