"""Block references for the per-block tap tests (test_block_taps.py, test_block_taps_gpu.py).

The engine's debug taps (sd_unet_tap / sd_vae_tap) hand out the input and the output of every UNet / VAE block of one
forward.  For each tapped block this module gives, from the oracle alone,

  reference(model, block, x_in)        the float64 block on the ENGINE's tapped fp16 input (teacher forcing: errors of
                                       earlier blocks do not enter), through oracle.unet_ref / oracle.vae_ref
  yardstick(model, block, x_in)        the same block with every tensor the engine stores as fp16 rounded to fp16 once:
                                       the error a correct fp16-storage implementation may have
  defect(model, block, x_in, kind)     the float64 block with one seeded composition mistake (the `defect=` pattern of
                                       ln_cases.emulate_ffn): what the tolerance must be able to see

and the tolerance both test files read: a block passes when, with e = tapped output - reference and
y = yardstick - reference,   rel_l2(e) <= m rel_l2(y)   and   max|e| <= m max|y|,   m = MARGIN[block.kind].

The hooked restatements below (`q` = the storage rounding, `defect` = the mistake) repeat the oracle's operations in the
oracle's order; test_block_taps.py asserts that without hooks they ARE the oracle's blocks and that walking a model
block by block reproduces oracle.unet_ref.unet_forward / oracle.vae_ref.vae_decode / vae_encode_moments.

MARGIN is measured, not chosen: twice the worst ratio the engine showed per block kind on the MI355X over every case
of test_block_taps_gpu.py, rounded up to one digit (profiles/block_taps.txt holds the table).  What keeps it honest is
test_block_taps.py: every listed defect must exceed m x yardstick by 3x in at least one metric.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import unet_ref, vae_ref
from oracle.unet_ref import _conv, _lin, attention
from stablediffusion_amd import config, weights

# ---- the tolerance: m per block kind (see the module docstring and profiles/block_taps.txt) ----
# worst measured ratio per kind: resnet 1.78, transformer 2.30, resampler 1.57, edge 1.04, VAE attention 1.32
MARGIN = {"resnet": 4.0, "transformer": 5.0, "resampler": 4.0, "edge": 3.0, "vae_attention": 3.0}
SEPARATION = 3.0            # a defect must exceed MARGIN x yardstick by this factor in rel-L2 or in max-abs
# The time embedding is fp32 end to end on the device and float32-sinusoid + float64 linears in the oracle.  The angle
# t f_i carries a relative error of 2^-23 (one rounding of the product, one of exp()), i.e. up to 1000 x 1.2e-7 = 1.2e-4
# absolute at the highest frequency for t <= 1000, in a unit-amplitude sinusoid; the two fp32 GEMVs add ~1e-6.  Eight
# times that; a structural mistake (an add_embedding term dropped, sin / cos not flipped) is O(1).
EMB_TOL = 1e-3

UNET_DEFECTS = ("no_temb", "no_shortcut_bias", "skip_half_zeroed", "replicate_pad", "no_attn2", "attn1_tail16",
                "ff_residual_missing", "wrong_image")
VAE_DEFECTS = ("no_shortcut_bias", "replicate_pad", "attn_bias_missing")


def rel_l2(a: torch.Tensor, ref: torch.Tensor) -> float:
    a, ref = a.double(), ref.double()
    return (torch.linalg.vector_norm(a - ref) / torch.linalg.vector_norm(ref).clamp_min(1e-300)).item()


def max_abs(a: torch.Tensor, ref: torch.Tensor) -> float:
    return (a.double() - ref.double()).abs().max().item()


def ident(t):
    return t


def q16(t):
    """One fp16 storage rounding."""
    return t.half().to(t.dtype)


# ------------------------------------------------------------------------------------------ hooked blocks
def _conv3(x, w, p, stride=1, replicate=False):
    """3x3 convolution, padding 1; replicate: the border taps clamped instead of zero (the seeded padding mistake)."""
    if replicate:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w[p + ".weight"], w[p + ".bias"], stride=stride)
    return _conv(x, w, p, stride=stride, padding=1)


def resnet(x, temb, w, p, groups, eps, q=ident, defect=None, c1=None):
    """unet_ref.resnet_block with the engine's fp16 stores (h after conv1 + temb, the shortcut, the output)."""
    rep = defect == "replicate_pad"
    if defect == "skip_half_zeroed":
        x = torch.cat([x[:, :c1], torch.zeros_like(x[:, c1:])], dim=1)
    h = F.group_norm(x, groups, w[p + ".norm1.weight"], w[p + ".norm1.bias"], eps)
    h = F.silu(h)
    h = _conv3(h, w, p + ".conv1", replicate=rep)
    if temb is not None and defect != "no_temb":
        te = temb.roll(-1, 0) if defect == "wrong_image" else temb
        h = h + _lin(F.silu(te), w, p + ".time_emb_proj")[:, :, None, None]
    h = q(h)
    h = F.group_norm(h, groups, w[p + ".norm2.weight"], w[p + ".norm2.bias"], eps)
    h = F.silu(h)
    h = _conv3(h, w, p + ".conv2", replicate=rep)
    if (p + ".conv_shortcut.weight") in w:
        bias = None if defect == "no_shortcut_bias" else w[p + ".conv_shortcut.bias"]
        x = q(F.conv2d(x, w[p + ".conv_shortcut.weight"], bias))
    return q(x + h)


def transformer_block(x, ctx, w, p, heads, q=ident, defect=None):
    """unet_ref.basic_transformer_block with the engine's fp16 stores (the three residual sums, the GEGLU hidden tensor)."""
    C = x.shape[-1]
    h = F.layer_norm(x, (C,), w[p + ".norm1.weight"], w[p + ".norm1.bias"], 1e-5)
    kv = h[:, :-16] if defect == "attn1_tail16" else h
    x = q(x + attention(h, kv, w, p + ".attn1", heads))
    h = F.layer_norm(x, (C,), w[p + ".norm2.weight"], w[p + ".norm2.bias"], 1e-5)
    if defect != "no_attn2":
        x = x + attention(h, ctx.roll(-1, 0) if defect == "wrong_image" else ctx, w, p + ".attn2", heads)
    x = q(x)
    h = F.layer_norm(x, (C,), w[p + ".norm3.weight"], w[p + ".norm3.bias"], 1e-5)
    hidden, gate = _lin(h, w, p + ".ff.net.0.proj").chunk(2, dim=-1)
    h = q(hidden * F.gelu(gate))
    ff = _lin(h, w, p + ".ff.net.2")
    return q(ff if defect == "ff_residual_missing" else x + ff)


def transformer(x, ctx, w, p, heads, depth, linear, groups, q=ident, defect=None):
    """unet_ref.transformer_2d with the engine's fp16 stores (proj_in's output, the blocks', the output)."""
    B, C, H, W = x.shape
    res = x
    h = F.group_norm(x, groups, w[p + ".norm.weight"], w[p + ".norm.bias"], 1e-6)
    if not linear:
        h = _conv(h, w, p + ".proj_in", padding=0)
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
    else:
        h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
        h = _lin(h, w, p + ".proj_in")
    h = q(h)
    for d in range(depth):
        h = transformer_block(h, ctx, w, f"{p}.transformer_blocks.{d}", heads, q, defect)
    if not linear:
        h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
        h = _conv(h, w, p + ".proj_out", padding=0)
    else:
        h = _lin(h, w, p + ".proj_out")
        h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
    return q(h + res)


def vae_attn(x, w, p, groups, q=ident, defect=None):
    """vae_ref.vae_attention with the engine's fp16 stores (the normalised input, q | k | v, the attention output, the
    output); attn_bias_missing: q / k / v computed without their biases (the UNet's projections have none)."""
    B, C, H, W = x.shape
    res = x
    bias = defect != "attn_bias_missing"
    h = q(F.group_norm(x, groups, w[p + ".group_norm.weight"], w[p + ".group_norm.bias"], vae_ref.VAE_EPS))
    h = h.view(B, C, H * W).transpose(1, 2)
    qq, k, v = (q(_lin(h, w, p + n, bias)) for n in (".to_q", ".to_k", ".to_v"))
    o = q(F.scaled_dot_product_attention(qq[:, None], k[:, None], v[:, None])[:, 0])
    o = _lin(o, w, p + ".to_out.0")
    o = o.transpose(1, 2).reshape(B, C, H, W)
    return q(o + res)


def _norm_act_conv(x, w, norm, conv, groups, eps, q, rep):
    """conv_norm_out -> SiLU -> conv_out (the normalised tensor is stored where the tail is not one launch)."""
    h = F.group_norm(x, groups, w[norm + ".weight"], w[norm + ".bias"], eps)
    return q(_conv3(q(F.silu(h)), w, conv, replicate=rep))


# ------------------------------------------------------------------------------------------ models and their blocks
@dataclass
class Block:
    name: str                       # the engine's tap name (a diffusers prefix)
    kind: str                       # MARGIN key
    op: str                         # which restatement evaluates it
    args: dict = field(default_factory=dict)
    defects: tuple = ()             # the seeded mistakes that apply to it


@dataclass
class Model:
    """One model case: config, weights (fp16-representable, in the references' dtype on their device) and, for a UNet,
    the conditioning of this forward."""
    cfg: object
    w: Dict[str, torch.Tensor]
    blocks: List[Block]
    emb: Optional[torch.Tensor] = None      # time embedding (+ add embedding), before any SiLU
    ctx: Optional[torch.Tensor] = None      # encoder_hidden_states
    B: int = 1

    @property
    def dtype(self):
        return next(iter(self.w.values())).dtype

    @property
    def device(self):
        return next(iter(self.w.values())).device

    def block(self, name: str) -> Block:
        return next(b for b in self.blocks if b.name == name)


def unet_emb(cfg, w, timestep, B, added=None, dtype=torch.float64):
    """The time embedding of unet_ref.unet_forward (its lines up to `ctx = encoder_hidden_states`)."""
    t = torch.as_tensor(timestep)
    if t.ndim == 0:
        t = t[None]
    t = t.expand(B)
    boc = cfg.block_out_channels
    t_emb = unet_ref.timestep_sinusoid(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(dtype)
    emb = _lin(F.silu(_lin(t_emb, w, "time_embedding.linear_1")), w, "time_embedding.linear_2")
    if cfg.addition_embed_type == "text_time":
        te = unet_ref.timestep_sinusoid(added["time_ids"].flatten(), cfg.addition_time_embed_dim, cfg.flip_sin_to_cos,
                                        cfg.freq_shift)
        te = te.reshape(B, -1).to(dtype)
        add = torch.cat([added["text_embeds"].to(dtype), te], dim=-1)
        emb = emb + _lin(F.silu(_lin(add, w, "add_embedding.linear_1")), w, "add_embedding.linear_2")
    return emb


def unet_blocks(cfg, B: int, H: int, W: int) -> List[Block]:
    """The tapped blocks of a UNet forward in execution order, with the defects that apply to each (wrong_image needs a
    second image, attn1_tail16 at least 32 tokens, no_shortcut_bias a shortcut, skip_half_zeroed a concatenation)."""
    boc = cfg.block_out_channels
    nb = len(boc)
    multi = ("wrong_image",) if B > 1 else ()

    def res(name, cin, cout, c1=None):
        d = ("no_temb", "replicate_pad") + multi + (("no_shortcut_bias",) if cin != cout else ())
        return Block(name, "resnet", "resnet", {"c1": c1}, d + (("skip_half_zeroed",) if c1 is not None else ()))

    def att(name, i, h, w):
        d = ("no_attn2", "ff_residual_missing") + multi + (("attn1_tail16",) if h * w >= 32 else ())
        return Block(name, "transformer", "transformer",
                     {"heads": cfg.attention_head_dim[i], "depth": cfg.transformer_layers_per_block[i]}, d)

    out = [Block("conv_in", "edge", "conv_in", {}, ("replicate_pad",))]
    h, w = H, W
    ch = boc[0]
    for i, btype in enumerate(cfg.down_block_types):
        for j in range(cfg.layers_per_block):
            out.append(res(f"down_blocks.{i}.resnets.{j}", ch, boc[i]))
            ch = boc[i]
            if btype == "CrossAttnDownBlock2D":
                out.append(att(f"down_blocks.{i}.attentions.{j}", i, h, w))
        if i != nb - 1:
            out.append(Block(f"down_blocks.{i}.downsamplers.0", "resampler", "down", {"pad": "unet"}, ("replicate_pad",)))
            h, w = h // 2, w // 2
    out.append(res("mid_block.resnets.0", ch, ch))
    out.append(att("mid_block.attentions.0", nb - 1, h, w))
    out.append(res("mid_block.resnets.1", ch, ch))
    rev = list(reversed(boc))
    for i, btype in enumerate(cfg.up_block_types):
        prev = ch
        ch = rev[i]
        in_ch = rev[min(i + 1, nb - 1)]
        for j in range(cfg.layers_per_block + 1):
            c1 = prev if j == 0 else ch
            c2 = in_ch if j == cfg.layers_per_block else ch
            out.append(res(f"up_blocks.{i}.resnets.{j}", c1 + c2, ch, c1))
            if btype == "CrossAttnUpBlock2D":
                out.append(att(f"up_blocks.{i}.attentions.{j}", nb - 1 - i, h, w))
        if i != nb - 1:
            out.append(Block(f"up_blocks.{i}.upsamplers.0", "resampler", "up", {}, ("replicate_pad",)))
            h, w = 2 * h, 2 * w
    out.append(Block("tail", "edge", "unet_tail", {}, ("replicate_pad",)))
    return out


def vae_blocks(cfg, which: str) -> List[Block]:
    """The tapped blocks of a VAE decode (`which` = "decoder") or encode ("encoder") in execution order."""
    boc = cfg.block_out_channels
    nb = len(boc)

    def res(name, cin, cout):
        return Block(name, "resnet", "vae_resnet", {},
                     ("replicate_pad",) + (("no_shortcut_bias",) if cin != cout else ()))

    mid = lambda c: [res(f"{which}.mid_block.resnets.0", c, c),
                     Block(f"{which}.mid_block.attentions.0", "vae_attention", "vae_attn", {}, ("attn_bias_missing",)),
                     res(f"{which}.mid_block.resnets.1", c, c)]
    if which == "decoder":
        out = [Block("decoder.conv_in", "edge", "dec_head", {}, ("replicate_pad",))] + mid(boc[-1])
        ch = boc[-1]
        for i, c in enumerate(reversed(boc)):
            for j in range(cfg.layers_per_block + 1):
                out.append(res(f"decoder.up_blocks.{i}.resnets.{j}", ch, c))
                ch = c
            if i != nb - 1:
                out.append(Block(f"decoder.up_blocks.{i}.upsamplers.0", "resampler", "up", {}, ("replicate_pad",)))
        out.append(Block("decoder.tail", "edge", "dec_tail", {}, ("replicate_pad",)))
        return out
    out = [Block("encoder.conv_in", "edge", "conv_in", {}, ("replicate_pad",))]
    ch = boc[0]
    for i, c in enumerate(boc):
        for j in range(cfg.layers_per_block):
            out.append(res(f"encoder.down_blocks.{i}.resnets.{j}", ch, c))
            ch = c
        if i != nb - 1:
            out.append(Block(f"encoder.down_blocks.{i}.downsamplers.0", "resampler", "down", {"pad": "vae"},
                             ("replicate_pad",)))
    return out + mid(ch) + [Block("encoder.tail", "edge", "enc_tail", {}, ("replicate_pad",))]


def _oracle_block(m: Model, b: Block, x):
    """The block through the oracle's own functions where it has one, else the lines of its forward."""
    cfg, w, p = m.cfg, m.w, b.name
    g = cfg.norm_num_groups
    if b.op == "resnet":
        return unet_ref.resnet_block(x, m.emb, w, p, g, cfg.norm_eps)
    if b.op == "vae_resnet":
        return unet_ref.resnet_block(x, None, w, p, g, vae_ref.VAE_EPS)
    if b.op == "transformer":
        return unet_ref.transformer_2d(x, m.ctx, w, p, b.args["heads"], b.args["depth"], cfg.use_linear_projection, g)
    if b.op == "vae_attn":
        return vae_ref.vae_attention(x, w, p, g)
    return None


def evaluate(m: Model, b: Block, x_in, q: Callable = ident, defect: Optional[str] = None):
    """Block `b` of model `m` on x_in (NCHW, any float type): the hooked restatement in the model's dtype."""
    if defect is not None and defect not in b.defects:
        raise ValueError(f"defect {defect!r} does not apply to {b.name}")
    cfg, w, p = m.cfg, m.w, b.name
    g = cfg.norm_num_groups
    x = x_in.to(device=m.device, dtype=m.dtype)
    rep = defect == "replicate_pad"
    if b.op == "resnet":
        return resnet(x, m.emb, w, p, g, cfg.norm_eps, q, defect, b.args["c1"])
    if b.op == "vae_resnet":
        return resnet(x, None, w, p, g, vae_ref.VAE_EPS, q, defect)
    if b.op == "transformer":
        return transformer(x, m.ctx, w, p, b.args["heads"], b.args["depth"], cfg.use_linear_projection, g, q, defect)
    if b.op == "vae_attn":
        return vae_attn(x, w, p, g, q, defect)
    if b.op == "conv_in":
        return q(_conv3(x, w, p, replicate=rep))
    if b.op == "down":
        conv = p + ".conv"
        if b.args["pad"] == "vae":      # Downsample2D of the VAE encoder: pad (0, 1, 0, 1), stride 2, padding 0
            x = F.pad(x, (0, 1, 0, 1), mode="replicate" if rep else "constant")
            return q(_conv(x, w, conv, stride=2, padding=0))
        return q(_conv3(x, w, conv, stride=2, replicate=rep))
    if b.op == "up":
        return q(_conv3(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, p + ".conv", replicate=rep))
    if b.op == "unet_tail":
        return _norm_act_conv(x, w, "conv_norm_out", "conv_out", g, cfg.norm_eps, q, rep)
    if b.op == "dec_head":
        return q(_conv3(q(_conv(x, w, "post_quant_conv", padding=0)), w, "decoder.conv_in", replicate=rep))
    if b.op == "dec_tail":
        return _norm_act_conv(x, w, "decoder.conv_norm_out", "decoder.conv_out", g, vae_ref.VAE_EPS, q, rep)
    if b.op == "enc_tail":
        h = _norm_act_conv(x, w, "encoder.conv_norm_out", "encoder.conv_out", g, vae_ref.VAE_EPS, q, rep)
        return q(_conv(h, w, "quant_conv", padding=0))
    raise ValueError(b.op)


def reference(m: Model, b: Block, x_in):
    """The float64 block on the given input: the oracle's own function where the oracle has one for the block."""
    x = x_in.to(device=m.device, dtype=m.dtype)
    y = _oracle_block(m, b, x)
    return y if y is not None else evaluate(m, b, x)


def yardstick(m: Model, b: Block, x_in):
    return evaluate(m, b, x_in, q=q16)


def defect(m: Model, b: Block, x_in, kind: str):
    return evaluate(m, b, x_in, defect=kind)


def walk(m: Model, x):
    """The model block by block through reference(): {name: (x_in, x_out)} of the oracle's own intermediates, and the
    output.  The UNet's skip bookkeeping is unet_ref.unet_forward's."""
    rec = {}
    x = x.to(device=m.device, dtype=m.dtype)
    skips = []
    for b in m.blocks:
        if b.op == "resnet" and b.args["c1"] is not None:
            x = torch.cat([x, skips.pop()], dim=1)
        y = reference(m, b, x)
        rec[b.name] = (x, y)
        x = y
        n = b.name
        if n == "conv_in" or n.startswith("down_blocks.") and (
                ".downsamplers." in n or ".attentions." in n or
                ".resnets." in n and m.cfg.down_block_types[int(n.split(".")[1])] == "DownBlock2D"):
            skips.append(x)
    assert not skips
    return rec, x


# ------------------------------------------------------------------------------------------ the cases
def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


def _case_d_cfg():
    """A two-level SD1.5 front end: the only configuration of the suite's block tests at which ffn_fused_kernel, the
    weight-stationary K = 320 GEMMs and the one-launch conv_in run inside a model (M = 8192 rows at C = 320 with B = 2)."""
    return config.UNetConfig(down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                             up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"), block_out_channels=(320, 640),
                             layers_per_block=1, cross_attention_dim=768, attention_head_dim=(8, 8),
                             transformer_layers_per_block=(1, 1))


UNET_CASES = {
    "a": dict(cfg=lambda: config.tiny_unet(), B=2, H=16, W=16, t=981.0, L=77),
    "b": dict(cfg=lambda: config.tiny_unet(linear=True, sdxl_cond=True), B=1, H=8, W=24, t=1.0, L=77),
    "c": dict(cfg=lambda: config.tiny_unet(), B=3, H=32, W=32, t=500.0, L=77),
    "d": dict(cfg=_case_d_cfg, B=2, H=64, W=64, t=601.0, L=77),
    # d at the benchmark's batch: the tile table is tuned for M = 32768 rows, and only there do conv_tail_kernel and
    # the persistent GEGLU projection run inside a model
    "e": dict(cfg=_case_d_cfg, B=8, H=64, W=64, t=901.0, L=77),
}
WEIGHT_SEED = 21


def unet_inputs(case: str, B=None, H=None, W=None):
    """(cfg, fp16-rounded fp32 state dict, sample, timesteps [B], ehs, added) of a UNet case, all seeded; B / H / W
    override the case's shape (the CPU test runs case d's configuration on a smaller map)."""
    c = UNET_CASES[case]
    cfg = c["cfg"]()
    B, H, W = B or c["B"], H or c["H"], W or c["W"]
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=WEIGHT_SEED, perturb=0.1))
    # The synthetic projections are N(0, 1 / fan_in): self-attention logits ~ N(0, 1), a softmax that is nearly uniform
    # over its T keys, so at T = 4096 no 16 keys carry anything a comparison could see (attn1_tail16 measured 0.8x the
    # tolerance there).  Trained self-attention is peaked.  Twice the query and key weights (exact in fp16) gives
    # logits ~ N(0, 16) in every case: the reference alone then shows the defect 8x (rel-L2) / 80x (max-abs) above it.
    for k in sd:
        if k.endswith((".attn1.to_q.weight", ".attn1.to_k.weight")):
            sd[k] = sd[k] * 2.0
    g = torch.Generator().manual_seed(1000 + ord(case))
    x = torch.randn(B, cfg.in_channels, H, W, generator=g).half()
    ehs = torch.randn(B, c["L"], cfg.cross_attention_dim, generator=g).half()
    # per-image timesteps, so that an image computed from its neighbour's embedding (wrong_image) shows
    t = torch.tensor([c["t"] - 110.0 * i for i in range(B)]).abs()
    added = None
    if cfg.addition_embed_type == "text_time":
        pooled = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
        added = {"text_embeds": torch.randn(B, pooled, generator=g).half(),
                 "time_ids": torch.tensor([[128.0, 96, 0, 8, 128, 96]] * B)}
    return cfg, sd, x, t, ehs, added


def unet_model(cfg, sd, t, ehs, added, H, W, dtype=torch.float64, device="cpu") -> Model:
    w = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    B = ehs.shape[0]
    # (the sinusoid is float32 on the CPU in the oracle whatever the references' dtype)
    w_cpu = w if device == "cpu" else {k: v.to(dtype) for k, v in sd.items() if "embedding" in k}
    a = None if added is None else {"text_embeds": added["text_embeds"].float(), "time_ids": added["time_ids"]}
    emb = unet_emb(cfg, w_cpu, t, B, a, dtype).to(device)
    return Model(cfg, w, unet_blocks(cfg, B, H, W), emb, ehs.to(device=device, dtype=dtype), B)


def vae_inputs(which: str, B: int, h: int, w: int, seed: int = 0):
    """(cfg, fp16-rounded state dict, input) of a VAE case: latents [B, 4, h, w] (decoder) or an image [B, 3, h, w]."""
    cfg = config.tiny_vae()
    sd = _f16_round(weights.synth_state_dict(weights.vae_manifest(cfg), seed=WEIGHT_SEED + 1, perturb=0.1))
    g = torch.Generator().manual_seed(2000 + seed + B * 7 + h)
    ch = cfg.latent_channels if which == "decoder" else cfg.in_channels
    return cfg, sd, torch.randn(B, ch, h, w, generator=g).half()


def vae_model(cfg, sd, which: str, B: int, dtype=torch.float64, device="cpu") -> Model:
    w = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    return Model(cfg, w, vae_blocks(cfg, which), B=B)


def unscale(taps: dict, first: str, last: str) -> dict:
    """Undo the stream scale the encoder's stored activations carry (sd_vae_encode_range_shift): every tensor the
    device recorded, i.e. all but the caller's input of `first` and output of `last`, divided by it in float64."""
    out = {}
    for name, rec in taps.items():
        s = rec.get("scale", 1.0)
        r = dict(rec)
        for k in ("in", "out"):
            if k in r and not (name == first and k == "in") and not (name == last and k == "out"):
                r[k] = r[k].double() / s
        out[name] = r
    return out


def ratios(m: Model, b: Block, x_in, x_out):
    """(rel_l2(e), rel_l2(y), max|e|, max|y|) of a block: e = x_out - reference, y = yardstick - reference."""
    ref = reference(m, b, x_in)
    yard = yardstick(m, b, x_in)
    got = x_out.to(device=m.device, dtype=m.dtype)
    return rel_l2(got, ref), rel_l2(yard, ref), max_abs(got, ref), max_abs(yard, ref)
