"""AnimateDiff motion adapters: configuration, the manifest of an adapter's weights and the loaders.

Two file layouts hold the same tensors:
  * diffusers `MotionAdapter` (a folder with config.json + diffusion_pytorch_model.safetensors, or its state dict):
    "down_blocks.0.motion_modules.1.transformer_blocks.0.attn1.to_q.weight", ...
  * the original `mm_sd_v15*` checkpoints:
    "down_blocks.0.motion_modules.1.temporal_transformer.transformer_blocks.0.attention_blocks.0.to_q.weight", ...
    with attention_blocks.{0,1} -> attn1 / attn2, norms.{0,1} -> norm1 / norm2, ff_norm -> norm3.
Both store the sinusoidal position rows (`pos_embed.pe` / `pos_encoder.pe`); the engine builds them in closed form, so a
stored table is compared with it and dropped.

Recalled from diffusers 0.27.2 (not installed where this was written); tests/motion_oracle.py restates the semantics."""
from __future__ import annotations

import dataclasses
import json
import math
import os
import re
from typing import Dict, Optional, Tuple

import torch

from .config import UNetConfig


@dataclasses.dataclass(frozen=True)
class MotionAdapterConfig:
    """diffusers MotionAdapter.config, as far as the engine reads it."""
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    motion_layers_per_block: int = 2
    motion_mid_block_layers_per_block: int = 1
    motion_num_attention_heads: Tuple[int, ...] = (8, 8, 8, 8)      # an int in the file means every block
    motion_norm_num_groups: int = 32
    motion_max_seq_length: int = 32
    use_motion_mid_block: bool = True

    @staticmethod
    def from_dict(d: dict) -> "MotionAdapterConfig":
        if d.get("conv_in_channels"):
            raise NotImplementedError("motion adapters with conv_in (SparseCtrl, PIA: conv_in_channels) are not supported")
        boc = tuple(int(c) for c in d.get("block_out_channels", (320, 640, 1280, 1280)))
        heads = d.get("motion_num_attention_heads", 8)
        heads = tuple(int(h) for h in heads) if isinstance(heads, (list, tuple)) else (int(heads),) * len(boc)
        return MotionAdapterConfig(boc, int(d.get("motion_layers_per_block", 2)), int(d.get("motion_mid_block_layers_per_block", 1)),
                                   heads, int(d.get("motion_norm_num_groups", 32)), int(d.get("motion_max_seq_length", 32)),
                                   bool(d.get("use_motion_mid_block", True)))

    def check(self, unet: UNetConfig):
        """Raises unless this adapter fits `unet` and the engine's temporal attention."""
        if tuple(self.block_out_channels) != tuple(unet.block_out_channels):
            raise ValueError(f"motion adapter block_out_channels {tuple(self.block_out_channels)} differ from the UNet's "
                             f"{tuple(unet.block_out_channels)}")
        if self.motion_layers_per_block != unet.layers_per_block:
            raise ValueError("motion adapter motion_layers_per_block differs from the UNet's layers_per_block")
        if len(self.motion_num_attention_heads) != len(self.block_out_channels):
            raise ValueError("motion_num_attention_heads needs one entry per block")
        if self.motion_norm_num_groups != 32:
            raise NotImplementedError("motion_norm_num_groups other than 32 is not supported")
        if self.motion_mid_block_layers_per_block != 1:
            raise NotImplementedError("motion_mid_block_layers_per_block other than 1 is not supported")
        if not 1 <= self.motion_max_seq_length <= 32:
            raise NotImplementedError("motion_max_seq_length must be in 1..32 (longer clips need sliding context windows)")
        if unet.addition_embed_type == "text_time":
            raise NotImplementedError("AnimateDiff-SDXL (a text_time UNet) is not supported")


def tiny_motion_adapter(unet: UNetConfig) -> MotionAdapterConfig:
    """The adapter of the test UNets (config.tiny_unet): the UNet's own heads, so every head dim is 32."""
    return MotionAdapterConfig(tuple(unet.block_out_channels), unet.layers_per_block, 1, tuple(unet.attention_head_dim))


def module_prefixes(cfg: MotionAdapterConfig):
    """Every motion module as (prefix, channels, heads), in execution order of the forward (down, mid, up)."""
    nb = len(cfg.block_out_channels)
    out = []
    for i in range(nb):
        for j in range(cfg.motion_layers_per_block):
            out.append((f"down_blocks.{i}.motion_modules.{j}", cfg.block_out_channels[i], cfg.motion_num_attention_heads[i]))
    if cfg.use_motion_mid_block:
        out.append(("mid_block.motion_modules.0", cfg.block_out_channels[-1], cfg.motion_num_attention_heads[-1]))
    for i in range(nb):
        for j in range(cfg.motion_layers_per_block + 1):
            out.append((f"up_blocks.{i}.motion_modules.{j}", cfg.block_out_channels[nb - 1 - i],
                        cfg.motion_num_attention_heads[nb - 1 - i]))
    return out


def module_manifest(prefix: str, c: int):
    b = f"{prefix}.transformer_blocks.0"
    m = [(f"{prefix}.norm.weight", (c,)), (f"{prefix}.norm.bias", (c,)),
         (f"{prefix}.proj_in.weight", (c, c)), (f"{prefix}.proj_in.bias", (c,))]
    for n in ("norm1", "norm2", "norm3"):
        m += [(f"{b}.{n}.weight", (c,)), (f"{b}.{n}.bias", (c,))]
    for a in ("attn1", "attn2"):
        m += [(f"{b}.{a}.to_q.weight", (c, c)), (f"{b}.{a}.to_k.weight", (c, c)), (f"{b}.{a}.to_v.weight", (c, c)),
              (f"{b}.{a}.to_out.0.weight", (c, c)), (f"{b}.{a}.to_out.0.bias", (c,))]
    m += [(f"{b}.ff.net.0.proj.weight", (8 * c, c)), (f"{b}.ff.net.0.proj.bias", (8 * c,)),
          (f"{b}.ff.net.2.weight", (c, 4 * c)), (f"{b}.ff.net.2.bias", (c,)),
          (f"{prefix}.proj_out.weight", (c, c)), (f"{prefix}.proj_out.bias", (c,))]
    return m


def manifest(cfg: MotionAdapterConfig):
    """[(key, shape)] of the engine's adapter weights: the diffusers names without the stored position tables."""
    out = []
    for p, c, _ in module_prefixes(cfg):
        out += module_manifest(p, c)
    return out


def position_table(frames: int, channels: int) -> torch.Tensor:
    """float64 pe[f, 2i] = sin(f 10000^(-2i/C)), pe[f, 2i+1] = cos(same)."""
    pos = torch.arange(frames, dtype=torch.float64)[:, None]
    div = torch.exp(torch.arange(0, channels, 2, dtype=torch.float64) * (-math.log(10000.0) / channels))
    pe = torch.zeros(frames, channels, dtype=torch.float64)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


_ORIG = re.compile(r"\.temporal_transformer\.")
_PE = re.compile(r"\.(pos_embed|pos_encoder)\.pe$")


def is_original(sd: Dict[str, torch.Tensor]) -> bool:
    return any(_ORIG.search(k) for k in sd)


def original_to_diffusers_key(k: str) -> str:
    k = k.replace(".temporal_transformer.", ".")
    k = k.replace(".attention_blocks.0.", ".attn1.").replace(".attention_blocks.1.", ".attn2.")
    k = k.replace(".norms.0.", ".norm1.").replace(".norms.1.", ".norm2.").replace(".ff_norm.", ".norm3.")
    return k.replace(".pos_encoder.pe", ".pos_embed.pe")


def diffusers_to_original_key(k: str) -> str:
    """The inverse map (tests round-trip through it)."""
    k = re.sub(r"(motion_modules\.\d+)\.", r"\1.temporal_transformer.", k, count=1)
    k = k.replace(".attn1.", ".attention_blocks.0.").replace(".attn2.", ".attention_blocks.1.")
    k = k.replace(".norm1.", ".norms.0.").replace(".norm2.", ".norms.1.").replace(".norm3.", ".ff_norm.")
    return k.replace(".pos_embed.pe", ".pos_encoder.pe")


def infer_config(sd: Dict[str, torch.Tensor], unet: UNetConfig, heads=8) -> MotionAdapterConfig:
    """The configuration of a diffusers-named state dict without a config.json: sizes from the shapes, heads as given
    (every published SD 1.5 adapter has 8)."""
    boc, i = [], 0
    while f"down_blocks.{i}.motion_modules.0.proj_in.weight" in sd:
        boc.append(int(sd[f"down_blocks.{i}.motion_modules.0.proj_in.weight"].shape[0]))
        i += 1
    if not boc:
        raise KeyError("state_dict holds no motion module (down_blocks.0.motion_modules.0.proj_in.weight)")
    layers = 0
    while f"down_blocks.0.motion_modules.{layers}.proj_in.weight" in sd:
        layers += 1
    max_seq = 32
    for k, v in sd.items():
        if _PE.search(k):
            max_seq = int(v.shape[-2])
            break
    h = tuple(heads) if isinstance(heads, (list, tuple)) else (int(heads),) * len(boc)
    return MotionAdapterConfig(tuple(boc), layers, 1, h, 32, max_seq, "mid_block.motion_modules.0.proj_in.weight" in sd)


def convert(sd: Dict[str, torch.Tensor], cfg: MotionAdapterConfig) -> Dict[str, torch.Tensor]:
    """A diffusers- or original-named state dict as the engine's: keys mapped, stored position tables checked against
    the closed form (refused when they differ by more than fp16 rounding) and dropped, then strict key and shape checks."""
    if any(".conv_in." in k or k.startswith("conv_in.") for k in sd):
        raise NotImplementedError("motion adapters with conv_in (SparseCtrl, PIA) are not supported")
    if is_original(sd):
        sd = {original_to_diffusers_key(k): v for k, v in sd.items()}
    out = {}
    for k, v in sd.items():
        if _PE.search(k):
            pe = v.reshape(-1, v.shape[-1]).double()
            want = position_table(pe.shape[0], pe.shape[1])
            # fp16 rounding of values in [-1, 1]: 2^-11, plus the fp32 arithmetic the file's table was built with
            if pe.shape[0] < cfg.motion_max_seq_length or (pe - want).abs().max().item() > 2.0 ** -11 + 1e-5:
                raise ValueError(f"{k}: the stored position table is not the sinusoidal closed form the engine builds")
            continue
        out[k] = v
    want = manifest(cfg)
    names = {k for k, _ in want}
    missing = [k for k, _ in want if k not in out]
    extra = [k for k in out if k not in names]
    if missing or extra:
        raise KeyError(f"motion adapter state dict: missing {missing[:3]}, unexpected {extra[:3]}")
    for k, shape in want:
        if tuple(out[k].shape) != shape:
            raise ValueError(f"motion adapter {k}: expected shape {shape}, got {tuple(out[k].shape)}")
    return out


def load(source, unet: UNetConfig, config: Optional[MotionAdapterConfig] = None):
    """(MotionAdapterConfig, engine-named state dict) from a diffusers MotionAdapter folder, an original `mm_sd_v15*`
    `.ckpt` / `.safetensors` file, or a state dict in either naming.  Nothing here reaches the network."""
    from . import checkpoints
    cfg = config
    if isinstance(source, dict):
        sd = source
    else:
        path = os.fspath(source)
        if os.path.isdir(path):
            with open(os.path.join(path, "config.json")) as f:
                cfg = cfg or MotionAdapterConfig.from_dict(json.load(f))
            st = os.path.join(path, "diffusion_pytorch_model.safetensors")
            sd = checkpoints.load_safetensors(st) if os.path.isfile(st) else torch.load(
                os.path.join(path, "diffusion_pytorch_model.bin"), map_location="cpu", weights_only=True)
        elif path.endswith(".safetensors"):
            sd = checkpoints.load_safetensors(path)
        elif os.path.isfile(path):
            sd = torch.load(path, map_location="cpu", weights_only=True)
            sd = sd.get("state_dict", sd)
        else:
            raise ValueError(f"motion adapter: {path!r} is neither a folder nor a weights file")
    if any(".conv_in." in k or k.startswith("conv_in.") for k in sd):
        raise NotImplementedError("motion adapters with conv_in (SparseCtrl, PIA) are not supported")
    if cfg is None:
        probe = {original_to_diffusers_key(k): v for k, v in sd.items()} if is_original(sd) else sd
        cfg = infer_config(probe, unet)
    cfg.check(unet)
    return cfg, convert(sd, cfg)


def synth_state_dict(cfg: MotionAdapterConfig, seed: int = 0, out_scale: float = 0.5) -> Dict[str, torch.Tensor]:
    """Random fp16-exact weights for tests and tools: norms near identity, linears at 1 / sqrt(fan_in), a NON-zero
    proj_out (the published adapters zero-initialise it; a zero one would hide the module)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in manifest(cfg):
        if k.endswith("norm.weight") or re.search(r"norm\d\.weight$", k):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
            if k.endswith("proj_out.weight"):
                t = t * out_scale
        sd[k] = t.half().float()
    return sd
