"""float64 restatement of diffusers 0.27.2's LCMScheduler, of the LCM pipeline's guidance-scale embedding and of
UNet2DConditionModel.forward(timestep_cond=) (TimestepEmbedding.cond_proj), for the tests (not a test module).  The UNet is
built from oracle.unet_ref's pieces the way freeu_oracle and cn_oracle are; nothing under oracle/ is edited.  Recalled,
not pinned: diffusers is not installed where this was written.

Also the inputs and the reference of the device step's test (`step_inputs`, `step_reference`), shared by the GPU test
and by the CPU test that checks the reference itself."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from cn_oracle import _encoder
from oracle.unet_ref import _conv, _lin, resnet_block, timestep_sinusoid, transformer_2d


# ------------------------------------------------------------------------------------------------ scheduler
class LCMOracle:
    """LCMScheduler in plain float64 numpy: scaled_linear betas, set_alpha_to_one, sigma_data 0.5."""

    def __init__(self, T=1000, beta_start=0.00085, beta_end=0.012, original_inference_steps=50, timestep_scaling=10.0,
                 prediction_type="epsilon"):
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float64) ** 2
        self.ac = np.cumprod(1.0 - betas)
        self.T, self.original, self.scaling, self.pred = T, original_inference_steps, timestep_scaling, prediction_type

    def timesteps(self, n, strength=1.0):
        k = self.T // self.original
        origin = [i * k - 1 for i in range(1, int(self.original * strength) + 1)][::-1]
        return [origin[int(math.floor(i * len(origin) / n))] for i in range(n)]

    def step(self, model_output, i, ts, sample, noise):
        """Step i of the schedule ts on float64 arrays -> (prev, denoised)."""
        t = ts[i]
        a = self.ac[t]
        s = t * self.scaling
        c_skip = 0.25 / (s * s + 0.25)
        c_out = s / math.sqrt(s * s + 0.25)
        if self.pred == "epsilon":
            x0 = (sample - math.sqrt(1 - a) * model_output) / math.sqrt(a)
        else:
            x0 = math.sqrt(a) * sample - math.sqrt(1 - a) * model_output
        denoised = c_out * x0 + c_skip * sample
        if i == len(ts) - 1:
            return denoised, denoised
        ap = self.ac[ts[i + 1]]
        return math.sqrt(ap) * denoised + math.sqrt(1 - ap) * noise, denoised


def guidance_scale_embedding(w, dim):
    """w [B] float64 -> [B, dim]: [sin | cos] of 1000 w exp(-i ln(1e4) / (half - 1)), zero-padded when dim is odd."""
    w = np.asarray(w, dtype=np.float64).reshape(-1) * 1000.0
    half = dim // 2
    freq = np.exp(-np.arange(half, dtype=np.float64) * (math.log(10000.0) / (half - 1)))
    ang = w[:, None] * freq[None, :]
    emb = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    if dim % 2:
        emb = np.concatenate([emb, np.zeros((len(w), 1))], axis=1)
    return emb


# ------------------------------------------------------------------------------------------------ device step
def step_inputs(n, seed):
    """fp16 inputs of one sd_lcm_step case: model output [2n] (rows = 1 reads the first n), latents, noise."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2 * n, generator=g).half(), torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half())


def cfg_combine_f16(mo, n, g):
    """fp16(u + g (t - u)) with the rounding the issue names (cfg_linear_kernel's): t - u rounded to fp32, one fused
    multiply-add rounded to fp32, then fp16.  The fp32 steps are emulated in float64 (products of two fp32 are exact there)."""
    u, t = mo[:n].double().numpy(), mo[n:2 * n].double().numpy()
    d = (t - u).astype(np.float32).astype(np.float64)
    m32 = (np.float64(np.float32(g)) * d + u).astype(np.float32)
    return torch.from_numpy(m32).half()


def step_reference(mo, rows, lat, noise, n, g, d_x, d_out, p_den, p_noise):
    """float64 evaluation of the step on the fp16 inputs with the fp32 coefficients the entry point receives:
    (denoised, latents) as float64 tensors, unrounded."""
    m = (cfg_combine_f16(mo, n, g) if rows == 2 else mo[:n]).double()
    c = [float(np.float32(v)) for v in (d_x, d_out, p_den, p_noise)]
    den = c[0] * lat.double() + c[1] * m
    out = c[2] * den
    if noise is not None:
        out = out + c[3] * noise.double()
    return den, out


def to_f16(x):
    """float64 tensor -> fp16 with ONE rounding (torch's .half() goes through fp32: two)."""
    return torch.from_numpy(x.double().numpy().astype(np.float16))


def ulp_diff_f16(a, b):
    """|a - b| in fp16 ulps (a, b fp16 tensors), through the monotone integer order of IEEE halves."""
    def key(x):
        i = x.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


# ------------------------------------------------------------------------------------------------ UNet
def unet_forward(cfg, w, sample, timestep, ehs, timestep_cond=None, added_cond_kwargs=None):
    """UNet2DConditionModel.forward with timestep_cond: emb = MLP(sinusoid(t) + cond_proj(timestep_cond))."""
    B = sample.shape[0]
    t = torch.as_tensor(timestep)
    t = (t[None] if t.ndim == 0 else t).expand(B)
    boc = cfg.block_out_channels
    t_emb = timestep_sinusoid(t, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift).to(sample.dtype)
    if timestep_cond is not None:
        t_emb = t_emb + F.linear(timestep_cond.to(sample.dtype), w["time_embedding.cond_proj.weight"])
    emb = _lin(F.silu(_lin(t_emb, w, "time_embedding.linear_1")), w, "time_embedding.linear_2")
    if cfg.addition_embed_type == "text_time":
        te = timestep_sinusoid(added_cond_kwargs["time_ids"].flatten(), cfg.addition_time_embed_dim,
                               cfg.flip_sin_to_cos, cfg.freq_shift).reshape(B, -1).to(sample.dtype)
        add = torch.cat([added_cond_kwargs["text_embeds"].to(sample.dtype), te], dim=-1)
        emb = emb + _lin(F.silu(_lin(add, w, "add_embedding.linear_1")), w, "add_embedding.linear_2")
    skips, x = _encoder(cfg, w, _conv(sample, w, "conv_in"), emb, ehs)
    g, eps, lin = cfg.norm_num_groups, cfg.norm_eps, cfg.use_linear_projection
    nblk = len(boc)
    rev_heads = list(reversed(cfg.attention_head_dim))
    rev_depth = list(reversed(cfg.transformer_layers_per_block))
    for i, btype in enumerate(cfg.up_block_types):
        for j in range(cfg.layers_per_block + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = resnet_block(x, emb, w, f"up_blocks.{i}.resnets.{j}", g, eps)
            if btype == "CrossAttnUpBlock2D":
                x = transformer_2d(x, ehs, w, f"up_blocks.{i}.attentions.{j}", rev_heads[i], rev_depth[i], lin, g)
        if i != nblk - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = _conv(x, w, f"up_blocks.{i}.upsamplers.0.conv")
    x = F.group_norm(x, g, w["conv_norm_out.weight"], w["conv_norm_out.bias"], eps)
    return _conv(F.silu(x), w, "conv_out")
