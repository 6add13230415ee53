#!/usr/bin/env python3
"""ControlNet timings (GPU box):
python tools/run_unet_controlnet.py [--preset sd15] [--batch 8] [--latent 64] [--iters 20] [--reps 3]
  1. the UNet forward with and without a ControlNet attached (synthetic weights, one control image per prompt pair,
     conditioning scale 1, text / conditioning caches on as inside the denoise loop), alternating so that box drift hits
     both alike;
  2. the grouped zero-conv residual launch against the unfused form (one GEMM per site with the residual in its
     epilogue) on the same sites, alternating;
  3. the conditioning embedding of 4 control images at 512 x 512."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cn_oracle import synth_cn_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipControlNetModel, HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="sd15")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
cfg = config.PRESETS[args.preset][0]()
dev = "cuda"
lib = _lib.load()
net = HipUNet2DConditionModel(cfg, dev).load_state_dict(weights.synth_state_dict(weights.unet_manifest(cfg), seed=2,
                                                                                 dtype=torch.float16))
ccfg = controlnet.encoder_config(cfg)
cn = HipControlNetModel(net, ccfg).load_state_dict({k: v.half() for k, v in synth_cn_state_dict(ccfg, seed=3).items()})
B, hw = args.batch, args.latent
x = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16)
e = torch.randn(B, 77, cfg.cross_attention_dim, device=dev, dtype=torch.float16)
img = torch.rand(max(1, B // 2), 3, 8 * hw, 8 * hw, device=dev, dtype=torch.float16)
added = {}
if cfg.addition_embed_type == "text_time":
    pdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    added = {"text_embeds": torch.randn(B, pdim, device=dev, dtype=torch.float16),
             "time_ids": torch.tensor([[hw * 8.0, hw * 8, 0, 0, hw * 8, hw * 8]] * B, device=dev)}


def timed(with_cn):
    net.attach_controlnet(cn if with_cn else None)
    kw = dict(controlnet_cond=img, controlnet_conditioning_scale=1.0) if with_cn else {}
    net.text_kv_cache(True)
    for _ in range(3):
        net(x, 501.0, e, added_cond_kwargs=added or None, **kw)
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.iters):
        net(x, 501.0, e, added_cond_kwargs=added or None, **kw)
    t.record()
    t.synchronize()
    net.text_kv_cache(False)
    return s.elapsed_time(t) / args.iters


for rep in range(args.reps):
    a, b = timed(False), timed(True)
    print(f"{args.preset} B={B} {hw}x{hw} rep {rep}: UNet plain {a:.3f} ms  with ControlNet {b:.3f} ms  ratio {b / a:.3f}",
          flush=True)
net.attach_controlnet(None)

# ---- grouped residual launch vs the unfused form on this configuration's sites ----
sites = []
h = hw
boc = cfg.block_out_channels
sites.append((B * h * h, boc[0]))
for i, c in enumerate(boc):
    sites += [(B * h * h, c)] * cfg.layers_per_block
    if i != len(boc) - 1:
        h //= 2
        sites.append((B * h * h, c))
sites.append((B * h * h, boc[-1]))
keep = []
arr = (_lib.SdCnProblem * len(sites))()
for i, (M, Cc) in enumerate(sites):
    xs = torch.randn(M, Cc, device=dev, dtype=torch.float16)
    w = torch.randn(Cc, Cc, device=dev, dtype=torch.float16) / Cc ** 0.5
    bias = torch.zeros(Cc, device=dev)
    y = torch.zeros(M, 2 * Cc, device=dev, dtype=torch.float16)
    keep += [xs, w, bias, y]
    arr[i] = _lib.SdCnProblem(xs.data_ptr(), Cc, w.data_ptr(), bias.data_ptr(), y.data_ptr(), 2 * Cc, M, Cc)
flop = sum(2.0 * M * Cc * Cc for M, Cc in sites)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for rep in range(args.reps):
    ms = []
    for mode in (0, 1):
        t = C.c_float()
        _lib.check(lib.sd_op_controlnet_residuals(arr, len(sites), 1e-3, mode, 50, C.byref(t), stream), "residuals")
        ms.append(t.value)
    print(f"residuals {len(sites)} sites, {flop / 1e9:.1f} GFLOP, rep {rep}: grouped {ms[0] * 1e3:.1f} us "
          f"({flop / ms[0] / 1e9:.0f} TF/s)  unfused {ms[1] * 1e3:.1f} us  ratio {ms[0] / ms[1]:.3f}", flush=True)

# ---- conditioning embedding, 4 images at 512 x 512 ----
ci = torch.rand(4, 3, 512, 512, device=dev, dtype=torch.float16)
out = torch.empty(4, 64, 64, boc[0], device=dev, dtype=torch.float16)
for rep in range(args.reps):
    t = C.c_float()
    _lib.check(lib.sd_op_controlnet_cond_embed(cn._h, C.c_void_p(ci.data_ptr()), 4, 64, 64, C.c_void_p(out.data_ptr()),
                                               20, C.byref(t), stream), "cond_embed")
    print(f"cond embedding 4 x 512x512 rep {rep}: {t.value:.3f} ms", flush=True)
