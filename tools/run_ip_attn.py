#!/usr/bin/env python3
"""Time IP-Adapter's decoupled cross-attention on one attn2 shape (GPU box):
python tools/run_ip_attn.py [--batch 8] [--tq 4096] [--heads 8] [--d 40] [--L 77] [--tip 4] [--iters 200]

Three numbers from sd_op_ip_cross_attention's timing mode, each `iters` back-to-back launches between HIP events:
the fused kernel (ip_xattn_kernel), the existing text-only cross-attention launch on the same operands
(attn_kernel), and the unfused composition (text attention + image attention + add).  Operands are laid out the way
the UNet holds them: prescaled queries, text and image K / V as slices of stacked [K | V] rows.  Default = the SD1.5
64 x 64 latent site (B = 8 after CFG)."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--tq", type=int, default=4096)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--d", type=int, default=40)
ap.add_argument("--L", type=int, default=77)
ap.add_argument("--tip", type=int, default=4)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

lib = _lib.load()
B, Tq, H, d, L, Tip = args.batch, args.tq, args.heads, args.d, args.L, args.tip
Cc = H * d
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
q = (torch.randn(B, Tq, Cc, device=dev, generator=g) * (1.4426950408889634 / d ** 0.5)).half()
kv = torch.randn(B, L, 2 * Cc, device=dev, generator=g).half()
kvi = torch.randn(B, Tip, 2 * Cc, device=dev, generator=g).half()
out = torch.empty(B, Tq, Cc, device=dev, dtype=torch.float16)
ms = (C.c_float * 3)()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
for rep in range(args.reps):
    rc = lib.sd_op_ip_cross_attention(P(q), P(kv), P(kv[..., Cc:]), P(kvi), P(kvi[..., Cc:]), P(out), B, Tq, L, Tip, H, d,
                                      Cc, 2 * Cc, 2 * Cc, 2 * Cc, 2 * Cc, Cc, args.scale, 1, args.iters, ms, st)
    _lib.check(rc, "sd_op_ip_cross_attention")
    print(f"B={B} Tq={Tq} heads={H} d={d} L={L} T_ip={Tip} rep {rep}: fused {ms[0] * 1e3:.2f} us  "
          f"text-only {ms[1] * 1e3:.2f} us  unfused {ms[2] * 1e3:.2f} us  "
          f"fused/text {ms[0] / ms[1]:.2f}  fused/unfused {ms[0] / ms[2]:.2f}", flush=True)
