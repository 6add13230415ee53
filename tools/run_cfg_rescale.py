#!/usr/bin/env python3
"""Time the guidance-rescale step on the denoise-step shapes (GPU box):
python tools/run_cfg_rescale.py [--iters 500] [--reps 3] [--phi 0.7]

Per shape three figures, each `iters` back-to-back calls between HIP events on torch's stream (no synchronisation inside
the window), best of `reps`:
  rescale   sd_cfg_rescale_linear_step (statistics launch + update launch)
  linear    sd_cfg_linear_step, the step without rescale that the parent already has
  torch     the composition the op replaces, on the device: CFG combine, std x 2, rescale, mix, affine update
Shapes: C2 (B = 4, 4 x 64 x 64), C4 (B = 2, 4 x 128 x 128), C5 (B = 4, 4 x 96 x 96); with and without the fp32 history
(DPM++ 2M keeps one).  `--unet-ms` is the UNet forward the added time is read against (profiles/r03_bench.json,
`unet_forward_ms`, measured at C2)."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--phi", type=float, default=0.7)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--unet-ms", type=float, default=10.1)
args = ap.parse_args()

_lib.require_gpu()
lib = _lib.load()
dev = "cuda"
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
# an update that keeps the latents bounded over many in-place applications
CX, CE, CH, HX, HE = 0.5, 0.1, 0.05, 0.5, 0.1


def timed(fn, iters, reps):
    best = float("inf")
    for _ in range(reps):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters)
    return best * 1e3          # microseconds per call


for name, B, h in (("C2", 4, 64), ("C4", 2, 128), ("C5", 4, 96)):
    n = 4 * h * h
    g = torch.Generator(device=dev).manual_seed(B * h)
    eps = torch.randn(2 * B, 4, h, h, device=dev, generator=g).half()
    lat = torch.randn(B, 4, h, h, device=dev, generator=g).half()
    for with_hist in (False, True):
        hist = torch.zeros(B, 4, h, h, device=dev) if with_hist else None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def rescale():
            rc = lib.sd_cfg_rescale_linear_step(P(eps), P(lat), P(hist), B, n, args.guidance, args.phi, CX, CE, CH, HX, HE,
                                                None, st)
            assert rc == 0

        def linear():
            rc = lib.sd_cfg_linear_step(P(eps), P(lat), P(hist), B * n, args.guidance, CX, CE, CH, HX, HE, st)
            assert rc == 0

        def composed():
            u, t = eps.chunk(2)
            e = args.guidance * (t - u) + u
            dims = [1, 2, 3]
            e = args.phi * (e * (t.std(dim=dims, keepdim=True) / e.std(dim=dims, keepdim=True))) + (1 - args.phi) * e
            x = lat.float()
            out = CX * x + CE * e.float()
            if hist is not None:
                out = out + CH * hist
                hist.copy_(HX * x + HE * e.float())
            lat.copy_(out)

        t_r, t_l, t_t = (timed(f, args.iters, args.reps) for f in (rescale, linear, composed))
        assert torch.isfinite(lat.float()).all()
        added = t_r - t_l
        print(f"{name} B={B} 4x{h}x{h} hist={int(with_hist)}: rescale {t_r:.2f} us  linear {t_l:.2f} us  torch {t_t:.2f} us  "
              f"added {added:.2f} us = {added / (args.unet_ms * 1e3) * 100:.3f} % of a {args.unet_ms} ms UNet forward  "
              f"rescale/torch {t_r / t_t:.3f}", flush=True)
