#!/usr/bin/env python3
"""Time the UNet forward alone (GPU box): python tools/run_unet.py [--preset sd15] [--batch 8] [--latent 64] [--iters 20]
Prints ms per forward (events around the whole loop, no per-launch brackets); run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/run_unet.py` for per-kernel durations.
--freeu: every round times the forward with FreeU off, then on (s1 0.9, s2 0.2, b1 1.5, b2 1.6), alternating in one
process, and ends with the FreeU kernel's time per launch from the engine's event brackets."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import config, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="sd15")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--freeu", action="store_true")
args = ap.parse_args()
ucfg, _ = (f() for f in config.PRESETS[args.preset])
dev = "cuda"
sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
x = torch.randn(args.batch, 4, args.latent, args.latent, device=dev, dtype=torch.float16)
e = torch.randn(args.batch, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16)
added = None
if args.preset == "sdxl":
    pdim = ucfg.projection_class_embeddings_input_dim - 6 * ucfg.addition_time_embed_dim
    added = {"text_embeds": torch.randn(args.batch, pdim, device=dev, dtype=torch.float16),
             "time_ids": torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * args.batch)}
t = torch.tensor(501.0)
for _ in range(3):
    net(x, t, e, added_cond_kwargs=added)
torch.cuda.synchronize()


def timed():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        net(x, t, e, added_cond_kwargs=added)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


tag = " ".join(f"{k}={v}" for k, v in os.environ.items() if k.startswith("SD_"))
head = f"unet forward {args.preset} B{args.batch} {args.latent}x{args.latent}"
if not args.freeu:
    res = [timed() for _ in range(args.rounds)]
    print(f"{head}: " + " / ".join(f"{r:.3f}" for r in res) + f" ms  [{tag}]", flush=True)
else:
    from stablediffusion_amd import _lib
    FACTORS = (0.9, 0.2, 1.5, 1.6)
    net.enable_freeu(*FACTORS)
    net(x, t, e, added_cond_kwargs=added)
    off, on = [], []
    for _ in range(args.rounds):
        net.disable_freeu()
        off.append(timed())
        net.enable_freeu(*FACTORS)
        on.append(timed())
    print(f"{head} FreeU off: " + " / ".join(f"{r:.3f}" for r in off) + f" ms  [{tag}]")
    print(f"{head} FreeU on : " + " / ".join(f"{r:.3f}" for r in on) + f" ms  [{tag}]")
    lib = _lib.load()
    lib.sd_prof_enable(1)
    for _ in range(3):
        net(x, t, e, added_cond_kwargs=added)
    ents = (_lib.SdProfEntry * 512)()
    n = C.c_int()
    _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    lib.sd_prof_enable(0)
    for ent in ents[: n.value]:
        if ent.kernel.decode() == "freeu_kernel":
            print(f"freeu_kernel: {ent.launches // 3} launches per forward, {ent.ms / ent.launches * 1e3:.1f} us per launch "
                  f"(event brackets), {ent.bytes / ent.ms / 1e6:.0f} GB/s", flush=True)
