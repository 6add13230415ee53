#!/usr/bin/env python3
"""Time a 30-step loop of euler_a, DPM++ 2M SDE Karras, PNDM and uni_pc at the C2 shape (GPU box):
python tools/run_sched_step.py [--root TREE] [--against PARENT_TREE --rounds 3] [--only NAME] [--reps 5] [--warmup 2]

SD1.5 configuration with synthetic weights, batch 4, 64x64 latents, CFG on, output_type="latents" (no VAE decode).  Only
the public pipeline API is used, so the script runs unchanged on a tree that lacks the device step (`--root`: the tree
whose package is imported; default: the one this file is in).  Each loop is timed with a host clock around a final
synchronise, after `--warmup` untimed loops; printed per scheduler: one JSON line with the `--reps` times in ms.

`--against PARENT_TREE` is the measurement: it starts this script as a fresh process on this tree and on a built copy of
the parent commit in turn, `--rounds` times each, and prints per scheduler both medians, both spreads (max - min over all
repetitions of all rounds) and the difference.  The baseline is the parent's own code, not this tree with the path off.

`--only NAME --reps 1 --warmup 0` is one loop of one scheduler: the form to run under a kernel trace for launch counts."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

NAMES = ["euler_a", "DPM++ 2M SDE Karras", "PNDM", "uni_pc"]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ap.add_argument("--against")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--only")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--tiny", action="store_true", help="tiny UNet (a rehearsal of the script, not a measurement)")
args = ap.parse_args()


def compare():
    times = {"this": {n: [] for n in NAMES}, "parent": {n: [] for n in NAMES}}
    base = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup), "--steps",
            str(args.steps), "--batch", str(args.batch), "--latent", str(args.latent)] + (["--tiny"] if args.tiny else [])
    for _ in range(args.rounds):
        for which, root in (("this", args.root), ("parent", args.against)):
            r = subprocess.run(base + ["--root", os.path.abspath(root)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit(f"{which} ({root}) failed:\n{r.stdout}\n{r.stderr}")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    times[which][d["scheduler"]] += d["ms"]
    print(f"{args.steps}-step loop, B={args.batch} 4x{args.latent}x{args.latent}, CFG on; {args.rounds} alternating rounds of "
          f"{args.reps} loops per tree (ms per loop: median, spread = max - min)")
    for n in NAMES:
        a, b = times["this"][n], times["parent"][n]
        ma, mb = statistics.median(a), statistics.median(b)
        print(f"  {n:20s} this tree {ma:8.2f} (spread {max(a) - min(a):5.2f})   parent {mb:8.2f} (spread {max(b) - min(b):5.2f})   "
              f"this - parent {ma - mb:+7.2f} ms = {(ma - mb) / mb * 100:+.2f} %")


def measure():
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from stablediffusion_amd import _lib, config, weights
    from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    _lib.require_gpu()
    ucfg = config.tiny_unet() if args.tiny else config.sd15_unet()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=21, dtype=torch.float16)
    unet = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    del usd
    model = SDModelWrapper(base=unet, vae=HipAutoencoderKL(config.tiny_vae()), device="cuda")    # (the VAE is never run)
    B, h = args.batch, args.latent
    g = torch.Generator().manual_seed(1)
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(B, 4, h, h, generator=g).half().cuda()
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=args.steps, guidance_scale=7.5,
              height=8 * h, width=8 * h)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    for name in ([args.only] if args.only else NAMES):
        model.set_scheduler(name)
        ms = []
        for i in range(args.warmup + args.reps):
            torch.manual_seed(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe(model, **kw)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(out.float()).all(), name
        print(json.dumps({"scheduler": name, "root": os.path.abspath(args.root), "steps": args.steps,
                          "ms": [round(v, 3) for v in ms]}), flush=True)


if args.against:
    compare()
else:
    measure()
