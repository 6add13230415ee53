#!/usr/bin/env python3
"""MultiDiffusion (GPU box): python tools/run_views.py [--height 64] [--width 256] [--window 64] [--stride 32]
                                                      [--view-batch 4] [--steps 10] [--rounds 3] [--out FILE]
An SD1.5-width UNet on synthetic weights, one latent canvas (B = 1) under CFG.  Defaults: a 64 x 256 canvas, window 64,
stride 32 (7 views), 4 views per forward (chunks 4, 3: CFG batches 8 and 6 of the headline 64 x 64 shape).  Prints
  * ms per step of the window path: sd_views_gather, one forward_cfg per chunk into the runner's buffer, sd_views_merge,
    sd_cfg_linear_step on the canvas (the pipeline's "linear" loop written out, DDIM);
  * ms per step of the same canvas through one plain forward_cfg at the canvas's size and the same step;
  * event times of the gather and the merge launches alone, and of one sd_cfg_linear_step over the same canvas as the
    memory-bound yardstick on the same box;
  * the box's probe (bench.py box_probe), so that runs on different boxes can be compared.
The two paths compute different things (that is the point of the windows): this is a cost comparison, not an A/B of one
result.  Synthetic weights: nothing here is an image-quality figure.  --out FILE also writes the text there
(profiles/views.txt is one such run).  --tiny: the width-reduced test configuration on a 24 x 40 canvas, window 16."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, schedulers, views, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=64)
ap.add_argument("--width", type=int, default=256)
ap.add_argument("--window", type=int, default=64)
ap.add_argument("--stride", type=int, default=32)
ap.add_argument("--view-batch", type=int, default=4)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.tiny:
    ucfg = config.tiny_unet()
    args.height, args.width, args.window, args.stride = 24, 40, 16, 8
    args.steps = min(args.steps, 4)
else:
    ucfg = config.sd15_unet()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


dev = "cuda"
B, G, GUIDANCE = 1, 2, 7.5
lib = _lib.load()


def box_probe():
    """bench.py's box_probe: the box's sustained MFMA rate, copy bandwidth and LDS-DMA operand rates."""
    tf, gb, d1, d2 = C.c_float(), C.c_float(), C.c_float(), C.c_float()
    _lib.check(lib.sd_probe_mfma(300000, C.byref(tf), None), "sd_probe_mfma")
    _lib.check(lib.sd_probe_copy(512 << 20, 5, C.byref(gb), None), "sd_probe_copy")
    _lib.check(lib.sd_probe_lds_dma(1 << 20, 64, 4, 1, C.byref(d1), None), "sd_probe_lds_dma")
    _lib.check(lib.sd_probe_lds_dma(1 << 20, 64, 4, 0, C.byref(d2), None), "sd_probe_lds_dma")
    return {"mfma_tflops": round(tf.value, 1), "hbm_gbs": round(gb.value, 1), "l2_to_lds_shared_gbs": round(d1.value, 1),
            "l2_to_lds_own_gbs": round(d2.value, 1)}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
del sd
g = torch.Generator(device=dev).manual_seed(1)
Hc, Wc = args.height, args.width
lat0 = torch.randn(B, 4, Hc, Wc, device=dev, dtype=torch.float16, generator=g)
ehs = torch.randn(G * B, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16, generator=g)
plan = views.plan_views(Hc, Wc, args.window, args.stride)
runner = views.ViewRunner(plan, B, G, args.view_batch, "uniform", ehs, lib=lib)
sched = schedulers.DDIMScheduler()


def step(out, lat, p):
    new = lat.clone()
    rc = lib.sd_cfg_linear_step(ptr(out), ptr(new), None, new.numel(), GUIDANCE, p.c_x, p.c_eps, p.c_hist, p.h_x, p.h_eps,
                                stream())
    assert rc == 0, lib.sd_last_error()
    sched.fused_commit()
    return new


def loop(kind):
    sched.set_timesteps(args.steps)
    lat = lat0.clone()
    net.text_kv_cache(True)
    try:
        for t in [float(v) for v in sched.timesteps.tolist()]:
            p = sched.fused_plan(t)
            assert not p.use_hist
            if kind == "windows":
                def run(windows, embeds, dst):
                    net.forward_cfg(windows, t, embeds, in_scale=p.in_scale, out=dst)
                out = runner.forward(lat, run)
            else:
                out = net.forward_cfg(lat, t, ehs, in_scale=p.in_scale)[0]
            lat = step(out, lat, p)
    finally:
        net.text_kv_cache(False)
    return lat


KINDS = ("windows", "one forward")
say(f"MultiDiffusion, {'width-reduced' if args.tiny else 'sd15-width'} UNet, canvas {Hc}x{Wc} latent pixels, B = {B}, CFG; window "
    f"{plan.h}x{plan.w}, stride {args.stride}: {plan.num_views} views in chunks {runner.sizes}; synthetic weights")
say("box_probe: " + json.dumps(box_probe()))
for k in KINDS:                                            # warm: plans, arenas, buffers
    loop(k)
say("")
say(f"ms per step over a {args.steps}-step DDIM loop (text K/V cache on, kinds alternating):")
lp = {k: [] for k in KINDS}
for _ in range(args.rounds):
    for k in KINDS:
        lp[k].append(timed(lambda: loop(k), 1) / args.steps)
med = {k: statistics.median(v) for k, v in lp.items()}
for k in KINDS:
    say(f"  {k:12s} median {med[k]:8.3f}  ({' '.join(f'{v:.3f}' for v in lp[k])})  x{med[k] / med['one forward']:.3f} of one forward")

say("")
say("the launches around the forwards (event times, 200 launches each):")
V = plan.num_views
windows = torch.empty(V * B, 4, plan.h, plan.w, device=dev, dtype=torch.float16)
outs = torch.randn(G * V * B, 4, plan.h, plan.w, device=dev, dtype=torch.float16, generator=g)
eps = torch.empty(G * B, 4, Hc, Wc, device=dev, dtype=torch.float16)
ys, xs = (C.c_int * len(plan.ys))(*plan.ys), (C.c_int * len(plan.xs))(*plan.xs)
wt = views.window_weights("gaussian", plan.h, plan.w).to(dev)


def do_gather():
    assert lib.sd_views_gather(ptr(lat0), ptr(windows), B, 4, Hc, Wc, plan.h, plan.w, ys, len(plan.ys), xs, len(plan.xs), 0,
                               stream()) == 0, lib.sd_last_error()


def do_merge(w=None):
    assert lib.sd_views_merge(ptr(outs), ptr(eps), ptr(w) if w is not None else None, G, B, 4, Hc, Wc, plan.h, plan.w, ys,
                              len(plan.ys), xs, len(plan.xs), 0, runner.vpc, stream()) == 0, lib.sd_last_error()


lat1 = lat0.clone()


def do_step():
    assert lib.sd_cfg_linear_step(ptr(eps), ptr(lat1), None, lat1.numel(), 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, stream()) == 0


for name, fn, nbytes in (
        ("sd_views_gather", do_gather, 2 * 2 * windows.numel()),
        ("sd_views_merge (uniform)", do_merge, 2 * (outs.numel() + eps.numel())),
        ("sd_views_merge (gaussian)", lambda: do_merge(wt), 2 * (outs.numel() + eps.numel())),
        ("sd_cfg_linear_step", do_step, 2 * (eps.numel() + 2 * lat1.numel()))):
    fn()
    ms = timed(fn, 200)
    say(f"  {name:28s} {ms * 1e3:7.1f} us per launch, {nbytes / 1024:8.0f} KiB moved, {nbytes / ms / 1e6:7.1f} GB/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
