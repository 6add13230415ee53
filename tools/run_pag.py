#!/usr/bin/env python3
"""Perturbed-attention guidance (GPU box): python tools/run_pag.py [--latents 4] [--latent 64] [--steps 50] [--layers mid]
Synthetic SD1.5 weights at the headline shape (4 latents, 64 x 64).  Prints
  * ms per forward (events around 20 forwards, the kinds alternating in one process, `--rounds` rounds) of
    sd_unet_forward_cfg (8 images), sd_unet_forward_pag with late widening (`share`) and with up-front duplication
    (12 images), and the ratios;
  * from the engine's event brackets (sd_prof_*): launches per forward of the three kinds;
  * ms per 50-step DDIM loop (the pipeline's "linear" device-step loop written out) without PAG (forward_cfg +
    sd_cfg_linear_step) and with it (forward_pag + sd_pag_linear_step), late and up front, alternating;
  * the box's probe (bench.py box_probe), so that runs on different boxes can be compared.
Synthetic weights: nothing here is an image-quality figure.  --out FILE also writes the text there (profiles/pag.txt is
one such run).  --tiny: config.tiny_unet at 16 x 16, 6 steps."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, schedulers, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--latents", type=int, default=4)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--layers", default="mid")
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ucfg = config.tiny_unet() if args.tiny else config.sd15_unet()
if args.tiny:
    args.latent, args.steps, args.latents = min(args.latent, 16), min(args.steps, 6), min(args.latents, 2)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


dev = "cuda"
B, hw = args.latents, args.latent
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


probe = box_probe()
sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
del sd
net.set_pag_layers(args.layers.split(","))
g = torch.Generator(device=dev).manual_seed(1)
lat0 = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16, generator=g)
ehs = torch.randn(2 * B, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16, generator=g)
sched = schedulers.DDIMScheduler()
KINDS = ("cfg", "pag late", "pag up front")


def forward(kind, lat=None, t=501.0, in_scale=1.0):
    lat = lat0 if lat is None else lat
    if kind == "cfg":
        return net.forward_cfg(lat, t, ehs, in_scale=in_scale)[0]
    return net.forward_pag(lat, t, ehs, in_scale=in_scale, share=kind == "pag late")[0]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def loop(kind):
    sched.set_timesteps(args.steps)
    lat = lat0.clone()
    net.text_kv_cache(True)
    try:
        for t in [float(v) for v in sched.timesteps.tolist()]:
            plan = sched.fused_plan(t)
            assert not plan.use_hist
            out = forward(kind, lat, t, plan.in_scale)
            new = lat.clone()
            if kind == "cfg":
                rc = lib.sd_cfg_linear_step(ptr(out), ptr(new), None, new.numel(), 7.5, plan.c_x, plan.c_eps, plan.c_hist,
                                            plan.h_x, plan.h_eps, stream())
            else:
                rc = lib.sd_pag_linear_step(ptr(out), 3, ptr(new), None, new.numel(), 7.5, 3.0, plan.c_x, plan.c_eps,
                                            plan.c_hist, plan.h_x, plan.h_eps, stream())
            assert rc == 0, lib.sd_last_error()
            sched.fused_commit()
            lat = new
    finally:
        net.text_kv_cache(False)
    return lat


say(f"perturbed-attention guidance, {'tiny' if args.tiny else 'sd15'} UNet, {B} latents {hw}x{hw}, layers {args.layers} -> "
    f"{', '.join(net.pag_layers)}; synthetic weights")
say("box_probe: " + json.dumps(probe))
for k in KINDS:                         # warm: plans, arena
    forward(k)
    forward(k)
fwd = {k: [] for k in KINDS}
for _ in range(args.rounds):
    for k in KINDS:
        fwd[k].append(timed(lambda: forward(k), 20))
say("")
say("ms per forward (20 forwards per sample, kinds alternating):")
med = {k: statistics.median(v) for k, v in fwd.items()}
for k in KINDS:
    imgs = 2 * B if k == "cfg" else 3 * B
    say(f"  {k:13s} {imgs:3d} images  median {med[k]:8.3f}  ({' '.join(f'{v:.3f}' for v in fwd[k])})  x{med[k] / med['cfg']:.3f} of cfg")
say(f"  late widening / up-front duplication: {med['pag late'] / med['pag up front']:.3f}")

say("")
say("launches per forward (engine event brackets):")
for k in KINDS:
    lib.sd_prof_enable(1)
    forward(k)
    ents = (_lib.SdProfEntry * 256)()
    n = C.c_int(0)
    assert lib.sd_prof_collect(ents, 256, C.byref(n)) == 0, lib.sd_last_error()
    lib.sd_prof_enable(0)
    got = min(n.value, 256)
    launches = sum(e.launches for e in ents[:got])
    dup = [e for e in ents[:got] if e.kernel.decode() == "row_dup_kernel"]
    say(f"  {k:13s} {launches:5d} launches; row_dup_kernel: {sum(e.launches for e in dup)} launches, "
        f"{sum(e.bytes for e in dup) / 1e6:.2f} MB moved, {sum(e.ms for e in dup) * 1e3:.1f} us")

say("")
say(f"ms per {args.steps}-step DDIM loop (text K/V cache on, kinds alternating):")
for k in KINDS:
    loop(k)
lp = {k: [] for k in KINDS}
for _ in range(args.rounds):
    for k in KINDS:
        lp[k].append(timed(lambda: loop(k), 1))
lmed = {k: statistics.median(v) for k, v in lp.items()}
for k in KINDS:
    say(f"  {k:13s} median {lmed[k]:9.2f}  ({' '.join(f'{v:.2f}' for v in lp[k])})  x{lmed[k] / lmed['cfg']:.3f} of cfg")
say(f"  late widening / up-front duplication: {lmed['pag late'] / lmed['pag up front']:.3f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
