#!/usr/bin/env python3
"""InstructPix2Pix (GPU box): python tools/run_pix2pix.py [--latents 4] [--latent 64] [--steps 20] [--rounds 3]
An SD1.5-width UNet with in_channels = 8 on synthetic weights at the headline shape (4 latents, 64 x 64, 12 rows).  Prints
  * ms per step and engine launches per step of the new path: sd_unet_forward_concat on the un-duplicated latents and
    the image latents, then sd_ip2p_linear_step (the pipeline's "linear" loop written out, DDIM);
  * the same for the path without it: the 8-channel sample built with torch every step (cat x 3, scale, cat against a
    [3B, 4, H, W] image-latent tensor), the plain forward, pix2pix.combine and scheduler.step on the host;
  * sd_op_unet_conv_in2 per launch for that problem, and what the general path spends on it: a child process under
    SD_NO_EDGE_KERNELS=1 reports concat_sample_kernel and im2col_nchw3x3_kernel from the engine's event brackets, and
    sd_bench_conv2d times the K = 128 GEMM behind them;
  * the box's probe (bench.py box_probe), so that runs on different boxes can be compared.
Synthetic weights: nothing here is an image-quality figure.  --out FILE also writes the text there (profiles/pix2pix.txt
is one such run).  --tiny: the width-reduced 320-wide test configuration at 16 x 16, 6 steps."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, pix2pix, schedulers, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--latents", type=int, default=4)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--general-only", action="store_true", help="(the child run: print the general path's conv_in brackets)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.tiny:
    ucfg = config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=8, block_out_channels=(320, 128, 256, 256),
                                    attention_head_dim=(8, 4, 8, 8)))
    args.latent, args.steps, args.latents = min(args.latent, 16), min(args.steps, 6), min(args.latents, 2)
else:
    ucfg = config.UNetConfig(**dict(config.sd15_unet().to_dict(), in_channels=8))
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
G_T, G_I = 7.5, 1.5
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


def brackets(fn):
    """{kernel: (launches, ms)} of one call of fn, from the engine's event brackets."""
    lib.sd_prof_enable(1)
    try:
        fn()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int(0)
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {e.kernel.decode(): (e.launches, e.ms) for e in ents[:min(n.value, 512)]}


sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
del sd
g = torch.Generator(device=dev).manual_seed(1)
lat0 = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16, generator=g)
img = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16, generator=g)
ehs = torch.randn(3 * B, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16, generator=g)
img_rows = pix2pix.image_rows(img)


def forward_new(lat=lat0, t=501.0, in_scale=1.0):
    return net.forward_concat(lat, t, ehs, img, zero_from=2 * B, in_scale=in_scale)[0]


def forward_old(lat=lat0, t=501.0, in_scale=1.0):
    x = torch.cat([lat] * 3) * in_scale
    return net(torch.cat([x, img_rows], dim=1), t, ehs)[0]


if args.general_only:
    forward_new()
    got = brackets(forward_new)
    print(json.dumps({k: got[k] for k in ("concat_sample_kernel", "im2col_nchw3x3_kernel", "conv_head2_kernel") if k in got}))
    sys.exit(0)

probe = box_probe()
sched = schedulers.DDIMScheduler()


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
            if kind == "new":
                plan = sched.fused_plan(t)
                assert not plan.use_hist
                out = forward_new(lat, t, plan.in_scale)
                new = lat.clone()
                rc = lib.sd_ip2p_linear_step(ptr(out), ptr(new), None, new.numel(), G_T, G_I, plan.c_x, plan.c_eps,
                                             plan.c_hist, plan.h_x, plan.h_eps, stream())
                assert rc == 0, lib.sd_last_error()
                sched.fused_commit()
                lat = new
            else:
                x = sched.scale_model_input(torch.cat([lat] * 3), t)
                out = net(torch.cat([x, img_rows], dim=1), t, ehs)[0]
                lat = sched.step(pix2pix.combine(out, G_T, G_I), t, lat, return_dict=False)[0]
    finally:
        net.text_kv_cache(False)
    return lat


KINDS = ("new", "torch-built")
say(f"InstructPix2Pix, {'width-reduced' if args.tiny else 'sd15-width'} UNet with in_channels = 8, {B} latents {hw}x{hw}, "
    f"{3 * B} rows; synthetic weights")
say("box_probe: " + json.dumps(probe))
for fn in (forward_new, forward_old):                    # warm: plans, arena
    fn()
    fn()
say("")
say("engine launches per forward (event brackets; the torch ops of the torch-built path are not in them):")
for name, fn in (("forward_concat", forward_new), ("cat + scale + cat + forward", forward_old)):
    got = brackets(fn)
    head = {k: v for k, v in got.items() if k in ("conv_head2_kernel", "concat_sample_kernel", "im2col_nchw3x3_kernel",
                                                  "conv_head_kernel")}
    say(f"  {name:28s} {sum(v[0] for v in got.values()):5d} launches, {sum(v[1] for v in got.values()):8.3f} ms in brackets; "
        + ", ".join(f"{k} {v[0]} x {v[1] * 1e3 / max(v[0], 1):.1f} us" for k, v in head.items()))
say("  new path per step: the forward's launches + 1 (sd_ip2p_linear_step), no torch op but the latents' clone")
say("  torch-built per step: 3 torch launches for the sample (cat, mul, cat), the forward's, the host combine and scheduler.step")

say("")
say(f"ms per step over a {args.steps}-step DDIM loop (text K/V cache on, kinds alternating):")
for k in KINDS:
    loop(k)
lp = {k: [] for k in KINDS}
for _ in range(args.rounds):
    for k in KINDS:
        lp[k].append(timed(lambda: loop(k), 1) / args.steps)
med = {k: statistics.median(v) for k, v in lp.items()}
for k in KINDS:
    say(f"  {k:12s} median {med[k]:8.3f}  ({' '.join(f'{v:.3f}' for v in lp[k])})  x{med[k] / med['torch-built']:.3f} of torch-built")

say("")
say(f"conv_in of that problem ({3 * B} images, 4 + 4 channels, {hw}x{hw}):")
H = W = hw
Cout = 320
w = (torch.randn(Cout, 8, 3, 3, device=dev, generator=g) / 72 ** 0.5).half()
bias = torch.zeros(Cout, device=dev)
y = torch.empty(3 * B * H * W, Cout, device=dev, dtype=torch.float16)
summ = torch.empty(3 * B * (H * W // 128) * 32 * 2, device=dev)
ms = C.c_float()
rc = lib.sd_op_unet_conv_in2(ptr(lat0), B, 4, 0.5, ptr(img), B, 4, 2 * B, ptr(w), ptr(bias), ptr(y), Cout, ptr(summ), 32, 3 * B,
                             H, W, Cout, 50, C.byref(ms), stream())
if rc == 0:
    say(f"  sd_op_unet_conv_in2 (conv_head2_kernel, summaries on): {ms.value * 1e3:.1f} us per launch, "
        f"{2.0 * y.numel() / ms.value / 1e6:.0f} GB/s of output")
else:
    say("  sd_op_unet_conv_in2: " + lib.sd_last_error().decode())
col = torch.randn(3 * B, H, W, 128, device=dev, generator=g).half()
w1 = (torch.randn(Cout, 128, 1, 1, device=dev, generator=g) / 128 ** 0.5).half()
gm = C.c_float()
_lib.check(lib.sd_bench_conv2d(ptr(col), ptr(w1), ptr(y), 3 * B, H, W, 128, Cout, 1, 1, 0, 0, 50, C.byref(gm), stream()),
           "sd_bench_conv2d")
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--general-only", "--latents", str(B), "--latent", str(hw)]
                       + (["--tiny"] if args.tiny else []), env=dict(os.environ, SD_NO_EDGE_KERNELS="1"),
                       capture_output=True, text=True, timeout=600)
gen = json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0 and child.stdout.strip() else {}
parts = {k: v[1] * 1e3 / max(v[0], 1) for k, v in gen.items()}
say(f"  general path (SD_NO_EDGE_KERNELS=1): " + ", ".join(f"{k} {v:.1f} us" for k, v in parts.items())
    + f", K = 128 GEMM {gm.value * 1e3:.1f} us (sd_bench_conv2d) = {sum(parts.values()) + gm.value * 1e3:.1f} us")
if child.returncode != 0:
    say("  (the child run failed: " + child.stderr.strip().splitlines()[-1][:200] + ")")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
