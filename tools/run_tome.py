#!/usr/bin/env python3
"""Token merging on the UNet forward (GPU box): python tools/run_tome.py [--out FILE] [--tiny]
Synthetic SD1.5 weights.  For B 8 / 64 x 64 latents and B 2 / 128 x 128 latents prints
  * ms per UNet forward (events around 10 forwards) with token merging off and at ratio 0.25 / 0.5, the settings
    alternating over --rounds passes in one process, and the ratio against the off forwards,
  * from the engine's event brackets (sd_prof_*) per forward: the time and launches of the new kernels, the attention
    launches off (at T) and on (at T'), and the match kernel's TFLOP/s against the box's sd_probe_mfma rate.
Image quality is NOT judged: the weights are synthetic.  --out FILE also writes the text there (profiles/tome.txt is one
such run).  --tiny: config.tiny_unet at 16 x 16."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ucfg = config.tiny_unet() if args.tiny else config.sd15_unet()
SHAPES = [(2, 16)] if args.tiny else [(8, 64), (2, 128)]
RATIOS = [0.0, 0.25, 0.5]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


lib = _lib.load()
sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=1, perturb=0.1)
net = HipUNet2DConditionModel(ucfg).load_state_dict({k: v.half() for k, v in sd.items()})
del sd
probe = C.c_float()
_lib.check(lib.sd_probe_mfma(100000, C.byref(probe), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sd_probe_mfma")
say(f"box probe: sd_probe_mfma {probe.value:.1f} TFLOP/s; device {torch.cuda.get_device_name(0)}")
say("synthetic weights: timings only, image quality is not judged")


def setup(ratio):
    if ratio > 0:
        net.enable_tome(ratio, seed=1)
    else:
        net.disable_tome()


def profile(run):
    lib.sd_prof_enable(1)
    try:
        run()
        ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {ents[i].kernel.decode(): (float(ents[i].ms), int(ents[i].launches), float(ents[i].flops)) for i in range(n.value)}


for B, hw in SHAPES:
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 4, hw, hw, generator=g).half().cuda()
    ehs = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    t = torch.tensor(501.0)
    run = lambda: net(x, t, ehs)
    times = {r: [] for r in RATIOS}
    for r in RATIOS:                        # plans and buffers first
        setup(r)
        run()
    for _ in range(args.rounds):
        for r in RATIOS:
            setup(r)
            run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[r].append(e0.elapsed_time(e1) / args.iters)
    say()
    say(f"UNet forward, B {B}, {hw} x {hw} latents, ms (median of {args.rounds} alternating passes of {args.iters} forwards; all passes)")
    off = statistics.median(times[0.0])
    for r in RATIOS:
        m = statistics.median(times[r])
        say(f"  ratio {r:4.2f}: {m:8.3f} ms  x{off / m:5.3f} vs off   {['%.3f' % v for v in times[r]]}")
    setup(0.0)
    p_off = profile(run)
    for r in RATIOS[1:]:
        setup(r)
        p_on = profile(run)
        say(f"  per forward at ratio {r} (engine event brackets):")
        for k in ("tome_prep_kernel", "tome_match_kernel", "tome_select_kernel", "tome_merge_kernel", "tome_unmerge_kernel"):
            ms, n, fl = p_on[k]
            extra = f", {fl / ms / 1e9:7.1f} TFLOP/s = {100 * fl / ms / 1e9 / probe.value:4.1f} % of the probe" if fl > 0 else ""
            say(f"    {k:22s} {ms:7.3f} ms in {n} launches{extra}")
        new = sum(v[0] for k, v in p_on.items() if k.startswith("tome_"))
        for k in sorted(p_off):
            if k.startswith("attn_kernel") and p_on.get(k, p_off[k])[2] != p_off[k][2]:
                say(f"    {k:22s} off {p_off[k][0]:7.3f} ms -> on {p_on[k][0]:7.3f} ms ({p_off[k][1]} launches, self-attention at T -> T')")
        a_off = sum(v[0] for k, v in p_off.items() if k.startswith("attn_kernel"))
        a_on = sum(v[0] for k, v in p_on.items() if k.startswith("attn_kernel"))
        say(f"    attention saved {a_off - a_on:7.3f} ms, new kernels cost {new:7.3f} ms; sum of launches off "
            f"{sum(v[0] for v in p_off.values()):.3f} ms, on {sum(v[0] for v in p_on.values()):.3f} ms")
    setup(0.0)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
