#!/usr/bin/env python3
"""HyperTile on the UNet forward (GPU box): python tools/run_hypertile.py [--out FILE] [--tiny] [--skip-sdxl]
Synthetic weights.  For SD1.5 at B 8 / 64 x 64 and B 2 / 128 x 128 latents (max_depth 0) and SDXL at B 4 / 128 x 128
latents (max_depth 1: its level 0 has no attention) prints
  * ms per UNet forward (events around --iters forwards, forward i under hypertile_step(i)) plain and with tile_size 32
    at swap_size 1 and 2, the settings alternating over --rounds passes in one process, and the ratio against plain,
  * from the engine's event brackets (sd_prof_*) over those steps: the gather / scatter launches and their time, the
    attention time plain and tiled, and the FLOPs the counts predict,
  * per site of the shallowest level with attention, at operator level: the attention launch plain against every
    division the rule offers, and the gather / scatter launches with their GB/s next to the box's sd_probe_copy rate.
Image quality is NOT judged: the weights are synthetic.  --out FILE also writes the text there (profiles/hypertile.txt
is one such run).  --tiny: config.tiny_unet at 16 x 16 with tile_size 8."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, hypertile, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--skip-sdxl", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def P(t):
    return C.c_void_p(t.data_ptr())


lib = _lib.load()
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
mfma, copy = C.c_float(), C.c_float()
_lib.check(lib.sd_probe_mfma(100000, C.byref(mfma), stream()), "sd_probe_mfma")
_lib.check(lib.sd_probe_copy(512 << 20, 5, C.byref(copy), stream()), "sd_probe_copy")
say(f"box probe: sd_probe_mfma {mfma.value:.1f} TFLOP/s, sd_probe_copy {copy.value:.0f} GB/s (read + write); "
    f"device {torch.cuda.get_device_name(0)}")
say("synthetic weights: timings only, image quality is not judged")


def events(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def profile(run):
    lib.sd_prof_enable(1)
    try:
        run()
        ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {ents[i].kernel.decode(): (float(ents[i].ms), int(ents[i].launches), float(ents[i].flops), float(ents[i].bytes))
            for i in range(n.value)}


def site_ops(B, Hs, Ws, heads, d, tile, swap):
    """One self-attention site at operator level: plain against every division of the rule."""
    Cw, T = heads * d, Hs * Ws
    M = B * T
    qkv = torch.randn(M, 3 * Cw, device="cuda").half()
    qg, og, out = qkv.clone(), torch.empty(M, Cw, device="cuda").half(), torch.empty(M, Cw, device="cuda").half()

    def attn(buf, dst, batch, tokens):
        _lib.check(lib.sd_op_attention_ex(P(buf[:, :Cw]), P(buf[:, Cw:2 * Cw]), P(buf[:, 2 * Cw:]), P(dst), batch, tokens, tokens,
                                          heads, d, 3 * Cw, 3 * Cw, 3 * Cw, Cw, 0, 1, stream()), "sd_op_attention_ex")

    divs = [(nh, nw) for nh in hypertile.counts(Hs, tile, swap) for nw in hypertile.counts(Ws, tile, swap)]
    t = {k: [] for k in ["plain"] + divs}
    tg, ts = [], []
    for _ in range(args.rounds):
        t["plain"].append(events(lambda: attn(qkv, out, B, T), args.iters))
        for nh, nw in divs:
            src = qkv if nw == 1 else qg
            t[(nh, nw)].append(events(lambda: attn(src, og, B * nh * nw, T // (nh * nw)), args.iters))
        nh, nw = divs[0]
        tg.append(events(lambda: _lib.check(lib.sd_op_hypertile_gather(P(qkv), 3 * Cw, 3 * Cw, B, Hs, Ws, nh, max(nw, 2), P(qg), 3 * Cw,
                                                                       stream()), "gather"), args.iters))
        ts.append(events(lambda: _lib.check(lib.sd_op_hypertile_scatter(P(og), Cw, Cw, B, Hs, Ws, nh, max(nw, 2), P(out), Cw, stream()),
                                            "scatter"), args.iters))
    plain = statistics.median(t["plain"])
    say(f"  one site at operator level: B {B}, {Hs} x {Ws} tokens, {heads} heads x d {d} (median of {args.rounds} alternating passes)")
    say(f"    attention plain          {plain * 1e3:9.1f} us")
    for nh, nw in divs:
        m = statistics.median(t[(nh, nw)])
        say(f"    attention tiled {nh} x {nw}      {m * 1e3:9.1f} us  x{plain / m:6.2f} (FLOPs fall x{nh * nw})"
            + ("  [band: no copy]" if nw == 1 and nh > 1 else ""))
    g, s = statistics.median(tg), statistics.median(ts)
    gb, sb = 12.0 * M * Cw, 4.0 * M * Cw
    say(f"    hypertile_gather_kernel  {g * 1e3:9.1f} us  {gb / 1e6:7.1f} MB moved, {gb / g / 1e6:6.0f} GB/s = "
        f"{100 * gb / g / 1e6 / copy.value:4.1f} % of sd_probe_copy")
    say(f"    hypertile_scatter_kernel {s * 1e3:9.1f} us  {sb / 1e6:7.1f} MB moved, {sb / s / 1e6:6.0f} GB/s = "
        f"{100 * sb / s / 1e6 / copy.value:4.1f} % of sd_probe_copy")
    del qkv, qg, og, out


def build(ucfg):
    sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=1, perturb=0.1)
    return HipUNet2DConditionModel(ucfg).load_state_dict({k: v.half() for k, v in sd.items()})


def measure(name, net, B, hw, depth, tile, added_fn):
    ucfg = net.cfg
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 4, hw, hw, generator=g).half().cuda()
    ehs = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    added = added_fn(B) if added_fn else None
    t = torch.tensor(501.0)
    step = [0]
    modes = [None, 1, 2]                                    # plain, swap_size 1, swap_size 2

    def setup(swap):
        if swap is None:
            net.disable_hypertile()
        else:
            net.enable_hypertile(tile, swap, depth, 0)
        step[0] = 0

    def run():
        if net.hypertile is not None:
            net.hypertile_step(step[0])                    # forward i of a pass runs under step i, as the pipeline's loop
        step[0] += 1
        return net(x, t, ehs, added_cond_kwargs=added)

    times = {m: [] for m in modes}
    for m in modes:                                         # plans and buffers first
        setup(m)
        run()
    for _ in range(args.rounds):
        for m in modes:
            setup(m)
            run()
            step[0] = 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1) / args.iters)
    say()
    say(f"{name} UNet forward, B {B}, {hw} x {hw} latents, tile_size {tile}, max_depth {depth}: ms per forward over steps "
        f"0..{args.iters - 1} (median of {args.rounds} alternating passes; all passes)")
    off = statistics.median(times[None])
    for m in modes:
        med = statistics.median(times[m])
        label = "plain      " if m is None else f"swap_size {m}"
        say(f"  {label}: {med:8.3f} ms  x{off / med:5.3f} vs plain   {['%.3f' % v for v in times[m]]}")

    def steps():
        for _ in range(args.iters):
            run()

    setup(None)
    p_off = profile(steps)
    for swap in (1, 2):
        setup(swap)
        p_on = profile(steps)
        sites = net.hypertile_sites()
        n = args.iters
        a_off = sum(v[0] for k, v in p_off.items() if k.startswith("attn_kernel")) / n
        a_on = sum(v[0] for k, v in p_on.items() if k.startswith("attn_kernel")) / n
        f_off = sum(v[2] for k, v in p_off.items() if k.startswith("attn_kernel")) / n
        f_on = sum(v[2] for k, v in p_on.items() if k.startswith("attn_kernel")) / n
        gk, sk = p_on.get("hypertile_gather_kernel", (0, 0, 0, 0)), p_on.get("hypertile_scatter_kernel", (0, 0, 0, 0))
        say(f"  swap_size {swap}, per forward (engine event brackets over {n} steps; {len(sites)} sites take part):")
        say(f"    all attention launches   plain {a_off:8.3f} ms ({f_off / 1e12:6.3f} TFLOP) -> tiled {a_on:8.3f} ms ({f_on / 1e12:6.3f} TFLOP)")
        for k, v in (("hypertile_gather_kernel", gk), ("hypertile_scatter_kernel", sk)):
            if v[1]:
                say(f"    {k:24s} {v[0] / n:8.3f} ms in {v[1] / n:4.1f} launches, {v[3] / 1e6 / n:8.1f} MB, "
                    f"{v[3] / v[0] / 1e6:6.0f} GB/s = {100 * v[3] / v[0] / 1e6 / copy.value:4.1f} % of sd_probe_copy")
        say(f"    attention saved {a_off - a_on:7.3f} ms, copies cost {(gk[0] + sk[0]) / n:7.3f} ms; sum of launches plain "
            f"{sum(v[0] for v in p_off.values()) / n:.3f} ms, tiled {sum(v[0] for v in p_on.values()) / n:.3f} ms")
    setup(None)


def sdxl_added(B):
    return {"text_embeds": torch.randn(B, 1280).half().cuda(),
            "time_ids": torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * B)}


if args.tiny:
    measure("tiny", build(config.tiny_unet()), 2, 16, 0, 8, None)
    site_ops(2, 16, 16, 2, 32, 8, 2)
else:
    net = build(config.sd15_unet())
    measure("SD1.5", net, 8, 64, 0, 32, None)
    site_ops(8, 64, 64, 8, 40, 32, 2)
    measure("SD1.5", net, 2, 128, 0, 32, None)
    site_ops(2, 128, 128, 8, 40, 32, 2)
    del net
    torch.cuda.empty_cache()
    if not args.skip_sdxl:
        measure("SDXL", build(config.sdxl_unet()), 4, 128, 1, 32, sdxl_added)
        site_ops(4, 64, 64, 10, 64, 32, 2)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
