#!/usr/bin/env python3
"""Time the IP-Adapter Plus Resampler (GPU box):  python tools/run_resampler.py [--iters 50] [--reps 3] [--no-unet]

Three sections, appended to profiles/resampler.txt; every comparison alternates its sides inside one process:
  1. the Resampler forward alone (sd_ip_adapter_project) at the SD1.5-Plus (dim 768, 12 heads) and SDXL-Plus (dim 1280,
     20 heads) sizes -- D_emb 1280, depth 4, 16 queries, 257 feature rows -- for 2 and 8 images: ms per forward between
     events, bracketed launches per forward and its kernels (sd_prof_*), and rel-L2 of the tokens against the float64
     oracle of tests/resampler_oracle.py;
  2. resampler_attn_kernel against the composed form (two concatenation copies + attn_kernel<64> on the concatenated
     K | V) through sd_op_resampler_attention's timing mode, operands laid out as the graph holds them;
  3. the SD1.5 UNet forward (B 8, 64 x 64 latents, text and image K / V caches on): plain, with a 4-token base adapter,
     with a 16-token Plus adapter whose Resampler ran in the warm-up forward (steady state: the per-step cost).
No number here is a pass / fail bound."""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resampler_oracle as ro  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resampler.txt"))
args = ap.parse_args()
lib = _lib.load()
dev = "cuda"
log = open(args.out, "a")
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def say(s=""):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


def events(fn, iters):
    for _ in range(3):
        fn()
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    t.record()
    t.synchronize()
    return s.elapsed_time(t) / iters


def profiled(fn):
    fn()
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    try:
        fn()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return sorted(((e.kernel.decode(), e.launches, e.ms) for e in ents[: n.value]), key=lambda r: -r[2])


SIZES = {"sd15-plus": ("sd15", 768, 12), "sdxl-plus": ("sdxl", 1280, 20)}
say(f"# tools/run_resampler.py --iters {args.iters} --reps {args.reps} on {torch.cuda.get_device_name(0)}")
say("# 1. Resampler forward (D_emb 1280, depth 4, 16 queries, T_feat 257), ms between events; launches are the bracketed ones")
adapters = {}
for name, (preset, dim, heads) in SIZES.items():
    cfg = config.PRESETS[preset][0]()
    net = HipUNet2DConditionModel(cfg, dev)
    sd = ro.synth_resampler_state_dict(cfg, 1280, dim, heads, 4, 16, seed=22)
    adapters[name] = (net.make_ip_adapter(sd, 1280, 16), sd, net)
for rep in range(args.reps):
    for name, (ad, sd, _) in adapters.items():
        for rows in (2, 8):
            x = torch.randn(rows, 257, 1280, generator=torch.Generator().manual_seed(rows)).half().to(dev)
            ms = events(lambda: ad.project(x), args.iters)
            line = f"{name} images={rows} rep {rep}: {ms * 1e3:.1f} us per forward"
            if rep == 0:
                prof = profiled(lambda: ad.project(x))
                err = float((ad.project(x).double().cpu() - ro.resampler_forward(sd, x.float().cpu())).norm()
                            / ro.resampler_forward(sd, x.float().cpu()).norm())
                line += f"  launches {sum(r[1] for r in prof)}  tokens rel-L2 vs float64 oracle {err:.2e}"
                say(line)
                say("    " + "; ".join(f"{k} x{n} {t * 1e3:.1f} us" for k, n, t in prof[:6]))
            else:
                say(line)

say("# 2. resampler_attn_kernel vs composed (2 concat copies + attn_kernel<64>), T_feat 257, n_q 16, prescaled q, k | v slices")
ms2 = (C.c_float * 2)()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for rep in range(args.reps):
    for heads in (12, 20):
        for B in (2, 8):
            A = heads * 64
            g = torch.Generator(device=dev).manual_seed(heads + B)
            q = (torch.randn(B * 16, A, device=dev, generator=g) * (ro.LOG2E / 8)).half()
            kvx = torch.randn(B * 257, 2 * A, device=dev, generator=g).half()
            kvl = torch.randn(B * 16, 2 * A, device=dev, generator=g).half()
            out = torch.empty(B * 16, A, device=dev, dtype=torch.float16)
            rc = lib.sd_op_resampler_attention(P(q), P(kvx), P(kvx[:, A:]), P(kvl), P(kvl[:, A:]), P(out), B, 16, 257, heads, A,
                                               2 * A, 2 * A, 2 * A, 2 * A, A, 1, 4 * args.iters, ms2, st)
            _lib.check(rc, "sd_op_resampler_attention")
            say(f"heads={heads} images={B} rep {rep}: resampler_attn_kernel {ms2[0] * 1e3:.2f} us  composed {ms2[1] * 1e3:.2f} us  "
                f"kernel/composed {ms2[0] / ms2[1]:.2f}")

if not args.no_unet:
    say("# 3. SD1.5 UNet forward, B=8, 64x64 latents, K/V caches on (steady state), alternating")
    cfg = config.sd15_unet()
    ad_plus, _, net = adapters["sd15-plus"]
    net.load_state_dict(weights.synth_state_dict(weights.unet_manifest(cfg), seed=2, dtype=torch.float16))
    ad_base = HipIPAdapter(net, 1024, 4).load_state_dict(synth_ip_state_dict(cfg, 1024, 4, seed=3))
    B, hw = 8, 64
    x = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16)
    e = torch.randn(B, 77, cfg.cross_attention_dim, device=dev, dtype=torch.float16)
    emb = {None: None, ad_base: torch.randn(B, 1, 1024, device=dev, dtype=torch.float16),
           ad_plus: torch.randn(B, 1, 257, 1280, device=dev, dtype=torch.float16)}

    def unet_ms(ad):
        net.attach_ip_adapter(ad)
        kw = {"image_embeds": [emb[ad]]} if ad is not None else None
        net.text_kv_cache(True)
        ms = events(lambda: net(x, 501.0, e, added_cond_kwargs=kw), 20)
        net.text_kv_cache(False)
        return ms

    for rep in range(args.reps):
        a, b, c = unet_ms(None), unet_ms(ad_base), unet_ms(ad_plus)
        say(f"sd15 B=8 64x64 rep {rep}: plain {a:.3f} ms  4-token base adapter {b:.3f} ms (ratio {b / a:.3f})  "
            f"16-token Plus adapter {c:.3f} ms (ratio {c / a:.3f})")
    net.attach_ip_adapter(None)
