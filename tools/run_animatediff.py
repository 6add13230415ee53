#!/usr/bin/env python3
"""AnimateDiff on the engine (GPU box): python tools/run_animatediff.py [--out FILE] [--tiny] [--skip-loop]
Synthetic weights.  Prints
  * per SD 1.5 level (C / HW = 320 / 64^2, 640 / 32^2, 1280 / 16^2, 1280 / 8^2; V = 2 videos of F = 16 frames, 8 heads):
    the temporal attention launch (sd_op_temporal_attention on the q|k|v rows in place), its bytes over the box's
    sd_probe_copy rate, and the route through the code that existed before it, built only here -- a torch permute copy of
    the q|k|v rows to [V HW, F, 3C], sd_op_attention_ex, a torch permute copy of the output back -- the two routes
    alternating over --rounds passes in one process, with the run-to-run spread of each;
  * one UNet forward with the motion adapter attached (num_frames = 16) against the plain forward on the same V F frames:
    ms, ratio, launches;
  * the 16-frame, 512 px, 25-step loop (`animate`, DDIM, CFG) in seconds, latents out.
Image quality is NOT judged: the weights are synthetic.  --out FILE also writes the text there (profiles/animatediff.txt
is one such run).  --tiny: config.tiny_unet at 16 x 16 latents with the tiny adapter."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, animatediff, config, motion, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipMotionAdapter, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--skip-loop", action="store_true")
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
copy = C.c_float()
_lib.check(lib.sd_probe_copy(512 << 20, 5, C.byref(copy), stream()), "sd_probe_copy")
say(f"box probe: sd_probe_copy {copy.value:.0f} GB/s (read + write); device {torch.cuda.get_device_name(0)}")
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


def attention_site(V, F, HW, heads, d):
    Cw, M = heads * d, V * F * HW
    qkv = torch.randn(M, 3 * Cw, device="cuda").half()
    table = (0.5 * torch.randn(32, 3 * Cw, device="cuda")).contiguous()
    out = torch.empty(M, Cw, device="cuda").half()
    o2 = torch.empty(M, Cw, device="cuda").half()

    def fused():
        _lib.check(lib.sd_op_temporal_attention(P(qkv), P(qkv[:, Cw:]), P(qkv[:, 2 * Cw:]), P(out), P(table), 3 * Cw, 3 * Cw, 3 * Cw,
                                                Cw, 3 * Cw, V, F, HW, heads, d, 1, stream()), "sd_op_temporal_attention")

    def route():
        # (the position term would be one more pass over q|k|v on this route; it is left out in its favour)
        p = qkv.view(V, F, HW, 3 * Cw).permute(0, 2, 1, 3).contiguous().view(M, 3 * Cw)
        _lib.check(lib.sd_op_attention_ex(P(p), P(p[:, Cw:]), P(p[:, 2 * Cw:]), P(o2), V * HW, F, F, heads, d, 3 * Cw, 3 * Cw, 3 * Cw,
                                          Cw, 0, 1, stream()), "sd_op_attention_ex")
        return o2.view(V, HW, F, Cw).permute(0, 2, 1, 3).contiguous()

    tf, tr = [], []
    for _ in range(args.rounds):
        tf.append(events(fused, args.iters))
        tr.append(events(route, args.iters))
    mf, mr = statistics.median(tf), statistics.median(tr)
    bytes_fused = 2.0 * M * 4 * Cw
    plan = (C.c_int64 * 7)()
    _lib.check(lib.sd_temporal_attention_plan(V, F, HW, heads, d, plan), "sd_temporal_attention_plan")
    say(f"  C {Cw:4d}, HW {HW:5d} (V {V}, F {F}, {heads} heads x d {d}; plan: {plan[2]} pixels x {plan[3]} waves per block, "
        f"PV 16x16x{plan[4]}, {plan[5]} B LDS, {plan[6]} blocks)")
    say(f"    temporal_attn_kernel     {mf * 1e3:9.1f} us  (min {min(tf) * 1e3:.1f}, max {max(tf) * 1e3:.1f})  {bytes_fused / 1e6:7.1f} MB, "
        f"{bytes_fused / mf / 1e6:6.0f} GB/s = {100 * bytes_fused / mf / 1e6 / copy.value:4.1f} % of sd_probe_copy")
    say(f"    permute + attn + permute {mr * 1e3:9.1f} us  (min {min(tr) * 1e3:.1f}, max {max(tr) * 1e3:.1f})  x{mr / mf:5.2f} of the fused launch; "
        f"spreads {'do not overlap' if min(tr) > max(tf) else 'OVERLAP'}")
    del qkv, out, o2


say()
say("temporal attention, per level (median of %d alternating passes of %d launches):" % (args.rounds, args.iters))
levels = [(64, 16 * 16, 2, 32)] if args.tiny else [(320, 64 * 64, 8, 40), (640, 32 * 32, 8, 80), (1280, 16 * 16, 8, 160),
                                                     (1280, 8 * 8, 8, 160)]
for Cw, HW, heads, d in levels:
    attention_site(2, 16, HW, heads, d)

# ---- one forward with and without the modules ----
ucfg = config.tiny_unet() if args.tiny else config.sd15_unet()
mcfg = motion.tiny_motion_adapter(ucfg) if args.tiny else motion.MotionAdapterConfig()
lat = 16 if args.tiny else 64
V, F = 2, 16
usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=1, perturb=0.1)
net = HipUNet2DConditionModel(ucfg, "cuda").load_state_dict(usd)
adapter = HipMotionAdapter(net, mcfg).load_state_dict(motion.synth_state_dict(mcfg, 2))
net.attach_motion_adapter(adapter)
x = torch.randn(V * F, 4, lat, lat, device="cuda").half()
ehs = torch.randn(V, 1, 77, ucfg.cross_attention_dim, device="cuda").half().expand(V, F, -1, -1).reshape(V * F, 77, -1).contiguous()
t = torch.tensor(501.0)


def launches(fn):
    lib.sd_prof_enable(1)
    try:
        fn()
        ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {ents[i].kernel.decode(): (int(ents[i].launches), float(ents[i].ms)) for i in range(n.value)}


plain_fn = lambda: net(x, t, ehs)
motion_fn = lambda: net(x, t, ehs, num_frames=F)
tp, tm = [], []
for _ in range(3):
    tp.append(events(plain_fn, 3))
    tm.append(events(motion_fn, 3))
lp, lm = launches(plain_fn), launches(motion_fn)
say()
say(f"UNet forward on {V} x {F} frames of {lat} x {lat} latents (median of 3 alternating passes):")
say(f"  plain                    {statistics.median(tp):8.2f} ms, {sum(v[0] for v in lp.values())} launches")
say(f"  with 21 motion modules   {statistics.median(tm):8.2f} ms, {sum(v[0] for v in lm.values())} launches  "
    f"x{statistics.median(tm) / statistics.median(tp):.3f}")
ta = {k: v for k, v in lm.items() if k.startswith("temporal_attn_kernel")}
say("  temporal attention launches: " + ", ".join(f"{k} x{v[0]} {v[1]:.3f} ms" for k, v in sorted(ta.items())))
say("  groupnorm launches of the modules run their own statistics pass over a whole video")

if not args.skip_loop:
    vcfg = config.tiny_vae() if args.tiny else config.sd15_vae()
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), 2, perturb=0.1)
    model = SDModelWrapper(base=net, vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), device="cuda")
    model.set_scheduler("DDIM")
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    pos, neg = (torch.randn(1, 77, ucfg.cross_attention_dim, device="cuda").half() for _ in range(2))
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_frames=16, height=8 * lat, width=8 * lat, num_inference_steps=25,
              guidance_scale=7.5, seed=0, output_type="latents")
    animatediff.animate(pipe, model, None, **{**kw, "num_inference_steps": 2})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    animatediff.animate(pipe, model, None, **kw)
    torch.cuda.synchronize()
    say()
    say(f"animate: 1 video x 16 frames, {8 * lat} px, 25 DDIM steps under CFG, latents out: {time.perf_counter() - t0:.2f} s")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
