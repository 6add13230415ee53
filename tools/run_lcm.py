#!/usr/bin/env python3
"""Time the 4-step LCM loop with the device step (sd_lcm_step) and with the host scheduler.step (GPU box):
python tools/run_lcm.py [--loops 20] [--reps 7] [--batch 4] [--latent 64] [--steps 4]

Synthetic weights at SD1.5 width with time_cond_proj_dim = 256 (a guidance-embedded UNet: one forward of B images per
step, no CFG), output_type="latents" (no VAE decode).  Both loops run in this process on the same engine, alternating:
each repetition times `loops` pipeline calls of one kind between device events (ending in a synchronise), then the same
of the other kind.  Printed: the median ms per loop of each kind, its run-to-run spread (max - min over the
repetitions), and the difference.  Then the step kernel alone (rows = 1, with noise, fp64 arithmetic) next to
sd_cfg_linear_step on the same element count (fp32 arithmetic, the same four fp16 streams), microseconds per call over
back-to-back calls.  Last the sd_prof_collect launch count of one forward with timestep_cond next to one plain forward.
That profiler brackets the conv / norm / attention launches only: the time-embedding launches, where the projection
rides on the sinusoid's, are NOT in either count, so the pair shows that nothing else changed, not the one-for-one
replacement itself (that is Encoder::run_temb's single `tcond ? launch_timestep_cond : launch_timestep_sinusoid`)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline, guidance_scale_embedding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--loops", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--tiny", action="store_true", help="tiny UNet (a rehearsal of the script, not a measurement)")
args = ap.parse_args()

_lib.require_gpu()
lib = _lib.load()
base = config.tiny_unet(time_cond=32) if args.tiny else config.UNetConfig(time_cond_proj_dim=256)
usd = weights.synth_state_dict(weights.unet_manifest(base), seed=21, dtype=torch.float16)
unet = HipUNet2DConditionModel(base).load_state_dict(usd)
del usd
model = SDModelWrapper(base=unet, vae=HipAutoencoderKL(config.tiny_vae()), device="cuda")     # (the VAE is never run)
model.set_scheduler("lcm")
B, h = args.batch, args.latent
g = torch.Generator().manual_seed(1)
pos = torch.randn(B, 77, base.cross_attention_dim, generator=g).half().cuda()
lat0 = torch.randn(B, 4, h, h, generator=g).half().cuda()
kw = dict(prompt_embeds=pos, latents=lat0, num_inference_steps=args.steps, guidance_scale=8.0, height=8 * h, width=8 * h,
          seed=7)

fused = StableDiffusionUnifiedPipeline(do_cfg=False, device="cuda", output_type="latents")
host = StableDiffusionUnifiedPipeline(do_cfg=False, device="cuda", output_type="latents")
host._lcm_step_available = lambda *a: False


def timed(pipe):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.loops):
        out = pipe(model, **kw)
    e1.record()
    e1.synchronize()
    assert torch.isfinite(out.float()).all()
    return e0.elapsed_time(e1) / args.loops


for p in (fused, host):                     # warm-up: plans, code objects, the allocator
    for _ in range(3):
        p(model, **kw)
a, b = fused(model, **kw), host(model, **kw)
assert fused._lcm_step_available(model, lat0) and not host._lcm_step_available(model, lat0)
err = ((a.float() - b.float()).norm() / b.float().norm()).item()
tf, th = [], []
for _ in range(args.reps):
    tf.append(timed(fused))
    th.append(timed(host))
mf, mh = statistics.median(tf), statistics.median(th)
print(f"LCM loop B={B} 4x{h}x{h} {args.steps} steps, {args.loops} loops x {args.reps} repetitions, alternating")
print(f"  device step (sd_lcm_step): median {mf:.3f} ms per loop, spread {max(tf) - min(tf):.3f} ms  {[round(v, 3) for v in tf]}")
print(f"  host scheduler.step      : median {mh:.3f} ms per loop, spread {max(th) - min(th):.3f} ms  {[round(v, 3) for v in th]}")
print(f"  device - host = {mf - mh:+.3f} ms per loop ({(mf - mh) / mh * 100:+.2f} %); same seed, rel-L2 between them {err:.2e}")


def per_call_us(fn, iters=2000):
    for _ in range(20):
        fn()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e3)
    return best


n = lat0.numel()
gd = torch.Generator(device="cuda").manual_seed(2)
mo = torch.randn(2 * n, device="cuda", generator=gd).half()
xs = torch.randn(n, device="cuda", generator=gd).half()
nz = torch.randn(n, device="cuda", generator=gd).half()
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
# coefficients that keep the latents bounded over many in-place applications
us_lcm = per_call_us(lambda: lib.sd_lcm_step(P(mo), 1, P(xs), P(nz), None, n, 1.0, 0.5, 0.1, 0.9, 0.1, st))
us_lin = per_call_us(lambda: lib.sd_cfg_linear_step(P(mo), P(xs), None, n, 1.5, 0.5, 0.1, 0.0, 0.0, 0.0, st))
assert torch.isfinite(xs.float()).all()
print(f"  step kernel alone, n = {n}: sd_lcm_step (fp64 arithmetic) {us_lcm:.2f} us per call = {4 * 2 * n / us_lcm / 1e3:.0f} GB/s "
      f"over its four fp16 streams; sd_cfg_linear_step (fp32 arithmetic, four fp16 streams) {us_lin:.2f} us")


def launches(**extra):
    entries = (_lib.SdProfEntry * 256)()
    n = C.c_int()
    lib.sd_prof_enable(1)
    try:
        unet(lat0, 501.0, pos, **extra)
        _lib.check(lib.sd_prof_collect(entries, 256, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return sum(entries[i].launches for i in range(n.value))


tc = guidance_scale_embedding(torch.full((B,), 7.0), base.time_cond_proj_dim).cuda()
for _ in range(2):
    n_tc, n_plain = launches(timestep_cond=tc), launches()
print(f"  profiled launches of one forward (conv / norm / attention; the time-embedding launches are not bracketed): "
      f"with timestep_cond {n_tc}, plain {n_plain}")
