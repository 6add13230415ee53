#!/usr/bin/env python3
"""DeepCache on the 50-step DDIM loop (GPU box): python tools/run_deepcache.py [--latents 4] [--latent 64] [--steps 50]
Synthetic SD1.5 weights at the headline shape (4 latents, CFG batch 8, 64 x 64).  The loop is the pipeline's "linear"
device-step loop written out: fused_plan, sd_unet_forward_cfg, sd_cfg_linear_step.  Prints
  * ms per loop (events around whole loops) with DeepCache off and at (interval, depth) in {(2,1), (3,1), (5,1), (3,2)},
    the settings alternating in one process, the ratio against the off loops and the ratio the measured step times
    predict, 1 / ((1 + (N - 1) f) / N),
  * ms per forward of each step kind (plain / store / plain / reuse, events around 20 forwards) and, from the engine's
    event brackets (sd_prof_*), launches per forward and the slowest kernels of a reuse step,
  * host time inside sd_unet_forward_cfg of a reuse step that follows a store step against one that follows a reuse step
    (a dry planning pass at every mode switch would show here),
  * the bytes the handle keeps for the cached feature, and the distance of the final latents from the off loop's --
    synthetic weights, so that distance is NOT an image-quality figure.
--out FILE also writes the text there (profiles/deepcache.txt is one such run).  --tiny: config.tiny_unet at 16 x 16, 6 steps."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

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
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ucfg = config.tiny_unet() if args.tiny else config.sd15_unet()
if args.tiny:
    args.latent, args.steps, args.latents = min(args.latent, 16), min(args.steps, 6), min(args.latents, 2)
SETTINGS = [None, (2, 1), (3, 1), (5, 1), (3, 2)]
PLAIN, STORE, REUSE = HipUNet2DConditionModel.DC_PLAIN, HipUNet2DConditionModel.DC_STORE, HipUNet2DConditionModel.DC_REUSE
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
sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
del sd
g = torch.Generator(device=dev).manual_seed(1)
lat0 = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16, generator=g)
ehs = torch.randn(2 * B, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16, generator=g)
sched = schedulers.DDIMScheduler()


def loop(setting, host=None):
    """One denoising loop -> the final latents.  `host`: list that receives (iteration, seconds inside forward_cfg)."""
    sched.set_timesteps(args.steps)
    ts = [float(v) for v in sched.timesteps.tolist()]
    lat = lat0.clone()
    if setting is not None and net.deepcache != setting:
        net.enable_deepcache(*setting)
    net.text_kv_cache(True)
    try:
        for i, t in enumerate(ts):
            plan = sched.fused_plan(t)
            if setting is not None:
                net.deep_cache_mode(STORE if i % setting[0] == 0 else REUSE)
            h0 = time.perf_counter()
            out = net.forward_cfg(lat, t, ehs, in_scale=plan.in_scale)[0]
            if host is not None:
                host.append((i, time.perf_counter() - h0))
            new = lat.clone()
            assert not plan.use_hist
            rc = lib.sd_cfg_linear_step(ptr(out), ptr(new), None, new.numel(), 7.5, plan.c_x, plan.c_eps, plan.c_hist,
                                        plan.h_x, plan.h_eps, stream())
            assert rc == 0, lib.sd_last_error()
            sched.fused_commit()
            lat = new
    finally:
        if setting is not None:
            net.deep_cache_mode(PLAIN)
        net.text_kv_cache(False)
    return lat


def timed_loop(setting, host=None):
    # outside the timed region: the setting itself (switching it off releases the buffer, on allocates it at the first
    # store forward) and one forward
    if setting is None:
        net.disable_deepcache()
    elif net.deepcache != setting:
        net.enable_deepcache(*setting)
    net.deep_cache_mode(PLAIN if setting is None else STORE)
    net.forward_cfg(lat0, 501.0, ehs)
    net.deep_cache_mode(PLAIN)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    lat = loop(setting, host)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), lat


def name(setting):
    return "off" if setting is None else f"interval {setting[0]} depth {setting[1]}"


say(f"DeepCache, {'tiny' if args.tiny else 'sd15'} UNet, {B} latents (CFG batch {2 * B}) {hw}x{hw}, {args.steps}-step DDIM loop, "
    f"synthetic weights")
base_bytes = None
for s in SETTINGS:                      # warm every setting: plans, arena, the persistent buffer
    net.disable_deepcache()
    loop(s)
    if s is None:
        net.forward_cfg(lat0, 501.0, ehs)       # (without the text K/V cache, as timed_loop's own warm-up forward)
        base_bytes = net.memory()[1]
ms = {s: [] for s in SETTINGS}
final = {}
host = {s: [] for s in SETTINGS}
kept = {}
for r in range(args.rounds):
    for s in SETTINGS + [None]:         # off first and last in every round
        m, final[s] = timed_loop(s, host[s])
        ms[s].append(m)
        if s is not None:
            kept[s] = net.memory()[1] - base_bytes
net.disable_deepcache()

# ---- the step kinds on their own ----
N_FWD = 20
t_mid = 501.0


def timed_forwards(mode):
    if mode != PLAIN:
        net.deep_cache_mode(STORE)
        net.forward_cfg(lat0, t_mid, ehs)
    net.deep_cache_mode(mode)
    net.forward_cfg(lat0, t_mid, ehs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(N_FWD):
        net.forward_cfg(lat0, t_mid, ehs)
    e1.record()
    torch.cuda.synchronize()
    net.deep_cache_mode(PLAIN)
    return e0.elapsed_time(e1) / N_FWD


def profiled(mode):
    if mode != PLAIN:
        net.deep_cache_mode(STORE)
        net.forward_cfg(lat0, t_mid, ehs)
    net.deep_cache_mode(mode)
    net.forward_cfg(lat0, t_mid, ehs)
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    try:
        net.forward_cfg(lat0, t_mid, ehs)
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
        net.deep_cache_mode(PLAIN)
    return sorted(((e.kernel.decode(), e.launches, e.ms) for e in ents[: n.value]), key=lambda r: -r[2])


say()
say(f"ms per forward (text K/V kept, as inside a loop), events around {N_FWD} forwards, in this order:")
step_ms = {}
net.text_kv_cache(True)
for d in (1, 2):
    net.enable_deepcache(3, d)
    seq = [("plain", PLAIN), ("store", STORE), ("plain", PLAIN), ("reuse", REUSE), ("plain", PLAIN)]
    got = [(k, timed_forwards(m)) for k, m in seq]
    plain = [v for k, v in got if k == "plain"]
    store = dict(got)["store"]
    reuse = dict(got)["reuse"]
    step_ms[d] = (statistics.median(plain), store, reuse)
    say(f"  depth {d}: " + "  ".join(f"{k} {v:.3f}" for k, v in got)
        + f"   (plain spread {max(plain) - min(plain):.3f}; store - median plain {store - statistics.median(plain):+.3f}; "
          f"f = reuse / plain = {reuse / statistics.median(plain):.3f})")
    prof = {k: profiled(m) for k, m in (("plain", PLAIN), ("store", STORE), ("reuse", REUSE))}
    for k, rows in prof.items():
        say(f"    {k}: {sum(r[1] for r in rows)} bracketed launches, {sum(r[2] for r in rows):.3f} ms bracketed")
    say("    slowest kernels of the reuse step (launches, ms):")
    for kname, launches, kms in prof["reuse"][:8]:
        say(f"      {kname:<52s} {launches:4d} {kms:8.3f}")
    net.disable_deepcache()
net.text_kv_cache(False)

say()
say(f"ms per {args.steps}-step loop, {args.rounds} rounds alternating (off runs first and last in each round):")
off = statistics.median(ms[None])
say(f"  {'off':<20s} " + " / ".join(f"{v:.2f}" for v in ms[None]) + f"   median {off:.2f}")
for s in SETTINGS[1:]:
    med = statistics.median(ms[s])
    N, d = s
    n_store = len(range(0, args.steps, N))
    plain_ms, store_ms, reuse_ms = step_ms[d]
    f = reuse_ms / plain_ms
    pred = args.steps / (n_store + (args.steps - n_store) * f)
    say(f"  {name(s):<20s} " + " / ".join(f"{v:.2f}" for v in ms[s]) + f"   median {med:.2f}  off / on = {off / med:.2f}x  "
        f"(1 / ((1 + (N - 1) f) / N) = {1.0 / ((1 + (N - 1) * f) / N):.2f}x; with this loop's {n_store} store steps {pred:.2f}x)  "
        f"kept {kept[s]} bytes")

say()
say("host seconds inside forward_cfg on a reuse step, by what ran before it (median, min .. max, in microseconds):")
for s in SETTINGS[1:]:
    N = s[0]
    if N < 3:
        continue
    after_store = [v * 1e6 for i, v in host[s] if i % N == 1]
    after_reuse = [v * 1e6 for i, v in host[s] if i % N >= 2]
    stores = [v * 1e6 for i, v in host[s] if i % N == 0]
    fmt = lambda v: f"{statistics.median(v):.0f} ({min(v):.0f} .. {max(v):.0f})"   # noqa: E731
    say(f"  {name(s):<20s} after a store step {fmt(after_store)}   after a reuse step {fmt(after_reuse)}   store steps {fmt(stores)}")

say()
say("distance of the final latents from the off loop's (rel-L2; synthetic weights: this is NOT an image-quality figure):")
for s in SETTINGS[1:]:
    a, b = final[s].float(), final[None].float()
    say(f"  {name(s):<20s} {(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item():.3f}")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
