#!/usr/bin/env python3
"""The SDXL refiner's UNet forward alone (GPU box): python tools/run_refiner.py [--batch 2] [--latent 128] [--iters 5]
Synthetic weights at the full refiner configuration (384 / 768 / 1536 / 1536, five time ids).  Prints
  * ms per forward (events around the whole loop) and kernel launches per forward (the engine's event brackets),
  * per kernel name: launches per forward, ms per forward, TFLOP/s (sd_prof_*),
  * per distinct conv / linear shape: the kernel and tile the planner gives it (sd_igemm_plan; bias only, no fused norm).
--out FILE also writes the text there (profiles/refiner.txt is one such run).  --tiny: config.tiny_refiner_unet at 16 x 16."""
import argparse
import ctypes as C
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, shapes, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ucfg = config.tiny_refiner_unet() if args.tiny else config.sdxl_refiner_unet()
if args.tiny:
    args.latent = min(args.latent, 16)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


dev = "cuda"
B, hw = args.batch, args.latent
sd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=2, dtype=torch.float16)
net = HipUNet2DConditionModel(ucfg, dev).load_state_dict(sd)
del sd
x = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16)
e = torch.randn(B, 77, ucfg.cross_attention_dim, device=dev, dtype=torch.float16)
added = {"text_embeds": torch.randn(B, ucfg.pooled_projection_dim, device=dev, dtype=torch.float16),
         "time_ids": torch.tensor([[hw * 8.0, hw * 8, 0, 0, 6.0]] * B, device=dev)}
t = torch.tensor(501.0)
for _ in range(2):
    net(x, t, e, added_cond_kwargs=added)
torch.cuda.synchronize()


def timed():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        net(x, t, e, added_cond_kwargs=added)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


res = [timed() for _ in range(args.rounds)]
say(f"refiner forward ({'tiny' if args.tiny else 'sdxl_refiner'}) B{B} {hw}x{hw}, {ucfg.num_time_ids} time ids: "
    + " / ".join(f"{r:.3f}" for r in res) + " ms")

lib = _lib.load()
lib.sd_prof_enable(1)
net(x, t, e, added_cond_kwargs=added)
ents = (_lib.SdProfEntry * 512)()
n = C.c_int()
_lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
lib.sd_prof_enable(0)
rows = sorted(ents[: n.value], key=lambda r: -r.ms)
say(f"bracketed launches per forward: {sum(r.launches for r in rows)}; bracketed time {sum(r.ms for r in rows):.3f} ms")
say(f"{'kernel':<56s} {'launches':>8s} {'ms':>9s} {'TFLOP/s':>8s}")
for r in rows:
    say(f"{r.kernel.decode():<56s} {r.launches:8d} {r.ms:9.3f} {r.flops / max(r.ms, 1e-9) / 1e9:8.1f}")

say()
say("planned kernel per distinct conv / linear shape (N H W Cin Cout ks stride up geglu):")
uniq = OrderedDict()
for c in shapes.unet_convs(ucfg, B, hw, hw):
    if c.Cout % 8 or c.Cin % 64:
        continue
    ent = uniq.setdefault(c.key(), {"shape": c, "count": 0})
    ent["count"] += 1
for key, ent in uniq.items():
    c = ent["shape"]
    geom = (C.c_int * 9)(c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.up, -1)
    flags = (C.c_int * 10)(c.geglu, 0, 0, 0, 1, 0, 0, 0, 0, 0)
    out = (C.c_int64 * 12)()
    name = C.create_string_buffer(64)
    _lib.check(lib.sd_igemm_plan(geom, flags, out, name), "sd_igemm_plan")
    say(f"  {c.tag:<22s} x{ent['count']:<3d} M={c.M:6d} N={c.Cout:5d} K={c.K:6d} ks{c.ks} s{c.stride} u{c.up} g{c.geglu} -> "
        f"kind {out[0]:3d} tile {out[10]}x{out[11]} split {out[2]}  {name.value.decode()}")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
