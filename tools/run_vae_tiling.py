#!/usr/bin/env python3
"""Tiled VAE (GPU box): python tools/run_vae_tiling.py [--rounds 3] [--tile-batch 4] [--tiny] [--out FILE]
The SD1.5 VAE on synthetic weights, decode and encode of 1024 x 1024, 512 x 2048 and 2048 x 2048 at B = 1 and of
1024 x 1024 at B = 4, plain (sd_vae_decode / sd_vae_encode on the whole canvas) and tiled (enable_tiling(): tiles of 64
latents / 512 pixels, overlap factor 0.25, tile_batch images per stacked chunk).  Prints per case
  * the tile count per shape class;
  * ms of the plain and the tiled decode and encode, medians over --rounds with the two kinds alternating, same box;
  * the workspace of each: sd_vae_memory's arena after the plain call on a fresh handle, and arena + tile buffers
    (sd_vae_memory_tiled) after the tiled calls on another fresh handle;
  * event times of one gather launch (one chunk) and of the merge launch alone, through the operator entries.
The tiled result is not the plain result (each tile has its own GroupNorm statistics and attention): this is a cost
comparison.  Synthetic weights: nothing here is an image-quality figure.  --out FILE also writes the text there
(profiles/vae_tiling.txt is one such run).  --tiny: the width-reduced test VAE at an eighth of the sizes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, vae_tiles, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tile-batch", type=int, default=4)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
cfg = config.tiny_vae() if args.tiny else config.sd15_vae()
SCALE = 8
TS = cfg.sample_size
TL = TS // SCALE
unit = TL // 2                  # half a tile of latents: the cases below in units of it
CASES = [(1, 4 * unit, 4 * unit), (1, 2 * unit, 8 * unit), (1, 8 * unit, 8 * unit), (4, 4 * unit, 4 * unit)]
lines = []
lib = _lib.load()
dev = "cuda"


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def box_probe():
    tf, gb = C.c_float(), C.c_float()
    _lib.check(lib.sd_probe_mfma(300000, C.byref(tf), None), "sd_probe_mfma")
    _lib.check(lib.sd_probe_copy(512 << 20, 5, C.byref(gb), None), "sd_probe_copy")
    return {"mfma_tflops": round(tf.value, 1), "hbm_gbs": round(gb.value, 1)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


sd = weights.synth_state_dict(weights.vae_manifest(cfg), seed=42, dtype=torch.float16, perturb=0.1)


def fresh(tiling):
    vae = HipAutoencoderKL(cfg, dev).load_state_dict(sd)
    vae.tile_batch = args.tile_batch
    vae.enable_tiling(tiling)
    return vae


say(f"tiled VAE, {'width-reduced' if args.tiny else 'SD1.5'} VAE, tile {TL} latents / {TS} px, overlap factor 0.25, "
    f"tile_batch {args.tile_batch}; synthetic weights")
say("box_probe: " + json.dumps(box_probe()))
g = torch.Generator(device=dev).manual_seed(1)
for B, h, w in CASES:
    H, W = h * SCALE, w * SCALE
    say("")
    say(f"{H} x {W} px ({h} x {w} latents), B = {B}")
    pd = vae_tiles.plan(False, h, w, TS, TL, 0.25)
    cls = ", ".join(f"{c['h']}x{c['w']}: {len(c['tiles'])}" for c in vae_tiles.classes(pd))
    say(f"  tiles {pd.ny} x {pd.nx}; per shape class (latents): {cls}")
    z = torch.randn(B, 4, h, w, device=dev, dtype=torch.float16, generator=g)
    img = torch.randn(B, 3, H, W, device=dev, dtype=torch.float16, generator=g).clamp(-1, 1)
    vaes = {"plain": fresh(False), "tiled": fresh(True)}
    ops = {"decode": lambda v: v.decode(z), "encode": lambda v: v.encode_moments(img)}
    for op, fn in ops.items():
        ms = {k: [] for k in vaes}
        ok = True
        for k, v in vaes.items():                              # warm: plans, arenas, buffers
            try:
                fn(v)
            except _lib.EngineError as e:
                say(f"  {op} {k}: refused ({e})")
                ok = False
        if not ok:
            continue
        for _ in range(args.rounds):
            for k, v in vaes.items():                          # kinds alternating
                ms[k].append(timed(lambda: fn(v)))
        med = {k: statistics.median(x) for k, x in ms.items()}
        for k in vaes:
            say(f"  {op} {k:5s} median {med[k]:9.2f} ms  ({' '.join(f'{x:.2f}' for x in ms[k])})  x{med[k] / med['plain']:.2f} of plain")
    _, arena_p = vaes["plain"].memory()
    _, arena_t, tiles_t = vaes["tiled"].memory_tiled()
    say(f"  workspace after decode + encode: plain {arena_p / 2**20:9.1f} MiB; tiled {arena_t / 2**20:9.1f} MiB arena + "
        f"{tiles_t / 2**20:7.1f} MiB tile buffers")
    del vaes
    torch.cuda.empty_cache()
    # the two launches alone
    n = min(args.tile_batch, B * pd.ny * pd.nx)
    stack = torch.empty(n, 4, min(TL, h), min(TL, w), device=dev, dtype=torch.float16)
    zeros = (C.c_int * n)(*([0] * n))
    ms_g = C.c_float()
    _lib.check(lib.sd_op_vae_tiles_gather(ptr(z), w, ptr(stack), zeros, zeros, zeros, n, B, 4, h, w, stack.shape[2], stack.shape[3],
                                          200, C.byref(ms_g), None), "sd_op_vae_tiles_gather")
    _, total = vae_tiles.stack_offsets(pd, B, 3)
    tiles = torch.randn(total, device=dev, dtype=torch.float16, generator=g)
    out = torch.empty(B, 3, H, W, device=dev, dtype=torch.float16)
    ms_m = C.c_float()
    _lib.check(lib.sd_op_vae_tiles_merge(ptr(tiles), total, ptr(out), W, C.byref(pd), B, 3, 50, C.byref(ms_m), None),
               "sd_op_vae_tiles_merge")
    gb = 2 * 2 * stack.numel()
    mb = 2 * 2 * out.numel()          # every pixel written once and its own tile's element read; the strips read up to 3 more
    say(f"  gather (one chunk of {n}): {ms_g.value * 1e3:7.1f} us, {gb / 1024:8.0f} KiB moved, {gb / ms_g.value / 1e6:7.1f} GB/s")
    say(f"  merge (image, one launch): {ms_m.value * 1e3:7.1f} us, >= {mb / 2**20:6.1f} MiB moved, >= {mb / ms_m.value / 1e6:7.1f} GB/s")
    del tiles, out, z, img
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
