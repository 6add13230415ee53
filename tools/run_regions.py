#!/usr/bin/env python3
"""Regional prompts on the UNet forward (GPU box): python tools/run_regions.py [--out FILE] [--tiny] [--only sd15|sdxl]
Synthetic weights.  For SD1.5 at CFG batch 8 / 64 x 64 latents and SDXL at batch 4 / 128 x 128 latents, and for R = 2, 4,
8 regions under vertical-stripe masks (the first half of the batch is the uncond half: one-hot on region 0), prints
  * ms per UNet forward with regions and of the plain forward (77 tokens, no regions set: the launches of the forward
    as it was before the feature), alternating over --rounds passes of --iters forwards between device events in one
    process, their ratio, and R plain forwards (R x the plain time: what region-based MultiDiffusion costs);
  * one fully overlapping soft-mask case at R = 4, where no segment is skipped;
  * per transformer level, the region launch alone (sd_op_region_cross_attention on the level's shape and weights)
    against the plain attn2 launch (sd_op_attention_ex, 77 keys) on the same queries, us per launch.
Image quality is NOT judged: the weights are synthetic.  --out FILE also writes the text there (profiles/regions.txt is
one such run).  --tiny: config.tiny_unet at batch 2 / 16 x 16."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--op-iters", type=int, default=200)
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--only", default=None, choices=["sd15", "sdxl"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = 77
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def P(t):
    return C.c_void_p(t.data_ptr())


def stripes(N, R, h, w, soft=False):
    """[N, R, h, w]: the first N / 2 rows (uncond) one-hot on region 0, the others R vertical stripes of equal width, or,
    `soft`, positive weights everywhere."""
    out = torch.zeros(N, R, h, w)
    out[:N // 2, 0] = 1.0
    if soft:
        m = torch.rand(N - N // 2, R, h, w, generator=torch.Generator().manual_seed(R)) + 0.05
        out[N // 2:] = m / m.sum(1, keepdim=True)
    else:
        for r in range(R):
            out[N // 2:, r, :, (w * r) // R:(w * (r + 1)) // R] = 1.0
    return out


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def levels_of(cfg):
    """(level, heads, head dim) of every transformer level of the UNet."""
    out, nb = [], len(cfg.block_out_channels)
    for i, bt in enumerate(cfg.down_block_types):
        if bt.startswith("CrossAttn"):
            out.append((i, cfg.attention_head_dim[i], cfg.block_out_channels[i] // cfg.attention_head_dim[i]))
    if all(lv != nb - 1 for lv, _, _ in out):
        out.append((nb - 1, cfg.attention_head_dim[-1], cfg.block_out_channels[-1] // cfg.attention_head_dim[-1]))
    return out


def run_shape(name, cfg, N, hw, added):
    lib = _lib.load()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=1, dtype=torch.float16, perturb=0.1)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    del sd
    g = torch.Generator().manual_seed(N)
    x = torch.randn(N, 4, hw, hw, generator=g).half().cuda()
    t = torch.tensor(501.0)
    ctx = cfg.cross_attention_dim
    plain_ehs = torch.randn(N, L, ctx, generator=g).half().cuda()
    kw = {"added_cond_kwargs": {k: v.cuda() for k, v in added.items()}} if added else {}
    cases = [(2, False), (4, False), (8, False), (4, True)]
    ehs = {R: torch.randn(N, R * L, ctx, generator=g).half().cuda() for R in (2, 4, 8)}
    wts = {(R, soft): stripes(N, R, hw, hw, soft).cuda() for R, soft in cases}

    def plain():
        net.clear_regions()
        return lambda: net(x, t, plain_ehs, **kw)

    def regional(R, soft):
        net.set_regions(wts[(R, soft)])
        return lambda: net(x, t, ehs[R], **kw)

    times = {c: [] for c in [None] + cases}
    for c in [None] + cases:                    # plans and buffers first
        (plain() if c is None else regional(*c))()
    for _ in range(args.rounds):
        for c in [None] + cases:
            times[c].append(timed(plain() if c is None else regional(*c), args.iters))
    net.clear_regions()
    say()
    say(f"{name}: UNet forward, batch {N}, {hw} x {hw} latents, ms (median of {args.rounds} alternating passes of "
        f"{args.iters} forwards; all passes)")
    off = statistics.median(times[None])
    say(f"  plain, 77 tokens        : {off:8.3f} ms                               {['%.3f' % v for v in times[None]]}")
    for c in cases:
        R, soft = c
        m = statistics.median(times[c])
        say(f"  R = {R}, {'soft overlap ' if soft else 'disjoint strip'}: {m:8.3f} ms  x{m / off:5.3f} of plain; R plain forwards "
            f"{R * off:8.3f} ms (x{m / (R * off):5.3f})  {['%.3f' % v for v in times[c]]}")
    say(f"  per level, us per launch ({args.op_iters} back-to-back launches between events): the region launch on the level's "
        "weights | the plain attn2 launch on 77 keys")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lvl, heads, d in levels_of(cfg):
        Tq, Cc = (hw >> lvl) ** 2, heads * d
        q = (torch.randn(N, Tq, Cc, generator=g) * (1.4426950408889634 / d ** 0.5)).half().cuda()
        out = torch.empty(N, Tq, Cc, device="cuda", dtype=torch.float16)
        kv1 = torch.randn(N, L, 2 * Cc, generator=g).half().cuda()

        def attn():
            _lib.check(lib.sd_op_attention_ex(P(q), P(kv1), P(kv1[..., Cc:]), P(out), N, Tq, L, heads, d, Cc, 2 * Cc, 2 * Cc, Cc,
                                              0, 1, st), "sd_op_attention_ex")
        base = timed(attn, args.op_iters) * 1e3
        row = [f"    level {lvl} (Tq {Tq:5d}, {heads:2d} heads of {d:3d}): plain {base:7.1f}"]
        plan = (C.c_int * 4)()
        for R, soft in cases:
            kv = torch.randn(N, R * L, 2 * Cc, generator=g).half().cuda()
            wl = wts[(R, soft)]
            for _ in range(lvl):
                wl = F.avg_pool2d(wl, 2)
            wl = wl.flatten(2).transpose(1, 2).contiguous()

            def reg():
                _lib.check(lib.sd_op_region_cross_attention(P(q), P(kv), P(kv[..., Cc:]), P(wl), P(out), N, Tq, L, R, heads, d,
                                                            Cc, 2 * Cc, 2 * Cc, Cc, N, 1, st), "sd_op_region_cross_attention")
            us = timed(reg, args.op_iters) * 1e3
            lib.sd_region_plan(R, L, d, plan)
            row.append(f"R{R}{'s' if soft else ''} {us:7.1f} (x{us / base:4.2f}, {plan[1]} grp)")
        say(" | ".join(row))
    del net
    torch.cuda.empty_cache()


say(f"device {torch.cuda.get_device_name(0)}; synthetic weights: timings only, image quality is not judged")
if args.tiny:
    run_shape("tiny", config.tiny_unet(), 2, 16, None)
else:
    if args.only in (None, "sd15"):
        run_shape("SD1.5", config.sd15_unet(), 8, 64, None)
    if args.only in (None, "sdxl"):
        g0 = torch.Generator().manual_seed(9)
        run_shape("SDXL", config.sdxl_unet(), 4, 128,
                  {"text_embeds": torch.randn(4, 1280, generator=g0).half(),
                   "time_ids": torch.tensor([[1024.0, 1024, 0, 0, 1024, 1024]] * 4)})
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
