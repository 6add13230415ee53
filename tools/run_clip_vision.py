#!/usr/bin/env python3
"""Time the CLIP vision tower (GPU box):  python tools/run_clip_vision.py [--layers 32] [--iters 20] [--rounds 3]

ViT-H/14 on synthetic weights at B = 1 and 4: ms per forward of the engine (HipCLIPVisionModelWithProjection, image_embeds
only) and of the installed transformers CLIPVisionModelWithProjection in fp16 on the same device, in alternating rounds
(engine, torch, engine, torch, ...) so that clock drift hits both; the embedding stage alone (sd_op_vit_patch_embed);
bracketed launches per forward and the slowest kernels (sd_prof_*: the three launches of the projection head are not
bracketed).  There is no pass / fail number; both figures are reported, and which side is faster is said in words.
Appends to profiles/clip_vision.txt."""
import argparse
import ctypes as C
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stablediffusion_amd import _lib, config  # noqa: E402
from stablediffusion_amd.models import HipCLIPVisionModelWithProjection  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision.txt"))
args = ap.parse_args()

log = open(args.out, "a")


def say(s=""):
    print(s, flush=True)
    log.write(s + "\n")
    log.flush()


cfg = dataclasses.replace(config.clip_vit_h14(), num_hidden_layers=args.layers)
dev = "cuda"
hf = None
try:
    import transformers
    hf_cfg = transformers.CLIPVisionConfig(
        hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, image_size=cfg.image_size, patch_size=cfg.patch_size,
        hidden_act=cfg.hidden_act, projection_dim=cfg.projection_dim, layer_norm_eps=cfg.layer_norm_eps)
    torch.manual_seed(0)
    hf = transformers.CLIPVisionModelWithProjection(hf_cfg).eval().half()
    sd = {k: v.clone() for k, v in hf.state_dict().items()}
except ImportError:
    raise SystemExit("transformers is needed for the synthetic weights and the baseline")
eng = HipCLIPVisionModelWithProjection.from_state_dict(cfg, sd, device=dev)
del sd
if args.no_torch:
    hf = None
else:
    hf = hf.to(dev)
lib = _lib.load()
say(f"# ViT-H/14 vision tower, {cfg.num_hidden_layers} layers, synthetic weights, torch {torch.__version__}, "
    f"{torch.cuda.get_device_name(0)}")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


for B in args.batches:
    px = (torch.rand(B, 3, cfg.image_size, cfg.image_size, device=dev) * 4.0 - 1.8).half()
    run_eng = lambda: eng(px).image_embeds                      # noqa: E731
    with torch.no_grad():
        run_hf = (lambda: hf(px).image_embeds) if hf is not None else None   # noqa: E731
        for _ in range(2):
            run_eng()
            if run_hf:
                run_hf()
        torch.cuda.synchronize()
        te, tt = [], []
        for _ in range(args.rounds):
            te.append(timed(run_eng))
            if run_hf:
                tt.append(timed(run_hf))
    say(f"B={B} engine ms/forward: " + " / ".join(f"{t:.3f}" for t in te))
    if tt:
        say(f"B={B} torch fp16 ms/forward: " + " / ".join(f"{t:.3f}" for t in tt))
        a, b = min(te), min(tt)
        say(f"B={B} best of rounds: engine {a:.3f} ms, torch {b:.3f} ms -> the engine is "
            + (f"{b / a:.2f}x faster" if a <= b else f"SLOWER by {a / b:.2f}x"))

    # the embedding stage alone
    T = 1 + (cfg.image_size // cfg.patch_size) ** 2
    H = cfg.hidden_size
    w = torch.randn(H, 3, cfg.patch_size, cfg.patch_size, device=dev).half() * 0.02
    cls, pos = torch.randn(H, device=dev).half(), torch.randn(T, H, device=dev).half()
    out = torch.empty(B, T, H, device=dev, dtype=torch.float16)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def embed():
        _lib.check(lib.sd_op_vit_patch_embed(P(px), P(w), P(cls), P(pos), P(out), H, B, cfg.image_size, cfg.patch_size, H, st),
                   "sd_op_vit_patch_embed")
    embed()
    ms = min(timed(embed) for _ in range(args.rounds))
    fl = 2.0 * B * (T - 1) * H * 3 * cfg.patch_size ** 2
    say(f"B={B} embedding stage (1 launch, back to back): {ms * 1e3:.1f} us, {fl / ms / 1e9:.1f} TFLOP/s")

    lib.sd_prof_enable(1)
    run_eng()
    ents = (_lib.SdProfEntry * 512)()
    n = C.c_int()
    _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    lib.sd_prof_enable(0)
    rows = sorted(ents[: n.value], key=lambda r: -r.ms)
    say(f"B={B} bracketed launches per forward: {sum(r.launches for r in rows)} (+3 in the projection head); "
        f"bracketed time {sum(r.ms for r in rows):.3f} ms")
    say(f"  {'kernel':<56s} {'launches':>8s} {'ms':>9s} {'TFLOP/s':>8s}")
    for r in rows[:8]:
        say(f"  {r.kernel.decode():<56s} {r.launches:8d} {r.ms:9.3f} {r.flops / max(r.ms, 1e-9) / 1e9:8.1f}")
    say()
