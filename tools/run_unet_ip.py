#!/usr/bin/env python3
"""UNet forward time with and without an IP-Adapter attached (GPU box):
python tools/run_unet_ip.py [--preset sd15] [--batch 8] [--latent 64] [--d-img 1024] [--iters 20] [--reps 3]
Same engine, same inputs; the adapter (synthetic weights, 4 tokens, one image per prompt) is attached and detached
between the timed runs, which alternate so that box drift hits both alike.  Text and image K / V caches are on, as
inside the pipeline's denoise loop."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import config, weights  # noqa: E402
from stablediffusion_amd.models import HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--preset", default="sd15")
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--d-img", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
cfg = config.PRESETS[args.preset][0]()
dev = "cuda"
net = HipUNet2DConditionModel(cfg, dev).load_state_dict(weights.synth_state_dict(weights.unet_manifest(cfg), seed=2,
                                                                                 dtype=torch.float16))
ad = HipIPAdapter(net, args.d_img, 4).load_state_dict(synth_ip_state_dict(cfg, args.d_img, 4, seed=3))
B, hw = args.batch, args.latent
x = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16)
e = torch.randn(B, 77, cfg.cross_attention_dim, device=dev, dtype=torch.float16)
img = torch.randn(B, 1, args.d_img, device=dev, dtype=torch.float16)
added = {}
if cfg.addition_embed_type == "text_time":
    pdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    added = {"text_embeds": torch.randn(B, pdim, device=dev, dtype=torch.float16),
             "time_ids": torch.tensor([[hw * 8.0, hw * 8, 0, 0, hw * 8, hw * 8]] * B, device=dev)}


def timed(with_ip):
    net.attach_ip_adapter(ad if with_ip else None)
    kw = dict(added, image_embeds=[img]) if with_ip else added
    net.text_kv_cache(True)
    for _ in range(3):
        net(x, 501.0, e, added_cond_kwargs=kw)
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.iters):
        net(x, 501.0, e, added_cond_kwargs=kw)
    t.record()
    t.synchronize()
    net.text_kv_cache(False)
    return s.elapsed_time(t) / args.iters


for rep in range(args.reps):
    a, b = timed(False), timed(True)
    print(f"{args.preset} B={B} {hw}x{hw} rep {rep}: plain {a:.3f} ms  with IP-Adapter {b:.3f} ms  ratio {b / a:.3f}",
          flush=True)
