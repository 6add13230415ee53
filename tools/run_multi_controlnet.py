#!/usr/bin/env python3
"""MultiControlNet timings (GPU box), written to profiles/multi_controlnet.txt:
python tools/run_multi_controlnet.py [--presets sd15,sdxl] [--iters 20] [--reps 3] [--parent-tree DIR] [--out FILE]
  1. the UNet forward: plain; one net through attach_controlnet; one net through a list; two nets in the chained and
     in the K-concatenated form; three nets -- alternating over `reps` rounds, each as a ratio to the plain forward
     (synthetic weights, text / conditioning caches on as inside the denoise loop);
  2. the residual stage alone for 2, 3 and 4 nets on the configuration's sites: chained per-net GEMMs against one
     K-concatenated GEMM per site, the grouped fold launch, the kernels the planner picked for the K = n C shapes, and
     how many folds a 50-step loop with two different guidance windows runs;
  3. with --parent-tree (a checkout of the parent commit, built): the plain and the single-net forward of both builds,
     one fresh process per measurement, alternating, with the spread of the parent's own repetitions.
SD1.5 runs at B 8 / 64 x 64, SDXL at B 4 / 128 x 128."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--presets", default="sd15,sdxl")
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_controlnet.txt"))
ap.add_argument("--child-tree", default=None, help="(internal) time the plain and single-net forward of this tree")
args = ap.parse_args()
TREE = args.child_tree or ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tests"))

import torch  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipControlNetModel, HipUNet2DConditionModel  # noqa: E402

SHAPES = {"sd15": (8, 64), "sdxl": (4, 128)}
dev = "cuda"
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def setup(preset, n_nets):
    cfg = config.PRESETS[preset][0]()
    B, hw = SHAPES[preset]
    net = HipUNet2DConditionModel(cfg, dev).load_state_dict(
        weights.synth_state_dict(weights.unet_manifest(cfg), seed=2, dtype=torch.float16))
    ccfg = controlnet.encoder_config(cfg)
    cns = [HipControlNetModel(net, ccfg).load_state_dict({k: v.half() for k, v in synth_cn_state_dict(ccfg, seed=3 + i).items()})
           for i in range(n_nets)]
    x = torch.randn(B, 4, hw, hw, device=dev, dtype=torch.float16)
    e = torch.randn(B, 77, cfg.cross_attention_dim, device=dev, dtype=torch.float16)
    imgs = [torch.rand(max(1, B // 2), 3, 8 * hw, 8 * hw, device=dev, dtype=torch.float16) for _ in range(max(n_nets, 1))]
    added = None
    if cfg.addition_embed_type == "text_time":
        pdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
        added = {"text_embeds": torch.randn(B, pdim, device=dev, dtype=torch.float16),
                 "time_ids": torch.tensor([[hw * 8.0, hw * 8, 0, 0, hw * 8, hw * 8]] * B, device=dev)}
    return cfg, net, cns, x, e, imgs, added


def timed(net, x, e, added, kw, iters):
    net.text_kv_cache(True)
    for _ in range(3):
        net(x, 501.0, e, added_cond_kwargs=added, **kw)
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        net(x, 501.0, e, added_cond_kwargs=added, **kw)
    t.record()
    t.synchronize()
    net.text_kv_cache(False)
    return s.elapsed_time(t) / iters


# ------------------------------------------------------------------------------------------------ child process
if args.child_tree:
    for preset in args.presets.split(","):
        cfg, net, cns, x, e, imgs, added = setup(preset, 1)
        net.attach_controlnet(None)
        plain = timed(net, x, e, added, {}, args.iters)
        net.attach_controlnet(cns[0])
        one = timed(net, x, e, added, dict(controlnet_cond=imgs[0], controlnet_conditioning_scale=1.0), args.iters)
        print(f"CHILD {preset} {plain:.4f} {one:.4f}", flush=True)
        del net, cns
        torch.cuda.empty_cache()
    sys.exit(0)

lib = _lib.load()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
say(f"# tools/run_multi_controlnet.py --presets {args.presets} --iters {args.iters} --reps {args.reps}"
    f"{' --parent-tree <parent checkout>' if args.parent_tree else ''}")
say(f"# {torch.cuda.get_device_name(0)}; device events around {args.iters} warmed forwards; cases alternate within a round")
decide = {}

for preset in args.presets.split(","):
    cfg, net, cns, x, e, imgs, added = setup(preset, 3)
    B, hw = SHAPES[preset]
    say()
    say(f"== {preset} B {B} / {hw} x {hw}: forward ==")
    cases = [("plain", lambda: net.attach_controlnets([]), {}, -1),
             ("N=1 attach_controlnet", lambda: net.attach_controlnet(cns[0]),
              dict(controlnet_cond=imgs[0], controlnet_conditioning_scale=1.0), -1),
             ("N=1 list", lambda: net.attach_controlnets(cns[:1]),
              dict(controlnet_cond=imgs[:1], controlnet_conditioning_scale=[1.0]), -1),
             ("N=2 chained", lambda: net.attach_controlnets(cns[:2]),
              dict(controlnet_cond=imgs[:2], controlnet_conditioning_scale=[1.0, 0.8]), 0),
             ("N=2 K-concatenated", lambda: net.attach_controlnets(cns[:2]),
              dict(controlnet_cond=imgs[:2], controlnet_conditioning_scale=[1.0, 0.8]), 1),
             ("N=3 chained", lambda: net.attach_controlnets(cns[:3]),
              dict(controlnet_cond=imgs[:3], controlnet_conditioning_scale=[1.0, 0.8, 0.6]), 0),
             ("N=3 K-concatenated", lambda: net.attach_controlnets(cns[:3]),
              dict(controlnet_cond=imgs[:3], controlnet_conditioning_scale=[1.0, 0.8, 0.6]), 1)]
    res = {name: [] for name, *_ in cases}
    for rep in range(args.reps):
        for name, attach, kw, form in cases:
            attach()
            lib.sd_cn_kcat_force(form)
            res[name].append(timed(net, x, e, added, kw, args.iters))
    lib.sd_cn_kcat_force(-1)
    for name, *_ in cases:
        v = res[name]
        ratios = [a / p for a, p in zip(v, res["plain"])]
        say(f"{name:24s} ms per round {' '.join(f'{t:8.3f}' for t in v)}   ratio to plain {' '.join(f'{r:.3f}' for r in ratios)}")
    for n in (2, 3):
        d = [k - c for k, c in zip(res[f"N={n} K-concatenated"], res[f"N={n} chained"])]
        say(f"N={n} K-concatenated minus chained, per round: {' '.join(f'{v * 1e3:+.0f} us' for v in d)}; "
            f"spread of the chained form over the rounds {1e3 * (max(res[f'N={n} chained']) - min(res[f'N={n} chained'])):.0f} us")
    decide[preset] = (res["N=2 chained"], res["N=2 K-concatenated"])

    # ---- folds of a 50-step loop with two different guidance windows ----
    net.attach_controlnets(cns[:2])
    lib.sd_cn_kcat_force(1)
    rows = controlnet.keep_schedule(50, [1.0, 0.8], [0.0, 0.3], [0.6, 1.0])
    f0 = net.cn_fold_count()
    net.text_kv_cache(True)
    for row in rows:
        net(x, 501.0, e, added_cond_kwargs=added, controlnet_cond=imgs[:2], controlnet_conditioning_scale=row)
    net.text_kv_cache(False)
    torch.cuda.synchronize()
    both = sum(1 for r in rows if r[0] and r[1])
    say(f"50-step loop, windows (0.0, 0.6) and (0.3, 1.0): {both} steps run both nets, {net.cn_fold_count() - f0} fold launch(es)")
    lib.sd_cn_kcat_force(-1)
    net.attach_controlnets([])

    # ---- the residual stage alone ----
    say()
    say(f"== {preset} B {B} / {hw} x {hw}: residual stage alone ==")
    sites = []
    h = hw
    boc = cfg.block_out_channels
    sites.append((B * h * h, boc[0]))
    for i, c in enumerate(boc):
        sites += [(B * h * h, c)] * cfg.layers_per_block
        if i != len(boc) - 1:
            h //= 2
            sites.append((B * h * h, c))
    sites.append((B * h * h, boc[-1]))
    for n in (2, 3, 4):
        keep = []
        arr = (_lib.SdCnMultiProblem * len(sites))()
        for i, (M, Cc) in enumerate(sites):
            xs = torch.randn(M, n * Cc, device=dev, dtype=torch.float16)
            y = torch.zeros(M, 2 * Cc, device=dev, dtype=torch.float16)
            q = _lib.SdCnMultiProblem()
            for j in range(n):
                w = torch.randn(Cc, Cc, device=dev, dtype=torch.float16) / Cc ** 0.5
                bias = torch.zeros(Cc, device=dev)
                keep += [w, bias]
                q.x[j], q.ldx[j], q.w[j], q.bias[j] = xs.data_ptr() + 2 * j * Cc, n * Cc, w.data_ptr(), bias.data_ptr()
            q.y, q.ldy, q.M, q.C = y.data_ptr(), 2 * Cc, M, Cc
            arr[i] = q
            keep += [xs, y]
        scales = (C.c_float * n)(*[1e-3] * n)
        for rep in range(args.reps):
            t0, t1 = (C.c_float * 2)(), (C.c_float * 2)()
            _lib.check(lib.sd_op_controlnet_residuals_multi(arr, len(sites), scales, n, 0, 50, t0, stream), "residuals_multi")
            _lib.check(lib.sd_op_controlnet_residuals_multi(arr, len(sites), scales, n, 1, 50, t1, stream), "residuals_multi")
            say(f"N={n} {len(sites)} sites rep {rep}: chained {t0[0] * 1e3:7.1f} us ({n * len(sites)} launches)   "
                f"K-concatenated {t1[0] * 1e3:7.1f} us ({len(sites)} launches)   ratio {t1[0] / t0[0]:.3f}   "
                f"fold launch {t1[1] * 1e3:.1f} us")
        # the kernels the planner picked for the K = n C shapes (heuristic tiles: no tuned rows for them)
        lib.sd_prof_enable(1)
        _lib.check(lib.sd_op_controlnet_residuals_multi(arr, len(sites), scales, n, 1, 0, None, stream), "residuals_multi")
        ents = (_lib.SdProfEntry * 64)()
        cnt = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 64, C.byref(cnt)), "sd_prof_collect")
        lib.sd_prof_enable(0)
        say(f"N={n} kernels of the K-concatenated GEMMs: " +
            "; ".join(f"{ents[i].kernel.decode()} x{ents[i].launches}" for i in range(cnt.value)))
        del keep
    del net, cns
    torch.cuda.empty_cache()

# ------------------------------------------------------------------------- parent commit against this build
if args.parent_tree:
    say()
    say("== plain and single-net forward: parent commit against this build (fresh process each, alternating) ==")
    got = {"parent": {}, "this": {}}
    for rnd in range(args.reps):
        for who, tree in (("parent", args.parent_tree), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-tree", tree, "--presets", args.presets,
                                  "--iters", str(args.iters)], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                say(f"{who} round {rnd}: child failed ({out.returncode}): {out.stderr[-300:]}")
                break
            for ln in out.stdout.splitlines():
                if ln.startswith("CHILD "):
                    _, preset, plain, one = ln.split()
                    got[who].setdefault(preset, []).append((float(plain), float(one)))
    for preset in args.presets.split(","):
        for k, what in enumerate(("plain", "single net")):
            p = [v[k] for v in got["parent"].get(preset, [])]
            t = [v[k] for v in got["this"].get(preset, [])]
            if not p or not t:
                continue
            say(f"{preset} {what:10s}: parent {' '.join(f'{v:.3f}' for v in p)} ms (spread {max(p) - min(p):.3f})   "
                f"this {' '.join(f'{v:.3f}' for v in t)} ms   mean difference {sum(t) / len(t) - sum(p) / len(p):+.3f} ms")

say()
for preset, (ch, kc) in decide.items():
    spread = max(max(ch) - min(ch), max(kc) - min(kc))
    diff = sum(kc) / len(kc) - sum(ch) / len(ch)
    say(f"decision input {preset}: N=2 K-concatenated minus chained {diff * 1e3:+.0f} us (mean), spread {spread * 1e3:.0f} us: "
        f"{'slower beyond the spread' if diff > spread else 'not slower beyond the spread'}")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
