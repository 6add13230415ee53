#!/usr/bin/env python3
"""Generates tests/golden/conv_route.json: the whole decision for a convolution / linear launch -- folded upsample,
80-column halo tile or a row of the variant table -- on the problems the UNet and VAE graphs issue, host code only.
tests/test_conv_route.py asks sd_conv_plan (conv_plan of csrc/igemm2.hip, the one function op_conv plans by) for every
row and compares every field.

    python tests/golden/make_conv_route.py            # rewrites the fixture from the library as built

The committed fixture was written BEFORE conv_plan existed, when op_conv walked the three stages by hand.  It is composed
here from the three narrower entries in op_conv's order, so it pins conv_plan to that chain and not to itself:
    1. the folded upsample.  The library exposes only its shape predicate (sd_upconv_fold_supported), so the rest of the
       five-line rule of its plan function is RESTATED in fold_route() below: up = 1, 3x3, stride 1, the default padding,
       a folded pack at hand, none of GEGLU / activation / row add / residual / LayerNorm fold / fused input GroupNorm /
       row statistics; 160 columns where they divide Cout, else 128; summaries of 256 pixels under the channels-per-group
       and tile-boundary rule;
    2. sd_halo80_plan;
    3. sd_igemm_plan.
Fields the two narrower stages do not answer are fixed as their launches behave: no row statistics from the epilogue
(one part of Cout columns is what launch_row_stats leaves), output scales honoured, 256 tile rows, variant = kind.
Regenerate only when a routing change is intended, and review the diff of the fixture.

A row is [kind, variant, splits, workspace, rs_own, rs_parts, rs_part_w, gn_emit, gn_rows, scales_ok, bm, bn, name]; the
fixture is packed as igemm_plan.json is (names / plans / cases / blocks), one case per geometry holding one plan index
per (have_fold, cus, flag set) in the order of variants().
"""
import ctypes as C
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_route.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("make_igemm_plan", os.path.join(HERE, "make_igemm_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

KIND_FOLD, KIND_HALO80 = 220, 80
CUS = (256, 304)
# (sd_halo80_force mode, sd_igemm_force arguments): the rule, the hook off and on, and a forced tile
MODES = [(-1, None), (0, None), (1, None), (-1, (15, 1))]


def geoms():
    """[(geom, geglu)]: the UNet and VAE-decoder launches, then make_igemm_plan's off-table and forced geometries."""
    from stablediffusion_amd import config, shapes
    seen = {}
    for preset, latent in (("sd15", 64), ("sdxl", 128)):
        ucfg, vcfg = (f() for f in config.PRESETS[preset])
        convs = [c for b in (8, 4, 2) for c in shapes.unet_convs(ucfg, b, latent, latent)]
        convs += [c for b in (4, 1) for c in shapes.vae_decoder_convs(vcfg, b, latent, latent)]
        for c in convs:
            seen.setdefault(c.key(), ((c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.up, -1), c.geglu))
    out = list(seen.values())
    out += [(g, 0) for g in gen.off_table_geoms() if (g, 0) not in out]
    out += [f for f in gen.FORCE_GEOMS if f not in out]
    return out


def variants(geom, geglu):
    """[(have_fold, cus, flags)] of one geometry: a folded pack only where the launch upsamples."""
    return [(hf, cus, fl) for hf in ((0, 1) if geom[7] == 1 else (0,)) for cus in CUS
            for fl in gen.with_geglu(gen.GRAPH_FLAGS, geglu)]


def fold_route(lib, geom, fl, have_fold):
    """The folded upsample's plan, restated (see above); None when the launch stays on the 9-tap kernels."""
    n, h, w, cin, cout, ks, stride, up, pad = geom
    geglu, act, res, rowadd, _, ln, rs, G, gni, _ = fl
    if not (have_fold and up == 1 and ks == 3 and stride == 1 and pad in (-1, 1)) or geglu or act or rowadd or res or ln or gni or rs:
        return None
    if not lib.sd_upconv_fold_supported(n, h, w, cin, cout):
        return None
    bn = 160 if cout % 160 == 0 else 128
    cpg = cout // G if G > 0 and cout % G == 0 else 0
    gn = int((cpg >= 8 or cpg == 4) and (bn % cpg == 0 or cout <= bn))
    return [KIND_FOLD, KIND_FOLD, 1, 0, 0, 1, cout, gn, 256 * gn, 1, 256, bn, "conv3x3_halo_kernel<%d>/up2x2" % bn]


def parent_route(lib, geom, fl, have_fold, cus):
    """The three entries in op_conv's order."""
    row = fold_route(lib, geom, fl, have_fold)
    if row:
        return row
    out = (C.c_int64 * 6)()
    name = C.create_string_buffer(64)
    rc = lib.sd_halo80_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*fl), cus, out, name)
    assert rc == 0, (geom, fl, lib.sd_last_error())
    ok, bn, splits, gn, gn_rows, workspace = list(out)
    if ok:
        return [KIND_HALO80, KIND_HALO80, splits, workspace, 0, 1, geom[4], gn, gn_rows, 1, 256, bn, name.value.decode()]
    rc, out, name = gen.plan(lib, geom, fl)
    assert rc == 0, (geom, fl, lib.sd_last_error())
    return out + [name]


def conv_route(lib, geom, fl, have_fold, cus):
    """sd_conv_plan's answer in the same form."""
    out = (C.c_int64 * 12)()
    name = C.create_string_buffer(64)
    rc = lib.sd_conv_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*fl), have_fold, cus, out, name)
    assert rc == 0, (geom, fl, lib.sd_last_error())
    return list(out) + [name.value.decode()]


def run_block(lib, mode, route):
    """The answers of one mode: per geometry, one row per entry of variants()."""
    halo80, force = mode
    lib.sd_halo80_force(halo80)
    lib.sd_igemm_force(*(force or (-1, 0)))
    try:
        return [[route(lib, g, fl, hf, cus) for hf, cus, fl in variants(g, geglu)] for g, geglu in geoms()]
    finally:
        lib.sd_halo80_force(-1)
        lib.sd_igemm_force(-1, 0)


def pack(answers):
    names, plans, cases, blocks = [], [], [], []

    def index(table, x):
        if x not in table:
            table.append(x)
        return table.index(x)
    for block in answers:
        blocks.append([index(cases, [index(plans, r[:12] + [index(names, r[12])]) for r in rows]) for rows in block])
    return {"names": names, "plans": plans, "cases": cases, "blocks": blocks}


def unpack(fix):
    return [[[fix["plans"][p][:12] + [fix["names"][fix["plans"][p][12]]] for p in fix["cases"][c]] for c in block]
            for block in fix["blocks"]]


def main():
    from stablediffusion_amd import _lib
    lib = _lib.load()
    answers = [run_block(lib, mode, parent_route) for mode in MODES]
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        gen.dump(pack(answers), f)
    rows = [r for b in answers for rows in b for r in rows]
    print(f"{out}: {len(rows)} rows ({sum(r[0] == KIND_FOLD for r in rows)} folded, "
          f"{sum(r[0] == KIND_HALO80 for r in rows)} on the 80-column tile), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
