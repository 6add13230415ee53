#!/usr/bin/env python3
"""Generates tests/golden/igemm_plan.json: what sd_igemm_plan (the launch planner of csrc/igemm2.hip, host code only,
no GPU) answers on a grid of convolution / linear problems.  tests/test_igemm_plan.py replays every row and compares
every field, so a change to the variant table, the tuned table or the routing rules that moves a launch shows up
without a GPU.

    python tests/golden/make_igemm_plan.py            # rewrites the fixture from the library as built

The committed fixture was written by the selection code as it stood BEFORE it was gathered into one planner (the entry
then ran the old pick / emits / workspace / launch-kind functions in op_conv's order), so it pins the planner to that
logic and not to itself.  Regenerate only when a routing change is intended, and review the diff of the fixture.

The fixture holds answers only; the problems come from grid() below, which the test walks in the same order:
    names:  the distinct kernel names
    plans:  the distinct answers [kind, variant, splits, workspace, rs_own, rs_parts, rs_part_w, gn_emit, gn_rows,
            scales_ok, name index]
    cases:  the distinct lists of plan indices, one index per flag set of a geometry
    blocks: per block of grid(), one case index per geometry
A block with an env runs in a fresh process (the switches are read once per process).
"""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "igemm_plan.json")
TABLE = os.path.join(ROOT, "stablediffusion_amd", "csrc", "igemm2_table.inc")
ENV_SWITCHES = ("SD_NO_WSGEMM", "SD_NO_PGEMM", "SD_IGEMM3")


# flags[10] = geglu, act, res, rowadd, bias, ln_parts, rowstats wanted, gn groups wanted, fused gn-in groups, scaled
def flags(geglu=0, act=0, res=0, rowadd=0, bias=1, ln=0, rs=0, gn=0, gni=0, scaled=0):
    return (geglu, act, res, rowadd, bias, ln, rs, gn, gni, scaled)


# the combinations the UNet / VAE / CLIP / ControlNet graphs issue
GRAPH_FLAGS = [flags(), flags(res=1), flags(rowadd=1), flags(gn=32), flags(rs=1), flags(ln=1), flags(ln=4), flags(ln=20),
               flags(geglu=1, ln=4)]
EXTRA_FLAGS = [flags(act=1), flags(act=2), flags(gni=32), flags(scaled=1), flags(bias=0), flags(geglu=1),
               flags(geglu=1, bias=0), flags(res=1, rs=1), flags(rowadd=1, gn=32), flags(gn=8), flags(res=1, ln=4),
               flags(gn=32, scaled=1)]
FORCE_FLAGS = [flags(), flags(res=1), flags(gn=32), flags(rs=1), flags(ln=4)]


def image_shape(pixels):
    """OH x OW = pixels, as square as it gets."""
    oh = int(math.isqrt(pixels))
    while pixels % oh:
        oh -= 1
    return oh, pixels // oh


def table_geoms():
    """Every row of the tuned table as (geom, geglu): one image, and eight where M divides."""
    out = []
    for line in open(TABLE):
        m = re.match(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+),", line)
        if not m:
            continue
        M, N, K, ks, stride, up, geglu = map(int, m.groups())
        for imgs in (1, 8):
            if M % imgs:
                continue
            oh, ow = image_shape(M // imgs)
            if up and (oh % 2 or ow % 2):
                oh, ow = 2, M // imgs // 2
            h, w = (oh * stride, ow * stride) if not up else (oh // 2, ow // 2)
            out.append(((imgs, h, w, K // (ks * ks), N, ks, stride, up, -1), geglu))
    return out


def pw(M, K, N, imgs=1):
    return (imgs, M // imgs, 1, K, N, 1, 1, 0, -1)


def off_table_geoms():
    g = []
    # M no multiple of 128 / 256; OH * OW no multiple of the tile rows; Cout % 160 != 0; Cout = 8
    g += [(1, 10, 10, 320, 320, 1, 1, 0, -1), (1, 24, 24, 320, 320, 3, 1, 0, -1), (2, 8, 8, 1280, 1280, 3, 1, 0, -1),
          (1, 24, 24, 640, 512, 3, 1, 0, -1), (4, 32, 32, 256, 768, 1, 1, 0, -1), (1, 64, 64, 128, 8, 3, 1, 0, -1),
          (3, 40, 40, 320, 640, 3, 1, 0, -1), (1, 48, 80, 128, 128, 3, 1, 0, -1)]
    # K = 64 / 128, with the GEGLU widths
    g += [pw(16384, 64, 320), pw(16384, 128, 320), pw(16384, 64, 2048), pw(16384, 128, 2048), pw(300, 64, 64)]
    # channels per group of 4 (accepted) and 2 (refused) at G = 32
    g += [(1, 32, 32, 128, 128, 3, 1, 0, -1), (1, 32, 32, 128, 64, 3, 1, 0, -1), (2, 16, 16, 256, 128, 1, 1, 0, -1)]
    # CLIP's MLPs (act = 1 / 2 among the flag sets)
    for b in (1, 2, 8, 16):
        g += [pw(77 * b, 768, 3072), pw(77 * b, 3072, 768), pw(77 * b, 1280, 5120), pw(77 * b, 5120, 1280)]
    # the M x N x K of a halo row of the table from an image no halo patch tiles, and as a stride-2 / an upsampled conv
    g += [(1, 2, 2048, 320, 320, 3, 1, 0, -1), (8, 2, 2048, 320, 320, 3, 1, 0, -1), (1, 1, 4096, 640, 640, 3, 1, 0, -1),
          (8, 128, 128, 320, 320, 3, 2, 0, -1), (8, 128, 128, 320, 320, 3, 2, 0, 0), (8, 32, 32, 320, 320, 3, 1, 1, -1),
          (2, 1, 1024, 1280, 1280, 3, 1, 1, -1), (1, 256, 256, 128, 128, 3, 2, 0, 0)]
    # K = 320 pointwise around the weight-stationary route's conditions (with / without residual among the flag sets)
    g += [pw(4096, 320, 320), pw(4096, 320, 640), pw(4096, 320, 2560), pw(1024, 320, 320), pw(896, 320, 320),
          pw(4096, 320, 512), pw(8192, 320, 1280, 2)]
    # GEGLU projections on both sides of the persistent kernel's 512 tiles of 256 x 128
    g += [pw(3328, 640, 5120), pw(3072, 640, 5120), pw(8192, 640, 5120), pw(2048, 1280, 10240), pw(1536, 1280, 10240),
          pw(2048, 640, 5120)]
    # large and deep off-table problems (heuristic split-K, 128 x 160 rule)
    g += [pw(2048, 2560, 1280), pw(512, 5120, 640), (2, 16, 16, 1920, 1280, 3, 1, 0, -1), (1, 96, 96, 512, 512, 3, 1, 0, -1)]
    return g


FORCE_GEOMS = [((2, 64, 64, 320, 320, 3, 1, 0, -1), 0), (pw(32768, 320, 2560, 8), 1), (pw(2048, 1280, 1280), 0)]


def with_geglu(fls, geglu):
    return [tuple([f[0] | geglu]) + f[1:] for f in fls]


def off_table_cases():
    return [(g, GRAPH_FLAGS + EXTRA_FLAGS) for g in off_table_geoms()]


def grid():
    """[(env, force, [(geom, [flags, ...]), ...]), ...]: the default block, every forced id, every switch."""
    blocks = [({}, None, [(g, with_geglu(GRAPH_FLAGS, geglu)) for g, geglu in table_geoms()] + off_table_cases())]
    blocks += [({}, (v, sp), [(g, with_geglu(FORCE_FLAGS, geglu)) for g, geglu in FORCE_GEOMS])
               for v in range(19) for sp in (1, 2, 4)]
    blocks += [({sw: "1"}, None, off_table_cases()) for sw in ENV_SWITCHES]
    return blocks


def plan(lib, geom, fl):
    out = (C.c_int64 * 12)()
    name = C.create_string_buffer(64)
    rc = lib.sd_igemm_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*fl), out, name)
    return rc, list(out), name.value.decode()


def run_block(lib, block):
    """The answers of one block of grid(): per geometry, per flag set, out[0..9] + [name]."""
    _, force, cases = block
    lib.sd_igemm_force(*(force or (-1, 0)))
    try:
        res = []
        for geom, fls in cases:
            rows = []
            for fl in fls:
                rc, out, name = plan(lib, geom, fl)
                assert rc == 0, (geom, fl, force, lib.sd_last_error())
                rows.append(out[:10] + [name])
            res.append(rows)
        return res
    finally:
        lib.sd_igemm_force(-1, 0)


def pack(answers):
    """Interns names, plans and per-geometry lists of plans (see the layout above)."""
    names, plans, cases, blocks = [], [], [], []

    def index(table, x):
        if x not in table:
            table.append(x)
        return table.index(x)
    for block in answers:
        blocks.append([index(cases, [index(plans, r[:10] + [index(names, r[10])]) for r in rows]) for rows in block])
    return {"names": names, "plans": plans, "cases": cases, "blocks": blocks}


def unpack(fix):
    """The inverse of pack()."""
    return [[[fix["plans"][p][:10] + [fix["names"][fix["plans"][p][10]]] for p in fix["cases"][c]] for c in block]
            for block in fix["blocks"]]


def dump(fix, f):
    """Compact JSON, the entries of each table packed into lines of at most 200 characters."""
    def packed(items):
        lines = [""]
        for x in (json.dumps(x, separators=(",", ":")) for x in items):
            if lines[-1] and len(lines[-1]) + len(x) >= 200:
                lines[-1] += ","
                lines.append("")
            lines[-1] += ("," if lines[-1] else "") + x
        return "\n".join(lines)
    f.write("{\n" + ",\n".join('"%s":[\n%s]' % (k, packed(fix[k])) for k in ("names", "plans", "cases", "blocks")) + "}\n")


def main():
    sys.path.insert(0, ROOT)
    from stablediffusion_amd import _lib
    lib = _lib.load()
    if len(sys.argv) > 1 and sys.argv[1] == "--block":             # child process under one switch
        json.dump(run_block(lib, grid()[int(sys.argv[2])]), sys.stdout)
        return
    answers = []
    for i, block in enumerate(grid()):
        if block[0]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--block", str(i)],
                               env=dict(os.environ, **block[0]), capture_output=True, text=True, check=True)
            answers.append(json.loads(r.stdout.strip().splitlines()[-1]))
        else:
            answers.append(run_block(lib, block))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        dump(pack(answers), f)
    print(f"{out}: {sum(len(rows) for b in answers for rows in b)} rows, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
