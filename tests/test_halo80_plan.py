"""The 80-column halo tile's routing (halo80_plan, through sd_halo80_plan) pinned on the CPU: which launches of the
SD1.5 and SDXL UNets move to conv3x3_halo_kernel<80> on 256 compute units, the rule's thresholds, the switches, and that
the planner (sd_igemm_plan) answers every problem exactly as before whatever the 80-column hook is set to."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from stablediffusion_amd import config, shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_igemm_plan", os.path.join(ROOT, "tests", "golden", "make_igemm_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CUS = 256
NAME = "conv3x3_halo_kernel<80>"


def hplan(lib, geom, fl=None, cus=CUS):
    """sd_halo80_plan -> dict(ok, bn, splits, gn, gn_rows, workspace, name)."""
    out = (C.c_int64 * 6)()
    name = C.create_string_buffer(64)
    rc = lib.sd_halo80_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*(fl or gen.flags())), cus, out, name)
    assert rc == 0, lib.sd_last_error()
    return dict(zip(("ok", "bn", "splits", "gn", "gn_rows", "workspace"), list(out)), name=name.value.decode())


def cdiv(a, b):
    return (a + b - 1) // b


def rule(lib, geom, fl, cus=CUS):
    """The rule as DESIGN.md states it: Cout % 80 == 0, at most 10 slabs of K, the unsplit 80-column tiles one round on
    more than 3/4 of the CUs; over a halo or a streamed tile of the planner's table."""
    n, h, w, cin, cout, ks, stride, up, _ = geom
    rc, out, _ = gen.plan(lib, geom, fl)
    assert rc == 0
    if out[0] not in range(19) or out[0] in (13, 14, 18) or ks != 3 or stride != 1 or up != 0 or fl[5] or fl[6] or fl[8]:
        return False
    t80 = n * h * w // 256 * cdiv(cout, 80)
    return cout % 80 == 0 and cin <= 640 and t80 <= cus and 4 * t80 > 3 * cus


def unet_3x3(preset, batch, latent):
    ucfg = config.PRESETS[preset][0]()
    seen = {}
    for c in shapes.unet_convs(ucfg, batch, latent, latent):
        if c.ks == 3 and c.stride == 1 and c.up == 0 and c.Cin % 64 == 0 and c.Cout % 8 == 0:
            seen.setdefault(c.key(), c)
    return list(seen.values())


# (preset, UNet batch, latent) -> the (M, Cout, K) that run on the 80-column tile; everything else stays
MOVED = {
    ("sd15", 8, 64): {(8192, 640, 2880), (8192, 640, 5760)},
    ("sd15", 4, 64): {(16384, 320, 2880), (16384, 320, 5760)},
    ("sdxl", 8, 128): set(),
    ("sdxl", 4, 128): {(4096, 1280, 5760)},
}
GRAPH_FLAGS = [gen.flags(), gen.flags(res=1), gen.flags(rowadd=1), gen.flags(gn=32), gen.flags(res=1, gn=32)]


@pytest.mark.parametrize("preset,batch,latent", sorted(MOVED))
def test_unet_convs_on_256_cus(engine_lib, preset, batch, latent):
    convs = unet_3x3(preset, batch, latent)
    sizes = {c.H for c in convs}
    assert sizes == ({64, 32, 16, 8} if preset == "sd15" else {128, 64, 32}), sizes
    moved = set()
    for c in convs:
        geom = (c.N, c.H, c.W, c.Cin, c.Cout, 3, 1, 0, -1)
        for fl in GRAPH_FLAGS:
            got = hplan(engine_lib, geom, fl)
            assert bool(got["ok"]) == rule(engine_lib, geom, fl), (geom, fl, got)
            if got["ok"]:
                moved.add((c.M, c.Cout, c.K))
                assert (got["bn"], got["splits"], got["workspace"], got["name"]) == (80, 1, 0, NAME), got
                assert (got["gn"], got["gn_rows"]) == ((1, 256) if fl[7] else (0, 0)), (geom, fl, got)
            else:
                assert got == dict(ok=0, bn=0, splits=1, gn=0, gn_rows=0, workspace=0, name=""), got
        # every flag set of one geometry moves together: the planner's tile does not depend on them here
        assert len({hplan(engine_lib, geom, fl)["ok"] for fl in GRAPH_FLAGS}) == 1, geom
    assert moved == MOVED[(preset, batch, latent)], moved
    if preset == "sd15":        # the 8-pixel maps have no 256-pixel patch at batch 4, and never move
        assert not any(hplan(engine_lib, (c.N, c.H, c.W, c.Cin, c.Cout, 3, 1, 0, -1))["ok"] for c in convs if c.H == 8)


def test_thresholds_just_below_and_at(engine_lib):
    g = (8, 32, 32, 640, 640, 3, 1, 0, -1)          # 32 x 5 tiles of 128 columns, 32 x 8 = 256 of 80
    ok = lambda cus, geom=g: hplan(engine_lib, geom, cus=cus)["ok"]
    assert ok(256) == 1                             # one round, every CU busy
    assert ok(255) == 0                             # 256 tiles on 255 CUs: a second round for one tile
    assert ok(341) == 1 and ok(342) == 0            # 4 x 256 > 3 x 341, but not 3 x 342: at most 3/4 of the chip
    # two rounds of 80-column tiles (the planner's 64 x 4 tiles of 160 columns cover the chip)
    assert hplan(engine_lib, (8, 64, 32, 640, 640, 3, 1, 0, -1))["ok"] == 0
    # K: 10 slabs at most
    assert hplan(engine_lib, (8, 32, 32, 704, 640, 3, 1, 0, -1))["ok"] == 0
    assert hplan(engine_lib, (8, 32, 32, 960, 640, 3, 1, 0, -1))["ok"] == 0
    # half a round is not taken with two slices (2048 x 1280: the planner's 128 columns x 3 slices stay)
    for cin in (640, 1280):
        assert hplan(engine_lib, (8, 16, 16, cin, 1280, 3, 1, 0, -1))["ok"] == 0
    # what it takes over: an unsplit 128-column halo grid on 160 of 256 CUs, a 160-column halo grid in two slices, and the
    # streamed 128 x 80 tile
    for geom, kind, splits in (((8, 32, 32, 640, 640, 3, 1, 0, -1), 15, 1), ((4, 64, 64, 640, 320, 3, 1, 0, -1), 10, 2),
                               ((4, 64, 64, 320, 320, 3, 1, 0, -1), 12, 1)):
        rc, out, _ = gen.plan(engine_lib, geom, gen.flags())
        assert (out[0], out[2]) == (kind, splits), (geom, out)
        assert hplan(engine_lib, geom) == dict(ok=1, bn=80, splits=1, gn=0, gn_rows=0, workspace=0, name=NAME), geom
    # Cout no multiple of 80 (12 x 27 = 324 tiles of 80 on 342 CUs would be one round)
    assert hplan(engine_lib, (3, 32, 32, 640, 2112, 3, 1, 0, -1), cus=342)["ok"] == 0
    assert hplan(engine_lib, (3, 32, 32, 640, 2160, 3, 1, 0, -1), cus=342)["ok"] == 1
    # a forced tile runs as itself
    engine_lib.sd_igemm_force(15, 1)
    try:
        assert ok(256) == 0
    finally:
        engine_lib.sd_igemm_force(-1, 0)
    assert ok(256) == 1


def test_what_the_kernel_does_not_take(engine_lib):
    """Under sd_halo80_force(1) every problem the kernel takes is ok; these are not, in either mode."""
    f = gen.flags
    refused = [((8, 32, 32, 640, 640, 3, 2, 0, -1), f()), ((8, 16, 16, 640, 640, 3, 1, 1, -1), f()),
               ((8, 32, 32, 640, 640, 1, 1, 0, -1), f()), ((8, 32, 32, 640, 640, 3, 1, 0, 0), f()),
               ((8, 32, 32, 640, 640, 3, 1, 0, -1), f(gni=32)), ((8, 32, 32, 640, 640, 3, 1, 0, -1), f(rs=1)),
               ((8, 32, 32, 640, 636, 3, 1, 0, -1), f()), ((8, 32, 32, 96, 640, 3, 1, 0, -1), f()),
               ((8, 24, 24, 640, 640, 3, 1, 0, -1), f()), ((8, 32, 32, 640, 640, 3, 1, 0, -1), f(act=1))]
    for mode in (-1, 1):
        engine_lib.sd_halo80_force(mode)
        try:
            for geom, fl in refused:
                assert hplan(engine_lib, geom, fl)["ok"] == 0, (mode, geom, fl)
        finally:
            engine_lib.sd_halo80_force(-1)


def test_force_modes(engine_lib):
    g = (8, 32, 32, 640, 640, 3, 1, 0, -1)
    try:
        engine_lib.sd_halo80_force(0)
        assert hplan(engine_lib, g)["ok"] == 0
        engine_lib.sd_halo80_force(1)
        # whenever supported: any Cout % 8, small grids; split-K = the fewest slices that cover the CUs while the longest
        # keeps two slabs
        for geom, splits in (((1, 16, 16, 64, 80, 3, 1, 0, -1), 1), ((2, 16, 16, 128, 88, 3, 1, 0, -1), 1),
                             ((1, 16, 16, 192, 80, 3, 1, 0, -1), 2), ((8, 16, 16, 1280, 1280, 3, 1, 0, -1), 2),
                             ((4, 64, 64, 320, 320, 3, 1, 0, -1), 1), ((1, 4, 64, 64, 80, 3, 1, 0, -1), 1),
                             ((2, 16, 16, 2560, 1280, 3, 1, 0, -1), 8)):
            got = hplan(engine_lib, geom)
            m, cout = geom[0] * geom[1] * geom[2], geom[4]
            assert (got["ok"], got["bn"], got["splits"], got["name"]) == (1, 80, splits, NAME), (geom, got)
            assert got["workspace"] == (splits * m * cout if splits > 1 else 0)
        # summaries: from the epilogue when groups end on tile boundaries, from the reduction behind a split, else none
        assert hplan(engine_lib, (2, 16, 16, 64, 320, 3, 1, 0, -1), gen.flags(gn=32))["gn_rows"] == 256
        assert hplan(engine_lib, (2, 16, 16, 64, 640, 3, 1, 0, -1), gen.flags(gn=32))["gn_rows"] == 256
        assert hplan(engine_lib, (2, 16, 16, 64, 768, 3, 1, 0, -1), gen.flags(gn=32))["gn"] == 0       # 24 per group
        assert hplan(engine_lib, (8, 16, 16, 1280, 1280, 3, 1, 0, -1), gen.flags(gn=32))["gn_rows"] == 4
        engine_lib.sd_halo80_force(7)               # out of range: the rule
        assert hplan(engine_lib, g)["ok"] == 1 and hplan(engine_lib, (1, 16, 16, 64, 80, 3, 1, 0, -1))["ok"] == 0
    finally:
        engine_lib.sd_halo80_force(-1)
    assert hplan(engine_lib, g)["ok"] == 1


def test_environment_switch():
    """SD_NO_HALO80 is read once per process: a fresh interpreter, the rule and the force hook both off under it."""
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_halo80_plan as t\nfrom stablediffusion_amd import _lib\n"
            "lib = _lib.load(); g = (8, 32, 32, 640, 640, 3, 1, 0, -1); a = t.hplan(lib, g)['ok']\n"
            "lib.sd_halo80_force(1); b = t.hplan(lib, g)['ok']; print(json.dumps([a, b]))\n") % (ROOT, os.path.join(ROOT, "tests"))
    res = {}
    for sw in ("", "1"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
        if sw:
            env["SD_NO_HALO80"] = sw
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        res[sw] = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"": [1, 1], "1": [0, 0]}, res


def test_the_planner_answers_as_before(engine_lib):
    """Every default-block row of tests/golden/igemm_plan.json under each mode of the hook: the 80-column form is
    decided outside igemm2_plan, which must not notice it."""
    with open(os.path.join(ROOT, "tests", "golden", "igemm_plan.json")) as f:
        want = gen.unpack(json.load(f))
    block = gen.grid()[0]
    assert not block[0] and block[1] is None
    for mode in (-1, 0, 1):
        engine_lib.sd_halo80_force(mode)
        try:
            got = gen.run_block(engine_lib, block)
        finally:
            engine_lib.sd_halo80_force(-1)
        assert got == want[0], mode
    # and on the launches that move, by name
    rc, out, name = gen.plan(engine_lib, (8, 32, 32, 640, 640, 3, 1, 0, -1), gen.flags())
    assert (out[0], out[2], name) == (15, 1, "conv3x3_halo_kernel<128>")
