"""The launch planner of the convolution / linear kernels (igemm2_plan, through sd_igemm_plan) pinned on the CPU: every
field of every row of tests/golden/igemm_plan.json (written by tests/golden/make_igemm_plan.py from the selection logic
as it stood before it was gathered into one planner), and the variant table itself under sd_igemm_force."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_plan.json")
FIELDS = ("kind", "variant", "splits", "workspace", "rs_own", "rs_parts", "rs_part_w", "gn_emit", "gn_rows", "scales_ok", "name")

# the generator owns the grid of problems; the fixture holds the answers in the grid's order
_spec = importlib.util.spec_from_file_location("make_igemm_plan", os.path.join(ROOT, "tests", "golden", "make_igemm_plan.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
plan = gen.plan


def golden():
    with open(FIXTURE) as f:
        return gen.unpack(json.load(f))


def mismatches(lib, block, want):
    """Replays one block of the grid; returns (rows checked, the rows on which any field differs)."""
    env, force, cases = block
    assert [len(fls) for _, fls in cases] == [len(rows) for rows in want]
    bad, n = [], 0
    lib.sd_igemm_force(*(force or (-1, 0)))
    try:
        for (geom, fls), rows in zip(cases, want):
            for fl, w in zip(fls, rows):
                rc, out, name = plan(lib, geom, fl)
                got = out[:10] + [name]
                n += 1
                if rc != 0 or got != w:
                    bad.append({"geom": geom, "flags": fl, "force": force, "env": env, "rc": rc,
                                "diff": {f: (x, y) for f, x, y in zip(FIELDS, w, got) if x != y}})
    finally:
        lib.sd_igemm_force(-1, 0)
    return n, bad


def test_grid_covers_the_issue():
    grid = gen.grid()
    assert len(grid) == len(golden())
    assert [f for _, f, _ in grid if f] == [(v, sp) for v in range(19) for sp in (1, 2, 4)]
    assert [e for e, _, _ in grid if e] == [{"SD_NO_WSGEMM": "1"}, {"SD_NO_PGEMM": "1"}, {"SD_IGEMM3": "1"}]
    keys = set()
    for line in open(gen.TABLE):
        m = re.match(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+),", line)
        if m:
            keys.add(tuple(map(int, m.groups())))
    assert len(keys) >= 200
    seen = set()
    for (n, h, w, cin, cout, ks, stride, up, _), fls in grid[0][2]:
        oh, ow = ((h << up) + stride - 1) // stride, ((w << up) + stride - 1) // stride
        seen.update((n * oh * ow, cout, ks * ks * cin, ks, stride, up, fl[0]) for fl in fls)
    assert keys <= seen, sorted(keys - seen)[:5]
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_every_row_in_process(engine_lib):
    total = 0
    for block, want in zip(gen.grid(), golden()):
        if block[0]:
            continue
        n, bad = mismatches(engine_lib, block, want)
        assert not bad, (len(bad), bad[:5])
        total += n
    assert total > 5000


@pytest.mark.parametrize("switch", ["SD_NO_WSGEMM", "SD_NO_PGEMM", "SD_IGEMM3"])
def test_every_row_under_switch(switch):
    """The routing switches are read once per process: their rows are replayed in a fresh interpreter."""
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_igemm_plan as t\nfrom stablediffusion_amd import _lib\n"
            "b = [(b, w) for b, w in zip(t.gen.grid(), t.golden()) if b[0] == {%r: '1'}]\n"
            "assert len(b) == 1\n"
            "n, bad = t.mismatches(_lib.load(), *b[0])\n"
            "print(json.dumps([n, len(bad), bad[:5]]))\n") % (ROOT, os.path.join(ROOT, "tests"), switch)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n, nbad, bad = json.loads(r.stdout.strip().splitlines()[-1])
    assert n > 1000 and nbad == 0, (nbad, bad)


def test_variant_table_under_force(engine_lib):
    """ids 0-18 all resolve, an id outside the table is an error, and each variant's tile is the one in its name."""
    problems = [((2, 64, 64, 320, 320, 3, 1, 0, -1), 0), ((8, 4096, 1, 320, 2560, 1, 1, 0, -1), 1),
                ((1, 2048, 1, 1280, 1280, 1, 1, 0, -1), 0), ((8, 4096, 1, 320, 320, 1, 1, 0, -1), 0)]
    ran = set()
    try:
        for v in range(19):
            engine_lib.sd_igemm_force(v, 1)
            for geom, geglu in problems:
                rc, out, name = plan(engine_lib, geom, (geglu, 0, 0, 0, 1, 0, 0, 0, 0, 0))
                assert rc == 0, (v, geom, engine_lib.sd_last_error())
                kind, bm, bn = out[0], out[10], out[11]
                assert 0 <= kind <= 18 and out[1] in range(19)
                ran.add(kind)
                m = re.match(r"igemm2_kernel<(\d+),(\d+),", name)
                if m:
                    assert (bm, bn) == (int(m.group(1)), int(m.group(2))), (v, name, bm, bn)
                elif name.startswith("conv3x3_halo_kernel<"):
                    assert (bm, bn) == (256, int(re.search(r"<(\d+)>", name).group(1))), (v, name, bm, bn)
                elif name.startswith("wsgemm_kernel<"):
                    assert (bm, bn) == (128, int(re.search(r"<(\d+),", name).group(1))), (v, name, bm, bn)
                else:
                    assert name == "igemm3_kernel" and kind == 18 and (bm, bn) == (128, 80), (v, name, bm, bn)
        assert ran == set(range(19))          # every id runs as itself on at least one of the problems
        for v in (19, 25, 1000):
            engine_lib.sd_igemm_force(v, 1)
            rc, _, _ = plan(engine_lib, problems[2][0], (0, 0, 0, 0, 1, 0, 0, 0, 0, 0))
            assert rc == 1 and b"bad variant" in engine_lib.sd_last_error(), v
    finally:
        engine_lib.sd_igemm_force(-1, 0)
