"""The whole decision for a convolution launch (conv_plan, through sd_conv_plan) pinned on the CPU: folded upsample,
80-column halo tile or a row of the variant table, every field of every row of tests/golden/conv_route.json.  The
fixture was composed from the three narrower entries in op_conv's order before conv_plan existed
(tests/golden/make_conv_route.py), so the one function is held to the chain it replaced."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_route.json")
FIELDS = ("kind", "variant", "splits", "workspace", "rs_own", "rs_parts", "rs_part_w", "gn_emit", "gn_rows", "scales_ok",
          "bm", "bn", "name")

_spec = importlib.util.spec_from_file_location("make_conv_route", os.path.join(ROOT, "tests", "golden", "make_conv_route.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return gen.unpack(json.load(f))


def test_grid_covers_the_issue(golden):
    from stablediffusion_amd import config, shapes
    assert os.path.getsize(FIXTURE) < 1 << 20
    assert gen.MODES == [(-1, None), (0, None), (1, None), (-1, (15, 1))] and gen.CUS == (256, 304)
    geoms = gen.geoms()
    assert len(golden) == len(gen.MODES) and all(len(block) == len(geoms) for block in golden)
    have = {g for g, _ in geoms}
    for preset, latent in (("sd15", 64), ("sdxl", 128)):
        ucfg, vcfg = (f() for f in config.PRESETS[preset])
        convs = [c for b in (8, 4, 2) for c in shapes.unet_convs(ucfg, b, latent, latent)]
        convs += [c for b in (4, 1) for c in shapes.vae_decoder_convs(vcfg, b, latent, latent)]
        assert {(c.N, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.up, -1) for c in convs} <= have
    assert set(gen.gen.off_table_geoms()) | {g for g, _ in gen.gen.FORCE_GEOMS} <= have
    for (g, geglu), rows in zip(geoms, golden[0]):
        combos = gen.variants(g, geglu)
        assert len(rows) == len(combos) == (2 if g[7] == 1 else 1) * 2 * len(gen.gen.GRAPH_FLAGS)
    # all three stages answer in the recording, and the hook's modes move launches between the last two
    kinds = [{r[0] for rows in block for r in rows} for block in golden]
    assert {gen.KIND_FOLD, gen.KIND_HALO80, 10, 15, 13, 100, -1} <= kinds[0]
    assert gen.KIND_HALO80 not in kinds[1] and gen.KIND_HALO80 not in kinds[3] and gen.KIND_FOLD in kinds[3]
    count = lambda block: sum(r[0] == gen.KIND_HALO80 for rows in block for r in rows)
    assert count(golden[2]) > count(golden[0]) > 0


@pytest.mark.parametrize("mode", range(len(gen.MODES)), ids=["rule", "halo80_off", "halo80_on", "force_15_1"])
def test_every_row(engine_lib, golden, mode):
    got = gen.run_block(engine_lib, gen.MODES[mode], gen.conv_route)
    want = golden[mode]
    bad, n = [], 0
    for (geom, geglu), rows_got, rows_want in zip(gen.geoms(), got, want):
        assert len(rows_got) == len(rows_want)
        for (hf, cus, fl), g, w in zip(gen.variants(geom, geglu), rows_got, rows_want):
            n += 1
            if g != w:
                bad.append({"geom": geom, "flags": fl, "have_fold": hf, "cus": cus,
                            "diff": {f: (x, y) for f, x, y in zip(FIELDS, w, g) if x != y}})
    assert not bad, (len(bad), bad[:5])
    assert n == sum(len(rows) for rows in want) and n > 5000
