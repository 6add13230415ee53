"""The cases of tests/ln_cases.py checked on the CPU: an fp32 emulation of the folded-LayerNorm consumers stays inside
the element-wise bound on every case, layout and profile the GPU suite runs; the same emulation with one of four seeded
defects breaks it on every profile that defect is claimed for; every case plans (sd_igemm_plan, host code only) to the
kernel it names, and together they reach the kinds the chain can run on; statistics layouts beyond a consumer's capacity
are refused before anything touches a device.

Margin: the worst emulated |err| / bound is printed per kernel family by test_report: 0.63 over the linear consumers
(the `spikes` rows, where the fp16 rounding of the stored value is most of the bound), 0.09 on the feed-forward, whose
bound adds the hidden tensor's worst case over 1280 terms.  So the emulation leaves a margin of 0.37 to 1.0; what the
bound gives away is the K-term worst case of an fp32 accumulation in any order against three fixed orders.  Each seeded
defect lands at 8 times the bound or more on every profile it is claimed for (test_report prints the smallest)."""
import ctypes as C
import os

import pytest
import torch

import conv_cases as cc
import ln_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_ROWS = 192          # rows of a large case the emulation runs (the bound is per element; neighbours stay neighbours)

_worst = {}             # family -> worst emulated |err| / bound
_least = {}             # defect -> smallest max |err| / bound over the profiles claimed for it


def _plan(lib, geom, flags, force):
    out = (C.c_int64 * 12)()
    name = C.create_string_buffer(64)
    lib.sd_igemm_force(*(force or (-1, 0)))
    try:
        rc = lib.sd_igemm_plan((C.c_int * 9)(*geom), (C.c_int * 10)(*flags), out, name)
    finally:
        lib.sd_igemm_force(-1, 0)
    assert rc == 0, lib.sd_last_error()
    return list(out), name.value.decode()


def _sub(c, ops):
    return ops.x[:EMU_ROWS] if c.M > EMU_ROWS else ops.x


def _ratio(c, x, ops, lay, order="slabs", defect=None):
    """max |emulation - reference| / bound of one consumer run on the rows x."""
    if c.entry == "ffn":
        r, _, bound = lc.reference_ffn(x, ops, lay)
        got = lc.emulate_ffn(x, ops, lay, order, defect)
    else:
        r, bound = lc.reference_linear(x, ops, lay, c.geglu)
        got = lc.emulate_linear(x, ops, lay, c.geglu, order, defect)
    assert (bound > 0).all() and torch.isfinite(bound).all() and torch.isfinite(r).all()
    # (a defect may overflow fp16: a non-finite result is as far outside the bound as can be)
    return torch.nan_to_num((got.double() - r).abs() / bound, nan=float("inf")).max().item()


def test_ids_are_unique_and_every_family_has_cases():
    ids = [lc.run_id(c, lay, prof) for c in lc.CONSUMERS for lay, prof in c.runs]
    assert len(ids) == len(set(ids))
    assert {c.family for c in lc.CONSUMERS} == lc.CONSUMER_FAMILIES
    pids = [lc.producer_id(p) for p in lc.PRODUCERS]
    assert len(pids) == len(set(pids))
    for c in lc.CONSUMERS:
        assert c.runs and all(prof in lc.PROFILES for _, prof in c.runs)
        for lay, _ in c.runs:
            lc.part_widths(c.C, lay)                            # a valid layout of C columns
            assert lay[0] <= lc.MAX_PARTS


def test_every_unrestricted_consumer_gets_the_layouts():
    """(1, C), (2, C / 2), (4, C / 4), (5, 64), (20, 16), the ragged (3, 128) and (7, 48) at C = 320 and (20, 64) at C = 1280
    for every consumer that takes any layout; geglu_persist_kernel only sees C = 320 from five parts up (the plan sends
    fewer to wsgemm), so it gets the same set at C = 640 instead.  wsgemm: 1, 2, 3 (128 | 128 | 64) and 4 parts."""
    def layouts(family, C):
        return {lay for c in lc.CONSUMERS if c.family == family and c.C == C for lay, prof in c.runs if prof == "rows"}
    for family in ("tile", "tile-geglu", "igemm3", "ffn"):
        assert layouts(family, 320) >= set(lc.L320), family
    for family in ("tile", "tile-geglu", "igemm3", "pgemm"):
        assert (20, 64) in layouts(family, 1280), family
    assert layouts("pgemm", 640) >= set(lc.L640) and layouts("pgemm", 320) >= {(5, 64), (20, 16), (7, 48)}
    assert layouts("wsgemm", 320) == set(lc.LWS)
    assert layouts("wsgemm-declines", 320) == {(5, 64)}
    # every profile on every family
    for family in lc.CONSUMER_FAMILIES - {"wsgemm-declines"}:
        assert {prof for c in lc.CONSUMERS if c.family == family for _, prof in c.runs} == set(lc.PROFILES), family


@pytest.mark.parametrize("case", lc.CONSUMERS, ids=[lc.consumer_id(c) for c in lc.CONSUMERS])
def test_fp32_emulation_stays_inside_the_bound(case):
    """Every (layout, profile) the GPU suite runs, the accumulation in three orders: 64-deep slabs first to last, last to
    first, and 16 columns at a time."""
    worst = 0.0
    for lay, prof in case.runs:
        ops = lc.consumer_operands(case, prof)
        x = _sub(case, ops)
        for order in lc.ORDERS if case.entry != "ffn" else lc.ORDERS[:2]:
            ratio = _ratio(case, x, ops, lay, order)
            assert ratio <= 1.0, (lc.run_id(case, lay, prof), order, ratio)
            worst = max(worst, ratio)
    print("%s: worst emulated |err| / bound %.3f" % (lc.consumer_id(case), worst))
    _worst[case.family] = max(_worst.get(case.family, 0.0), worst)


# The defects the bound is for, and the profiles each is claimed for (where the defect moves the result by more than the
# fp32 accumulation of that profile can): rows of the `rows` profile differ in level and spread, so another row's
# statistics are plainly wrong, while offset:50 and spikes rows share theirs; a wrong weight of the short last part
# moves the mean by (part_w - n_last) / C of that part's distance from it, a spread's worth under `rows`, a spike's under
# `spikes` ((7, 48) has channel C - 2 in its last part), 0.05 under offset:50, below that profile's accumulation term; a
# missing mean * wsum shows wherever the mean is not about zero; a missing 21st part shows under `rows` and `spikes`, but
# not under offset:50 at C = 1344: there (K + 3) u32 rstd |mean| S alone is of the order of the output (rstd 10, |mean| 50,
# S about 30), the price of a bound that holds for any summation order, and the collapsed result (mean 47.6, rstd 0.4)
# stays just inside it (0.92 of the bound), so that profile is not claimed for it.
_OVER = [lc.Consumer("over", "linear", 64, C_, 128, geglu, None, None, (), (((parts, w), "rows"),))
         for (C_, parts, w) in lc.OVER_CAPACITY for geglu in (0, 1)]
_SMALL = [c for c in lc.CONSUMERS if c.C == 320 and (c.M == 130 or c.family == "ffn" and c.M == 8192)]
CLAIMS = {
    "swap": (("rows",), _SMALL, lc.L320),
    "ragged-weight": (("rows", "spikes"), _SMALL, ((3, 128), (7, 48))),
    "truncated": (("rows", "spikes"), _OVER, None),
    "no-wsum": (("rows", "offset:50"), _SMALL, ((1, 320), (5, 64), (7, 48))),
}


@pytest.mark.parametrize("defect", lc.DEFECTS)
def test_bound_sees_the_seeded_defect(defect):
    """The bound as a condition: the emulation with the defect exceeds it on every case, layout and profile claimed."""
    profiles, cases, layouts = CLAIMS[defect]
    assert cases
    least = float("inf")
    for case in cases:
        for prof in profiles:
            ops = lc.consumer_operands(case, prof)
            x = _sub(case, ops)
            for lay in layouts or [r[0] for r in case.runs]:
                if defect == "ragged-weight" and case.entry == "ffn":
                    continue        # (5 % of a spread in the hidden tensor is inside the feed-forward's 1280-term bound)
                clean = _ratio(case, x, ops, lay)
                ratio = _ratio(case, x, ops, lay, defect=defect)
                assert clean <= 1.0 < ratio, (defect, lc.consumer_id(case), lay, prof, clean, ratio)
                least = min(least, ratio)
    print("%s: smallest |err| / bound over %s: %.1f" % (defect, "/".join(profiles), least))
    _least[defect] = least


def test_every_consumer_case_plans_to_the_kernel_it_names(engine_lib):
    moved = []
    for c in lc.CONSUMERS:
        if c.entry == "ffn":
            continue            # ffn_fused_supported is not part of igemm2_plan: the GPU suite asserts `fused`
        for parts in sorted({lay[0] for lay, _ in c.runs}):
            geom, flags = lc.consumer_plan_args(c, parts)
            out, name = _plan(engine_lib, geom, flags, c.force)
            ok = out[0] == c.want if c.want is not None else (out[0] not in c.avoid and out[0] in cc.TILE)
            if not ok or out[2] != 1:
                moved.append((lc.consumer_id(c), parts, c.want, c.avoid, out[0], out[2], name))
    assert not moved, "the plan moved: these cases no longer run the kernel they were written for: %r" % moved[:8]


def test_every_producer_case_plans_to_the_kernel_and_layout_it_names(engine_lib):
    moved = []
    for p in lc.PRODUCERS + [ch.prod for ch in lc.CHAINS]:
        geom, flags = lc.producer_plan_args(p)
        out, name = _plan(engine_lib, geom, flags, p.force)
        got = (out[0] if out[4] else -1, out[5], out[6])
        if got != (p.want, p.parts, p.part_w) or (p.want == -1) != (out[2] > 1):
            moved.append((lc.producer_id(p), (p.want, p.parts, p.part_w), got, out[2], name))
    assert not moved, "the plan moved: %r" % moved[:8]
    for ch in lc.CHAINS:
        c = lc.chain_consumer(ch)
        out, name = _plan(engine_lib, *lc.consumer_plan_args(c, ch.prod.parts), c.force)
        assert out[0] == ch.want, ("the plan moved", ch.name, out[0], name)
        assert ch.prod.family.split("-")[0] not in ch.name.split("->")[1], ch.name       # a consumer of another family


def test_cases_reach_every_kernel_of_the_chain():
    want = lambda fam: {c.want for c in lc.CONSUMERS if c.family == fam}       # noqa: E731
    # consumers: a 64-, a 128- and a 160-column streamed tile, the GEGLU tiles, igemm3, wsgemm 13 / 14, pgemm, ffn
    assert {cc.TILE[v][1] for v in want("tile")} == {64, 128, 160}
    assert want("tile-geglu") == {0, 1} and want("igemm3") == {cc.REG} and want("wsgemm") == {13, 14}
    assert want("pgemm") == {100} and want("ffn") == {1}
    assert {c.geglu for c in lc.CONSUMERS if c.family == "wsgemm-declines"} == {0, 1}
    assert {lay[0] for c in lc.CONSUMERS if c.family == "wsgemm" for lay, _ in c.runs} == set(range(1, lc.WS_MAX_PARTS + 1))
    assert all(lay[0] == lc.WS_MAX_PARTS + 1 for c in lc.CONSUMERS if c.family == "wsgemm-declines" for lay, _ in c.runs)
    # ragged M on the tiles and igemm3; wsgemm at its minimum, with a run of three tiles, with an uneven split
    for fam in ("tile", "tile-geglu", "igemm3"):
        assert any(c.M % 128 for c in lc.CONSUMERS if c.family == fam)
    for geglu in (0, 1):
        ms = {c.M for c in lc.CONSUMERS if c.family == "wsgemm" and c.geglu == geglu}
        assert ms == {1024, 4096, 1152}
    for c in lc.CONSUMERS:
        if c.family == "wsgemm" and c.M == 4096:
            # the launcher's run arithmetic (wsgemm.hip): 32 blocks per XCD over L = tiles_n * nm entries
            tiles_n = (2 if c.geglu else 1) * c.O // (128 if c.geglu else 160)
            nm = c.M // 128 // 8
            runs = []
            for kblk in range(32):
                lo, hi = kblk * tiles_n * nm // 32, (kblk + 1) * tiles_n * nm // 32
                while lo < hi:
                    T = min(nm - lo % nm, hi - lo)
                    runs.append(T)
                    lo += T
            assert max(runs) >= 3, runs
        if c.family == "pgemm":
            tiles_m, tiles_n = c.M // 256, 2 * c.O // 128
            assert tiles_m * tiles_n >= 512 > (tiles_m - 1) * tiles_n           # the least the plan still sends there
            assert tiles_n % min(256 // tiles_m, tiles_n) != 0                  # a ragged tiles-per-block split
    assert {c.M for c in lc.CONSUMERS if c.family == "ffn"} == {8192, 8320}
    # producers: the three tile widths, wsgemm, igemm3, row_stats_kernel, each with and without a residual
    assert {(p.want, p.res) for p in lc.PRODUCERS} == {(v, r) for v in (3, 1, 2, 13, cc.REG, -1) for r in (False, True)}
    assert any(p.C % p.part_w for p in lc.PRODUCERS if p.family == "tile")      # a short last part
    assert {ch.prod.family for ch in lc.CHAINS} == {"tile", "wsgemm", "igemm3", "row_stats"}


def test_layouts_beyond_capacity_are_refused_before_any_launch(engine_lib):
    """sd_op_ln_linear and sd_op_ln_ffn_geglu refuse more parts than a consumer kernel holds per row (the streamed tiles,
    where such a launch would land, would merge the first 20 only), naming ln_parts and the limit, on the host."""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    got = C.c_int(-7)
    for (Cc, parts, w) in lc.OVER_CAPACITY:
        assert parts > lc.MAX_PARTS
        lc.part_widths(Cc, (parts, w))                          # a valid layout otherwise
        for geglu in (0, 1):
            rc = engine_lib.sd_op_ln_linear(p, p, parts, w, p, p, 1e-5, p, p, p, 128, Cc, 128, geglu, 0, 1.0, C.byref(got), None)
            msg = engine_lib.sd_last_error()
            assert rc == 1 and b"sd_op_ln_linear" in msg and b"ln_parts %d" % parts in msg and b"20" in msg, (rc, msg)
        rc = engine_lib.sd_op_ln_ffn_geglu(p, p, parts, w, p, p, 1e-5, p, p, p, p, p, 8192, Cc, C.byref(got), None)
        msg = engine_lib.sd_last_error()
        assert rc == 1 and b"sd_op_ln_ffn_geglu" in msg and b"ln_parts %d" % parts in msg and b"20" in msg, (rc, msg)
    assert got.value == -7


def test_no_case_is_skipped_or_expected_to_fail():
    for mod in ("test_ln_gpu.py", "ln_cases.py"):
        src = open(os.path.join(ROOT, "tests", mod)).read()
        for word in ("skip", "xfail"):
            assert word not in src, (mod, word)


def test_report():
    """Prints what the tests above measured (run the module as a whole): the margin stated in the module docstring."""
    for fam in sorted(_worst):
        print("worst emulated |err| / bound, %-16s %.3f" % (fam, _worst[fam]))
    for d in sorted(_least):
        print("seeded defect %-14s smallest |err| / bound %.1f" % (d, _least[d]))
    assert all(v <= 1.0 for v in _worst.values()) and all(v > 1.0 for v in _least.values())
