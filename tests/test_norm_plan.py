"""The normalisation kernels' dispatch and the cases of tests/norm_cases.py, checked on the CPU through sd_norm_plan (host
code only; launch_groupnorm and launch_gn_stats decide through the same function): gn_slabs leaves no empty slab and moves
no sound slab count, each case plans to the kernels it names, together they reach every kernel form and every path of
the prologues, and an fp32 emulation of every kernel's summation order stays inside the element-wise bound of the GPU
suite while six plausible kernel bugs do not."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import norm_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = sorted({(c.C, c.G) for c in nc.CASES})


def plan(lib, c):
    out = (C.c_int64 * 10)()
    rc = lib.sd_norm_plan(c.N, c.HW, c.C, c.G, 1 if c.pre else 0, nc.cdiv(c.HW, c.pre) if c.pre else 0, out)
    assert rc == 0, (nc.case_id(c), lib.sd_last_error())
    return list(out)


def plan_batch(lib, N, hws, Cc, G):
    q = np.empty((len(hws), 4), np.int64)
    q[:, 0], q[:, 1], q[:, 2], q[:, 3] = N, hws, Cc, G
    out = np.empty((len(hws), 10), np.int64)
    rc = lib.sd_norm_plan_batch(len(hws), q.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0, lib.sd_last_error()
    return out


def parent_slabs(N, hws, Cc, G):
    cblocks = nc.cdiv(Cc, nc.block_channels(Cc, G))
    s = max(1024 // (N * cblocks), 1)
    return np.minimum(np.minimum(s, np.maximum(hws // 64, 1)), 256)


def test_no_slab_is_empty_and_sound_slab_counts_did_not_move(engine_lib):
    """(S - 1) rows < HW <= S rows with rows = ceil(HW / S) for every map size up to 30000; before the fix this failed
    from HW = 4225 on, e.g. at (N, HW, C, G) = (1, 4225, 128, 32): S = 66 slabs of 65 rows, the last one empty."""
    hws = np.arange(1, 30001, dtype=np.int64)
    assert (128, 32) in PAIRS
    unsound = 0
    for Cc, G in PAIRS:
        for N in (1, 2, 3, 4, 8, 16):
            out = plan_batch(engine_lib, N, hws, Cc, G)
            S, rows, scratch = out[:, 5], out[:, 6], out[:, 8]
            assert (rows == (hws + S - 1) // S).all()
            bad = ~(((S - 1) * rows < hws) & (hws <= S * rows))
            assert not bad.any(), ("empty slab", N, int(hws[bad][0]), Cc, G, int(S[bad][0]), int(rows[bad][0]))
            assert (S >= 1).all() and (S <= 256).all()
            assert (scratch >= N * S * G * 2).all()
            ps = parent_slabs(N, hws, Cc, G)
            sound = (ps - 1) * ((hws + ps - 1) // ps) < hws
            assert (S[sound] == ps[sound]).all(), (N, Cc, G, int(hws[sound][(S != ps)[sound]][0]))
            assert (S[~sound] < ps[~sound]).all()
            unsound += int((~sound).sum())
    assert unsound > 1000          # the restatement does see the old defect


# GroupNorm shapes of the benchmark's two configurations (SD1.5 512 x 512 batch 4, SDXL 1024 x 1024 batch 2; UNet with
# and without the CFG pair, VAE decode): (N values, HW, widths)
BENCH_SHAPES = [
    ((4, 8), 64, (1280, 2560)), ((4, 8), 256, (640, 1280, 1920, 2560)), ((4, 8), 1024, (320, 640, 960, 1280, 1920)),
    ((4, 8), 4096, (320, 640, 960)),
    ((1, 4), 4096, (512,)), ((1, 4), 16384, (512,)), ((1, 4), 65536, (256, 512)), ((1, 4), 262144, (128, 256)),
    ((2, 4), 1024, (640, 1280, 1920, 2560)), ((2, 4), 4096, (320, 640, 960, 1280, 1920)), ((2, 4), 16384, (320, 640, 960)),
    ((1, 2), 16384, (512,)), ((1, 2), 65536, (512,)), ((1, 2), 262144, (256, 512)), ((1, 2), 1048576, (128, 256)),
]


def test_slab_counts_on_the_benchmark_shapes_are_the_parents(engine_lib):
    n = 0
    for Ns, HW, widths in BENCH_SHAPES:
        for N in Ns:
            for Cc in widths:
                for ch in {Cc, Cc // 2} if Cc >= 640 else {Cc}:           # and the halves sd_op_groupnorm_concat summarises
                    out = plan_batch(engine_lib, N, np.array([HW], np.int64), ch, 32)[0]
                    ps = int(parent_slabs(N, np.array([HW]), ch, 32)[0])
                    assert HW % ps == 0, (N, HW, ch, ps)                  # the parent's partition was exact here
                    assert (out[5], out[6]) == (ps, HW // ps), (N, HW, ch)
                    n += 1
    assert n > 100


def test_case_ids_are_unique_and_none_is_skipped():
    ids = [nc.case_id(c) for c in nc.CASES]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1][:5]
    for mod in ("test_norm_gpu.py", "norm_cases.py"):
        src = open(os.path.join(ROOT, "tests", mod)).read()
        for word in ("skip", "xfail"):
            assert word not in src, (mod, word)
    src = open(os.path.join(ROOT, "tests", "test_norm_gpu.py")).read()
    for group in {c.group for c in nc.CASES}:
        assert '"%s"' % group in src, group
    assert "LN_CASES" in src and "ROW_STATS_CASES" in src


def test_every_case_plans_to_the_kernels_it_names(engine_lib):
    moved = []
    for c in nc.CASES:
        p = plan(engine_lib, c)
        if tuple(p[:5]) != c.want:
            moved.append((nc.case_id(c), c.want, tuple(p[:5])))
        assert p[9] == int(bool(c.pre) and p[1] != 0), nc.case_id(c)
        if c.pre and p[9]:
            assert (p[5], p[6]) == (nc.cdiv(c.HW, c.pre), 0)
    assert not moved, "the plan moved: these cases no longer run the kernels they were written for: %r" % moved[:8]


def test_cases_reach_every_kernel_and_every_prologue_path(engine_lib):
    plans = [(c, plan(engine_lib, c)) for c in nc.CASES]
    wants = {c.want for c in nc.CASES}
    assert {w[2:4] for w in wants if w[1] == 0} == {(256, 4), (256, 16), (1024, 16)}
    assert {w[0] for w in wants} == {0, 1, 2}
    assert {w[1] for w in wants} == {0, 1, 2}
    assert {w[3] for w in wants if w[1] == 2} == {8, 4, 2, 1}
    assert {w[4] for w in wants if w[1] == 2} == {0, 1}
    # both statistics kernels in front of both apply kernels that take them
    assert {(w[0], w[1]) for w in wants if w[0]} >= {(1, 1), (1, 2), (2, 2)}
    equal, widths, lw, extra = set(), set(), set(), set()
    for c, p in plans:
        if p[1] != 2:
            continue
        eq, blocks = nc.apply2_paths(c, p)
        equal.add((eq, bool(c.pre)))
        widths.add(len(blocks) == 2)
        for cw, ng, LW, parts1, more in blocks:
            lw.add((LW, bool(p[4])))
            extra.add(more)
    assert equal >= {(True, False), (False, False), (True, True), (False, True)}     # equal and ragged, own and supplied
    assert widths == {True, False}                       # a full last channel block and a narrower one
    assert lw >= {(1, False), (4, False), (1, True)}     # one wave fetches / four do; behind the finalize one always
    assert extra == {True, False}                        # more than four summaries per loader thread
    # fused: every HW edge of the three forms, the widths and the fall-off
    assert {c.HW for c in nc.CASES if c.group == "fused" and c.C == 320} == {1, 63, 64, 65, 255, 256, 257, 510, 512}
    assert {(c.HW, c.want[1]) for c in nc.CASES if c.C == 5120} == {(48, 0), (49, 2), (200, 2)}
    assert {c.C // c.G for c in nc.CASES if c.want[0] == 1 and c.want[1] == 2} >= {1, 2, 3, 6}
    assert {c.G for c in nc.CASES} >= {1, 8, 16, 32, 256}
    # S at the cap; the supplied summaries on both sides of the finalize threshold, tiles of 128 and 256, ragged tiles
    assert any(p[5] == 256 and c.HW % p[6] for c, p in plans if p[0])
    sup = [(c, p) for c, p in plans if c.pre and p[9]]
    assert {(c.pre, p[5] > 64) for c, p in sup} == {(128, False), (128, True), (256, False), (256, True)}
    assert any(c.HW % c.pre for c, p in sup if p[4]) and any(c.HW % c.pre for c, p in sup if not p[4])
    assert any(c.pre and not p[9] for c, p in plans)     # a small map: the fused kernel ignores them
    # offsets with a constant group behind every kernel form
    off = {c.want[:2] + c.want[4:] for c in nc.CASES if c.profile != "randn"}
    assert off >= {(0, 0, 0), (1, 2, 0), (2, 2, 0), (1, 1, 0), (0, 2, 0), (0, 2, 1)}
    for g in ("strided",):
        assert all(c.layouts == ("dense", "left", "right") for c in nc.CASES if c.group == g)
    assert {c.want[:2] + c.want[4:] for c in nc.CASES if c.group == "strided"} >= {(0, 0, 0), (1, 2, 0), (2, 2, 0), (1, 1, 0), (0, 2, 1)}


def test_ex_entries_reject_bad_arguments(engine_lib):
    """Strides below C or no multiple of 8, a missing `ran`, and summaries with an empty or a missing tile are refused
    before anything touches a device."""
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    ran = (C.c_int64 * 10)()

    def gn(ldx=64, ldy=64, HW=1000, summ=None, S=0, rows=0, ran=ran, G=32):
        return engine_lib.sd_op_groupnorm_ex(p, ldx, p, p, p, ldy, 1, HW, 64, G, 1e-5, 0, summ, S, rows, ran, None)
    for kw in (dict(ldx=56), dict(ldx=68), dict(ldy=63), dict(ldy=100), dict(ran=None), dict(G=0), dict(G=5)):
        assert gn(**kw) == 1, kw                                    # SD_ERR_INVALID
        assert b"sd_op_groupnorm_ex" in engine_lib.sd_last_error(), kw
    # HW = 1000: (S - 1) rows < HW <= S rows fails -- tiles that stop short, and tiles of which the last is empty
    for S, rows in ((7, 128), (9, 128), (4, 128), (0, 128), (8, 0), (1001, 1), (2, 1000), (64, 16), (-1, 128)):
        assert gn(summ=p, S=S, rows=rows) == 1, (S, rows)
        assert b"no empty one" in engine_lib.sd_last_error()
    assert engine_lib.sd_op_layernorm_ex(p, 60, p, p, p, 64, 4, 64, 1e-5, None) == 1
    assert engine_lib.sd_op_layernorm_ex(p, 64, p, p, p, 68, 4, 64, 1e-5, None) == 1
    assert engine_lib.sd_op_row_stats(p, 60, C.cast(buf, C.POINTER(C.c_float)), 4, 64, None) == 1
    out = (C.c_int64 * 10)()
    assert engine_lib.sd_norm_plan(1, 64, 100, 32, 0, 0, out) == 1
    assert engine_lib.sd_norm_plan(1, 64, 64, 32, 1, 0, out) == 1
    assert engine_lib.sd_norm_plan(1, 64, 64, 32, 0, 0, None) == 1


# ------------------------------------------------------------------------------------------------ the bound, on the CPU
_SMALL = [c for c in nc.CASES if c.N * c.HW * c.C <= 1 << 21]
_worst = {}


@pytest.mark.parametrize("case", nc.CASES, ids=[nc.case_id(c) for c in nc.CASES])
def test_fp32_emulation_stays_inside_the_bound(engine_lib, case):
    """Every kernel's summation order in numpy float32: at most half the bound's statistics term, inside the bound."""
    p = plan(engine_lib, case)
    x, gamma, beta, r, bound = nc.inputs_and_reference(case)
    assert (bound > 0).all() and torch.isfinite(bound).all() and torch.isfinite(r).all()
    # not vacuous: the typical element is allowed a little more than its own rounding; at |mean| / std = 500 a few
    # fp16 steps, which is what u |mean| sc -- the rounding of the mean and of mean sc in fp32 -- comes to
    tight = (bound / nc.half_step(r)).median().item()
    assert tight <= (1.5 if case.profile == "randn" else 8.0), tight
    got = nc.emulate(case, p, x, gamma, beta)
    assert torch.isfinite(got.float()).all()
    ratio, used = nc.error_ratios(got, r, bound)
    _worst[case.group] = max(_worst.get(case.group, 0.0), used)
    print("%s: worst |err| / bound %.3f, fp32 terms used %.3f (group so far %.3f)" % (nc.case_id(case), ratio, used, _worst[case.group]))
    assert ratio <= 1.0, (nc.case_id(case), ratio)
    cg = nc.constant_group(case)
    if cg:                                          # the constant group: act(beta), finite, in the reference and the emulation
        b = beta.double()
        want = b * torch.sigmoid(b) if case.silu else b
        assert torch.equal(r[0, :, cg[0]:cg[1]], want[cg[0]:cg[1]].expand(case.HW, -1))


@pytest.mark.parametrize("case", nc.CASES, ids=[nc.case_id(c) for c in nc.CASES])
def test_statistics_constants_hold_twice_the_emulations_error(engine_lib, case):
    """STAT_A and STAT_R of the bound against the emulated statistics: a factor of two over the worst case."""
    p = plan(engine_lib, case)
    x = nc.make_inputs(case)[0]
    mean, var = nc.group_stats(x, case.G)
    m, rs = nc.emulate_stats(case, p, x)
    rstd = 1.0 / torch.sqrt(var + case.eps)
    dm = ((torch.from_numpy(m).double() - mean).abs() / (nc.U * (mean.abs() + var.sqrt()))).max().item()
    rel = (torch.from_numpy(rs).double() - rstd).abs() / rstd / nc.U
    live = var > 0                                  # (a constant group: rstd = eps^-1/2 whatever the statistics' error)
    rho = rel[live].max().item()
    share = (rel / (nc.STAT_R + nc.STAT_RM * mean.abs() / var.sqrt().clamp_min(1e-30)))[live].max().item()
    print("%s: mean error %.2f u (|mean| + std), rstd error %.2f u = %.3f of its term" % (nc.case_id(case), dm, rho, share))
    assert 2 * dm <= nc.STAT_A and 2 * share <= 1.0, (dm, rho, share)


MUTATIONS = {
    "drop": "one summary left out of the merge",
    "empty": "an empty slab merged with equal weight",
    "group": "the group index off by one in a chunk that straddles two groups",
    "ex2": "variance as E[x^2] - mean^2 at offset 50",
    "count": "a count of (HW - 1) cpg",
    "gb": "gamma / beta shifted by one channel block",
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_bound_sees_a_wrong_kernel(engine_lib, mutation):
    """Each wrong emulation breaks the bound, on every case it applies to among the small ones (`count`: where the
    missing pixel is at least 1 / 2000 of the map -- beyond, the slip is below fp16 resolution)."""
    n = 0
    for c in _SMALL:
        p = plan(engine_lib, c)
        if not nc.mutation_applies(c, p, mutation) or (mutation == "count" and c.HW > 1000) or c.HW == 1:
            continue
        x, gamma, beta, r, bound = nc.inputs_and_reference(c)
        got = nc.emulate(c, p, x, gamma, beta, mutation)
        ratio = ((got.double() - r).abs() / bound)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max().item()
        assert ratio > 1.0, (MUTATIONS[mutation], nc.case_id(c), ratio)
        n += 1
        if n >= 6:
            break
    assert n >= 2, mutation


@pytest.mark.parametrize("t", nc.LN_CASES, ids=[nc.ln_id(t) for t in nc.LN_CASES])
def test_layernorm_emulation_stays_inside_the_bound(t):
    rows, Cc, profile, _ = t
    x, gamma, beta, r, bound, stat = nc.ln_inputs_and_reference(rows, Cc, profile)
    got, mean, m2 = nc.emulate_layernorm(x, gamma, beta)
    ratio, used = nc.error_ratios(got, r, bound)
    print("layernorm %s: worst |err| / bound %.3f, fp32 terms used %.3f" % (nc.ln_id(t), ratio, used))
    assert ratio <= 1.0, ratio
    assert (bound / nc.half_step(r)).median().item() <= (1.5 if profile == "randn" else 8.0)


_DEFECT = [c for c in nc.CASES if c.group == "defect"]


@pytest.mark.parametrize("case", _DEFECT, ids=[nc.case_id(c) for c in _DEFECT])
def test_slab_summaries_of_the_emulation_stay_inside_their_terms(engine_lib, case):
    """What test_norm_gpu asks of sd_op_gn_stats, asked of the emulated statistics kernels: at most half."""
    p = plan(engine_lib, case)
    x = nc.make_inputs(case)[0]
    S, rows, CB = p[5], p[6], p[7]
    part = (nc.emu_stats2 if p[0] == 2 else nc.emu_stats1)(x.numpy().astype(np.float32), S, rows, CB, case.G)
    dm, dq = nc.summary_errors(torch.from_numpy(part), nc.tile_summaries(x, case.G, rows)[1],
                               nc.slab_counts(case.HW, S, rows, case.C // case.G))
    print("%s: worst mean error %.3f, worst M2 error %.3f of the terms" % (nc.case_id(case), dm, dq))
    assert dm <= 0.5 and dq <= 0.5


@pytest.mark.parametrize("t", nc.ROW_STATS_CASES, ids=[nc.ln_id(t) for t in nc.ROW_STATS_CASES])
def test_row_statistics_of_the_emulation_stay_inside_their_terms(t):
    rows, Cc, profile = t
    x, gamma, beta, _, _, want = nc.ln_inputs_and_reference(rows, Cc, profile)
    _, mean, m2 = nc.emulate_layernorm(x, gamma, beta)
    dm, dq = nc.summary_errors(torch.from_numpy(np.stack([mean, m2], axis=1)), want, float(Cc))
    print("row_stats %s: worst mean error %.3f, worst M2 error %.3f of the terms" % (nc.ln_id(t), dm, dq))
    assert dm <= 0.5 and dq <= 0.5
