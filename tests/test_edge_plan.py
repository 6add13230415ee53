"""The cases of tests/edge_cases.py, checked on the CPU: sd_small_linear_plan (host code only; launch_small_linear decides
through the same function) gives every linear case's kernel and both sides of every clause are reached; every exact
case is representable, so its float64 result is the fp32 / fp16 result of any summation order; fp32 emulations of the
three kernels' arithmetic stay inside the element bounds of the GPU suite, the emulated summaries inside half of theirs;
eight plausible kernel bugs do not; the refusals come before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import edge_cases as ec
import norm_cases as nc
from stablediffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sd_small_linear_plan", "sd_op_unet_conv_out_ex")
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    """The worst figures of every group of cases, printed once behind the module's last test."""
    yield
    for group, w in sorted(_worst.items()):
        print("\n[edge] %-20s worst %s" % (group, ", ".join("%.3f" % v if isinstance(v, float) else "%d cases" % v for v in w)), end="")
    print()


def note(group, ratio, used=None):
    w = _worst.setdefault(group, [0.0, 0.0])
    w[0] = max(w[0], ratio)
    if used is not None:
        w[1] = max(w[1], used)
    return "(group %s so far: worst |err| / bound %.3f, fp32 terms used %.3f)" % (group, w[0], w[1])


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def stats_plan(lib, c):
    """(S, rows, CB) of the statistics pass sd_op_unet_conv_out_ex makes without summaries (launch_gn_stats)."""
    out = (C.c_int64 * 10)()
    assert lib.sd_norm_plan(c.N, c.H * c.W, ec.C_OUT, c.G, 0, 0, out) == 0, lib.sd_last_error()
    assert (ec.C_OUT // c.G) >= 8                      # gn_stats2_kernel
    return out[5], out[6], out[7]


def tail_part(lib, c, x):
    if c.S:
        return ec.tail_supplied(c, x).numpy(), c.S, c.rows
    S, rows, CB = stats_plan(lib, c)
    return nc.emu_stats2(x.numpy().astype(np.float32), S, rows, CB, c.G), S, rows


# ------------------------------------------------------------------------------------------------------- the entries
def test_new_symbols_are_declared_bound_and_exported(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sd_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", src))
    so = os.path.join(ROOT, "stablediffusion_amd", "libsd_engine.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(engine_lib, name) is not None
        assert re.search(r"\bT %s\b" % name, exported), name
    assert len(_lib.SIGNATURES["sd_small_linear_plan"][1]) == 3
    assert len(_lib.SIGNATURES["sd_op_unet_conv_out_ex"][1]) == 21


def test_the_launchers_decide_through_the_shared_functions():
    """One call site each, and the predicate stands in one place."""
    misc = open(os.path.join(ROOT, "stablediffusion_amd", "csrc", "misc.hip")).read()
    capi = open(os.path.join(ROOT, "stablediffusion_amd", "csrc", "capi.cpp")).read()
    launcher = misc[misc.index("int launch_small_linear("):misc.index("int launch_add_f32(")]
    assert launcher.count("small_linear_plan(") == 1 and "SK_MAXKS" not in launcher and "% 32" not in launcher
    assert misc.count('getenv("SD_NO_SKINNY_LINEAR")') == 1 and "static const bool no_skinny" in misc
    assert capi.count("return small_linear_plan(") == 1
    old = capi[capi.index("int sd_op_unet_conv_out("):capi.index("int sd_bench_conv2d(")]
    assert old.count("sd_op_unet_conv_out_ex(") == 1 and "launch_conv_tail" not in old and "launch_gn_stats" not in old
    assert capi.count("launch_conv_tail(") == 1


def test_case_ids_are_unique_and_none_is_skipped():
    for cases, ident in ((ec.HEAD_CASES, ec.head_id), (ec.TAIL_CASES, ec.tail_id), (ec.LIN_CASES, ec.lin_id)):
        ids = [ident(c) for c in cases]
        assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1][:5]
    for mod in ("test_edge_gpu.py", "edge_cases.py"):
        src = open(os.path.join(ROOT, "tests", mod)).read()
        for word in ("skip", "xfail"):
            assert word not in src, (mod, word)


def test_small_linear_plan_gives_every_cases_kernel(engine_lib):
    plan = engine_lib.sd_small_linear_plan
    for c in ec.LIN_CASES:
        assert plan(c.B, c.K, c.n_out) == c.want, ec.lin_id(c)
    assert {c.want for c in ec.LIN_CASES} == {0, 1}
    for kind in ("grid", "split", "randn"):
        assert {c.want for c in ec.LIN_CASES if c.kind == kind} == {0, 1}
    # both sides of every clause, the other clauses holding
    for (B, K, n), want in ec.THRESHOLDS:
        assert plan(B, K, n) == want, (B, K, n)
    assert (plan(16, 64, 48), plan(17, 64, 48)) == (1, 0)                   # B <= 16
    assert (plan(8, 32, 16), plan(8, 40, 16)) == (1, 0)                     # K % 32
    assert (plan(8, 1280, 16), plan(8, 1312, 16)) == (1, 0)                 # K <= 1280
    assert (plan(8, 64, 16), plan(8, 64, 20)) == (1, 0)                     # n_out % 16
    for bad in ((8, 12, 16), (8, 33, 16), (0, 32, 16), (8, 32, 0), (8, 0, 16)):
        assert plan(*bad) == -1, bad
    # the time-embedding path of the UNets runs the MFMA kernel, the stacked time_emb_proj with the block loop
    for B in (1, 2, 4, 8, 16):
        for K, n in ((320, 1280), (1280, 1280), (256, 1280), (1280, 16 * 513)):
            assert plan(B, K, n) == 1
    assert plan(8, 2816, 1280) == 0                                         # SDXL's add_embedding.linear_1: the GEMV
    # the cases reach what the issue names
    sk = [c for c in ec.LIN_CASES if c.want == 1]
    gv = [c for c in ec.LIN_CASES if c.want == 0]
    assert {c.K for c in sk} >= set(ec.SK_K) and {c.n_out for c in sk} >= set(ec.SK_N) and {c.B for c in sk} >= set(ec.SK_B)
    assert {c.K for c in gv} >= set(ec.GV_K) and {c.n_out for c in gv} >= set(ec.GV_N) and {c.B for c in gv} >= set(ec.GV_B)
    assert any(c.n_out // 16 > 512 for c in sk) and any(c.B > 16 and c.K % 32 == 0 and c.K <= 1280 and c.n_out % 16 == 0 for c in gv)
    assert any(not c.bias for c in sk) and any(not c.bias for c in gv)
    assert {(c.silu_in, c.silu_out) for c in sk if c.kind == "randn"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c.silu_in, c.silu_out) for c in gv if c.kind == "randn"} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_cases_reach_what_they_were_written_for():
    h = ec.HEAD_CASES
    for kind in ("grid", "tap"):
        assert {(c.H, c.W) for c in h if c.kind == kind} == set(ec.HEAD_SHAPES)
        assert {(c.N, c.Cin) for c in h if c.kind == kind} == {(n, ci) for n in (1, 3) for ci in (1, 4, 7)}
        assert {c.G for c in h if c.kind == kind} == {0, 1, 5, 32}
        for G in (0, 1, 5, 32):
            assert {c.Cin for c in h if c.kind == kind and c.G == G} == {1, 4, 7}
    assert {(c.H, c.W) for c in h if c.kind == "randn"} == {(8, 16), (16, 24)}
    assert any(c.profile == "p50" for c in h)
    t = ec.TAIL_CASES
    assert {(c.H, c.W) for c in t} >= {(8, 16), (16, 16), (8, 32), (24, 48)}
    assert {c.N for c in t} == {1, 3} and {c.Cout for c in t} == {1, 2, 3, 4} and {c.silu for c in t} == {0, 1}
    assert {c.G for c in t} == {1, 5, 20, 32} and {c.layout for c in t} == {"dense", "ld328"}
    assert {(c.S, c.rows) for c in t if c.S and c.H * c.W == 512} == set(ec.TAIL_SUPPLIED)
    for c in t:
        if c.S:
            assert (c.S - 1) * c.rows < c.H * c.W <= c.S * c.rows
    assert {c.profile for c in t if c.kind == "randn"} == {"randn", "p50"}
    taps = {(ch, tp) for ts in ec.TAPSETS for ch, tp in ts}
    assert {tp for _, tp in taps} == set(range(9)) and {ch // 64 for ch, _ in taps} == set(range(5))
    assert {ch for ch, _ in taps} >= {0, 63, 64, 191, 319}
    assert {c.tapset for c in t if c.kind == "tap" and c.Cout == 4} == {0, 1, 2}


def test_refusals_come_before_anything_touches_a_device(engine_lib):
    """Host memory stands in for every pointer: a refused call returns SD_ERR_INVALID with a message and writes nothing."""
    buf = (C.c_uint16 * 64)()
    p = C.c_void_p(C.addressof(buf))
    for label, call in refusals(engine_lib, p, p, None):
        assert call() == 1, label
        assert b"sd_op_unet_conv" in engine_lib.sd_last_error(), label
    assert not any(buf)


def refusals(lib, ptr, y, stream):
    """(label, call) for every shape the two entries do not take; shared with the GPU suite."""
    def conv_in(N=1, Cin=4, H=8, W=16, Cout=320, G=32):
        return lambda: lib.sd_op_unet_conv_in(ptr, ptr, ptr, y, ptr, G, N, Cin, H, W, Cout, 0, None, stream)

    def conv_out(ldx=320, G=32, N=1, H=8, W=16, Cc=320, Cout=4, summ=None, S=0, rows=0):
        return lambda: lib.sd_op_unet_conv_out_ex(ptr, ldx, ptr, ptr, G, 1e-5, 1, ptr, ptr, y, N, H, W, Cc, Cout, summ, S, rows,
                                                  0, None, stream)
    return [
        ("conv_in: H W % 128", conv_in(H=8, W=8)), ("conv_in: H W % 128 (odd)", conv_in(H=9, W=16)),
        ("conv_in: 9 Cin > 64", conv_in(Cin=8)), ("conv_in: Cout", conv_in(Cout=328)),
        ("conv_in: groups = 64", conv_in(G=64)), ("conv_in: 320 % groups", conv_in(G=3)), ("conv_in: N = 0", conv_in(N=0)),
        ("conv_out: H % 8", conv_out(H=12, W=16)), ("conv_out: W % 16", conv_out(H=8, W=24)), ("conv_out: Cout = 5", conv_out(Cout=5)),
        ("conv_out: Cout = 0", conv_out(Cout=0)), ("conv_out: groups = 64", conv_out(G=64)), ("conv_out: 320 % groups", conv_out(G=3)),
        ("conv_out: C", conv_out(Cc=384, ldx=384)), ("conv_out: ldx < C", conv_out(ldx=312)), ("conv_out: ldx % 8", conv_out(ldx=324)),
        ("conv_out: an empty last summary", conv_out(H=16, W=32, summ=ptr, S=36, rows=15)),
        ("conv_out: summaries short of H W", conv_out(H=16, W=32, summ=ptr, S=34, rows=15)),
        ("conv_out: S = 0", conv_out(summ=ptr, S=0, rows=128)), ("conv_out: rows = 0", conv_out(summ=ptr, S=1, rows=0)),
    ]


# ------------------------------------------------------------------------------------------------ exact cases are exact
_HEAD_EXACT = [c for c in ec.HEAD_CASES if c.kind != "randn"]
_LIN_EXACT = [c for c in ec.LIN_CASES if c.kind != "randn"]


@pytest.mark.parametrize("case", _HEAD_EXACT, ids=[ec.head_id(c) for c in _HEAD_EXACT])
def test_conv_in_exact_cases_are_representable_and_the_emulation_matches(case):
    """grid: every product and partial sum is a multiple of 1/16 below 128, exact in fp32 in any order and an fp16
    number; tap: one non-zero product, the input itself.  So fp16(float64 result) is what any correct kernel stores."""
    x, w, bias, r, bound = ec.head_inputs_and_reference(case)
    if case.kind == "grid":
        mag = (bound - 2.0 ** -25 - ec.U16 * r.abs()) / ((9 * case.Cin + 3) * ec.U32)       # sum |x| |w| + |bias|
        assert mag.max().item() < 128 and torch.equal(r * 16, (r * 16).round())
        assert torch.equal(x.float(), x.float().round()) and torch.equal(w.float() * 16, (w.float() * 16).round())
    else:
        assert ((w != 0).sum(dim=(1, 2, 3)) == 1).all() and (w.float().sum(dim=(1, 2, 3)) == 1).all() and not bias.any()
        assert torch.equal(ec.head_tap_gather(case, x).double(), r)
        out = r == 0
        assert out.any() and same_bits(ec.head_tap_gather(case, x)[out], torch.zeros(int(out.sum()), dtype=torch.float16))
    assert torch.equal(r.half().double(), r)
    got, summ = ec.emulate_head(case, x, w, bias)
    assert same_bits(got, r.half()), ec.head_id(case)
    if case.G:
        check_head_summaries(case, got, summ, 0.5)


@pytest.mark.parametrize("case", _LIN_EXACT, ids=[ec.lin_id(c) for c in _LIN_EXACT])
def test_linear_exact_cases_are_representable_and_the_emulations_match(case):
    """grid: products multiples of 1/128, sums below 2^17 / 128; split: products multiples of 2^-16, sums below 256: 24
    bits either way, so every partial sum of either kernel is exact and the float64 result is an fp32 number.  split
    differs from the result on fp16(x) and x = fp16(x) + fp16(x - fp16(x)) exactly."""
    x, w, bias, r, bound = ec.lin_inputs_and_reference(case)
    unit = 2.0 ** -7 if case.kind == "grid" else 2.0 ** -16
    prod = x.double().abs().max() * w.double().abs().max()
    A = x.double().abs() @ w.double().abs().t() + (bias.double().abs() if case.bias else 0)
    assert torch.equal(x.double() / (unit * 16), (x.double() / (unit * 16)).round()) and prod <= 2.001 / 16
    assert torch.equal(w.double() * 16, (w.double() * 16).round())
    assert A.max().item() < unit * 2 ** 24 and torch.equal(r / unit, (r / unit).round())
    assert torch.equal(r.float().double(), r)
    if case.kind == "split":
        assert case.K * x.abs().max().item() / 16 < 256
        hi = x.half().float()
        lo = (x - hi).half().float()
        a = (x * 8).round() / 8
        assert torch.equal(hi + lo, x) and (hi != x).any() and set(((x - a) * 2.0 ** 12).unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert ((a.abs() >= 1).float().mean().item()) >= 0.5
        r16 = ec.lin_reference(case, hi, w, bias)[0]
        assert not torch.equal(r16, r) and (r16 != r).any(dim=1).all()            # every row loses something without lo
    # (the kernel the case runs; the GEMV takes every shape and the inputs are exact for it too: on the small ones, both)
    for kernel in sorted({case.want} | ({0} if case.n_out <= 48 else set())):
        got = torch.from_numpy(ec.emulate_linear(case, x, w, bias, kernel))
        assert (got[-ec.GUARD:] == 13.0).all()
        assert same_bits(got[:-ec.GUARD].reshape(case.B, case.n_out), r.float()), (ec.lin_id(case), kernel)


def test_conv_out_tap_weights_are_one_hot():
    for c in ec.TAIL_CASES:
        if c.kind == "tap":
            w, bias = ec.tail_weights(c)
            assert ((w != 0).sum(dim=(1, 2, 3)) == 1).all() and (w.float().sum(dim=(1, 2, 3)) == 1).all() and not bias.any()
            beta = ec.tail_inputs_and_reference(c)[2]
            chans = [ch for ch, _ in ec.TAPSETS[c.tapset][:c.Cout]]
            assert (beta[chans] != 0).all()                                  # zero after the norm is not act(beta)


# --------------------------------------------------------------------------------------------- emulations inside bounds
def check_head_summaries(case, y, summ, limit):
    want = ec.head_summary_reference(case, y)
    dm, dq = ec.head_summary_errors(case, summ, want)
    w = _worst.setdefault("conv_in summaries", [0.0, 0.0])
    w[0], w[1] = max(w[0], dm), max(w[1], dq)
    print("%s: summaries: worst mean error %.3f, worst M2 error %.3f of SLAB x the terms (so far %.3f, %.3f)"
          % (ec.head_id(case), dm, dq, w[0], w[1]))
    assert dm <= limit and dq <= limit, (ec.head_id(case), dm, dq)


_HEAD_RANDN = [c for c in ec.HEAD_CASES if c.kind == "randn"]


@pytest.mark.parametrize("case", _HEAD_RANDN, ids=[ec.head_id(c) for c in _HEAD_RANDN])
def test_conv_in_emulation_stays_inside_the_bound(case):
    """One 64-deep slab in fp32; head_epilogue's summation order against the float64 summaries of the stored values: at
    most half of SLAB times norm_cases' statistics terms, the factor of two test_norm_plan demands of its kernels."""
    x, w, bias, r, bound = ec.head_inputs_and_reference(case)
    got, summ = ec.emulate_head(case, x, w, bias)
    ratio, used = nc.error_ratios(got, r, bound)
    print("%s: worst |err| / bound %.3f, fp32 terms used %.3f %s" % (ec.head_id(case), ratio, used, note("conv_in", ratio, used)))
    assert ratio <= 1.0
    assert (bound / nc.half_step(r)).median().item() <= 2.5             # not vacuous: little more than the fp16 rounding
    check_head_summaries(case, got, summ, 0.5)


_TAIL = ec.TAIL_CASES


@pytest.mark.parametrize("case", _TAIL, ids=[ec.tail_id(c) for c in _TAIL])
def test_conv_out_emulation_stays_inside_the_bound(engine_lib, case):
    x, gamma, beta, w, bias, r, bound, outside = ec.tail_inputs_and_reference(case)
    part, S, rows = tail_part(engine_lib, case, x)
    got = ec.emulate_tail(case, x, gamma, beta, w, bias, part, S, rows)
    ratio = ec.worst_ratio(got, r, bound)
    if case.kind == "tap":
        assert outside.any() and not outside.all() and (r[outside] == 0).all() and (bound[outside] == 0).all()
        assert (got[outside].view(torch.int16) == 0).all()
        print("%s: worst |err| / bound %.3f %s" % (ec.tail_id(case), ratio, note("conv_out tap", ratio)))
    else:
        _, used = nc.error_ratios(got, r, bound)
        print("%s: worst |err| / bound %.3f, fp32 terms used %.3f %s" % (ec.tail_id(case), ratio, used, note("conv_out", ratio, used)))
        # sum |w| e_a adds the fp16 roundings of 2880 inputs as if they all pointed one way: about 0.01 at |y| ~ 1, some
        # sixty fp16 steps (more at p50, where e_a carries u |mean| sc).  The tap cases are the sharp ones.
        assert (bound / nc.half_step(r)).median().item() <= (128.0 if case.profile == "randn" else 512.0)
    assert ratio <= 1.0, (ec.tail_id(case), ratio)


_LIN_RANDN = [c for c in ec.LIN_CASES if c.kind == "randn"]


@pytest.mark.parametrize("case", _LIN_RANDN, ids=[ec.lin_id(c) for c in _LIN_RANDN])
def test_linear_emulations_stay_inside_the_bound(case):
    x, w, bias, r, bound = ec.lin_inputs_and_reference(case)
    assert (bound > 0).all()
    got = torch.from_numpy(ec.emulate_linear(case, x, w, bias, case.want))[:-ec.GUARD].reshape(case.B, case.n_out)
    ratio = ec.worst_ratio(got, r, bound)
    group = "skinny" if case.want else "gemv"
    print("%s: worst |err| / bound %.3f %s" % (ec.lin_id(case), ratio, note(group, ratio)))
    assert ratio <= 1.0, (ec.lin_id(case), ratio)


# ------------------------------------------------------------------------------------------------------------ mutations
def _first(cases, pred):
    return next(c for c in cases if pred(c))


def test_bound_sees_lo_dropped():
    n = 0
    for c in ec.LIN_CASES:
        if c.want == 1 and c.kind == "split":
            x, w, bias, r, bound = ec.lin_inputs_and_reference(c)
            got = torch.from_numpy(ec.emulate_linear(c, x, w, bias, 1, "lo"))[:-ec.GUARD].reshape(c.B, c.n_out)
            assert not same_bits(got, r.float()), ec.lin_id(c)
            n += 1
    assert n >= 20


def test_bound_sees_the_second_reduction_buffer_aliased():
    n = 0
    for c in ec.LIN_CASES:
        if c.want == 1 and c.n_out // 16 > 512 and c.kind != "randn":
            x, w, bias, r, bound = ec.lin_inputs_and_reference(c)
            got = torch.from_numpy(ec.emulate_linear(c, x, w, bias, 1, "alias"))[:-ec.GUARD].reshape(c.B, c.n_out)
            assert not same_bits(got[:, :16], r.float()[:, :16]) and same_bits(got[:, 16:], r.float()[:, 16:]), ec.lin_id(c)
            n += 1
    assert n >= 4


def test_guards_see_the_clamped_column_written():
    n = 0
    for c in ec.LIN_CASES:
        if c.want == 0 and c.n_out % 4 and c.kind == "grid":
            x, w, bias, r, bound = ec.lin_inputs_and_reference(c)
            got = torch.from_numpy(ec.emulate_linear(c, x, w, bias, 0, "clamp"))
            assert (got[-ec.GUARD:] != 13.0).any(), ec.lin_id(c)
            n += 1
    assert n >= 12


def test_bits_see_the_tap_order_transposed_and_the_pad_column_used():
    for kind in ("grid", "tap"):
        for c in ec.HEAD_CASES:
            if c.kind == kind and c.H > 1 and c.W > 1 and c.N == 1:
                x, w, bias, r, bound = ec.head_inputs_and_reference(c)
                assert not same_bits(ec.emulate_head(c, x, w, bias, "kwmajor")[0], r.half()), ec.head_id(c)
                if c.Cin == 7 and c.H > 2:
                    assert not same_bits(ec.emulate_head(c, x, w, bias, "pad63")[0], r.half()), ec.head_id(c)
    c = _first(ec.HEAD_CASES, lambda c: c.kind == "randn" and c.Cin == 7)
    x, w, bias, r, bound = ec.head_inputs_and_reference(c)
    for m in ("kwmajor", "pad63"):
        assert nc.error_ratios(ec.emulate_head(c, x, w, bias, m)[0], r, bound)[0] > 1.0, m
    n = 0
    for c in ec.TAIL_CASES:                              # conv_out: every tap launch of four holds an off-diagonal tap
        if c.kind == "tap" and c.Cout == 4 and c.S:
            x, gamma, beta, w, bias, r, bound, outside = ec.tail_inputs_and_reference(c)
            got = ec.emulate_tail(c, x, gamma, beta, w, bias, ec.tail_supplied(c, x).numpy(), c.S, c.rows, "kwmajor")
            assert ec.worst_ratio(got, r, bound) > 1.0, ec.tail_id(c)
            n += 1
    assert n >= 3


def test_summaries_see_the_tile_index_off_by_one_image():
    n = 0
    for c in ec.HEAD_CASES:
        if c.N > 1 and c.G and c.kind != "grid":
            x, w, bias, r, bound = ec.head_inputs_and_reference(c)
            y, summ = ec.emulate_head(c, x, w, bias, "image")
            dm, dq = ec.head_summary_errors(c, summ, ec.head_summary_reference(c, y))
            assert max(dm, dq) > 1.0, ec.head_id(c)
            n += 1
    assert n >= 10


def test_bound_sees_the_halo_padded_before_the_norm_and_the_ragged_part_miscounted(engine_lib):
    seen = {"prepad": 0, "ragged": 0}
    for c in ec.TAIL_CASES:
        x, gamma, beta, w, bias, r, bound, outside = ec.tail_inputs_and_reference(c)
        part, S, rows = tail_part(engine_lib, c, x)
        if c.kind == "tap":
            got = ec.emulate_tail(c, x, gamma, beta, w, bias, part, S, rows, "prepad")
            assert ec.worst_ratio(got, r, bound) > 1.0, ("prepad", ec.tail_id(c))
            assert (got[outside].view(torch.int16) != 0).any()
            seen["prepad"] += 1
        if (c.H * c.W) % rows and c.H * c.W - (S - 1) * rows <= rows // 2 and c.profile == "randn":
            got = ec.emulate_tail(c, x, gamma, beta, w, bias, part, S, rows, "ragged")
            assert ec.worst_ratio(got, r, bound) > 1.0, ("ragged", ec.tail_id(c))
            seen["ragged"] += 1
    assert seen["prepad"] >= 9 and seen["ragged"] >= 2, seen
