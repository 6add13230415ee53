"""Which attn_kernel<D, QT, KT, PRESC, NWV> launch_attention runs (attention_plan in csrc/attention.hip, through
sd_attention_plan), pinned on the CPU for the shapes the engine runs and at every threshold; that the GPU cases of
tests/test_attention_gpu.py reach every instantiation; and that the element-wise error bound those cases assert holds
for an emulation of the kernel's arithmetic."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest
import torch

import attn_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = 4


def plan(lib, B, heads, Tq, d, causal=0, presc=0, Tk=None):
    out = (C.c_int * 5)()
    rc = lib.sd_attention_plan(B, Tq, Tq if Tk is None else Tk, heads, d, causal, presc, out)
    return tuple(out) if rc == 0 else rc


# (B, heads, Tq, d, causal, prescaled) -> instantiation
ENGINE_SHAPES = [
    # SD1.5 at the benchmark configuration C2 (batch 8 = 4 images x 2 for guidance, 512 x 512): the UNet pre-scales q
    ((8, 8, 4096, 40, 0, 1), (40, 4, 64, 1, 8)),
    ((8, 8, 1024, 80, 0, 1), (80, 2, 64, 0, 8)),
    ((8, 8, 256, 160, 0, 1), (160, 1, 64, 0, 4)),
    ((8, 8, 64, 160, 0, 1), (160, 1, 64, 0, 4)),
    # one image with guidance: too few blocks for eight waves at the 32 x 32 level
    ((2, 8, 4096, 40, 0, 1), (40, 4, 64, 1, 4)),
    ((2, 8, 1024, 80, 0, 1), (80, 2, 64, 0, 4)),
    # SDXL: d = 64 at 10 and 20 heads, pre-scaled queries on the general kernel
    ((4, 10, 4096, 64, 0, 1), (64, 2, 64, 0, 4)),
    ((4, 20, 1024, 64, 0, 1), (64, 2, 64, 0, 4)),
    # VAE mid block: one head over 512 channels, not pre-scaled
    ((4, 1, 4096, 512, 0, 0), (512, 1, 64, 0, 4)),
    ((1, 1, 16384, 512, 0, 0), (512, 1, 64, 0, 4)),
    # CLIP ViT-L (12 heads) and OpenCLIP bigG (20 heads): causal, 77 tokens
    ((2, 12, 77, 64, 1, 0), (64, 2, 64, 0, 4)),
    ((2, 20, 77, 64, 1, 0), (64, 2, 64, 0, 4)),
    # test configurations
    ((2, 4, 64, 32, 0, 1), (32, 2, 64, 1, 4)),
    ((2, 4, 64, 32, 0, 0), (32, 2, 64, 0, 4)),
    ((1, 1, 192, 128, 0, 0), (128, 2, 64, 0, 4)),
    ((2, 8, 256, 40, 0, 0), (40, 4, 64, 0, 4)),
]


@pytest.mark.parametrize("shape,want", ENGINE_SHAPES)
def test_engine_shapes(engine_lib, shape, want):
    B, heads, Tq, d, causal, presc = shape
    assert plan(engine_lib, B, heads, Tq, d, causal, presc) == want
    assert plan(engine_lib, B, heads, Tq, d, causal, presc, Tk=77) == want      # the key count plays no part


def test_thresholds_just_below_and_at(engine_lib):
    p = lambda *a, **k: plan(engine_lib, *a, **k)
    # d = 40 pre-scaled: eight waves from cdiv(Tq, 512) * B * heads >= 512
    assert p(1, 511, 512, 40, presc=1) == (40, 4, 64, 1, 4)
    assert p(1, 512, 512, 40, presc=1) == (40, 4, 64, 1, 8)
    assert p(1, 256, 513, 40, presc=1) == (40, 4, 64, 1, 8)          # the ragged second block counts
    assert p(1, 255, 1024, 40, presc=1) == (40, 4, 64, 1, 4)
    assert p(8, 8, 4096, 40, presc=1) == (40, 4, 64, 1, 8)           # 8 * 64 = 512: exactly at it
    assert p(8, 8, 3584, 40, presc=1) == (40, 4, 64, 1, 4)           # 7 * 64
    assert p(64, 8, 4096, 40, presc=0) == (40, 4, 64, 0, 4)          # only pre-scaled queries have an eight-wave form
    # d = 80: eight waves from cdiv(Tq, 256) * B * heads >= 256, plain or pre-scaled
    for presc in (0, 1):
        assert p(1, 255, 256, 80, presc=presc) == (80, 2, 64, 0, 4)
        assert p(1, 256, 256, 80, presc=presc) == (80, 2, 64, 0, 8)
        assert p(1, 128, 257, 80, presc=presc) == (80, 2, 64, 0, 8)
        assert p(1, 127, 512, 80, presc=presc) == (80, 2, 64, 0, 4)
        assert p(8, 8, 1024, 80, presc=presc) == (80, 2, 64, 0, 8)   # 4 * 64 = 256
        assert p(8, 8, 768, 80, presc=presc) == (80, 2, 64, 0, 4)    # 3 * 64
    # d = 160: 128-query blocks from cdiv(Tq, 128) * B * heads >= 256, causal or not
    for causal, presc in itertools.product((0, 1), (0, 1)):
        assert p(1, 255, 128, 160, causal, presc) == (160, 1, 64, 0, 4)
        assert p(1, 256, 128, 160, causal, presc) == (160, 2, 64, 0, 4)
        assert p(1, 128, 129, 160, causal, presc) == (160, 2, 64, 0, 4)
        assert p(1, 127, 256, 160, causal, presc) == (160, 1, 64, 0, 4)


def test_causal_never_gets_eight_waves(engine_lib):
    for B, heads, Tq in [(1, 1, 77), (8, 8, 4096), (64, 32, 1024), (1024, 64, 8192)]:
        for presc in (0, 1):
            assert plan(engine_lib, B, heads, Tq, 40, 1, presc) == (40, 4, 64, presc, 4)
            assert plan(engine_lib, B, heads, Tq, 80, 1, presc) == (80, 2, 64, 0, 4)
            assert plan(engine_lib, B, heads, Tq, 64, 1, presc) == (64, 2, 64, 0, 4)


def test_unsupported_head_dim(engine_lib):
    for d in (0, 8, 16, 48, 96, 256, 1024, -40):
        assert plan(engine_lib, 2, 8, 256, d) == UNSUPPORTED
        assert b"unsupported head dim" in engine_lib.sd_last_error()
    assert engine_lib.sd_attention_plan(2, 256, 256, 8, 40, 0, 0, None) == 1


def test_sweep_reaches_exactly_the_listed_instantiations(engine_lib):
    """Whatever attention_plan answers on a grid that crosses every threshold is in ac.INSTANTIATIONS, and all of the
    list is reached: an instantiation added to the dispatch shows up here before it has a GPU case."""
    seen = set()
    for d in (32, 40, 64, 80, 128, 160, 512):
        for bh, Tq, causal, presc in itertools.product((1, 16, 255, 256, 511, 512, 4096), (1, 64, 129, 513, 4096),
                                                       (0, 1), (0, 1)):
            got = plan(engine_lib, 1, bh, Tq, d, causal, presc)
            assert got in ac.INSTANTIATIONS, (d, bh, Tq, causal, presc, got)
            seen.add(got)
    assert seen == set(ac.INSTANTIATIONS)
    assert len(set(ac.INSTANTIATIONS)) == len(ac.INSTANTIATIONS) == 12


def test_gpu_cases_cover_every_instantiation(engine_lib):
    """Each case of tests/test_attention_gpu.py runs the instantiation it names, and between them they run all."""
    for c in ac.GPU_CASES:
        assert plan(engine_lib, c.B, c.heads, c.Tq, c.d, c.causal, c.presc, Tk=c.Tk) == c.inst, ac.case_id(c)
    for group in ("edge", "constv"):
        assert {c.inst for c in ac.GPU_CASES if c.group == group} == set(ac.INSTANTIATIONS), group
    assert {c.inst for c in ac.GPU_CASES} == set(ac.INSTANTIATIONS)
    for inst in ac.INSTANTIATIONS:
        qb = ac.queries_per_block(inst)
        edges = {(c.Tq, c.Tk) for c in ac.GPU_CASES if c.group == "edge" and c.inst == inst}
        assert {(1, 1), (qb + 1, 65)} <= edges
        assert {tk for _, tk in edges} == {1, 16, 63, 64, 65, 128, 129}
        assert {tq for tq, _ in edges} == {1, qb - 1, qb, qb + 1}
    newly = {(40, 4, 64, 1, 8), (80, 2, 64, 0, 8), (160, 2, 64, 0, 4)}
    for group in ("threshold", "extreme"):
        assert newly <= {c.inst for c in ac.GPU_CASES if c.group == group}
    assert len({ac.case_id(c) for c in ac.GPU_CASES}) == len(ac.GPU_CASES)


def test_wave_switches_are_read_by_the_plan():
    """SD_ATTN_NWV / SD_ATTN_NWV80 are read once per process, by the plan as by the launch: a fresh interpreter."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_attention_plan as t\nfrom stablediffusion_amd import _lib\nlib = _lib.load()\n"
            "print(t.plan(lib, 8, 8, 4096, 40, 0, 1), t.plan(lib, 8, 8, 1024, 80, 0, 1))\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("SD_")}
    env.update(SD_ATTN_NWV="4", SD_ATTN_NWV80="4")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().splitlines()[-1] == "(40, 4, 64, 1, 4) (80, 2, 64, 0, 4)"


@pytest.mark.parametrize("group", ["threshold", "edge", "strided", "causal", "constv", "extreme"])
def test_emulated_arithmetic_stays_inside_the_elementwise_bound(group):
    """The bound test_attention_gpu.py asserts, proven here on its own inputs: probabilities truncated to fp16 (low 13
    mantissa bits of the fp32 value cleared), fp32 sums, the denominator from the truncated or from the exact
    probabilities, fp16 output -- against the float64 reference, for every case."""
    cases = [c for c in ac.GPU_CASES if c.group == group]
    assert cases
    for c in cases:
        q, k, v, O, A = ac.inputs_and_reference(c)
        bound = ac.elementwise_bound(O, A, c.Tk, v.abs().max().double())
        for packed in (True, False):
            out = ac.emulate(c, q, k, v, packed).double()
            assert torch.isfinite(out).all(), ac.case_id(c)
            excess = ((out - O).abs() - bound).max().item()
            assert excess <= 0, (ac.case_id(c), packed, excess)
            if c.Tk == 1:
                assert torch.equal(out.half(), v.expand(c.B, c.Tq, -1)), ac.case_id(c)
