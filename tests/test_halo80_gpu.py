"""conv3x3_halo_kernel<80> (the 80-column halo tile) at operator level, under sd_halo80_force(1): against the float64 CPU
reference and element-wise bound of tests/conv_cases.py (the bound the halo ids 10 and 15 are held to), with the guards
of tests/test_conv_gpu.py around every operand; bit for bit against forced variant 15; its GroupNorm summaries against
(mean, M2) of the stored output; and one tiny-UNet forward with the rule, the switch and the forced form."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_cases as cc
from conftest import rel_l2
from test_conv_gpu import P, check, run, stream
from test_ops_gpu import _conv_groupnorm_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K80 = 80                        # what sd_op_conv2d_ex reports as the kind that ran


def mk(N, H, W, Cin, Cout, ops="b", scales=(1.0, 1.0), gn=0, want=(K80, 1, 0), kind="randn", layouts=("dense",), force=None):
    return cc.Case("halo80", N, H, W, Cin, Cout, 3, 1, 0, -1, 0, 0, "b" in ops, "a" in ops, "r" in ops, float(scales[0]),
                   float(scales[1]), gn, force, tuple(want), kind, tuple(layouts))


CASES = [
    mk(1, 16, 16, 64, 80),                                          # one slab, one tile, all four borders in one patch
    mk(1, 16, 16, 64, 80, kind="grid"),
    mk(2, 16, 16, 128, 88, ops="bar"),                              # two slabs (halo buffers swap), ragged second column tile
    mk(2, 16, 16, 128, 88, ops="bar", kind="grid"),
    mk(1, 8, 32, 64, 160), mk(1, 16, 32, 64, 160),                  # width-32 patches, two per image
    mk(1, 4, 64, 64, 80), mk(2, 8, 64, 64, 88, ops="bar"),          # width-64 patches
    mk(1, 32, 32, 64, 80),                                          # patches with no border and with one
    mk(2, 16, 16, 64, 9 * 64, ops="", kind="tap"),                  # all nine taps as a pure copy, 8 column tiles
    mk(2, 8, 32, 64, 9 * 64, ops="", kind="tap"), mk(2, 4, 64, 64, 9 * 64, ops="", kind="tap"),
    mk(1, 16, 16, 192, 80, ops="bar", want=(K80, 2, 1)),            # split-K 2 over three slabs (2 + 1), reducer 1
    mk(1, 16, 16, 192, 80, ops="bar", want=(K80, 2, 1), kind="grid"),
    mk(1, 16, 16, 192, 80, ops="bar", gn=8, want=(K80, 2, 2)),      # ... and the summaries' reducer
    mk(2, 16, 16, 192, 9 * 192, ops="", want=(K80, 2, 1), kind="tap"),
]
EPILOGUE = [mk(2, 16, 16, 64, 88, ops=ops, scales=sc, kind="grid") for ops, sc in
            (("", (1, 1)), ("ba", (1, 1)), ("br", (1, 1)), ("bar", (2.0 ** -3, 2.0 ** 3)), ("bar", (2.0 ** 3, 2.0 ** -3)),
             ("b", (2.0 ** -3, 2.0 ** -3)), ("b", (2.0 ** 3, 2.0 ** 3)))]
STRIDED = [mk(2, 16, 16, 128, 88, ops="bar", layouts=("dense", "left", "right")),
           mk(1, 16, 16, 192, 80, ops="bar", want=(K80, 2, 1), layouts=("dense", "left", "right"))]


def ids(cs):
    return [cc.case_id(c) for c in cs]


@pytest.fixture
def forced80(engine_lib):
    engine_lib.sd_halo80_force(1)
    yield engine_lib
    engine_lib.sd_halo80_force(-1)


@pytest.mark.parametrize("case", CASES + EPILOGUE, ids=ids(CASES + EPILOGUE))
def test_halo80_against_float64(forced80, case):
    ins = cc.inputs_and_reference(case)
    out = run(forced80, case, ins[:5], "dense")
    check(case, out, ins[5], ins[6])


@pytest.mark.parametrize("case", STRIDED, ids=ids(STRIDED))
def test_halo80_strided_operands(forced80, case):
    """x a column slice, y and res the left / right columns of a wider buffer (ldres = ldy != Cout): bit-identical to the
    dense run, nothing outside the output written."""
    ins = cc.inputs_and_reference(case)
    dense = run(forced80, case, ins[:5], "dense")
    check(case, dense, ins[5], ins[6])
    for layout in case.layouts[1:]:
        out = run(forced80, case, ins[:5], layout)
        assert torch.equal(dense.view(torch.int16), out.view(torch.int16)), layout


@pytest.mark.parametrize("shape", [(2, 16, 16, 128, 160), (2, 8, 32, 128, 160), (2, 4, 64, 128, 160), (1, 32, 32, 64, 88)],
                         ids=lambda s: "x".join(map(str, s)))
def test_halo80_bit_equal_to_the_128_column_tile(engine_lib, shape):
    """The K order per output element is the same (slab, tap, two 32-deep MFMA steps), so an unsplit launch equals forced
    variant 15 bit for bit, on random operands with every epilogue term."""
    c80 = mk(*shape, ops="bar")
    c15 = mk(*shape, ops="bar", force=(15, 1), want=(15, 1, 0))
    ins = cc.make_inputs(c80)
    engine_lib.sd_halo80_force(1)
    try:
        a = run(engine_lib, c80, ins, "dense")
    finally:
        engine_lib.sd_halo80_force(-1)
    b = run(engine_lib, c15, ins, "dense")
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), int((a.view(torch.int16) != b.view(torch.int16)).sum())


@pytest.mark.parametrize("offset", [None, 50.0], ids=["randn", "offset50"])
@pytest.mark.parametrize("Cout", [320, 640])
def test_halo80_groupnorm_summaries(forced80, Cout, offset):
    """(mean, M2) per (image, 256-pixel patch, group) from the epilogue against float64 of the stored fp16 output, with
    the tolerances the project holds epilogue summaries to (tests/test_pout_fold_gpu.py); at an offset of 50 with a
    spread of 0.1 plain sums of squares would lose M2 entirely."""
    N, H, W, Cin, G = 2, 16, 16, 64, 32
    g = torch.Generator().manual_seed(Cout + (7 if offset else 0))
    x = torch.randn(N, H, W, Cin, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half()
    bias = torch.randn(Cout, generator=g) * 0.5
    if offset is not None:
        w = (0.1 * w.float()).half()
        bias = offset + 0.05 * torch.randn(Cout, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    y = torch.empty(N, H, W, Cout, dtype=torch.float16, device="cuda")
    floats = N * 64 * G * 2
    summ = torch.full((floats,), float("nan"), dtype=torch.float32, device="cuda")
    rows, ran = C.c_int(-1), (C.c_int * 4)()
    rc = forced80.sd_op_conv2d_gnstats(P(xd), P(wd), P(bd), None, P(y), N, H, W, Cin, Cout, 3, G, P(summ), floats,
                                       C.byref(rows), ran, stream())
    assert rc == 0, forced80.sd_last_error()
    torch.cuda.synchronize()
    assert tuple(ran) == (K80, K80, 1, 0) and rows.value == 256
    S = H * W // 256
    t = y.cpu().double().reshape(N, S, 256, G, Cout // G)
    mean = t.mean(dim=(2, 4))
    m2 = ((t - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    got = summ[:N * S * G * 2].cpu().reshape(N, S, G, 2)
    print("summaries Cout %d offset %s: max |mean err| %.2e, max |M2 err| / M2 %.2e" % (
        Cout, offset, (got[..., 0].double() - mean).abs().max().item(), ((got[..., 1].double() - m2).abs() / m2).max().item()))
    assert torch.allclose(got[..., 0], mean.float(), atol=2e-5, rtol=1e-4)
    assert torch.allclose(got[..., 1], m2.float(), atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("case", [(2, 16, 16, 64, 320, 3, 1, 0, True, 1), (2, 16, 16, 64, 640, 3, 1, 0, False, 1)],
                         ids=["320-res", "640"])
def test_halo80_conv_groupnorm_at_a_large_offset(forced80, case):
    """tests/test_ops_gpu.py::test_conv_groupnorm_statistics_at_a_large_offset's check and tolerance, with the summaries
    coming from the 80-column epilogue (a constant group's M2 exactly 0)."""
    _conv_groupnorm_case(forced80, case, 50.0)


_CHILD = r"""
import ctypes as C, importlib.util, json, os, sys
import numpy as np, torch
root, out, mode = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root)
from stablediffusion_amd import _lib
from stablediffusion_amd.models import HipUNet2DConditionModel
lib = _lib.load()
lib.sd_halo80_force(mode)
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(root, "tests", "golden", "make_golden.py"))
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)
ucfg, vcfg, uw, vw = mg.golden_weights()
d = np.load(os.path.join(root, "tests", "golden", "tiny_sd.npz"))
unet = HipUNet2DConditionModel(ucfg).load_state_dict(uw)
lib.sd_prof_enable(1)
y = unet(torch.from_numpy(d["unet_x"]).cuda(), torch.from_numpy(d["unet_t"]), torch.from_numpy(d["unet_ehs"]).cuda())[0]
ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
assert lib.sd_prof_collect(ents, 512, C.byref(n)) == 0
np.save(out, y.float().cpu().numpy())
print(json.dumps(sum(int(ents[i].launches) for i in range(n.value) if ents[i].kernel.decode().startswith("conv3x3_halo_kernel<80>"))))
"""


def test_tiny_unet_rule_switch_and_forced(engine_lib, tmp_path):
    """The golden tiny UNet in fresh processes: the rule, SD_NO_HALO80=1, and the 80-column form wherever the kernel
    takes the conv (through op_conv: its split-K workspace planned by the dry pass).  Each within the 1e-2 forward-level
    bar against the oracle's output; the mutual distances are reported.  Nothing of this model fills 256 CUs, so the rule
    moves no launch and equals the switch."""
    import numpy as np
    want = torch.from_numpy(np.asarray(np.load(os.path.join(ROOT, "tests", "golden", "tiny_sd.npz"))["unet_y"])).float()
    outs, launches = {}, {}
    for name, switch, mode in (("rule", None, -1), ("off", "1", -1), ("forced", None, 1)):
        env = {k: v for k, v in os.environ.items() if k != "SD_NO_HALO80"}
        if switch:
            env["SD_NO_HALO80"] = switch
        path = str(tmp_path / f"{name}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(mode)], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = torch.from_numpy(np.load(path))
        launches[name] = json.loads(r.stdout.strip().splitlines()[-1])
    msg = json.dumps({"launches<80>": launches, "rule_vs_oracle": rel_l2(outs["rule"], want),
                      "off_vs_oracle": rel_l2(outs["off"], want), "forced_vs_oracle": rel_l2(outs["forced"], want),
                      "rule_vs_off": rel_l2(outs["rule"], outs["off"]), "forced_vs_off": rel_l2(outs["forced"], outs["off"])})
    print(msg)
    assert all(torch.isfinite(o).all() for o in outs.values()), msg
    assert launches["rule"] == 0 and launches["off"] == 0 and launches["forced"] > 0, msg
    assert rel_l2(outs["rule"], want) < 1e-2 and rel_l2(outs["off"], want) < 1e-2 and rel_l2(outs["forced"], want) < 1e-2, msg
    assert rel_l2(outs["rule"], outs["off"]) < 1e-2 and rel_l2(outs["forced"], outs["off"]) < 1e-2, msg
