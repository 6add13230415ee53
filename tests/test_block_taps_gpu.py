"""Every UNet and VAE block alone, on the engine's own block inputs (sd_unet_tap / sd_vae_tap).

The whole-model tests compare the last tensor of ~500 launches with the oracle at relative L2 < 1e-2; a composition
mistake in one block (a dropped time embedding, a zeroed cross-attention, a wrong residual) moves that figure by
2e-3 .. 8e-3 and passes.  Here one forward per model case runs with the debug taps on, and every tapped block is
compared with the float64 block of the oracle evaluated on the block's OWN tapped input (tests/block_oracle.py), against
the error fp16 storage alone may cause: with e = tapped output - reference and y = yardstick - reference,

    rel_l2(e) <= m rel_l2(y)   and   max|e| <= m max|y|,    m = block_oracle.MARGIN[kind]   (profiles/block_taps.txt)

plus: the output is finite, and the columns of an output buffer outside the block's view are bit for bit what they
were before the block ran.  test_block_taps.py shows on the CPU that each seeded mistake exceeds this tolerance 3x.

Cases.  UNet a, b, c are the shapes of test_models_gpu.py; d is a two-level SD1.5 front end with B = 2 at 64 x 64 and
e the same at the benchmark's B = 8: the only places where ffn_fused_kernel, the weight-stationary K = 320 GEMMs and
the one-launch conv_in (d and e), the persistent GEGLU projection and the one-launch conv_out (e only: the tile table
is tuned for M = 32768 rows) run inside a model, asserted from the profile (HOT_KERNELS).  VAE: decode at
2 x 8 x 12, 1 x 65 x 65 and 2 x 32 x 32 (conv3x3_small_cout_kernel is the tail there), encode at 2 x 3 x 64 x 48 with
range shift 0 and 8.  References are float64 on the CPU for the small cases and float32 on the device for cases d, e
and the two large decodes; test_device_references_are_the_cpu_references bounds the difference by 1/20 of the yardstick.

SD_BLOCK_TAPS_REPORT=<file>: every block test appends its measured figures to the file (how profiles/block_taps.txt
and the margins were made); the assertions are the same.

Blind spots, not claimed here: on these inputs a GroupNorm eps of 1e-6 / 1e-5 / 1e-4 in place of the engine's
1e-5 / 1e-6, a LayerNorm eps of 1e-6 in place of 1e-5, and tanh-GELU in place of erf-GELU change a block's output by
2e-7 .. 9e-5 relative L2, below the 2e-4 fp16 floor: no fp16 comparison at these amplitudes sees them.  Those arguments
are covered at operator level by test_norm_gpu.py, test_ln_gpu.py and conv_cases.py.
"""
import ctypes as C
import os

import pytest
import torch

import block_oracle as bo
from stablediffusion_amd import _lib, config
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu
REPORT = os.environ.get("SD_BLOCK_TAPS_REPORT")

# where the references of a case are evaluated
DEVICE_REFS = {"d": ("cuda", torch.float32), "e": ("cuda", torch.float32), "dec_1x65x65": ("cuda", torch.float32), "dec_2x32x32": ("cuda", torch.float32)}
VAE_CASES = {
    "dec_2x8x12": ("decoder", 2, 8, 12, 0),
    "dec_1x65x65": ("decoder", 1, 65, 65, 0),
    "dec_2x32x32": ("decoder", 2, 32, 32, 0),       # 131072 output pixels: crosses kSmallCoutMinPixels
    "enc_2x64x48": ("encoder", 2, 64, 48, 0),
    "enc_2x64x48_shift8": ("encoder", 2, 64, 48, 8),
}
# Kernels that only cases d and e run inside a model, under the names sd_prof_collect reports, pinned so that the cases
# cannot silently stop covering them.  Measured, against what the cases were set up for:
#   - conv_tail_kernel needs the GroupNorm summaries of the last proj_out launch, and the persistent GEGLU projection
#     (geglu_persist_kernel) its M = 8192 rows at C = 640: the tile table has them at the benchmark's batch (case e,
#     M = 32768 rows at C = 320) and not at case d's B = 2, where the tail runs as GroupNorm kernel + small-Cout convolution.
#   - The GroupNorm-fused form of conv3x3_halo_kernel runs in no forward: op_gn_conv keeps it off unless SD_GN_FUSE=1
#     (measured slower, profiles/r03_gn_fused_conv.txt); sd_op_groupnorm_conv2d's operator test is its only cover.
HOT_KERNELS = {
    "d": ("ffn_fused_kernel", "wsgemm_kernel<160,false,...>", "conv_head_kernel", "conv3x3_halo_kernel<160>/up2x2"),
    "e": ("ffn_fused_kernel", "wsgemm_kernel<160,false,...>", "conv_head_kernel", "conv3x3_halo_kernel<160>/up2x2",
          "conv_tail_kernel", "geglu_persist_kernel"),
}


def _profile(lib, run):
    lib.sd_prof_enable(1)
    try:
        out = run()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return out, {e.kernel.decode(): e.launches for e in ents[: n.value]}


def _refs_on(case):
    return DEVICE_REFS.get(case, ("cpu", torch.float64))


# ------------------------------------------------------------------------------------------ one forward per case
_runs = {}


def _unet_run(lib, case):
    if case in _runs:
        return _runs[case]
    cfg, sd, x, t, ehs, added = bo.unet_inputs(case)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    kw = {} if added is None else {"added_cond_kwargs": {k: v.cuda() for k, v in added.items()}}
    args = (x.cuda(), t.cuda(), ehs.cuda())
    plain = net(*args, **kw)[0].clone()                          # (also plans the arena: the profiles below are steady state)
    off, prof_off = _profile(lib, lambda: net(*args, **kw)[0].clone())
    (on, taps), prof_on = _profile(lib, lambda: net.forward_tapped(*args, **kw))
    again = net(*args, **kw)[0]
    dev, dt = _refs_on(case)
    with torch.no_grad():
        model = bo.unet_model(cfg, sd, t, ehs, added, x.shape[2], x.shape[3], dt, dev)
    _runs[case] = dict(net=net, args=args, kw=kw, plain=plain, off=off, on=on.clone(), again=again, prof_off=prof_off,
                       prof_on=prof_on, taps=taps, model=model)
    return _runs[case]


def _vae_run(lib, case):
    if case in _runs:
        return _runs[case]
    which, B, h, w, shift = VAE_CASES[case]
    cfg, sd, x = bo.vae_inputs(which, B, h, w)
    net = HipAutoencoderKL(cfg).load_state_dict(sd)
    _lib.check(lib.sd_vae_encode_range_shift(net._h, shift), "sd_vae_encode_range_shift")
    fn = (lambda: net.decode(x.cuda())[0]) if which == "decoder" else (lambda: net.encode_moments(x.cuda()))
    tapped = net.decode_tapped if which == "decoder" else net.encode_tapped
    plain = fn().clone()
    off, prof_off = _profile(lib, lambda: fn().clone())
    (on, taps), prof_on = _profile(lib, lambda: tapped(x.cuda()))
    dev, dt = _refs_on(case)
    _runs[case] = dict(net=net, plain=plain, off=off, on=on.clone(), again=fn(), prof_off=prof_off, prof_on=prof_on,
                       taps=bo.unscale(taps, f"{which}.conv_in", f"{which}.tail"), raw=taps, shift=shift,
                       model=bo.vae_model(cfg, sd, which, B, dt, dev))
    return _runs[case]


def _run(lib, case):
    return _unet_run(lib, case) if case in bo.UNET_CASES else _vae_run(lib, case)


def _block_params():
    out = []
    for case, c in bo.UNET_CASES.items():
        out += [(case, b.name) for b in bo.unet_blocks(c["cfg"](), c["B"], c["H"], c["W"])]
    for case, (which, *_rest) in VAE_CASES.items():
        out += [(case, b.name) for b in bo.vae_blocks(config.tiny_vae(), which)]
    return out


# ------------------------------------------------------------------------------------------ the taps' own contract
@pytest.mark.parametrize("case", list(bo.UNET_CASES) + list(VAE_CASES))
def test_taps_change_nothing(engine_lib, case):
    """Taps on: the forward's output is bit for bit the one with taps off, and its profile lists the same kernels and
    launch counts (the copies are no kernels).  Taps off again: the same bits, and no record is left."""
    r = _run(engine_lib, case)
    assert torch.equal(r["off"], r["plain"]) and torch.equal(r["on"], r["plain"]) and torch.equal(r["again"], r["plain"])
    assert r["prof_on"] == r["prof_off"] and len(r["prof_off"]) > 3
    count = engine_lib.sd_unet_tap_count if case in bo.UNET_CASES else engine_lib.sd_vae_tap_count
    assert count(r["net"]._h) == 0
    names = [b.name for b in r["model"].blocks]
    assert [n for n in r["taps"] if n != "emb"] == names          # every block, in execution order, nothing else
    for n in names:
        assert set(("in", "out")) <= set(r["taps"][n]), n


@pytest.mark.parametrize("case", list(HOT_KERNELS))
def test_hot_path_kernels_run_inside_the_model(engine_lib, case):
    prof = _unet_run(engine_lib, case)["prof_off"]
    print(case, sorted(prof.items()))
    for k in HOT_KERNELS[case]:
        assert prof.get(k, 0) > 0, (k, sorted(prof))


def test_refused_modes(engine_lib):
    """With taps on, graph replay, forward_cfg where it would share, forward_pag, forward_concat and the DeepCache
    store / reuse modes return SD_ERR_UNSUPPORTED and launch nothing; the unshared forward_cfg is the plain forward and taps."""
    lib = engine_lib
    r = _unet_run(lib, "a")
    net, (x, t, ehs) = r["net"], r["args"]
    ehs2 = torch.cat([ehs, ehs])
    out = torch.empty(2 * x.shape[0], 4, 16, 16, device="cuda", dtype=torch.float16)

    def concat():
        p = lambda v: C.c_void_p(v.data_ptr())
        rc = lib.sd_unet_forward_concat(net._h, p(x), x.shape[0], 1.0, p(x), 4, x.shape[0], 0, p(t), p(ehs2), ehs2.shape[1],
                                        None, None, p(out), 2 * x.shape[0], 16, 16, None)
        _lib.check(rc, "sd_unet_forward_concat")

    _lib.check(lib.sd_unet_tap(net._h, 1), "sd_unet_tap")
    try:
        lib.sd_prof_enable(1)
        calls = {
            "cfg_share": lambda: net.forward_cfg(x, t, ehs2, share=True),
            "pag": lambda: net.forward_pag(x, t, ehs2),
            "concat": concat,
        }
        for name, call in calls.items():
            with pytest.raises(_lib.EngineError, match="error 4: .*debug taps are on"):
                call()
        net.use_graph(True)
        try:
            with pytest.raises(_lib.EngineError, match="error 4: .*debug taps are on"):
                net(x, t, ehs)
            with pytest.raises(_lib.EngineError, match="error 4: .*debug taps are on"):
                net.forward_cfg(x, t, ehs2, share=False)
        finally:
            net.use_graph(False)
        net.enable_deepcache(3, 1)
        try:
            for mode in (1, 2):
                net.deep_cache_mode(mode)
                with pytest.raises(_lib.EngineError, match="error 4: .*debug taps are on"):
                    net(x, t, ehs)
        finally:
            net.disable_deepcache()
        torch.cuda.synchronize()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
        assert n.value == 0 and lib.sd_unet_tap_count(net._h) == 0      # nothing launched, nothing recorded
        lib.sd_prof_enable(0)
        # not shared, forward_cfg is the plain forward on the duplicated latents: it runs and records
        got = net.forward_cfg(x, t, ehs2, share=False)[0]
        assert lib.sd_unet_tap_count(net._h) > 0
    finally:
        lib.sd_prof_enable(0)
        _lib.check(lib.sd_unet_tap(net._h, 0), "sd_unet_tap")
    assert torch.equal(got, net.forward_cfg(x, t, ehs2, share=False)[0])


# ------------------------------------------------------------------------------------------ the blocks
@pytest.mark.parametrize("case", list(bo.UNET_CASES))
def test_time_embedding(engine_lib, case):
    """The tapped fp32 embedding (the device keeps silu(emb)) against the oracle's, separately from the blocks."""
    r = _unet_run(engine_lib, case)
    got = r["taps"]["emb"]["out"]
    ref = torch.nn.functional.silu(r["model"].emb.double().cpu())
    assert got.dtype == torch.float32 and got.shape == ref.shape
    e = bo.rel_l2(got, ref)
    print(f"emb {case}: rel_l2 {e:.2e}")
    assert e <= bo.EMB_TOL


@pytest.mark.parametrize("case,name", _block_params())
def test_block(engine_lib, case, name):
    r = _run(engine_lib, case)
    m, rec = r["model"], r["taps"][name]
    b = m.block(name)
    x_in, x_out = rec["in"], rec["out"]
    assert torch.isfinite(x_out.float()).all()
    if "out_rows" in rec:
        # the view is narrower than its row: the other columns are what they were before the block ran
        pre, post, c0, Cv = rec["pre_rows"], rec["out_rows"], rec["out_c0"], x_out.shape[1]
        assert pre.shape == post.shape and c0 + Cv <= post.shape[-1] and Cv < post.shape[-1]
        keep = torch.ones(post.shape[-1], dtype=torch.bool)
        keep[c0:c0 + Cv] = False
        assert torch.equal(pre[..., keep].view(torch.int16), post[..., keep].view(torch.int16))
    with torch.no_grad():
        e_l2, y_l2, e_max, y_max = bo.ratios(m, b, x_in, x_out)
    mg = bo.MARGIN[b.kind]
    line = (f"{case:20s} {name:36s} {b.kind:14s} e {e_l2:.3e} y {y_l2:.3e} ratio {e_l2 / y_l2:6.2f}   "
            f"max e {e_max:.3e} y {y_max:.3e} ratio {e_max / y_max:6.2f}")
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")
    assert e_l2 <= mg * y_l2, line
    assert e_max <= mg * y_max, line


def test_encode_shift_scale_is_recorded(engine_lib):
    r0, r8 = _vae_run(engine_lib, "enc_2x64x48"), _vae_run(engine_lib, "enc_2x64x48_shift8")
    assert {v["scale"] for v in r0["raw"].values()} == {1.0}
    assert {v["scale"] for v in r8["raw"].values()} == {2.0 ** -8}
    a, b = r0["raw"]["encoder.mid_block.resnets.0"]["out"], r8["raw"]["encoder.mid_block.resnets.0"]["out"]
    assert 100 < (a.float().norm() / b.float().norm()).item() < 400          # the stored stream really is 2^-8 times smaller


# ------------------------------------------------------------------------------------------ the device references
def test_device_references_are_the_cpu_references(engine_lib):
    """Cases d, e and the large decodes take their block references in float32 on the device.  On case a those differ
    from the float64 CPU references by less than 1/20 of the yardstick, in both metrics, on every block.  The float32
    yardstick cannot be held to that element by element -- a value a few 1e-7 from an fp16 rounding boundary rounds the
    other way -- so its two FIGURES, which are what the tolerance is made of, are held to the float64 ones: relative L2
    within 10 %, max-abs (one element decides it) within 25 %, both a small part of the factor of two between the worst
    measured ratio and the margin."""
    r = _unet_run(engine_lib, "a")
    cfg, sd, x, t, ehs, added = bo.unet_inputs("a")
    with torch.no_grad():
        dev = bo.unet_model(cfg, sd, t, ehs, added, x.shape[2], x.shape[3], torch.float32, "cuda")
        for b in r["model"].blocks:
            x_in = r["taps"][b.name]["in"]
            ref, yard = bo.reference(r["model"], b, x_in), bo.yardstick(r["model"], b, x_in)
            ref32, yard32 = bo.reference(dev, b, x_in).cpu(), bo.yardstick(dev, b, x_in).cpu()
            y_l2, y_max = bo.rel_l2(yard, ref), bo.max_abs(yard, ref)
            d_l2, d_max = bo.rel_l2(ref32, ref), bo.max_abs(ref32, ref)
            y32_l2, y32_max = bo.rel_l2(yard32, ref32), bo.max_abs(yard32, ref32)
            print(f"{b.name:34s} ref32-ref64 {d_l2 / y_l2:.4f} {d_max / y_max:.4f} of the yardstick; "
                  f"yardstick32 / yardstick64 {y32_l2 / y_l2:.4f} {y32_max / y_max:.4f}")
            assert d_l2 <= y_l2 / 20 and d_max <= y_max / 20, b.name
            assert abs(y32_l2 / y_l2 - 1) <= 0.1 and abs(y32_max / y_max - 1) <= 0.25, b.name


@pytest.mark.parametrize("case", ["d", "e"])
def test_defects_exceed_the_tolerance_at_the_real_shape(engine_lib, case):
    """test_block_taps.py's separation at the 64 x 64 cases' real shape, on the engine's tapped inputs (float32 on the
    device)."""
    r = _unet_run(engine_lib, case)
    m = r["model"]
    low = []
    with torch.no_grad():
        for b in m.blocks:
            x_in = r["taps"][b.name]["in"]
            ref, yard = bo.reference(m, b, x_in), bo.yardstick(m, b, x_in)
            for kind in b.defects:
                bad = bo.defect(m, b, x_in, kind)
                mg = bo.MARGIN[b.kind]
                s = max(bo.rel_l2(bad, ref) / (mg * bo.rel_l2(yard, ref)), bo.max_abs(bad, ref) / (mg * bo.max_abs(yard, ref)))
                print(f"{case} {b.name:34s} {kind:20s} {s:10.1f}")
                if s < bo.SEPARATION:
                    low.append((b.name, kind, round(s, 2)))
    assert not low, low
