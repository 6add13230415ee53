"""InstructPix2Pix on the GPU: the dual-guidance step entries against the float64 formula, sd_unet_forward_concat against
sd_unet_forward_ex on the torch-built sample (bit for bit where it falls back, within the project's 1e-2 of the fp32
oracle where conv_head2_kernel runs), the pipeline's device loops against its host loops, and the refusals."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import p2p_oracle  # noqa: E402
import pag_oracle  # noqa: E402
from oracle import unet_ref  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from test_deepcache_gpu import _fails, _launches  # noqa: E402
from test_pag_gpu import COEF, GUARD, P, _guarded, _ulp16, stream  # noqa: E402
from test_pix2pix import call_step, edit_cfg, invalid_step_calls  # noqa: E402
from test_sched_step_gpu import LOOP_TOL  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, pix2pix, weights  # noqa: E402
from stablediffusion_amd.models import (HipAutoencoderKL, HipControlNetModel, HipIPAdapter,  # noqa: E402
                                        HipUNet2DConditionModel)
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402
from stablediffusion_amd.schedulers import DDIMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-2


# ------------------------------------------------------------------------------------------------ the device step
def _bounds(mo, x, hist, g_t, g_i, c):
    """float64 references and per-element bounds, test_pag_gpu._bounds' reasoning for this formula: one fp16 ulp of e
    plus the fp32 evaluation of the two fmas (each within 2^-24 of its result, so within 2^-23 of the sum of the terms'
    magnitudes); that bound goes through the update's coefficients, the latents add one fp16 ulp of their own and the
    fp32 evaluation of the update (2^-22 of the terms' magnitudes), the fp32 history only the latter."""
    t, i, u = mo.double().reshape(3, -1)
    e = p2p_oracle.combine(mo, g_t, g_i).reshape(-1)
    mag = u.abs() + (g_t * (t - i)).abs() + (g_i * (i - u)).abs()
    tol_e = _ulp16(e) + 2.0 ** -23 * mag
    cx, ce, ch, hx, he = c
    out, h_new = pag_oracle.linear_step(e, x, hist, cx, ce, ch, hx, he)
    xd = x.double().reshape(-1)
    mag_out = (cx * xd).abs() + (ce * e).abs() + (0 if hist is None else (ch * hist.double().reshape(-1)).abs())
    tol_out = abs(ce) * tol_e + _ulp16(out) + 2.0 ** -22 * mag_out
    tol_h = abs(he) * tol_e + 2.0 ** -22 * ((hx * xd).abs() + (he * e).abs())
    return e, tol_e, out, tol_out, h_new, tol_h


@pytest.mark.parametrize("with_hist", [False, True], ids=["nohist", "hist"])
@pytest.mark.parametrize("n,shift", [(8, 0), (8, 1), (4096 + 8, 0), (37, 0)])
def test_ip2p_step_entries(engine_lib, n, shift, with_hist):
    """sd_ip2p_linear_step and sd_ip2p_combine against the float64 formula for (g_t, g_i) in {7.5, 1} x {1.5, 0, 2.5};
    n = 37 and the base one element off the 16-byte alignment take the scalar kernel.  The guards around every buffer
    and the model output stay untouched; with the image row equal to the uncond row the step is bit for bit
    sd_cfg_linear_step on [uncond ; text], whatever g_i."""
    gen = torch.Generator().manual_seed(n * 10 + 3)
    mo = torch.randn(3 * n, generator=gen).half()
    x = (torch.randn(n, generator=gen) * 2).half()
    hist = torch.randn(n, generator=gen) if with_hist else None
    for g_t in (7.5, 1.0):
        for g_i in (1.5, 0.0, 2.5):
            e, tol_e, out, tol_out, h_new, tol_h = _bounds(mo, x, hist, g_t, g_i, COEF)
            mo_buf, mo_v = _guarded(mo, 3.0, shift)
            x_buf, x_v = _guarded(x, 5.0, shift)
            e_buf, e_v = _guarded(torch.zeros(n).half(), 7.0, shift)
            h_buf, h_v = _guarded(hist if with_hist else torch.zeros(n), 9.0, shift)
            assert engine_lib.sd_ip2p_combine(P(mo_v), P(e_v), n, g_t, g_i, stream()) == 0, engine_lib.sd_last_error()
            assert engine_lib.sd_ip2p_linear_step(P(mo_v), P(x_v), P(h_v) if with_hist else None, n, g_t, g_i, *COEF,
                                                  stream()) == 0, engine_lib.sd_last_error()
            torch.cuda.synchronize()
            got_e, got_x = e_v.cpu().double(), x_v.cpu().double()
            assert torch.isfinite(got_e).all() and torch.isfinite(got_x).all()
            worst_e = ((got_e - e).abs() / tol_e).max().item()
            worst_x = ((got_x - out).abs() / tol_out).max().item()
            assert worst_e <= 1.0, (n, shift, g_t, g_i, worst_e)
            assert worst_x <= 1.0, (n, shift, g_t, g_i, worst_x)
            if with_hist:
                worst_h = ((h_v.cpu().double() - h_new).abs() / tol_h).max().item()
                assert worst_h <= 1.0, (n, shift, g_t, g_i, worst_h)
            else:
                assert (h_v == 0).all()
            for buf, fill in ((mo_buf, 3.0), (x_buf, 5.0), (e_buf, 7.0)):
                assert (buf[:GUARD + shift] == fill).all() and (buf[-GUARD:] == fill).all()
            assert (h_buf[:GUARD + shift] == 9.0).all() and (h_buf[-GUARD:] == 9.0).all()
            assert torch.equal(mo_v.cpu(), mo)
            # i == u: [t ; u ; u] against sd_cfg_linear_step on [u ; t]
            t_row, u_row = mo[:n], mo[2 * n:]
            same_buf, same_v = _guarded(torch.cat([t_row, u_row, u_row]), 3.0, shift)
            cfg_buf, cfg_v = _guarded(torch.cat([u_row, t_row]), 3.0, shift)
            xa_buf, xa = _guarded(x, 5.0, shift)
            xb_buf, xb = _guarded(x, 5.0, shift)
            ha_buf, ha = _guarded(hist if with_hist else torch.zeros(n), 9.0, shift)
            hb_buf, hb = _guarded(hist if with_hist else torch.zeros(n), 9.0, shift)
            assert engine_lib.sd_ip2p_linear_step(P(same_v), P(xa), P(ha) if with_hist else None, n, g_t, g_i, *COEF,
                                                  stream()) == 0
            assert engine_lib.sd_cfg_linear_step(P(cfg_v), P(xb), P(hb) if with_hist else None, n, g_t, *COEF, stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(xa.view(torch.int16), xb.view(torch.int16)), (n, shift, g_t, g_i)
            assert torch.equal(ha.view(torch.int32), hb.view(torch.int32))


@pytest.mark.parametrize("n", [8, 5])
def test_ip2p_step_keeps_the_sign_of_zero_at_i_equal_u(engine_lib, n):
    """u = t = -0 under a negative g_t: sd_cfg_linear_step's eps is -0, and an outer fma that added g_i * (+0) would make
    it +0.  With c_x = 0 and c_eps = 1 the latents ARE eps, so its sign bit shows."""
    neg0 = torch.full((n,), -0.0).half()
    coef = (0.0, 1.0, 0.0, 0.0, 0.0)
    for zeros in (neg0, torch.zeros(n).half()):
        xa, xb = torch.ones(n).half().cuda(), torch.ones(n).half().cuda()
        e = torch.ones(n).half().cuda()
        three, two = torch.cat([zeros] * 3).cuda(), torch.cat([zeros] * 2).cuda()
        assert engine_lib.sd_ip2p_linear_step(P(three), P(xa), None, n, -2.0, 1.5, *coef, stream()) == 0
        assert engine_lib.sd_ip2p_combine(P(three), P(e), n, -2.0, 1.5, stream()) == 0
        assert engine_lib.sd_cfg_linear_step(P(two), P(xb), None, n, -2.0, *coef, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(xa.view(torch.int16), xb.view(torch.int16))
        assert torch.equal(e.view(torch.int16), zeros.cuda().view(torch.int16))      # -0 stays -0, +0 stays +0


def test_ip2p_step_invalid_arguments_launch_nothing(engine_lib):
    mo = torch.randn(24).half().cuda()
    lat = torch.randn(8).half().cuda()
    mo0, lat0 = mo.clone(), lat.clone()
    for label, entry, args in invalid_step_calls():
        assert call_step(engine_lib, entry, args, (mo.data_ptr(), lat.data_ptr()), stream()) == 1, label
    torch.cuda.synchronize()
    assert torch.equal(mo, mo0) and torch.equal(lat, lat0)
    assert engine_lib.sd_ip2p_linear_step(P(mo), P(lat), None, 8, 7.5, 1.5, *COEF, stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(lat, lat0)


# ------------------------------------------------------------------------------------------------ the forward
def _state_dict(cfg, seed):
    return {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=seed, perturb=0.1).items()}


def wide_cfg():
    """Width-reduced, with the first block 320 wide: the shape conv_head2_kernel takes (8 heads of 40 there)."""
    return config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=8, block_out_channels=(320, 128, 256, 256),
                                    attention_head_dim=(8, 4, 8, 8)))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, cfg, seed in (("tiny", edit_cfg(), 21), ("wide", wide_cfg(), 22)):
        sd = _state_dict(cfg, seed)
        out[name] = (cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd))
    return out


def _inputs(cfg, B_lat, groups, H=16, W=16, seed=None, same_text=False):
    g = torch.Generator().manual_seed(B_lat * 100 + groups if seed is None else seed)
    lat = (torch.randn(B_lat, 4, H, W, generator=g) * 3).half()
    img = torch.randn(B_lat, 4, H, W, generator=g).half()
    ehs = torch.randn(groups * B_lat, 77, cfg.cross_attention_dim, generator=g).half()
    if same_text:
        ehs = ehs[:B_lat].repeat(groups, 1, 1)
    return lat, img, ehs


def _sample(lat, img, groups, scale):
    """The 8-channel sample, built with torch as a caller of the plain forward would."""
    x = torch.cat([(lat.float() * scale).half()] * groups)
    im = pix2pix.image_rows(img) if groups == 3 else img
    return torch.cat([x, im], dim=1)


SCALE = torch.tensor(1.0 / (14.6 ** 2 + 1.0) ** 0.5, dtype=torch.float32).item()


@pytest.mark.parametrize("groups", [3, 1])
@pytest.mark.parametrize("B_lat", [1, 2])
def test_fallback_is_bitwise_the_forward_on_the_materialised_sample(engine_lib, nets, B_lat, groups):
    """tiny_unet with in_channels = 8: the first block is 64 wide, so the engine builds the sample itself and runs the
    general conv_in -- bit for bit the plain forward on the torch-built sample, per-latent timesteps repeated per group."""
    cfg, sd, net = nets["tiny"]
    lat, img, ehs = _inputs(cfg, B_lat, groups)
    t = torch.tensor([981.0, 301.0][:B_lat])
    zero_from = 2 * B_lat if groups == 3 else B_lat
    for scale in (1.0, SCALE):
        got = net.forward_concat(lat.cuda(), t.cuda(), ehs.cuda(), img.cuda(), zero_from=zero_from, in_scale=scale)[0]
        want = net(_sample(lat, img, groups, scale).cuda(), t.repeat(groups).cuda(), ehs.cuda())[0]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B_lat, groups, scale)
    names = _launches(engine_lib, lambda: net.forward_concat(lat.cuda(), t.cuda(), ehs.cuda(), img.cuda(), zero_from=zero_from))
    assert names.get("concat_sample_kernel") == 1 and names.get("im2col_nchw3x3_kernel") == 1 and "conv_head2_kernel" not in names
    # a scalar timestep and a plain call with the 8-channel sample keep working
    a = net.forward_concat(lat.cuda(), 501.0, ehs.cuda(), img.cuda(), zero_from=zero_from)[0]
    b = net(_sample(lat, img, groups, 1.0).cuda(), torch.tensor(501.0), ehs.cuda())[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize("groups", [3, 1])
@pytest.mark.parametrize("B_lat", [1, 2])
def test_two_source_conv_in_runs_and_matches_the_oracle(engine_lib, nets, B_lat, groups):
    """First block 320 wide at 16 x 16: conv_head2_kernel reads both sources, nothing is materialised and no im2col
    runs.  Against oracle/unet_ref.py on the concatenated sample (fp32) within the project's 1e-2 relative L2, and
    against the engine's own plain forward on that sample.  All groups get the same embeddings here: the text and the
    image group then read the same (latents, image latents) pair and come out bit-identical, and the third differs from
    them through its zero image latents alone."""
    cfg, sd, net = nets["wide"]
    lat, img, ehs = _inputs(cfg, B_lat, groups, same_text=True)
    zero_from = 2 * B_lat if groups == 3 else B_lat
    run = lambda: net.forward_concat(lat.cuda(), 501.0, ehs.cuda(), img.cuda(), zero_from=zero_from, in_scale=SCALE)[0]
    names = _launches(engine_lib, run)
    assert names.get("conv_head2_kernel") == 1, names
    assert not any(k.startswith("im2col") or k.startswith("concat_sample") for k in names), names
    got = run()
    sample = _sample(lat, img, groups, SCALE)
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, sd, sample.float(), torch.tensor(501.0), ehs.float())
    e = rel_l2(got, ref)
    plain = net(sample.cuda(), torch.tensor(501.0), ehs.cuda())[0]
    print(f"forward_concat wide B_lat={B_lat} groups={groups}: rel-L2 vs oracle {e:.2e}, vs the plain forward "
          f"{rel_l2(got, plain):.2e}")
    assert torch.isfinite(got.float()).all() and e < TOL
    assert rel_l2(got, plain) < 1e-3                     # (the same network through the other conv_in)
    if groups == 3:
        assert torch.equal(got[:B_lat].view(torch.int16), got[B_lat:2 * B_lat].view(torch.int16))
        assert rel_l2(got[2 * B_lat:], got[:B_lat]) > 10 * 1e-3          # the zero image latents are live
    assert torch.equal(run(), got)


def test_refusals_launch_nothing_and_leave_the_handle_usable(engine_lib, nets):
    cfg, sd, net = nets["tiny"]
    lat, img, ehs = _inputs(cfg, 2, 3, seed=51)
    ld, im, ed = lat.cuda(), img.cuda(), ehs.cuda()
    run = lambda: net.forward_concat(ld, 501.0, ed, im, zero_from=4)[0]
    want = run()
    # ---- SD_ERR_UNSUPPORTED ----
    # (a ControlNet attaches to 4-channel UNets only: the refusal is asked of one, at the C entry)
    pcfg = config.tiny_unet()
    pnet = HipUNet2DConditionModel(pcfg).load_state_dict(_state_dict(pcfg, 11))
    ccfg = controlnet.encoder_config(pcfg)
    cn = HipControlNetModel(pnet, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=6))
    out = torch.full((6, 4, 16, 16), 9.0, dtype=torch.float16, device="cuda")
    t = torch.full((2,), 501.0, device="cuda")

    def entry(latents=ld, B_lat=2, extra=im, extra_channels=4, extra_rows=2, zero_from=4, ts=t, ehs_=ed, B=6, handle=None):
        p = lambda v: None if v is None else P(v)
        return engine_lib.sd_unet_forward_concat(handle or net._h, p(latents), B_lat, 1.0, p(extra), extra_channels,
                                                 extra_rows, zero_from, p(ts), p(ehs_), 77, None, None, P(out), B, 16, 16,
                                                 stream())

    def refused(code, match, **kw):
        def call():
            _lib.check(entry(**kw), "sd_unet_forward_concat")
        _fails(engine_lib, call, code, match)

    pnet.attach_controlnet(cn)
    try:
        refused(4, "ControlNet", handle=pnet._h)
    finally:
        pnet.attach_controlnet(None)
    refused(1, "in_channels", handle=pnet._h)
    ad = HipIPAdapter(net, 128, 4).load_state_dict(synth_ip_state_dict(cfg, 128, 4, seed=3))
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.7)
    try:
        _fails(engine_lib, run, 4, "IP-Adapter")
        net.set_ip_adapter_scale(0.0)
        assert torch.equal(run(), want)                  # at scale 0 the text attention runs alone
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    net.enable_deepcache(2, 1)
    try:
        for mode in (net.DC_STORE, net.DC_REUSE):
            net.deep_cache_mode(mode)
            _fails(engine_lib, run, 4, "DeepCache")
        net.deep_cache_mode(net.DC_PLAIN)
        assert torch.equal(run(), want)
    finally:
        net.disable_deepcache()
    net.use_graph(True)
    try:
        _fails(engine_lib, run, 4, "graph")
    finally:
        net.use_graph(False)
    tcfg = config.UNetConfig(**dict(config.tiny_unet(time_cond=32).to_dict(), in_channels=8))
    tnet = HipUNet2DConditionModel(tcfg).load_state_dict(_state_dict(tcfg, 11))
    _fails(engine_lib, lambda: tnet.forward_concat(ld, 501.0, ed, im, zero_from=4), 4, "timestep_cond")
    # a text_time UNet: pooled text and time ids differ per group, the tiled time embedding would take the first group's
    xcfg = config.UNetConfig(**dict(config.tiny_unet(linear=True, sdxl_cond=True).to_dict(), in_channels=8))
    xnet = HipUNet2DConditionModel(xcfg).load_state_dict(_state_dict(xcfg, 13))
    g = torch.Generator().manual_seed(7)
    added = {"text_embeds": torch.randn(6, 64, generator=g).half().cuda(),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 6).cuda()}
    _fails(engine_lib, lambda: xnet.forward_concat(ld, 501.0, ed, im, zero_from=4, added_cond_kwargs=added), 4, "text_time")
    sample8 = _sample(lat, img, 3, 1.0).cuda()
    assert torch.isfinite(xnet(sample8, torch.tensor(501.0), ed, added_cond_kwargs=added)[0].float()).all()
    # ---- SD_ERR_INVALID, at the C entry (the Python shim checks the same things first) ----
    refused(1, "in_channels", extra_channels=5)
    refused(1, "in_channels", extra_channels=3)
    refused(1, "B_lat", B=5)
    refused(1, "B_lat", B_lat=4)
    refused(1, "zero_from", zero_from=7)
    refused(1, "second source", extra_rows=0)
    refused(1, "null", latents=None)
    refused(1, "null", extra=None)
    refused(1, "null", ts=None)
    refused(1, "null", ehs_=None)
    assert (out == 9.0).all()
    # a 4-channel UNet has no second source to take: the shim says so itself
    with pytest.raises(ValueError, match="in_channels"):
        pnet.forward_concat(ld, 501.0, ed, im, zero_from=4)
    assert entry() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(run(), want)


# ------------------------------------------------------------------------------------------------ the pipeline
STEPS = 3
ENTRIES = ("sd_cfg_linear_step", "sd_cfg_rescale_linear_step", "sd_pag_linear_step", "sd_pag_combine", "sd_lcm_step",
           "sd_sched_affine_step", "sd_ip2p_linear_step", "sd_ip2p_combine", "sd_unet_forward_concat", "sd_unet_forward",
           "sd_unet_forward_cfg")


class CountingLib:
    """The engine library with the calls to ENTRIES recorded as (name, arguments): test_device_step_dispatch_gpu's spy."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ENTRIES:
            return fn

        def counted(*args):
            self.calls.append((name, args))
            return fn(*args)
        return counted


@pytest.fixture(scope="module")
def model(nets):
    vcfg = config.tiny_vae()
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), 12).items()}
    return SDModelWrapper(base=nets["tiny"][2], vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(),
                          device="cuda")


def _loop_inputs(B=2):
    g = torch.Generator().manual_seed(3)
    dim = config.tiny_unet().cross_attention_dim
    return dict(prompt_embeds=torch.randn(B, 7, dim, generator=g).half().cuda(),
                negative_prompt_embeds=torch.randn(B, 7, dim, generator=g).half().cuda(),
                latents=torch.randn(B, 4, 16, 16, generator=g).half().cuda(),
                image=(torch.rand(B, 3, 128, 128, generator=g) * 2 - 1).half().cuda(),
                num_inference_steps=STEPS, guidance_scale=7.5, seed=2)


def _run(model, host, do_cfg=True, **kw):
    """One loop -> (latents, {entry: number of calls})."""
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    if host:
        pipe._device_step_kind = lambda *a: None
    args = dict(_loop_inputs(), **kw)
    if not do_cfg:
        args.pop("negative_prompt_embeds")
    real = model.base._lib
    proxy = model.base._lib = CountingLib(real)
    try:
        torch.manual_seed(3)
        out = pipe(model, **args)
    finally:
        model.base._lib = real
    counts = {}
    for entry, _ in proxy.calls:
        counts[entry] = counts.get(entry, 0) + 1
    return out, counts


@pytest.mark.parametrize("name", ["DDIM", "euler", "PNDM", "lcm"])
def test_device_loop_equals_host_loop(engine_lib, model, name):
    """Three steps at 128 px on the engine: the device step against scheduler.step on the same forward, within
    test_sched_step_gpu's LOOP_TOL; the spy says which entries ran; and image_guidance_scale is live."""
    model.set_scheduler(name)
    iters = STEPS + 1 if name == "PNDM" else STEPS
    dev, ran = _run(model, host=False, image_guidance_scale=1.0)
    host, ran_host = _run(model, host=True, image_guidance_scale=1.0)
    e = rel_l2(dev, host)
    print(f"pix2pix loop {name}: device vs host rel-L2 {e:.2e}")
    assert ran.pop("sd_unet_forward_concat") == iters and ran_host == {"sd_unet_forward_concat": iters}
    if name in ("DDIM", "euler"):
        assert ran == {"sd_ip2p_linear_step": iters}, ran
    else:
        assert ran == {"sd_ip2p_combine": iters, "sd_lcm_step" if name == "lcm" else "sd_sched_affine_step": iters}, ran
    assert torch.isfinite(dev.float()).all() and e < LOOP_TOL
    other, _ = _run(model, host=False, image_guidance_scale=2.5)
    apart = rel_l2(other, dev)
    print(f"pix2pix loop {name}: image_guidance_scale 2.5 is {apart:.2e} away from 1.0")
    assert apart > 10 * LOOP_TOL


def test_loop_without_cfg_is_one_group(engine_lib, model):
    model.set_scheduler("euler_a")
    dev, ran = _run(model, host=False, do_cfg=False)
    host, ran_host = _run(model, host=True, do_cfg=False)
    assert ran == {"sd_unet_forward_concat": STEPS, "sd_sched_affine_step": STEPS} and ran_host == {"sd_unet_forward_concat": STEPS}
    assert torch.isfinite(dev.float()).all() and rel_l2(dev, host) < LOOP_TOL
