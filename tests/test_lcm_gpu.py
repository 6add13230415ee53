"""LCM few-step sampling on the GPU: the two kernels against float64 (tests/lcm_oracle.py), the guidance-embedded UNet
against the oracle's restated forward, and the loop with the device step against the same loop on scheduler.step."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import lcm_oracle  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import ip_attention, project, synth_ip_state_dict  # noqa: E402
from oracle import unet_ref  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, schedulers, weights  # noqa: E402
from stablediffusion_amd.models import (HipAutoencoderKL, HipControlNetModel, HipIPAdapter,  # noqa: E402
                                        HipUNet2DConditionModel)
from stablediffusion_amd.pipeline import (SDModelWrapper, StableDiffusionUnifiedPipeline,  # noqa: E402
                                          guidance_scale_embedding)

pytestmark = pytest.mark.gpu

TOL = 1e-2          # engine vs the oracle with timestep_cond (BASELINE.json's bound, as test_freeu_gpu.py)
GAP = 0.1           # ... and this far from the oracle without it
COND_GAIN = 4.0     # on the synthetic cond_proj weight, so that the projection moves the output by more than GAP
STEP_CAP = 0.01     # share of elements that may differ, by one fp16 ulp, from the rounded float64 step


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ temb kernel
@pytest.mark.parametrize("B,dim,cond_dim", [(1, 64, 32), (3, 64, 33), (2, 320, 256), (5, 320, 40), (8, 128, 1024)])
@pytest.mark.parametrize("flip,shift", [(1, 0.0), (0, 1.0)])
def test_timestep_cond_embedding(engine_lib, B, dim, cond_dim, flip, shift):
    """sd_op_timestep_cond_embedding against float64, for t in {0, 1, 501, 999} (every row of the batch takes each).

    cond = 0 must give sd_op_timestep_sinusoid's bits.  Otherwise, per output,
        |got - ref| <= tol_sin + K 2^-23 sum_k |W_jk c_k|,   tol_sin = 5e-4,   K = cond_dim:
    tol_sin is test_ops_gpu.py::test_timestep_sinusoid's bound on the sinusoid itself (fp32 range reduction of arguments
    up to 1e3 rad); an fp32 dot product of K terms in any order is within (K - 1) u of sum |W c| plus u per product
    (u = 2^-24, fused multiply-adds), and the final addition to the sinusoid adds u (|sin| + |sum|): K 2^-23 sum |W c|
    covers the three with a factor two to spare (the weights are fp16 values and the cond is fp32, both exact inputs)."""
    from oracle.unet_ref import timestep_sinusoid
    g = torch.Generator().manual_seed(B * 1000 + cond_dim)
    w = (torch.randn(dim, cond_dim, generator=g) / cond_dim ** 0.5).half()
    cond = torch.randn(B, cond_dim, generator=g)
    wd, cd, zd = w.cuda(), cond.cuda(), torch.zeros(B, cond_dim, device="cuda")
    for tv in (0.0, 1.0, 501.0, 999.0):
        t = torch.full((B,), tv)
        td = t.cuda()
        plain = torch.zeros(B, dim, device="cuda")
        out0 = torch.full((B, dim), 7.0, device="cuda")
        out = torch.full((B, dim), 7.0, device="cuda")
        assert engine_lib.sd_op_timestep_sinusoid(P(td), P(plain), B, dim, flip, shift, stream()) == 0
        assert engine_lib.sd_op_timestep_cond_embedding(P(td), P(zd), P(wd), P(out0), B, dim, cond_dim, flip, shift,
                                                        stream()) == 0, engine_lib.sd_last_error()
        assert engine_lib.sd_op_timestep_cond_embedding(P(td), P(cd), P(wd), P(out), B, dim, cond_dim, flip, shift,
                                                        stream()) == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out0.view(torch.int32), plain.view(torch.int32)), tv
        sin64 = timestep_sinusoid(t.double(), dim, bool(flip), shift).double()        # (fp32 frequencies, as diffusers)
        terms = w.double()[None, :, :] * cond.double()[:, None, :]                    # [B, dim, cond_dim]
        ref = sin64 + terms.sum(-1)
        bound = 5e-4 + cond_dim * 2.0 ** -23 * terms.abs().sum(-1)
        err = (out.cpu().double() - ref).abs()
        print(f"temb_cond B={B} dim={dim} K={cond_dim} t={tv}: max err {err.max().item():.2e}, "
              f"max err / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), tv


def test_timestep_cond_embedding_rejects_bad_arguments(engine_lib):
    p = C.c_void_p(64)
    for dim, cd in ((63, 32), (64, 0), (64, 1025)):
        assert engine_lib.sd_op_timestep_cond_embedding(p, p, p, p, 1, dim, cd, 1, 0.0, None) == 1


# ------------------------------------------------------------------------------------------------ step kernel
@pytest.fixture(scope="module")
def plans():
    """(d_x, d_out, p_den, p_noise, needs_noise) of the first, a middle and the last step of a real 4-step schedule."""
    out = {}
    for pred in ("epsilon", "v_prediction"):
        s = schedulers.LCMScheduler(prediction_type=pred)
        s.set_timesteps(4)
        ps = []
        for t in s.timesteps.tolist():
            ps.append(s.fused_plan(t))
            s.fused_commit()
        out[pred] = [ps[0], ps[1], ps[3]]
    return out


@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("n", [1, 7, 8, 2047, 4 * 4 * 16 * 16, 3 * 4 * 24 * 40])
def test_lcm_step(engine_lib, plans, n, rows):
    """sd_lcm_step against the float64 evaluation of its formula on the same fp16 inputs (lcm_oracle.step_reference; for
    rows = 2 the guidance combine is rounded to fp16 the way the formula says, fp32 fused multiply-add first): both
    outputs equal the fp16 rounding of the float64 result except on at most 1 % of the elements, which may be one fp16
    ulp off.  That 1 % is a cap: fp32-vs-float64 flips at rounding ties are ~0.1 % (test_lcm.py checks that the
    reference alone stays under a quarter of the cap on these inputs).  noise and denoised absent and present, the
    coefficients of a first, a middle and a last step, epsilon and v; guard elements around every buffer stay as they
    were, at n that are no multiple of 8 (scalar kernel) and at an offset that breaks the 16-byte alignment."""
    G = 16                                                  # guard elements on both sides
    g = 1.5
    mo, lat, noise = lcm_oracle.step_inputs(n, seed=n)
    worst = 0.0

    def guarded(t, fill, shift=0):
        buf = torch.full((G + shift + t.numel() + G,), fill, dtype=torch.float16, device="cuda")
        buf[G + shift:G + shift + t.numel()] = t.cuda()
        return buf, buf[G + shift:G + shift + t.numel()]

    for pred in ("epsilon", "v_prediction"):
        for plan in plans[pred]:
            for want_den in (False, True):
                for shift in ((0, 1) if n == 8 else (0,)):     # n = 8 also off the 16-byte alignment: the scalar kernel
                    use_noise = plan.needs_noise
                    # (a last step takes noise = NULL; a noisy step is also run with p_noise = 0 and NULL)
                    for nz, p_noise in ((noise if use_noise else None, plan.p_noise), (None, 0.0)):
                        mo_buf, mo_v = guarded(mo[:rows * n], 3.0, shift)
                        lat_buf, lat_v = guarded(lat, 5.0, shift)
                        den_buf, den_v = guarded(torch.zeros(n), 9.0, shift)
                        nz_buf, nz_v = guarded(nz if nz is not None else torch.zeros(n), 11.0, shift)
                        rc = engine_lib.sd_lcm_step(P(mo_v), rows, P(lat_v), P(nz_v) if nz is not None else None,
                                                    P(den_v) if want_den else None, n, g, plan.d_x, plan.d_out, plan.p_den,
                                                    p_noise, stream())
                        assert rc == 0, engine_lib.sd_last_error()
                        torch.cuda.synchronize()
                        den64, out64 = lcm_oracle.step_reference(mo, rows, lat, nz, n, g, plan.d_x, plan.d_out,
                                                                 plan.p_den, p_noise)
                        checks = [("latents", lat_v.cpu(), out64)]
                        if want_den:
                            checks.append(("denoised", den_v.cpu(), den64))
                        else:
                            assert (den_v == 0).all()                 # denoised = NULL: nothing is written
                        for name, got, ref in checks:
                            ulps = lcm_oracle.ulp_diff_f16(got, lcm_oracle.to_f16(ref))
                            share = (ulps != 0).sum().item() / n
                            worst = max(worst, share)
                            assert ulps.max().item() <= 1, (name, pred, n, rows, ulps.max().item())
                            assert (ulps != 0).sum().item() <= STEP_CAP * n, (name, pred, n, rows, share)
                        # nothing outside [0, n) was written, inputs are unchanged
                        for buf, fill in ((mo_buf, 3.0), (lat_buf, 5.0), (den_buf, 9.0), (nz_buf, 11.0)):
                            assert (buf[:G + shift] == fill).all() and (buf[-G:] == fill).all()
                        assert torch.equal(mo_v.cpu(), mo[:rows * n])
    print(f"lcm_step n={n} rows={rows}: worst share of one-ulp elements {worst:.5f} (cap {STEP_CAP})")


# ------------------------------------------------------------------------------------------------ UNet
def _tc_weights(cfg, seed=11):
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=seed, perturb=0.1)
    sd["time_embedding.cond_proj.weight"] = sd["time_embedding.cond_proj.weight"] * COND_GAIN
    return _f16_round(sd)


@pytest.fixture(scope="module")
def tiny_tc():
    cfg = config.tiny_unet(time_cond=32)
    sd = _tc_weights(cfg)
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


@pytest.fixture(scope="module")
def tiny_tc_xl():
    cfg = config.tiny_unet(linear=True, sdxl_cond=True, time_cond=32)
    sd = _tc_weights(cfg)
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


def _inputs(cfg, B, H, W):
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    tc = guidance_scale_embedding(torch.linspace(0.5, 7.0, B), cfg.time_cond_proj_dim)
    added = None
    if cfg.addition_embed_type == "text_time":
        added = {"text_embeds": torch.randn(B, 64, generator=g).half(),
                 "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * B)}
    return x, ehs, tc, added


def _cuda(added):
    return None if added is None else {k: v.cuda() for k, v in added.items()}


def _check(got, with_tc, without, what):
    e_on, e_off, gap = rel_l2(got, with_tc), rel_l2(got, without), rel_l2(with_tc, without)
    print(f"{what}: vs oracle with timestep_cond {e_on:.2e}, vs oracle without {e_off:.2e} (oracles apart {gap:.2f})")
    assert e_on < TOL
    assert e_off > GAP


@pytest.mark.parametrize("which", ["tiny_tc", "tiny_tc_xl"])
@pytest.mark.parametrize("B,H,W", [(1, 8, 24), (2, 16, 16), (3, 24, 24)])
def test_unet_forward_tc_matches_oracle(engine_lib, request, which, B, H, W):
    cfg, sd, net = request.getfixturevalue(which)
    x, ehs, tc, added = _inputs(cfg, B, H, W)
    t = torch.tensor(501.0)
    ref_added = None if added is None else {k: v.float() for k, v in added.items()}
    with torch.no_grad():
        on = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), tc, ref_added)
        off = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), None, ref_added)
    got = net(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), timestep_cond=tc.cuda())[0]
    _check(got, on, off, f"{which} B={B} {H}x{W}")
    # any float dtype: the shim converts
    again = net(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), timestep_cond=tc.double().cuda())[0]
    assert torch.equal(again, got)
    # timestep_cond absent: the projection is skipped -- the plain forward, bit for bit through either entry
    plain = net(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added))[0]
    assert rel_l2(plain, off) < TOL
    xd, ed, td = x.cuda(), ehs.cuda(), torch.full((B,), 501.0, device="cuda")
    ad = _cuda(added)
    pt = P(ad["text_embeds"]) if ad else None
    pi = P(ad["time_ids"]) if ad else None              # (fp32 and contiguous as built)
    out = torch.empty_like(plain)
    rc = engine_lib.sd_unet_forward_tc(net._h, P(xd), P(td), P(ed), 77, pt, pi, None, 0, None, 0, P(out), B, H, W, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, plain)


def test_unet_forward_tc_odd_cond_dim(engine_lib):
    """time_cond_proj_dim = 33: the packed cond_proj rows are 64 halves wide (zero padded), the engine reads them with
    16-byte loads and must stop at column 33 of a timestep_cond row that is 33 floats long."""
    cfg = config.tiny_unet(time_cond=33)
    sd = _tc_weights(cfg)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    x, ehs, tc, _ = _inputs(cfg, 3, 16, 16)
    assert tc.shape == (3, 33)
    t = torch.tensor(501.0)
    with torch.no_grad():
        on = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), tc)
        off = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float())
    # the cond sits at the very end of its allocation's used part: a read past column 33 of the last row would meet the NaNs
    buf = torch.full((3 * 33 + 64,), float("nan"), device="cuda")
    buf[:3 * 33] = tc.reshape(-1).cuda()
    got = net(x.cuda(), t, ehs.cuda(), timestep_cond=buf[:3 * 33].view(3, 33))[0]
    assert torch.isfinite(got.float()).all()
    _check(got, on, off, "time_cond_proj_dim = 33")


def test_graph_replay_is_bitwise_eager(engine_lib, tiny_tc):
    cfg, sd, net = tiny_tc
    x, ehs, tc, _ = _inputs(cfg, 2, 16, 16)
    xd, ed, tcd = x.cuda(), ehs.cuda(), tc.cuda()
    eager = net(xd, 501.0, ed, timestep_cond=tcd)[0]
    eager_plain = net(xd, 501.0, ed)[0]
    tc2 = (tcd * 0.5).contiguous()
    eager2 = net(xd, 501.0, ed, timestep_cond=tc2)[0]
    assert not torch.equal(eager, eager2) and not torch.equal(eager, eager_plain)
    net.use_graph(True)
    try:
        first = net(xd, 501.0, ed, timestep_cond=tcd)[0]            # eager run + capture
        replay = net(xd, 501.0, ed, timestep_cond=tcd)[0]           # replay
        tcd.mul_(0.5)                                               # same buffer, other contents
        replay2 = net(xd, 501.0, ed, timestep_cond=tcd)[0]
        plain = net(xd, 501.0, ed)[0]                               # another key: captured anew, without the projection
        plain_replay = net(xd, 501.0, ed)[0]
    finally:
        net.use_graph(False)
    assert torch.equal(first, eager) and torch.equal(replay, eager)
    assert torch.equal(replay2, eager2)
    assert torch.equal(plain, eager_plain) and torch.equal(plain_replay, eager_plain)


def test_forward_tc_with_an_ip_adapter_attached(engine_lib, tiny_tc):
    """timestep_cond together with a live image branch (scale 0.7), against the oracle that has both (ip_oracle's
    attention under lcm_oracle's forward); the oracle with the projection but without the image branch is further away."""
    cfg, sd, net = tiny_tc
    ip_sd = synth_ip_state_dict(cfg, 128, 4, seed=3)
    ad = HipIPAdapter(net, 128, 4).load_state_dict(ip_sd)
    x, ehs, tc, _ = _inputs(cfg, 2, 16, 16)
    g = torch.Generator().manual_seed(6)
    img = torch.randn(2, 1, 128, generator=g).half()
    kw = {"added_cond_kwargs": {"image_embeds": [img.cuda()]}}
    t = torch.tensor(501.0)
    orig = unet_ref.attention
    unet_ref.attention = ip_attention(ip_sd, 0.7, orig)
    try:
        with torch.no_grad():
            ctx = (ehs.float(), project(ip_sd, img.float(), 4))
            on = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ctx, tc)
            off = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ctx)
            text_only = lcm_oracle.unet_forward(cfg, sd, x.float(), t, ehs.float(), tc)
    finally:
        unet_ref.attention = orig
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.7)
    try:
        got = net(x.cuda(), t, ehs.cuda(), timestep_cond=tc.cuda(), **kw)[0]
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    _check(got, on, off, "ip-adapter (scale 0.7) + timestep_cond")
    e_text = rel_l2(got, text_only)
    print(f"ip-adapter + timestep_cond: vs the oracle without the image branch {e_text:.2e} "
          f"(oracles apart {rel_l2(on, text_only):.2e})")
    assert e_text > 3 * TOL                         # the image branch is live in what was compared


def test_forward_tc_error_codes(engine_lib, tiny_tc):
    cfg, sd, net = tiny_tc
    x, ehs, tc, _ = _inputs(cfg, 2, 16, 16)
    xd, ed, tcd = x.cuda(), ehs.cuda(), tc.cuda()
    td = torch.full((2,), 501.0, device="cuda")
    out = torch.empty(2, 4, 16, 16, dtype=torch.float16, device="cuda")

    def call(handle, cond, cond_dim):
        return engine_lib.sd_unet_forward_tc(handle, P(xd), P(td), P(ed), 77, None, None, None, 0,
                                             P(cond) if cond is not None else None, cond_dim, P(out), 2, 16, 16, stream())

    assert call(net._h, tcd, 31) == 1 and b"cond_dim" in engine_lib.sd_last_error()
    with pytest.raises(_lib.EngineError, match="error 1"):
        net(xd, 501.0, ed, timestep_cond=tcd[:, :16])
    with pytest.raises(ValueError):
        net(xd, 501.0, ed, timestep_cond=tcd[:1])
    # a UNet without the projection takes no timestep_cond
    pcfg = config.tiny_unet()
    plain = HipUNet2DConditionModel(pcfg).load_state_dict(
        _f16_round(weights.synth_state_dict(weights.unet_manifest(pcfg), seed=11, perturb=0.1)))
    assert call(plain._h, tcd, 32) == 1 and b"time_cond_proj_dim" in engine_lib.sd_last_error()
    assert call(plain._h, None, 0) == 0
    # an attached ControlNet: unsupported
    ccfg = controlnet.encoder_config(cfg)
    cn = HipControlNetModel(net, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=4))
    net.attach_controlnet(cn)
    try:
        assert call(net._h, tcd, 32) == 4 and b"ControlNet" in engine_lib.sd_last_error()
    finally:
        net.attach_controlnet(None)
    assert call(net._h, tcd, 32) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ loop
def _model(ucfg, seed=11):
    vcfg = config.tiny_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed)
    if ucfg.time_cond_proj_dim:
        usd["time_embedding.cond_proj.weight"] = usd["time_embedding.cond_proj.weight"] * COND_GAIN
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(_f16_round(usd)),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), device="cuda")
    model.set_scheduler("lcm")
    return model


def _fused_vs_host(model, do_cfg, kw, what):
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    used = []
    real = pipe._device_iteration
    pipe._device_iteration = lambda *a, **k: (used.append(1), real(*a, **k))[1]
    fused = pipe(model, seed=3, **kw)
    assert len(used) == 4                                    # the device step ran on every iteration
    other = pipe(model, seed=4, **kw)
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    host_pipe._lcm_step_available = lambda *a: False
    host = host_pipe(model, seed=3, **kw)
    e, apart = rel_l2(fused, host), rel_l2(other, fused)
    print(f"lcm loop {what}: fused vs host rel-L2 {e:.2e}, another seed {apart:.2f} away")
    assert torch.isfinite(fused.float()).all()
    assert e < 3e-3                    # test_fused_device_step_equals_host_scheduler_loop's bound
    assert apart > 0.1                 # the noise really goes in
    return fused


def test_loop_guidance_embedded(engine_lib):
    ucfg = config.tiny_unet(time_cond=32)
    model = _model(ucfg)
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half().cuda()       # given: the seed then only feeds the loop's noise
    _fused_vs_host(model, True, dict(prompt_embeds=pos, latents=lat0, num_inference_steps=4, guidance_scale=8.0,
                                     height=128, width=128), "guidance-embedded (rows = 1)")


def test_loop_ordinary_unet_with_cfg(engine_lib):
    ucfg = config.tiny_unet()
    model = _model(ucfg)
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    _fused_vs_host(model, True, dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=4,
                                     guidance_scale=1.5, height=128, width=128), "ordinary UNet + CFG (rows = 2)")


def test_loop_inpaint_4_channels(engine_lib):
    ucfg = config.tiny_unet()
    model = _model(ucfg)
    g = torch.Generator().manual_seed(4)
    pos = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    # the image as latents (nothing is sampled from the VAE) and the initial latents given: the seed then only feeds the
    # loop's noise, as in the two cases above
    image = torch.randn(1, 4, 16, 16, generator=g).half().cuda()
    lat0 = torch.randn(1, 4, 16, 16, generator=g).half().cuda()
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    fused = _fused_vs_host(model, True, dict(prompt_embeds=pos, negative_prompt_embeds=neg, image=image, latents=lat0,
                                             mask_image=mask.cuda(), num_inference_steps=4, guidance_scale=1.5,
                                             height=128, width=128), "4-channel inpainting")
    w = fused.shape[-1]
    assert torch.equal(fused[..., : w // 2], image[..., : w // 2])           # outside the mask: the image's latents
    assert not torch.allclose(fused[..., w // 2:].float(), image[..., w // 2:].float(), atol=1e-2)
