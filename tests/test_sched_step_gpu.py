"""The device step of euler_a, DPM++ 2M SDE, PNDM and UniPC on the GPU: sd_sched_affine_step against the float64
evaluation of its rows (tests/sched_step_oracle.py), and the pipeline's loops against the same loops on scheduler.step."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import lcm_oracle  # noqa: E402
import sched_step_oracle as sso  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from test_sched_step import call, invalid_calls  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402
from stablediffusion_amd.schedulers import DDIMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu

G = 16              # guard elements around every buffer and between the bank's slots
LOOP_TOL = 3e-3     # test_fused_device_step_equals_host_scheduler_loop's bound for the same comparison


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def _guarded(t, fill, shift=0):
    buf = torch.full((G + shift + t.numel() + G,), fill, dtype=t.dtype, device="cuda")
    buf[G + shift:G + shift + t.numel()] = t.cuda()
    return buf, buf[G + shift:G + shift + t.numel()]


def _bank(values, n, shift=0):
    """[G | slot 0 | G | slot 1 | G | .. ] fp32, slots n + G apart; -> (buffer, pointer to slot 0, stride)."""
    stride = n + G
    buf = torch.full((G + shift + 4 * stride,), 13.0, device="cuda")
    for k in range(4):
        lo = G + shift + k * stride
        buf[lo:lo + n] = values[k].cuda()
    return buf, buf[G + shift:], stride


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.float16 else torch.int32))


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("n", sso.GPU_NS)
def test_sched_affine_step(engine_lib, n, rows):
    """sd_sched_affine_step against sched_step_oracle.apply_plan on the same inputs: the first, second, a middle and the
    last step of a 7-step schedule of each of the four schedulers (epsilon and v) and one dense synthetic plan.  Latents
    and written slots are the single rounding of the float64 result: bit for bit below 10^4 elements, above that at most
    1e-4 of the elements one ulp off (a cap; test_sched_step.py shows the reference alone stays far inside it).
    Operands whose column is zero -- unread slots, the noise -- are NaN and the outputs stay finite; the model output,
    the noise, the unwritten slots and the guards around every buffer and between the slots are unchanged.  n = 8 also
    runs one element off the 16-byte alignment, and noise = NULL where its column is zero."""
    g = sso.GPU_GUIDANCE
    mo, lat, noise, bank = sso.step_inputs(n, seed=n)
    nan = float("nan")
    worst16 = worst32 = 0
    for label, plan in sso.gpu_plans():
        used = sso.used_columns(plan)
        written = {k for k, _ in plan.writes}
        nz_in = noise if used[2] else torch.full_like(noise, nan)
        bank_in = torch.stack([bank[k] if used[3 + k] else torch.full_like(bank[k], nan) for k in range(4)])
        ref_x, ref_w = sso.reference(plan, mo, rows, lat, noise, bank, n, g)
        for shift in ((0, 1) if n == 8 else (0,)):
            for null_noise in ((False, True) if not used[2] else (False,)):
                mo_buf, mo_v = _guarded(mo[:rows * n], 3.0, shift)
                lat_buf, lat_v = _guarded(lat, 5.0, shift)
                nz_buf, nz_v = _guarded(nz_in, 11.0, shift)
                bank_buf, bank_v, stride = _bank(bank_in, n, shift)
                rc = engine_lib.sd_sched_affine_step(P(mo_v), rows, P(lat_v), None if null_noise else P(nz_v),
                                                     P(bank_v) if plan.n_slots else None, stride, n, g,
                                                     C.byref(_lib.step_plan(plan)), stream())
                assert rc == 0, (label, engine_lib.sd_last_error())
                torch.cuda.synchronize()
                got_x = lat_v.cpu()
                assert torch.isfinite(got_x.float()).all(), label
                ulps = lcm_oracle.ulp_diff_f16(got_x, sso.to_f16(ref_x))
                off = (ulps != 0).sum().item()
                worst16 = max(worst16, off)
                assert ulps.max().item() <= 1, (label, n, rows, shift)
                assert off <= (sso.GPU_CAP * n if n >= sso.GPU_LARGE_N else 0), (label, n, rows, shift, off)
                if off == 0:
                    assert _same_bits(got_x, sso.to_f16(ref_x)), label
                for k in range(4):
                    lo = G + shift + k * stride
                    got = bank_buf[lo:lo + n].cpu()
                    if k in written:
                        want = sso.to_f32(ref_w[k])
                        assert torch.isfinite(got).all(), (label, k)
                        ulps = sso.ulp_diff_f32(got, want)
                        off = (ulps != 0).sum().item()
                        worst32 = max(worst32, off)
                        assert ulps.max().item() <= 1, (label, n, rows, shift, k)
                        assert off <= (sso.GPU_CAP * n if n >= sso.GPU_LARGE_N else 0), (label, n, rows, shift, k, off)
                        if off == 0:
                            assert _same_bits(got, want), (label, k)
                    else:
                        assert _same_bits(got, bank_in[k]), (label, k)
                    assert (bank_buf[lo + n:lo + stride] == 13.0).all(), (label, k)
                assert (bank_buf[:G + shift] == 13.0).all()
                for buf, fill in ((mo_buf, 3.0), (lat_buf, 5.0), (nz_buf, 11.0)):
                    assert (buf[:G + shift] == fill).all() and (buf[-G:] == fill).all(), label
                assert _same_bits(mo_v.cpu(), mo[:rows * n]) and _same_bits(nz_v.cpu(), nz_in), label
    print(f"sched_affine_step n={n} rows={rows}: most elements one ulp off in a case: fp16 {worst16}, fp32 {worst32}")


# ------------------------------------------------------------------------------------------------ 2. error codes
def test_invalid_calls_launch_nothing(engine_lib):
    n = 8
    mo, lat, noise, bank = sso.step_inputs(n, seed=1)
    mo_d, lat_d, nz_d, bank_d = mo.cuda(), lat.cuda(), noise.cuda(), bank.cuda().contiguous()
    ptrs = {"mo": mo_d.data_ptr(), "lat": lat_d.data_ptr(), "nz": nz_d.data_ptr(), "bank": bank_d.data_ptr()}
    for label, (p_mo, rows, p_lat, p_nz, p_bank, stride, n_, g, plan) in invalid_calls():
        args = (p_mo and ptrs["mo"], rows, p_lat and ptrs["lat"], p_nz and ptrs["nz"], p_bank and ptrs["bank"], stride, n_, g,
                plan)
        assert call(engine_lib, args, stream()) == 1, label
    torch.cuda.synchronize()
    assert _same_bits(mo_d.cpu(), mo) and _same_bits(lat_d.cpu(), lat) and _same_bits(nz_d.cpu(), noise)
    assert _same_bits(bank_d.cpu(), bank)
    # ... and the same buffers are fine with a valid plan
    plan = sso.dense_plan()
    assert engine_lib.sd_sched_affine_step(P(mo_d), 2, P(lat_d), P(nz_d), P(bank_d), n, n, 1.0, C.byref(_lib.step_plan(plan)),
                                           stream()) == 0
    torch.cuda.synchronize()
    assert not _same_bits(lat_d.cpu(), lat)


# ------------------------------------------------------------------------------------------------ 3.-5. loops
def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def model():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    return SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                          vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")


def _embeds(B, seed=3, L=7):
    g = torch.Generator().manual_seed(seed)
    ucfg = config.tiny_unet()
    pos = torch.randn(B, L, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(B, L, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half().cuda()
    return pos, neg, lat0


def _device_vs_host(model, kw, calls, what, do_cfg=True, stochastic=False):
    """The device loop (its `_device_iteration` counted) against the same pipeline with the path switched off, the global
    generator seeded alike in front of each."""
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    used = []
    real = pipe._device_iteration
    pipe._device_iteration = lambda *a, **k: (used.append(1), real(*a, **k))[1]
    torch.manual_seed(3)
    dev = pipe(model, **kw)
    assert len(used) == calls, (what, len(used))                 # the device step ran on every iteration
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    host_pipe._affine_step_available = lambda *a: False
    torch.manual_seed(3)
    host = host_pipe(model, **kw)
    e = rel_l2(dev, host)
    print(f"affine loop {what}: device vs host rel-L2 {e:.2e}")
    assert torch.isfinite(dev.float()).all()
    assert e < LOOP_TOL, what
    if stochastic:
        torch.manual_seed(4)
        other = pipe(model, **kw)
        apart = rel_l2(other, dev)
        print(f"affine loop {what}: another seed {apart:.2f} away")
        assert apart > 0.1                                        # the noise really goes in
    return dev


@pytest.mark.parametrize("name", list(sso.NAMES))
def test_loop_equals_host_scheduler_loop(engine_lib, model, name):
    """test_fused_device_step_equals_host_scheduler_loop's set-up and bound for the four schedulers of the new path."""
    model.set_scheduler(name)
    pos, neg, lat0 = _embeds(2)
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=6, guidance_scale=5.0,
              height=128, width=128)
    _device_vs_host(model, kw, 7 if name == "PNDM" else 6, name, stochastic=sso.NAMES[name][1])


def test_loop_without_cfg(engine_lib, model):
    model.set_scheduler("euler_a")
    pos, _, lat0 = _embeds(2)
    kw = dict(prompt_embeds=pos, latents=lat0, num_inference_steps=6, guidance_scale=5.0, height=128, width=128)
    _device_vs_host(model, kw, 6, "euler_a without CFG (rows = 1)", do_cfg=False, stochastic=True)


def test_loop_inpaint_4_channels(engine_lib, model):
    model.set_scheduler("PNDM")
    pos, neg, lat0 = _embeds(1, seed=4)
    g = torch.Generator().manual_seed(5)
    image = torch.randn(1, 4, 16, 16, generator=g).half().cuda()          # the image as latents: nothing is sampled
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, image=image, latents=lat0, mask_image=mask.cuda(),
              num_inference_steps=6, guidance_scale=5.0, height=128, width=128, seed=2)
    dev = _device_vs_host(model, kw, 7, "PNDM 4-channel inpainting")
    w = dev.shape[-1]
    assert torch.equal(dev[..., : w // 2], image[..., : w // 2])           # outside the mask: the image's latents
    assert not torch.allclose(dev[..., w // 2:].float(), image[..., w // 2:].float(), atol=1e-2)


def test_loop_with_controlnet(engine_lib, model):
    from test_controlnet import _to_original
    ucfg = config.tiny_unet()
    ccfg = controlnet.encoder_config(ucfg)
    model.set_scheduler("uni_pc")
    model.load_controlnet(_to_original(synth_cn_state_dict(ccfg, seed=6), ccfg, "control_model."))
    try:
        pos, neg, lat0 = _embeds(2)
        ctrl = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(8))
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=6, guidance_scale=5.0,
                  height=128, width=128, control_image=ctrl, controlnet_conditioning_scale=0.9)
        with_cn = _device_vs_host(model, kw, 6, "uni_pc with a ControlNet")
    finally:
        model.unload_controlnet()
    kw.pop("control_image"), kw.pop("controlnet_conditioning_scale")
    plain = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")(model, **kw)
    assert rel_l2(plain, with_cn) > 10 * LOOP_TOL                         # the ControlNet was live in what was compared


def test_rescale_and_9_channel_unets_stay_on_the_host_path(engine_lib, model):
    model.set_scheduler("PNDM")
    pos, neg, lat0 = _embeds(1, seed=4)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    used = []
    real = pipe._device_iteration
    pipe._device_iteration = lambda *a, **k: (used.append(1), real(*a, **k))[1]
    assert pipe._affine_step_available(model, lat0, 4, 0.0)          # (a fresh pipeline can be asked)
    assert not pipe._affine_step_available(model, lat0, 4, 0.7)
    out = pipe(model, prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=3, guidance_scale=5.0,
               guidance_rescale=0.7, height=128, width=128)
    assert not used and torch.isfinite(out.float()).all()
    # a 9-channel inpainting UNet: latents + mask + masked-image latents go through the generic branch
    ucfg9 = config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=9))
    usd9 = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg9), 11))
    m9 = SDModelWrapper(base=HipUNet2DConditionModel(ucfg9).load_state_dict(usd9), vae=model.vae, scheduler=DDIMScheduler(),
                        device="cuda")
    m9.set_scheduler("PNDM")
    g = torch.Generator().manual_seed(5)
    image = torch.randn(1, 3, 128, 128, generator=g).clamp(-1, 1).half().cuda()
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    pipe.is_inpaint = True
    assert not pipe._affine_step_available(m9, lat0, 9, 0.0)
    out = pipe(m9, prompt_embeds=pos, negative_prompt_embeds=neg, image=image, mask_image=mask.cuda(), num_inference_steps=3,
               guidance_scale=5.0, seed=2)
    assert not used and torch.isfinite(out.float()).all()
