"""sd_cfg_rescale_linear_step (guidance rescale fused into the device CFG + scheduler step) against a float64 reference
computed from the same fp16 inputs, and the fused denoise loop against the host loop.

Bounds: latents rel-L2 < 1e-3 and history rel-L2 < 1e-5 are test_models_gpu.py::test_cfg_linear_step_kernel's; the factor
k_b = 1 + phi (std(t_b) / std(e_b) - 1) is held to 1e-5 relative, which centred fp32 statistics meet with two orders to
spare and a plain E[x^2] - E[x]^2 misses by orders of magnitude at a mean of 100; the loop bound 3e-3 is
test_fused_device_step_equals_host_scheduler_loop's."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2

gpu = pytest.mark.gpu
COEF = dict(cx=0.93, ce=-0.21, ch=0.07, hx=1.8, he=-1.5)
G = 7.5


def _inputs(B, n, seed, offset=0.0, su=1.0, st=1.0):
    g = torch.Generator().manual_seed(seed)
    u = (offset + su * torch.randn(B, n, generator=g)).half()
    t = (offset + st * torch.randn(B, n, generator=g)).half()
    lat = torch.randn(B, n, generator=g).half()
    hist = torch.randn(B, n, generator=g)
    return torch.cat([u, t]), lat, hist


def _large_offset_inputs():
    """t = 100 + N(0, 0.5), u = 100 + N(0, 0.4) in fp16, n = 16384: the sum of squares is about 1.6e8 (fp32 ulp 16) while
    the centred sum is about 4e3."""
    return _inputs(2, 16384, seed=41, offset=100.0, su=0.4, st=0.5)


def _reference(eps2b, lat, hist, g, phi, cx, ce, ch, hx, he):
    """float64, from the same fp16 inputs.  e is the fp16 value the kernels form: one fp32 fused multiply-add of the fp16
    operands (the product g (t - u) is exact in float64), rounded to fp16."""
    B = lat.shape[0]
    u, t = eps2b[:B].double().numpy(), eps2b[B:].double().numpy()
    g32 = float(np.float32(g))
    e = torch.from_numpy((g32 * (t - u) + u).astype(np.float32)).half().double().numpy()
    k = 1.0 + phi * (t.std(axis=1, ddof=1) / e.std(axis=1, ddof=1) - 1.0)
    ke = k[:, None] * e
    x = lat.double().numpy()
    out = cx * x + ce * ke
    new_hist = hx * x + he * ke
    if hist is not None:
        out = out + ch * hist.double().numpy()
    return torch.from_numpy(out), torch.from_numpy(new_hist), k


def _call(lib, eps2b, lat, hist, phi, want_factors=True, g=G, **coef):
    c = dict(COEF, **coef)
    B, n = lat.shape[0], lat[0].numel()
    eps_d, out = eps2b.cuda(), lat.clone().cuda()
    h = hist.clone().cuda() if hist is not None else None
    f = torch.full((B,), float("nan"), device="cuda") if want_factors else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sd_cfg_rescale_linear_step(C.c_void_p(eps_d.data_ptr()), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(h.data_ptr()) if h is not None else None, B, n, g, phi, c["cx"], c["ce"],
                                        c["ch"], c["hx"], c["he"], C.c_void_p(f.data_ptr()) if f is not None else None, st)
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return out.cpu(), (h.cpu() if h is not None else None), (f.cpu().double().numpy() if f is not None else None)


def test_fp32_two_pass_statistics_meet_the_factor_bound_on_the_large_offset_inputs():
    """CPU: before the 1e-5 bound is asked of the kernel on these inputs, an fp32 two-pass (centred) evaluation is shown
    to stay inside it and the plain fp32 sum of squares to miss it."""
    eps2b, lat, _ = _large_offset_inputs()
    B = lat.shape[0]
    u, t = eps2b[:B].float(), eps2b[B:].float()
    e = (G * (t - u) + u).half().float()
    _, _, k64 = _reference(eps2b, lat, None, G, 1.0, **COEF)

    def m2_two_pass(z):
        return ((z - z.mean(1, keepdim=True)) ** 2).sum(1)

    def m2_naive(z):
        n = z.shape[1]
        return (z * z).sum(1) - z.sum(1) ** 2 / n

    k_two = (m2_two_pass(t) / m2_two_pass(e)).sqrt().double().numpy()
    k_naive = (m2_naive(t) / m2_naive(e)).sqrt().double().numpy()
    err_two, err_naive = np.abs(k_two / k64 - 1).max(), np.abs(k_naive / k64 - 1).max()
    print(f"large offset: fp32 two-pass rel err {err_two:.2e}, fp32 E[x^2]-E[x]^2 rel err {err_naive:.2e}")
    assert err_two <= 1e-5
    assert not err_naive <= 1e-3


@gpu
@pytest.mark.parametrize("phi", [0.25, 1.0])
@pytest.mark.parametrize("with_hist", [True, False])
@pytest.mark.parametrize("B,n", [(3, 4 * 9 * 9), (2, 4 * 64 * 64), (1, 4)])
def test_kernel_against_float64(engine_lib, B, n, with_hist, phi):
    eps2b, lat, hist = _inputs(B, n, seed=B * 1000 + n)
    hist = hist if with_hist else None
    out, h, k = _call(engine_lib, eps2b, lat, hist, phi)
    ref, ref_hist, k64 = _reference(eps2b, lat, hist, G, phi, **COEF)
    e_out, e_k = rel_l2(out, ref), np.abs(k / k64 - 1).max()
    print(f"B={B} n={n} hist={with_hist} phi={phi}: latents {e_out:.2e} factors {e_k:.2e}", end="")
    assert e_k <= 1e-5
    assert e_out < 1e-3
    if with_hist:
        e_h = (torch.linalg.vector_norm(h.double() - ref_hist) / torch.linalg.vector_norm(ref_hist)).item()
        print(f" hist {e_h:.2e}")
        assert e_h < 1e-5
    # without the test hook the result is the same
    out2, _, _ = _call(engine_lib, eps2b, lat, hist, phi, want_factors=False)
    assert torch.equal(out, out2)


@gpu
def test_kernel_factors_at_a_large_offset(engine_lib):
    eps2b, lat, hist = _large_offset_inputs()
    out, h, k = _call(engine_lib, eps2b, lat, hist, 1.0)
    ref, ref_hist, k64 = _reference(eps2b, lat, hist, G, 1.0, **COEF)
    err = np.abs(k / k64 - 1).max()
    print(f"large offset: factors {k} vs {k64}, rel err {err:.2e}")
    assert err <= 1e-5
    assert rel_l2(out, ref) < 1e-3


@gpu
@pytest.mark.parametrize("B,n", [(3, 4 * 9 * 9), (2, 4 * 64 * 64)])
def test_phi_zero_is_bitwise_the_linear_step(engine_lib, B, n):
    eps2b, lat, hist = _inputs(B, n, seed=5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for hh in (hist, None):
        out, h, k = _call(engine_lib, eps2b, lat, hh, 0.0)
        eps_d, old = eps2b.cuda(), lat.clone().cuda()
        oh = hh.clone().cuda() if hh is not None else None
        rc = engine_lib.sd_cfg_linear_step(C.c_void_p(eps_d.data_ptr()), C.c_void_p(old.data_ptr()),
                                           C.c_void_p(oh.data_ptr()) if oh is not None else None, lat.numel(), G, COEF["cx"],
                                           COEF["ce"], COEF["ch"], COEF["hx"], COEF["he"], st)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out, old.cpu())
        assert (k == 1.0).all()
        if hh is not None:
            assert torch.equal(h, oh.cpu())


@gpu
def test_error_codes_launch_nothing(engine_lib):
    eps2b, lat, hist = _inputs(2, 64, seed=1)
    eps_d, out, f = eps2b.cuda(), lat.clone().cuda(), torch.full((2,), -3.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    tail = (G, 0.5, 0.9, -0.2, 0.0, 0.0, 0.0, P(f), st)
    assert engine_lib.sd_cfg_rescale_linear_step(P(eps_d), P(out), None, 2, 1, *tail) == 1        # n_per_sample < 2
    assert b"sd_cfg_rescale_linear_step" in engine_lib.sd_last_error()
    assert engine_lib.sd_cfg_rescale_linear_step(P(eps_d), P(out), None, 0, 64, *tail) == 1       # B < 1
    assert engine_lib.sd_cfg_rescale_linear_step(None, P(out), None, 2, 64, *tail) == 1
    assert engine_lib.sd_cfg_rescale_linear_step(P(eps_d), None, None, 2, 64, *tail) == 1
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), lat) and (f.cpu() == -3.0).all()


# ---------------------------------------------------------------------------------------------
# the fused loop (sd_cfg_duplicate + sd_cfg_rescale_linear_step) against the host loop, tests/golden/tiny_sd.npz model
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_models(engine_lib):
    import importlib.util
    from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    ucfg, vcfg, uw, vw = mg.golden_weights()
    return ucfg, HipUNet2DConditionModel(ucfg).load_state_dict(uw), HipAutoencoderKL(vcfg).load_state_dict(vw)


def _wrapper(tiny_models, sched, prediction_type):
    from stablediffusion_amd.pipeline import SDModelWrapper
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, unet, vae = tiny_models
    model = SDModelWrapper(base=unet, vae=vae, scheduler=DDIMScheduler(), device="cuda", prediction_type=prediction_type)
    model.set_scheduler(sched)
    assert model.scheduler.config.prediction_type == prediction_type
    return ucfg, model


def _fused_and_host(model, kw, lat_probe, channels=4):
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    calls = []
    real = model.base._lib.sd_cfg_rescale_linear_step

    class Spy:                                # the library object, with the new entry counted
        def __getattr__(self, name):
            return getattr(real_lib, name)

        def sd_cfg_rescale_linear_step(self, *a):
            calls.append(a[6])
            return real(*a)

    real_lib = model.base._lib
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    model.base._lib = Spy()
    try:
        fused = pipe(model, **kw)
    finally:
        model.base._lib = real_lib
    assert pipe._fused_step_available(model, lat_probe if lat_probe is not None else fused, channels)
    assert len(calls) == kw["num_inference_steps"] and all(abs(c - kw["guidance_rescale"]) < 1e-7 for c in calls)
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    host_pipe._fused_step_available = lambda *a: False
    host = host_pipe(model, **kw)
    return fused, host


@gpu
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("sched", ["DDIM", "euler", "DPM++ 2M"])
def test_fused_rescaled_loop_equals_host_loop(tiny_models, sched, prediction_type):
    ucfg, model = _wrapper(tiny_models, sched, prediction_type)
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=6, guidance_scale=5.0,
              guidance_rescale=0.7, height=128, width=128)
    fused, host = _fused_and_host(model, kw, lat0)
    err = rel_l2(fused, host)
    print(f"{sched} {prediction_type}: fused vs host rel-L2 {err:.2e}")
    assert torch.isfinite(fused.float()).all()
    assert err < 3e-3
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    plain = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")(
        model, **dict(kw, guidance_rescale=0.0))
    assert rel_l2(fused, plain) > 1e-2           # the rescale really acts on the device path


@gpu
def test_fused_rescaled_inpaint_blend_equals_host_loop(tiny_models):
    ucfg, model = _wrapper(tiny_models, "DDIM", "epsilon")
    g = torch.Generator().manual_seed(4)
    pos = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    image = torch.randn(1, 3, 128, 128, generator=g).clamp(-1, 1).half().cuda()
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, image=image, mask_image=mask.cuda(), num_inference_steps=4,
              seed=2, guidance_scale=5.0, guidance_rescale=0.7)
    fused, host = _fused_and_host(model, kw, None)
    assert torch.isfinite(fused.float()).all() and rel_l2(fused, host) < 3e-3
    w = fused.shape[-1]
    assert torch.allclose(fused[..., : w // 2].float(), host[..., : w // 2].float(), atol=2e-3)   # kept region
