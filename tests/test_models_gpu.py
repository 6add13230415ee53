"""Model-level parity: the HIP engine (through the C-ABI shims) against the fp32 CPU oracle on the
same seeded inputs and weights.  Weights and inputs are rounded to fp16 first so both sides start
from identical operands; tolerance is BASELINE.json's: relative L2 <= 1e-2."""
import pytest
import torch

from conftest import rel_l2
from oracle import pipeline_ref, unet_ref, vae_ref
from stablediffusion_amd import config, weights
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu
TOL = 1e-2


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def tiny_unet():
    cfg = config.tiny_unet()
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


@pytest.fixture(scope="module")
def tiny_vae():
    cfg = config.tiny_vae()
    sd = _f16_round(weights.synth_state_dict(weights.vae_manifest(cfg), seed=12, perturb=0.1))
    return cfg, sd, HipAutoencoderKL(cfg).load_state_dict(sd)


@pytest.mark.parametrize("B,H,W,t", [(2, 16, 16, 981.0), (1, 8, 24, 1.0), (3, 32, 32, 500.0)])
def test_unet_forward(engine_lib, tiny_unet, B, H, W, t):
    cfg, sd, net = tiny_unet
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    ref = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), ehs.float())
    got = net(x.cuda(), torch.tensor(t), ehs.cuda(), return_dict=False)[0]
    assert got.shape == ref.shape and got.dtype == torch.float16
    assert rel_l2(got, ref) < TOL


def test_unet_per_sample_timesteps_and_determinism(engine_lib, tiny_unet):
    cfg, sd, net = tiny_unet
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    t = torch.tensor([981.0, 21.0])
    ref = unet_ref.unet_forward(cfg, sd, x.float(), t, ehs.float())
    a = net(x.cuda(), t, ehs.cuda())[0]
    b = net(x.cuda(), t, ehs.cuda())[0]
    assert rel_l2(a, ref) < TOL
    assert torch.equal(a, b)                     # no atomics anywhere: bitwise reproducible


def test_text_kv_cache_reuses_and_invalidates(engine_lib, tiny_unet):
    """sd_unet_text_kv_cache: inside a denoise loop the cross-attention K/V of the (constant) prompt embeddings
    are computed once; the result is bitwise the uncached one, a float timestep takes the same path as a
    tensor, and re-arming the cache picks up new contents behind the same pointer."""
    cfg, sd, net = tiny_unet
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().cuda()
    base = net(x, torch.tensor(501.0), ehs)[0]
    try:
        net.text_kv_cache(True)
        a = net(x, 501.0, ehs)[0]                 # fills the cache
        b = net(x, 501.0, ehs)[0]                 # reuses it
        assert torch.equal(a, base) and torch.equal(b, base)
        ehs.mul_(0.5)                             # new contents, same pointer
        net.text_kv_cache(True)                   # what the pipeline does at the start of every call
        c = net(x, 501.0, ehs)[0]
    finally:
        net.text_kv_cache(False)
    fresh = net(x, torch.tensor(501.0), ehs)[0]
    assert torch.equal(c, fresh) and not torch.equal(c, base)


def test_unet_batch_independence(engine_lib, tiny_unet):
    """Sharding property: a sample's result does not depend on its batch mates.
    Tile shape / split-K are picked per problem size, so a different batch size may change the fp32
    summation order: equal to fp16 rounding (rel-L2 < 1e-3), and bitwise for equal shapes."""
    cfg, sd, net = tiny_unet
    g = torch.Generator().manual_seed(6)
    x = torch.randn(4, 4, 16, 16, generator=g).half().cuda()
    ehs = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).half().cuda()
    full = net(x, torch.tensor(301.0), ehs)[0]
    lo = net(x[:2], torch.tensor(301.0), ehs[:2])[0]
    hi = net(x[2:], torch.tensor(301.0), ehs[2:])[0]
    assert rel_l2(full, torch.cat([lo, hi])) < 1e-3
    assert torch.equal(lo, net(x[:2], torch.tensor(301.0), ehs[:2])[0])
    swapped = net(torch.cat([x[2:], x[:2]]), torch.tensor(301.0), torch.cat([ehs[2:], ehs[:2]]))[0]
    assert torch.equal(full, torch.cat([swapped[2:], swapped[:2]]))     # position in the batch is irrelevant


def test_unet_sdxl_style(engine_lib):
    """Linear projections + text_time conditioning (SDXL topology features) on a small config."""
    cfg = config.tiny_unet(linear=True, sdxl_cond=True)
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=13, perturb=0.1))
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    added = {"text_embeds": torch.randn(2, 64, generator=g).half(),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)}
    ref = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(741.0), ehs.float(),
                                {"text_embeds": added["text_embeds"].float(), "time_ids": added["time_ids"]})
    got = net(x.cuda(), torch.tensor(741.0), ehs.cuda(), added_cond_kwargs=added)[0]
    assert rel_l2(got, ref) < TOL


@pytest.mark.parametrize("B,h,w", [(1, 8, 8), (2, 8, 12)])
def test_vae_decode(engine_lib, tiny_vae, B, h, w):
    cfg, sd, vae = tiny_vae
    z = torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(h * w)).half()
    ref = vae_ref.vae_decode(cfg, sd, z.float())
    got = vae.decode(z.cuda(), return_dict=False)[0]
    assert got.shape == ref.shape
    assert rel_l2(got, ref) < TOL


def test_vae_decode_65x65_latent(engine_lib, tiny_vae):
    """A 520 x 520 image: 65 x 65, 130 x 130, 260 x 260 and 520 x 520 maps, none of which a convolution tile divides, so
    every GroupNorm runs its own statistics pass -- on map sizes whose last slabs were empty before gn_slabs dropped
    them (tests/test_norm_gpu.py has the operator-level cases)."""
    cfg, sd, vae = tiny_vae
    z = torch.randn(1, 4, 65, 65, generator=torch.Generator().manual_seed(65)).half()
    ref = vae_ref.vae_decode(cfg, sd, z.float())
    got = vae.decode(z.cuda(), return_dict=False)[0]
    assert got.shape == ref.shape
    assert torch.isfinite(got.float()).all()
    assert rel_l2(got, ref) < TOL


def test_vae_encode(engine_lib, tiny_vae):
    cfg, sd, vae = tiny_vae
    img = torch.randn(2, 3, 64, 48, generator=torch.Generator().manual_seed(3)).half()
    ref = vae_ref.vae_encode_moments(cfg, sd, img.float())
    got = vae.encode_moments(img.cuda())
    assert got.shape == ref.shape
    assert rel_l2(got, ref) < TOL
    dist = vae.encode(img.cuda()).latent_dist
    assert rel_l2(dist.mode(), ref[:, :4]) < TOL


def test_state_dict_errors(engine_lib):
    cfg = config.tiny_unet()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=1)
    bad = dict(sd)
    bad.pop("conv_in.weight")
    with pytest.raises(KeyError):
        HipUNet2DConditionModel(cfg).load_state_dict(bad)
    bad = dict(sd)
    bad["conv_in.weight"] = torch.zeros(64, 4, 3, 2)
    with pytest.raises(ValueError):
        HipUNet2DConditionModel(cfg).load_state_dict(bad)
    net = HipUNet2DConditionModel(cfg)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 4, 16, 16), 1.0, torch.zeros(1, 77, 64))    # forward before weights
    net.load_state_dict(sd)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 4, 12, 12), 1.0, torch.zeros(1, 77, 64))    # 12 not divisible by 8


# ---------------------------------------------------------------------------------------------
# committed golden vectors (tests/golden/tiny_sd.npz, produced by tests/golden/make_golden.py)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    import importlib.util
    import os

    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    ucfg, vcfg, uw, vw = mg.golden_weights()
    data = np.load(os.path.join(here, "golden", "tiny_sd.npz"))
    d = {k: torch.from_numpy(np.asarray(data[k])) for k in data.files}
    return ucfg, vcfg, uw, vw, d


def test_engine_against_golden_vectors(engine_lib, golden):
    ucfg, vcfg, uw, vw, d = golden
    unet = HipUNet2DConditionModel(ucfg).load_state_dict(uw)
    vae = HipAutoencoderKL(vcfg).load_state_dict(vw)
    y = unet(d["unet_x"].cuda(), d["unet_t"], d["unet_ehs"].cuda())[0]
    assert rel_l2(y, d["unet_y"]) < TOL
    assert rel_l2(vae.decode(d["vae_z"].cuda())[0], d["vae_img"]) < TOL
    assert rel_l2(vae.encode_moments(d["vae_pix"].cuda()), d["vae_moments"]) < TOL


def test_pipeline_end_to_end_against_golden(engine_lib, golden):
    """4-step DDIM + decode through StableDiffusionUnifiedPipeline.__call__ with the HIP engine in
    the .base / .vae slots, latents injected via `latents=` (sd_unified_pipeline.py:152,782-783).
    Tolerances: latents / image rel-L2 <= 1e-2; per-pixel in the uint8 domain of
    handler_logic.py:21-29: mean abs <= 1.0 level, 99.9 % of pixels within 4 levels."""
    import numpy as np
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg, uw, vw, d = golden
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(uw),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vw), scheduler=DDIMScheduler(), device="cuda")
    neg, pos = d["pipe_embeds2b"][:1].half(), d["pipe_embeds2b"][1:].half()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda")
    images = pipe(model, prompt_embeds=pos, negative_prompt_embeds=neg, latents=d["pipe_latents0"].half(),
                  num_inference_steps=4, guidance_scale=5.0, height=64, width=64)
    assert images.shape == (1, 3, 64, 64) and images.dtype == torch.float16
    assert rel_l2(images, d["pipe_images"]) < TOL
    u8 = pipeline_ref.to_uint8_hwc(images.float().cpu())
    diff = np.abs(u8.astype(int) - d["pipe_uint8"].numpy().astype(int))
    assert diff.mean() <= 1.0 and (diff <= 4).mean() >= 0.999
    lat_pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    lat = lat_pipe(model, prompt_embeds=pos, negative_prompt_embeds=neg, latents=d["pipe_latents0"].half(),
                   num_inference_steps=4, guidance_scale=5.0, height=64, width=64)
    assert rel_l2(lat, d["pipe_latents"]) < TOL


def test_cfg_duplicate_and_linear_step_as_ddim(engine_lib):
    """sd_cfg_duplicate, and sd_cfg_linear_step without a history (the DDIM form), against the host scheduler arithmetic."""
    import ctypes as C
    from stablediffusion_amd.schedulers import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(50)
    g = torch.Generator().manual_seed(2)
    lat = torch.randn(4, 4, 16, 16, generator=g).half().cuda()
    eps = torch.randn(8, 4, 16, 16, generator=g).half().cuda()
    dup = torch.empty(8, 4, 16, 16, dtype=torch.float16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert engine_lib.sd_cfg_duplicate(C.c_void_p(lat.data_ptr()), C.c_void_p(dup.data_ptr()), 4 * 16 * 16, 4, 1.0, st) == 0
    assert torch.equal(dup, torch.cat([lat, lat]))
    eu, et = eps.float().chunk(2)
    noise = (5.0 * (et - eu) + eu).half()
    ref = s.step(noise, 501, lat)[0]
    cx, ce = s.step_coefficients(501)
    out = lat.clone()
    assert engine_lib.sd_cfg_linear_step(C.c_void_p(eps.data_ptr()), C.c_void_p(out.data_ptr()), None, lat.numel(), 5.0, cx, ce,
                                         0.0, 0.0, 0.0, st) == 0
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < 1e-3


def test_images_to_uint8_matches_reference_op_sequence(engine_lib):
    """sd_images_to_uint8 / convert_pt_to_numpy: bit-exact with the reference's own op sequence
    (handler_logic.py:21-29) applied to the same fp16 tensor, including out-of-range and boundary values."""
    from stablediffusion_amd.pipeline import convert_pt_to_numpy
    g = torch.Generator().manual_seed(9)
    img = (torch.randn(3, 3, 37, 53, generator=g) * 0.9).half()
    img[0, 0, 0, :8] = torch.tensor([-1.0, 1.0, 0.0, 0.99951171875, -0.99951171875, 2.5, -3.0, 0.0039], dtype=torch.float16)
    dev = img.cuda()
    got = convert_pt_to_numpy(dev)
    for idx in range(3):
        ref = ((dev[idx] / 2 + 0.5).clamp(0, 1).permute(1, 2, 0) * 255).to(torch.uint8).cpu().numpy()
        assert got[idx].shape == (37, 53, 3) and got[idx].dtype == ref.dtype
        assert (got[idx] == ref).all()
    cpu = convert_pt_to_numpy(img)          # host tensors: the op sequence itself
    assert all((a == b).all() for a, b in zip(cpu, got))


def test_cfg_linear_step_kernel(engine_lib):
    """sd_cfg_linear_step (DPM++ 2M form: history read and replaced) against the same formula in torch."""
    import ctypes as C
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    eps = torch.randn(4, 4, 16, 16, generator=g).half().cuda()
    hist = torch.randn(2, 4, 16, 16, generator=g).cuda()
    cx, ce, ch, hx, he, gs = 0.93, -0.21, 0.07, 1.8, -1.5, 7.5
    eu, et = eps.float().chunk(2)
    e = (gs * (et - eu) + eu).half().float()
    ref = cx * lat.float() + ce * e + ch * hist
    ref_hist = hx * lat.float() + he * e
    out, h2 = lat.clone(), hist.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert engine_lib.sd_cfg_linear_step(C.c_void_p(eps.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(h2.data_ptr()),
                                         lat.numel(), gs, cx, ce, ch, hx, he, st) == 0
    torch.cuda.synchronize()
    assert rel_l2(out, ref) < 1e-3 and rel_l2(h2, ref_hist) < 1e-5
    out2 = lat.clone()                     # no history: DDIM / Euler form
    assert engine_lib.sd_cfg_linear_step(C.c_void_p(eps.data_ptr()), C.c_void_p(out2.data_ptr()), None,
                                         lat.numel(), gs, cx, ce, ch, hx, he, st) == 0
    torch.cuda.synchronize()
    assert rel_l2(out2, cx * lat.float() + ce * e) < 1e-3


@pytest.mark.parametrize("sched", ["DDIM", "DPM++ 2M", "euler"])
def test_fused_device_step_equals_host_scheduler_loop(engine_lib, sched):
    """The loop with CFG + scheduler update fused on the device (sd_cfg_duplicate / sd_cfg_linear_step)
    against the same engine driven through scheduler.scale_model_input / .step on the host."""
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler(sched)
    g = torch.Generator().manual_seed(3)
    pos = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=6, guidance_scale=5.0,
              height=128, width=128)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    fused = pipe(model, **kw)
    assert pipe._fused_step_available(model, lat0)
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    host_pipe._fused_step_available = lambda *a: False
    host = host_pipe(model, **kw)
    assert torch.isfinite(fused.float()).all()
    assert rel_l2(fused, host) < 3e-3


@pytest.mark.parametrize("sched", ["DDIM", "euler"])
def test_inpaint_device_blend_equals_host_loop(engine_lib, sched):
    """4-channel inpainting (sd_unified_pipeline.py:268-380, :492-506) with the per-step mask blend on the
    device (sd_inpaint_blend) against the same engine driven through the host torch blend; outside the
    mask the result is the encoded original."""
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler(sched)
    g = torch.Generator().manual_seed(4)
    pos = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(1, 7, ucfg.cross_attention_dim, generator=g).half().cuda()
    image = torch.randn(1, 3, 128, 128, generator=g).clamp(-1, 1).half().cuda()
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, image=image, mask_image=mask.cuda(), num_inference_steps=4,
              seed=2, guidance_scale=5.0)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    fused = pipe(model, **kw)
    assert pipe._fused_step_available(model, fused, 4)
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    host_pipe._fused_step_available = lambda *a: False
    host = host_pipe(model, **kw)
    assert torch.isfinite(fused.float()).all() and rel_l2(fused, host) < 3e-3
    w = fused.shape[-1]
    assert torch.allclose(fused[..., : w // 2].float(), host[..., : w // 2].float(), atol=2e-3)   # kept region
    assert not torch.allclose(fused[..., w // 2:].float(), fused[..., : w // 2].float().flip(-1), atol=1e-2)


# ---------------------------------------------------------------------------------------------
# full-size SD1.5 (BASELINE.json config C1: 256x256, 10-step DDIM, batch 1, CFG on)
# ---------------------------------------------------------------------------------------------
def test_sd15_full_size_c1_against_oracle(engine_lib):
    """The real SD1.5 topology and widths (859.5 M-parameter UNet, 83.7 M VAE) with seeded synthetic
    weights: one UNet forward, the 10-step DDIM latents and the decoded image against the fp32 CPU
    oracle on identical fp16-rounded weights / inputs.  Tolerance: rel-L2 <= 1e-2 (BASELINE.json)."""
    import os

    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ucfg, vcfg = config.sd15_unet(), config.sd15_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=21, dtype=torch.float16)
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=22, dtype=torch.float16)
    unet = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    vae = HipAutoencoderKL(vcfg).load_state_dict(vsd)
    uw = {k: v.float() for k, v in usd.items()}
    vw = {k: v.float() for k, v in vsd.items()}
    g = torch.Generator().manual_seed(77)
    lat0 = torch.randn(1, 4, 32, 32, generator=g).half()
    emb2 = torch.randn(2, 77, 768, generator=g).half()          # [negative ; positive]
    # (1) single forward at CFG batch 2
    x2 = torch.cat([lat0, lat0])
    with torch.no_grad():
        ref = unet_ref.unet_forward(ucfg, uw, x2.float(), torch.tensor(901.0), emb2.float())
    got = unet(x2.cuda(), torch.tensor(901.0), emb2.cuda())[0]
    assert rel_l2(got, ref) < TOL
    # (2) 10-step DDIM + decode through the pipeline surface
    model = SDModelWrapper(base=unet, vae=vae, scheduler=DDIMScheduler(), device="cuda")
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda")
    images = pipe(model, prompt_embeds=emb2[1:], negative_prompt_embeds=emb2[:1], latents=lat0,
                  num_inference_steps=10, guidance_scale=5.0, height=256, width=256)
    with torch.no_grad():
        ref_img, ref_lat = pipeline_ref.txt2img_ref(ucfg, uw, vcfg, vw, lat0.float(), emb2.float(), steps=10,
                                                    guidance_scale=5.0)
    assert images.shape == (1, 3, 256, 256)
    assert torch.isfinite(images.float()).all()
    assert rel_l2(images, ref_img) < TOL


def test_sdxl_full_size_unet_forward(engine_lib):
    """SDXL-base UNet (2.57 B parameters: linear projections, depth-2/10 transformer stacks, head dim 64,
    text_time conditioning) at a reduced spatial size against the fp32 CPU oracle."""
    import os
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ucfg = config.sdxl_unet()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=31, dtype=torch.float16)
    unet = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 32, 32, generator=g).half()
    ehs = torch.randn(2, 77, 2048, generator=g).half()
    added = {"text_embeds": torch.randn(2, 1280, generator=g).half(),
             "time_ids": torch.tensor([[256.0, 256, 0, 0, 256, 256]] * 2)}
    got = unet(x.cuda(), torch.tensor(621.0), ehs.cuda(), added_cond_kwargs=added)[0]
    uw = {k: v.float() for k, v in usd.items()}
    del usd
    with torch.no_grad():
        ref = unet_ref.unet_forward(ucfg, uw, x.float(), torch.tensor(621.0), ehs.float(),
                                    {"text_embeds": added["text_embeds"].float(), "time_ids": added["time_ids"]})
    assert rel_l2(got, ref) < TOL


def test_img2img_with_fused_lora_against_oracle(engine_lib):
    """BASELINE.json config C5 in miniature: LoRA (r=16, alpha=r, on to_q/to_k/to_v/to_out.0 as the
    reference trainer writes it, train_lora_pipeline.py:247-252) fused on the host, then the img2img
    branch of the pipeline (4-channel latents passed as `image`, `denoising_start` so no device-side
    noise is drawn) through the HIP engine vs the same pipeline code on oracle-backed doubles."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from doubles import OracleUNet, OracleVAE
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    base = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=41, perturb=0.1)
    g = torch.Generator().manual_seed(3)
    lora = {}
    for k, w in base.items():
        if k.endswith(("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight")):
            mod = k[: -len(".weight")]
            lora[f"unet.{mod}.lora.down.weight"] = torch.randn(16, w.shape[1], generator=g) * 0.05
            lora[f"unet.{mod}.lora.up.weight"] = torch.randn(w.shape[0], 16, generator=g) * 0.05
    fused = _f16_round(weights.fuse_lora(base, lora, adapter_weight=0.8))
    assert not torch.equal(fused["mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight"],
                           base["mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight"].half().float())
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), seed=42, perturb=0.1))
    init = torch.randn(2, 4, 8, 8, generator=g).half()
    pos = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(2, 77, ucfg.cross_attention_dim, generator=g).half()
    kw = dict(num_inference_steps=6, guidance_scale=4.0, denoising_start=0.5, strength=1.0)
    gpu_model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(fused),
                               vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    got = StableDiffusionUnifiedPipeline(True, "cuda", "latents")(
        gpu_model, prompt_embeds=pos, negative_prompt_embeds=neg, image=init, **kw)
    cpu_model = SDModelWrapper(base=OracleUNet(ucfg, fused), vae=OracleVAE(vcfg, vsd), scheduler=DDIMScheduler(),
                               device="cpu")
    ref = StableDiffusionUnifiedPipeline(True, "cpu", "latents")(
        cpu_model, prompt_embeds=pos.float(), negative_prompt_embeds=neg.float(), image=init.float(), **kw)
    assert got.shape == ref.shape == (2, 4, 8, 8)
    assert rel_l2(got, ref) < TOL
    # and the pixel-space img2img branch runs end to end on the engine (VAE encode -> noise -> loop -> decode)
    img = torch.randn(2, 3, 64, 64, generator=g).clamp(-1, 1).half()
    out = StableDiffusionUnifiedPipeline(True, "cuda")(gpu_model, prompt_embeds=pos, negative_prompt_embeds=neg,
                                                       image=img, strength=0.5, num_inference_steps=4, seed=7)
    assert out.shape == (2, 3, 64, 64) and torch.isfinite(out.float()).all()


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (5, 8, 16), (2, 40, 24), (7, 16, 8), (16, 8, 8)])
def test_unet_shape_sweep(engine_lib, tiny_unet, B, H, W):
    """Ragged batches / non-square latents: every tile variant's edge handling through the full graph
    (shapes outside the tuned table use the heuristic tile choice)."""
    cfg, sd, net = tiny_unet
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    t = torch.rand(B, generator=g) * 999
    ref = unet_ref.unet_forward(cfg, sd, x.float(), t, ehs.float())
    got = net(x.cuda(), t, ehs.cuda())[0]
    assert rel_l2(got, ref) < TOL


def test_sd15_full_size_odd_shapes_are_finite_and_deterministic(engine_lib):
    """Full-width SD1.5 UNet at shapes that are in no tuned table (batch 3, 40x56 latents; batch 1,
    96x96 = the C5 resolution): finite, deterministic, and a workspace re-plan between shapes."""
    ucfg = config.sd15_unet()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=51, dtype=torch.float16)
    unet = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    g = torch.Generator().manual_seed(1)
    for (B, H, W) in [(3, 40, 56), (1, 96, 96), (3, 40, 56)]:
        x = torch.randn(B, 4, H, W, generator=g).half().cuda()
        ehs = torch.randn(B, 77, 768, generator=g).half().cuda()
        a = unet(x, torch.tensor(500.0), ehs)[0]
        b = unet(x, torch.tensor(500.0), ehs)[0]
        assert a.shape == (B, 4, H, W) and torch.isfinite(a.float()).all()
        assert torch.equal(a, b)
        assert 0.05 < a.float().std().item() < 20.0


def test_unet_hipgraph_replay_is_bitwise_eager(engine_lib):
    """sd_unet_use_graph: captured-graph replay (staged I/O, event fences) == eager launches, across
    repeated calls with fresh tensors, a shape change (re-capture) and back."""
    cfg = config.tiny_unet()
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=61, perturb=0.1))
    eager = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    graph = HipUNet2DConditionModel(cfg).load_state_dict(sd).use_graph(True)
    g = torch.Generator().manual_seed(4)
    for (B, H, W) in [(2, 16, 16), (2, 16, 16), (2, 16, 16), (4, 8, 8), (2, 16, 16)]:
        x = torch.randn(B, 4, H, W, generator=g).half().cuda()
        ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half().cuda()
        t = torch.rand(B, generator=g) * 999
        a = eager(x, t, ehs)[0]
        b = graph(x.clone(), t.clone(), ehs.clone())[0]
        assert torch.equal(a, b), (B, H, W)
    # the first call, the shape change and the way back capture (one graph per handle); the other two replay
    assert graph.graph_stats() == (3, 2) and eager.graph_stats() == (0, 0)
