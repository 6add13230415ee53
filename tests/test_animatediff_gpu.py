"""`animate` on the engine: the tiny model with the tiny motion adapter, three steps of DDIM, Euler and LCM against a host
loop over tests/motion_oracle.py, the seed and noise layout, the chunked decode, the refusals, and the adapter surviving a
rebuild of the UNet."""
import pytest
import torch

import motion_oracle
from conftest import rel_l2
from stablediffusion_amd import animatediff, config, motion, weights
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

pytestmark = pytest.mark.gpu

LOOP_TOL = 3e-3     # the bound of the existing loop tests on the tiny model (tests/test_sched_step_gpu.py)
V, F, HW = 2, 3, 16


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def world():
    from types import SimpleNamespace
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    mcfg = motion.tiny_motion_adapter(ucfg)
    msd = motion.synth_state_dict(mcfg, 3)
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd), vae=HipAutoencoderKL(vcfg).load_state_dict(vsd),
                           device="cuda", unet_state_dict=usd)
    model.load_motion_adapter(dict(msd), config=mcfg)
    g = torch.Generator().manual_seed(3)
    pos, neg = (torch.randn(V, 7, ucfg.cross_attention_dim, generator=g).half() for _ in range(2))
    z = torch.randn(V, 4, F, HW, HW, generator=g).half()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="pt")
    return SimpleNamespace(ucfg=ucfg, usd=usd, mcfg=mcfg, msd=msd, model=model, pos=pos, neg=neg, z=z, pipe=pipe)


def _kw(w, **over):
    kw = dict(prompt_embeds=w.pos.cuda(), negative_prompt_embeds=w.neg.cuda(), num_frames=F, height=8 * HW, width=8 * HW,
              num_inference_steps=3, guidance_scale=4.0, output_type="latents")
    kw.update(over)
    return kw


def oracle_loop(w, name, seed):
    """AnimateDiffPipeline's loop in float on the CPU over motion_oracle; LCM's step noise from the device generator the
    pipeline seeds."""
    w.model.set_scheduler(name)
    sch = w.model.scheduler
    sch.set_timesteps(3, device="cpu")
    x = w.z.float().permute(0, 2, 1, 3, 4).reshape(V * F, 4, HW, HW) * float(sch.init_noise_sigma)
    ehs = torch.cat([w.neg.float().repeat_interleave(F, 0), w.pos.float().repeat_interleave(F, 0)])
    lcm = name == "lcm"
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ts = [float(t) for t in sch.timesteps.tolist()]
    with torch.no_grad():
        for t in ts:
            noise = None
            if lcm and t != ts[-1]:
                noise = torch.randn(x.shape, dtype=torch.float16, device="cuda", generator=gen).float().cpu()
            xin = sch.scale_model_input(torch.cat([x] * 2), t)
            u, c = motion_oracle.forward(w.ucfg, w.usd, w.mcfg, w.msd, xin, t, ehs, F).chunk(2)
            eps = 4.0 * (c - u) + u
            x = sch.step(eps, t, x, noise=noise, return_dict=False)[0] if lcm else sch.step(eps, t, x, return_dict=False)[0]
    return x.reshape(V, F, 4, HW, HW)


@pytest.mark.parametrize("name", ("DDIM", "euler", "lcm"))
def test_animate_equals_the_oracle_loop(engine_lib, world, name):
    w = world
    want = oracle_loop(w, name, 9)
    w.model.set_scheduler(name)
    used = []
    real = w.pipe._device_iteration
    w.pipe._device_iteration = lambda *a, **k: (used.append(1), real(*a, **k))[1]
    try:
        got = animatediff.animate(w.pipe, w.model, None, latents=w.z, seed=9, **_kw(w))
    finally:
        w.pipe._device_iteration = real
    assert len(used) == 3                                # the existing device step ran on every iteration
    assert got.shape == (V, F, 4, HW, HW) and torch.isfinite(got.float()).all()
    e = rel_l2(got, want)
    print("animate %s: rel-L2 %.2e against the oracle loop (bound %.0e)" % (name, e, LOOP_TOL))
    assert e < LOOP_TOL


def test_seed_and_noise_layout(engine_lib, world):
    w = world
    w.model.set_scheduler("DDIM")
    a, b, c = (animatediff.animate(w.pipe, w.model, None, seed=s, **_kw(w)) for s in (5, 5, 6))
    assert torch.equal(a, b) and rel_l2(c, a) > 0.1
    z = torch.randn((V, 4, F, HW, HW), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.float16)
    assert torch.equal(animatediff.animate(w.pipe, w.model, None, latents=z, **_kw(w)), a)


def test_decode_chunk_size_and_frames(engine_lib, world):
    w = world
    w.model.set_scheduler("DDIM")
    kw = _kw(w, output_type="pt", num_inference_steps=1, latents=w.z)
    frames = [animatediff.animate(w.pipe, w.model, None, decode_chunk_size=n, **kw).float().cpu() for n in (1, 4, 8)]
    assert frames[0].shape == (V, F, 3, 8 * HW, 8 * HW) and torch.isfinite(frames[0]).all()
    # (the engine plans a decode per batch size: another tile sums in another order and the fp16 tensors in between differ
    # by their storage rounding, 2^-11; a frame in the wrong place is O(1))
    for f in frames[1:]:
        e = rel_l2(f, frames[0])
        print("decode_chunk_size: rel-L2 %.2e" % e)
        assert e <= 2e-3


def test_refusals_leave_the_wrapper_untouched(engine_lib, world):
    w = world
    w.model.set_scheduler("DDIM")
    first = animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w))
    adapter = w.model.base.motion_adapter
    for on, off, match in ((lambda: w.model.enable_tome(0.5), w.model.disable_tome, "token merging"),
                           (lambda: w.model.enable_hypertile(8), w.model.disable_hypertile, "HyperTile"),
                           (lambda: w.model.enable_deepcache(2, 1), w.model.disable_deepcache, "DeepCache"),
                           (lambda: w.model.base.use_graph(True), lambda: w.model.base.use_graph(False), "graph replay")):
        on()
        try:
            with pytest.raises(NotImplementedError, match=match):
                animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w))
            assert w.model.base.motion_adapter is adapter and w.model.has_motion_adapter
        finally:
            off()
    with pytest.raises(ValueError, match="num_frames"):
        animatediff.animate(w.pipe, w.model, None, **_kw(w, num_frames=33))
    assert torch.equal(animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w)), first)


def test_adapter_survives_a_rebuild_and_unload(engine_lib, world):
    w = world
    w.model.set_scheduler("DDIM")
    first = animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w))
    # what a LoRA re-fuse does (apply_adapters -> _rebuild_from): the old engine goes, the new one gets an adapter packed
    # from the state dict the wrapper keeps -- once
    w.model._base_factory = w.model.base.rebuild_factory()
    w.model.base = None
    w.model.base = w.model._rebuild_from(w.usd, False)
    assert w.model.base.motion_adapter is not None
    assert torch.equal(animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w)), first)
    w.model.unload_motion_adapter()
    with pytest.raises(ValueError, match="load_motion_adapter"):
        animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w))
    w.model.load_motion_adapter(dict(w.msd), config=w.mcfg)
    assert torch.equal(animatediff.animate(w.pipe, w.model, None, latents=w.z, **_kw(w)), first)
