"""Regional prompts on the host (no GPU): the weights of stablediffusion_amd.regions, the pipeline's layout and
refusals on oracle doubles (tests/region_oracle.py), and that the inputs the GPU suite runs tell the regional forward
from the plain forward on the base prompt."""
import pytest
import torch
import torch.nn.functional as F

import region_oracle as ro
from conftest import rel_l2
from oracle import unet_ref
from stablediffusion_amd import config, regions, schedulers, weights
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


# ---------------------------------------------------------------------------------------------- region_weights
def test_weights_sum_to_one_and_disjoint_masks_are_one_hot():
    m = torch.zeros(2, 32, 48)
    m[0, :, :16] = 1.0
    m[1, :, 32:] = 1.0
    w = regions.region_weights(m, 32, 48)
    assert w.shape == (3, 32, 48) and w.dtype == torch.float32
    assert torch.equal(w.sum(0), torch.ones(32, 48))
    assert torch.equal(w[1], m[0]) and torch.equal(w[2], m[1])
    assert torch.equal(w[0, :, 16:32], torch.ones(32, 16)) and w[0, :, :16].abs().max() == 0
    assert torch.equal(regions.region_weights(m[:, None], 32, 48), w)           # [R-1, 1, H, W] alike


def test_base_weight_keeps_the_base_prompt_everywhere():
    m = torch.zeros(1, 8, 8)
    m[0, :, :4] = 1.0
    w = regions.region_weights(m, 8, 8, base_weight=0.5)
    assert torch.allclose(w[0, :, :4], torch.full((8, 4), 0.5 / 1.5)) and torch.allclose(w[1, :, :4], torch.full((8, 4), 1 / 1.5))
    assert torch.equal(w[0, :, 4:], torch.ones(8, 4)) and torch.equal(w[1, :, 4:], torch.zeros(8, 4))
    assert torch.allclose(w.sum(0), torch.ones(8, 8), atol=1e-6)


def test_overlapping_and_out_of_range_masks():
    m = torch.zeros(2, 4, 4)
    m[0] = 0.75
    m[1, :2] = 0.75                      # overlap: the masks alone sum to 1.5 there, the base gets nothing
    m[1, 3] = 7.0                        # clamped to 1
    w = regions.region_weights(m, 4, 4)
    assert torch.allclose(w.sum(0), torch.ones(4, 4), atol=1e-6)
    assert torch.allclose(w[:, 0, 0], torch.tensor([0.0, 0.5, 0.5]))
    assert torch.allclose(w[:, 2, 0], torch.tensor([0.25, 0.75, 0.0]))
    assert torch.allclose(w[:, 3, 0], torch.tensor([0.0, 0.75 / 1.75, 1.0 / 1.75]))
    assert (w >= 0).all()


def test_masks_are_resized_with_nearest():
    g = torch.Generator().manual_seed(0)
    m = (torch.rand(2, 64, 96, generator=g) > 0.5).float()
    w = regions.region_weights(m, 8, 12)
    near = F.interpolate(m[:, None], size=(8, 12), mode="nearest")[:, 0]
    m0 = (1 - near.sum(0)).clamp(0, 1)
    want = torch.cat([m0[None], near]) / (m0 + near.sum(0))
    assert torch.allclose(w, want)
    assert torch.equal(near, m[:, ::8, ::8])                                   # what "nearest" means here


def test_bad_weight_arguments():
    m = torch.zeros(1, 8, 8)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            regions.region_weights(m, 8, 8, bad)
    with pytest.raises(ValueError):
        regions.region_weights(torch.zeros(8, 8), 8, 8)
    with pytest.raises(ValueError):
        regions.region_weights(torch.zeros(8, 8, 8), 8, 8)                      # eight masks: nine regions
    with pytest.raises(ValueError):
        regions.region_weights(torch.zeros(1, 2, 8, 8), 8, 8)


def test_level_weights_are_the_average_pool_and_keep_the_sum():
    w = ro.stripe_weights(2, 3, 16, 24)
    for lvl in range(4):
        got = regions.level_weights(w, lvl)
        want = F.avg_pool2d(w, 1 << lvl) if lvl else w                          # every halving is exact: one block mean
        assert got.shape == (2, 3, 16 >> lvl, 24 >> lvl)
        assert torch.allclose(got, want, atol=1e-7)
        assert torch.allclose(got.sum(1), torch.ones_like(got[:, 0]), atol=1e-6)
        assert torch.equal(ro.weights_at(w, (16 >> lvl) * (24 >> lvl)), got.flatten(2))
    mixed = regions.level_weights(w, 1)
    assert ((mixed > 0) & (mixed < 1)).any()                                    # the stripes' edges are off the 2x2 grid


def test_batch_weights_layout():
    w = regions.region_weights(torch.ones(2, 4, 4) * 0.25, 4, 4)
    b = regions.batch_weights(w, 3, True)
    assert b.shape == (6, 3, 4, 4)
    assert torch.equal(b[:3, 0], torch.ones(3, 4, 4)) and b[:3, 1:].abs().max() == 0
    assert all(torch.equal(b[3 + i], w) for i in range(3))
    assert torch.equal(regions.batch_weights(w, 2, False), torch.stack([w, w]))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_with_one_region_is_the_plain_attention():
    cfg = config.tiny_unet()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), 1, perturb=0.1)
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, 1, seed=3)
    got = ro.forward(cfg, sd, x, torch.tensor(500.0), ehs, torch.ones(1, 1, 16, 16))
    with torch.no_grad():
        want = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(500.0), ehs.float())
    assert rel_l2(got, want) < 1e-5


def test_oracle_one_hot_rows_see_their_own_prompt_only():
    """A row whose weights are one-hot on region r everywhere equals the plain forward on prompt r."""
    cfg = config.tiny_unet()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), 1, perturb=0.1)
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, 3, seed=4)
    w = torch.zeros(2, 3, 16, 16)
    w[0, 2] = 1.0
    w[1, 1] = 1.0
    got = ro.forward(cfg, sd, x, torch.tensor(300.0), ehs, w)
    with torch.no_grad():
        picked = torch.stack([ehs[0, 2 * 77:], ehs[1, 77:2 * 77]]).float()
        want = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(300.0), picked)
    assert rel_l2(got, want) < 1e-5


GPU_INPUTS = [("tiny", dict(), 16, 16), ("tiny", dict(), 8, 24), ("tiny-xl", dict(linear=True, sdxl_cond=True), 16, 16),
              ("tiny-xl", dict(linear=True, sdxl_cond=True), 8, 24)]


@pytest.mark.parametrize("name,kw,h,w", GPU_INPUTS, ids=["%s-%dx%d" % (n, h, w) for n, _, h, w in GPU_INPUTS])
def test_gpu_inputs_tell_regions_from_the_base_prompt(name, kw, h, w):
    """For the inputs tests/test_regions_gpu.py runs: the oracle with regions is more than 5e-2 (rel-L2) away from the
    oracle on the base prompt alone, so a forward that ignored the regions could not pass there."""
    cfg = config.tiny_unet(**kw)
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), 1, perturb=0.1).items()}
    x, ehs = ro.unet_inputs(cfg, 2, h, w, 3, seed=11)
    cond = ro.sdxl_cond(cfg, 2, 5) if kw else None
    cond32 = None if cond is None else {k: v.float() for k, v in cond.items()}
    reg = ro.forward(cfg, sd, x, torch.tensor(981.0), ehs, ro.stripe_weights(2, 3, h, w), cond32)
    with torch.no_grad():
        base = unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(981.0), ehs[:, :77].float(), cond32)
    dist = rel_l2(reg, base)
    print("%s %dx%d: regional vs base prompt rel-L2 %.3f" % (name, h, w, dist))
    assert dist > 5e-2


# ---------------------------------------------------------------------------------------------- the pipeline
def _model(region=True, cfg=None):
    from doubles import OracleUNet, OracleVAE
    ucfg, vcfg = cfg or config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    base = ro.RegionOracleUNet(ucfg, uw) if region else OracleUNet(ucfg, uw)
    return SDModelWrapper(base=base, vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(), device="cpu",
                          unet_state_dict=uw)


def _embeds(B, R, seed=0):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 4, 8, 8, generator=g)
    pe = torch.randn(B, 77, 64, generator=g) * 2
    ne = torch.randn(B, 77, 64, generator=g)
    re = [torch.randn(B, 77, 64, generator=g) * 2 for _ in range(R - 1)]
    masks = torch.zeros(R - 1, 64, 64)
    for r in range(R - 1):
        masks[r, :, 16 * r + 8:16 * r + 24] = 1.0
    return lat, pe, ne, re, masks


def _kw(lat, pe, ne):
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64)


def test_pipeline_layout_uncond_rows_and_cleanup():
    B, R = 2, 3
    lat, pe, ne, re, masks = _embeds(B, R)
    m = _model()
    type(m.base).calls.clear()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    out = pipe(m, region_prompt_embeds=re, region_masks=masks, region_base_weight=0.25, **_kw(lat, pe, ne))
    calls = type(m.base).calls
    assert len(calls) == 2 and m.base.history == [("set", (2 * B, R, 8, 8)), ("clear",)] and m.base.weights is None
    ehs, w = calls[0]["ehs"], calls[0]["weights"]
    assert ehs.shape == (2 * B, R * 77, 64)
    assert torch.equal(ehs[B:, :77], pe) and all(torch.equal(ehs[B:, 77 * (r + 1):77 * (r + 2)], re[r]) for r in range(R - 1))
    assert all(torch.equal(ehs[:B, 77 * r:77 * (r + 1)], ne) for r in range(R))     # the negative repeats per segment
    assert torch.equal(w[:B, 0], torch.ones(B, 8, 8)) and w[:B, 1:].abs().max() == 0   # uncond rows: one-hot on region 0
    want = regions.region_weights(masks, 8, 8, 0.25)
    assert all(torch.equal(w[B + i], want) for i in range(B))
    plain = pipe(m, **_kw(lat, pe, ne))
    assert type(m.base).calls[-1]["weights"] is None and type(m.base).calls[-1]["ehs"].shape[1] == 77
    assert not torch.allclose(out, plain, atol=1e-3)
    # [R-1, 1, H, W] masks and no CFG
    nocfg = StableDiffusionUnifiedPipeline(do_cfg=False, device="cpu")
    m.base.history.clear()
    nocfg(m, region_prompt_embeds=re, region_masks=masks[:, None], prompt_embeds=pe, latents=lat, num_inference_steps=1,
          height=64, width=64)
    assert m.base.history == [("set", (B, R, 8, 8)), ("clear",)]
    assert type(m.base).calls[-1]["ehs"].shape == (B, R * 77, 64)


def test_pipeline_matches_the_reference_loop_with_the_patched_attention():
    from oracle import pipeline_ref
    B, R = 2, 3
    lat, pe, ne, re, masks = _embeds(B, R, seed=2)
    m = _model()
    m.set_scheduler("DDIM")
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    got = pipe(m, region_prompt_embeds=re, region_masks=masks, guidance_scale=5.0, **_kw(lat, pe, ne))
    w = regions.batch_weights(regions.region_weights(masks, 8, 8), B, True)
    ehs = torch.cat([torch.cat([ne] * R, 1), torch.cat([pe] + re, 1)])
    with ro.patched():
        want = pipeline_ref.denoise_ref(m.base.cfg, m.base.sd, lat, (ehs, w), 2, 5.0, "DDIM")
    assert rel_l2(got, want) < 1e-4


def test_clear_happens_when_the_loop_raises():
    lat, pe, ne, re, masks = _embeds(1, 2)
    m = _model()

    def boom(*a, **k):
        raise RuntimeError("forward failed")
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    pipe._denoise = boom
    with pytest.raises(RuntimeError):
        pipe(m, region_prompt_embeds=re, region_masks=masks, **_kw(lat, pe, ne))
    assert m.base.history[-1] == ("clear",) and m.base.weights is None


def test_rejected_combinations_raise_before_a_forward():
    lat, pe, ne, re, masks = _embeds(1, 3)
    m = _model()
    calls = type(m.base).calls
    calls.clear()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    ok = dict(region_prompt_embeds=re, region_masks=masks, **_kw(lat, pe, ne))

    def refused(exc, **over):
        with pytest.raises(exc):
            pipe(m, **{**ok, **over})
        assert not calls and not m.base.history

    # ValueError: arguments that contradict each other
    refused(ValueError, region_masks=masks[:1])                                  # two prompts, one mask
    refused(ValueError, region_prompt_embeds=re * 4, region_masks=torch.zeros(8, 64, 64))     # more than 7 region prompts
    refused(ValueError, region_base_weight=-0.5)
    refused(ValueError, region_masks=None)
    refused(ValueError, region_prompt_embeds=None, region_prompts="a cat")
    refused(ValueError, region_masks=torch.zeros(64, 64))
    # NotImplementedError: what regional prompts do not compose with
    refused(NotImplementedError, region_prompt_embeds=None, region_prompts=["a cat", "a dog"])      # prompt_embeds= without region embeds
    refused(NotImplementedError, ip_adapter_image_embeds=[torch.zeros(2, 1, 64)])
    refused(NotImplementedError, pag_scale=1.0)
    refused(NotImplementedError, view_window=8)
    refused(NotImplementedError, use_refiner=True)
    refused(NotImplementedError, refiner_start=0.5)
    refused(NotImplementedError, control_image=torch.zeros(1, 3, 64, 64))
    for attr, val in (("deepcache", (3, 1)), ("tome", (0.5, 1, 2, 2, True, 0)), ("_graph_on", True), ("_ip", object())):
        setattr(m.base, attr, val)
        try:
            refused(NotImplementedError)
        finally:
            delattr(m.base, attr)
    m._cn = (None, {})                   # what load_controlnet leaves: has_controlnet is True
    try:
        refused(NotImplementedError)
    finally:
        m._cn = None
    for cfg in (config.tiny_unet(time_cond=32),):
        mm = _model(cfg=cfg)
        with pytest.raises(NotImplementedError):
            pipe(mm, **ok)
        assert not mm.base.history
    for ch in (8, 9):
        m.base.config.in_channels = ch
        try:
            refused(NotImplementedError)
        finally:
            m.base.config.in_channels = 4
    # a UNet object without set_regions (a torch module, the plain oracle double)
    plain = _model(region=False)
    with pytest.raises(NotImplementedError, match="set_regions"):
        pipe(plain, **ok)
    # and the call still works afterwards
    pipe(m, **ok)
    assert len(calls) == 2


def test_engine_wrapper_has_the_regions_surface(engine_lib):
    from stablediffusion_amd.models import HipUNet2DConditionModel
    net = HipUNet2DConditionModel(config.tiny_unet())
    assert net.regions is None
    with pytest.raises(RuntimeError):
        net.set_regions(torch.ones(1, 1, 16, 16))            # weights not loaded
    assert net.clear_regions() is net                        # clearing needs no device
    assert engine_lib.sd_unet_set_regions(None, None, 0, 0, 0, 0, None) == 1
    # set before finalize is a state error; more than 8 regions is unsupported; nothing touches the device
    import ctypes as C
    buf = (C.c_float * 4)()
    assert engine_lib.sd_unet_set_regions(net._h, buf, 1, 2, 16, 16, None) == 2
