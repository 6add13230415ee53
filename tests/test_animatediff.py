"""CPU half of the AnimateDiff tests: the motion adapter loaders, and `animate` on oracle-backed doubles (tests/doubles.py)
against a hand-written host loop over tests/motion_oracle.py -- the noise layout, the per-frame text rows, the CFG
combine, the scheduler, the chunked decode and the refusals.  Nothing here needs a device."""
import math
from types import SimpleNamespace

import pytest
import torch

import motion_oracle
from conftest import rel_l2
from doubles import OracleVAE
from stablediffusion_amd import animatediff, config, motion, weights
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


# ------------------------------------------------------------------------------------------------ loaders
def _adapter():
    ucfg = config.tiny_unet()
    mcfg = motion.tiny_motion_adapter(ucfg)
    return ucfg, mcfg, motion.synth_state_dict(mcfg, 3)


def test_manifest_counts():
    ucfg, mcfg, sd = _adapter()
    assert len(motion.module_prefixes(mcfg)) == 21          # 2 per down block, the mid block's, 3 per up block
    assert len(sd) == 21 * 26
    sd15 = motion.MotionAdapterConfig()
    assert [c for _, c, _ in motion.module_prefixes(sd15)] == [320] * 2 + [640] * 2 + [1280] * 5 + [1280] * 3 + [1280] * 3 + \
        [640] * 3 + [320] * 3


def test_both_key_layouts_round_trip():
    ucfg, mcfg, sd = _adapter()
    pe = {}
    for p, c, _ in motion.module_prefixes(mcfg):
        for a in ("attn1", "attn2"):
            pe[f"{p}.transformer_blocks.0.{a}.pos_embed.pe"] = motion.position_table(32, c).float()[None]
    cfg1, out1 = motion.load({**sd, **pe}, ucfg, mcfg)
    assert cfg1 == mcfg and out1.keys() == sd.keys() and all(torch.equal(out1[k], sd[k]) for k in sd)
    orig = {motion.diffusers_to_original_key(k): v for k, v in {**sd, **pe}.items()}
    assert any(".temporal_transformer.transformer_blocks.0.attention_blocks.1.pos_encoder.pe" in k for k in orig)
    assert any(".ff_norm.weight" in k for k in orig) and any(".norms.1.bias" in k for k in orig)
    assert all(motion.original_to_diffusers_key(k) in {**sd, **pe} for k in orig)
    cfg2, out2 = motion.load(orig, ucfg, mcfg)
    assert out2.keys() == sd.keys() and all(torch.equal(out2[k], sd[k]) for k in sd)
    # without a configuration the sizes come from the shapes (heads default to the published adapters' 8)
    cfg3, _ = motion.load(orig, ucfg)
    assert cfg3.block_out_channels == mcfg.block_out_channels and cfg3.motion_num_attention_heads == (8, 8, 8, 8)
    assert cfg3.use_motion_mid_block and cfg3.motion_max_seq_length == 32


def test_strict_errors():
    ucfg, mcfg, sd = _adapter()
    k0 = "down_blocks.1.motion_modules.0.transformer_blocks.0.attn2.to_k.weight"
    with pytest.raises(KeyError, match="missing"):
        motion.load({k: v for k, v in sd.items() if k != k0}, ucfg, mcfg)
    with pytest.raises(KeyError, match="unexpected"):
        motion.load({**sd, "down_blocks.0.motion_modules.0.extra.weight": torch.zeros(1)}, ucfg, mcfg)
    with pytest.raises(ValueError, match="expected shape"):
        motion.load({**sd, k0: torch.zeros(128, 64)}, ucfg, mcfg)
    with pytest.raises(NotImplementedError, match="SparseCtrl"):
        motion.load({**sd, "conv_in.weight": torch.zeros(64, 5, 3, 3)}, ucfg, mcfg)
    with pytest.raises(NotImplementedError, match="conv_in"):
        motion.MotionAdapterConfig.from_dict({"conv_in_channels": 5})
    with pytest.raises(ValueError, match="block_out_channels"):
        motion.MotionAdapterConfig().check(ucfg)
    with pytest.raises(NotImplementedError, match="SDXL"):
        mcfg.check(config.tiny_unet(sdxl_cond=True))


def test_wrong_stored_position_table_is_refused():
    ucfg, mcfg, sd = _adapter()
    k = "up_blocks.0.motion_modules.1.transformer_blocks.0.attn1.pos_embed.pe"
    good = motion.position_table(32, 256)
    motion.load({**sd, k: good.half()[None]}, ucfg, mcfg)                  # fp16 rounding of the closed form passes
    bad = good.clone()
    bad[5, 7] += 2.0 ** -9
    with pytest.raises(ValueError, match="position table"):
        motion.load({**sd, k: bad.float()[None]}, ucfg, mcfg)
    with pytest.raises(ValueError, match="position table"):               # sin / cos swapped
        motion.load({**sd, k: torch.roll(good, 1, dims=1).float()[None]}, ucfg, mcfg)
    with pytest.raises(ValueError, match="position table"):               # fewer rows than max_seq_length
        motion.load({**sd, k: good[:24].float()[None]}, ucfg, mcfg)


# ------------------------------------------------------------------------------------------------ animate on doubles
class OracleMotionUNet:
    """The `.base` slot backed by motion_oracle: the call surface `animate` uses of HipUNet2DConditionModel."""

    def __init__(self, cfg, sd, mcfg, msd):
        self.cfg, self.sd, self.mcfg, self.msd = cfg, sd, mcfg, msd
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.motion_adapter = SimpleNamespace(cfg=mcfg)
        self.calls = []

    def to(self, *a, **k):
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False, num_frames=None):
        self.calls.append((tuple(sample.shape), num_frames))
        assert num_frames, "animate must name the frames on every forward"
        return (motion_oracle.forward(self.cfg, self.sd, self.mcfg, self.msd, sample.float(), t, ehs.float(), num_frames),)


@pytest.fixture(scope="module")
def world():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), 1, perturb=0.1)
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), 2, perturb=0.1)
    mcfg = motion.tiny_motion_adapter(ucfg)
    msd = motion.synth_state_dict(mcfg, 3)
    unet = OracleMotionUNet(ucfg, usd, mcfg, msd)
    model = SDModelWrapper(base=unet, vae=OracleVAE(vcfg, vsd), device="cpu")
    g = torch.Generator().manual_seed(0)
    pos, neg = (torch.randn(2, 7, ucfg.cross_attention_dim, generator=g) for _ in range(2))
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="pt")
    return SimpleNamespace(ucfg=ucfg, usd=usd, mcfg=mcfg, msd=msd, unet=unet, model=model, pos=pos, neg=neg, pipe=pipe)


V, F, HW = 2, 3, 8


def host_loop(w, name, seed, steps, g_scale):
    """AnimateDiffPipeline's loop by hand: noise [V, 4, F, h, w] -> frame-major, CFG on 2 V F rows, scheduler.step."""
    w.model.set_scheduler(name)
    sch = w.model.scheduler
    sch.set_timesteps(steps, device="cpu")
    z = torch.randn((V, 4, F, HW, HW), generator=torch.Generator().manual_seed(seed))
    x = z.permute(0, 2, 1, 3, 4).reshape(V * F, 4, HW, HW) * sch.init_noise_sigma
    ehs = torch.cat([w.neg.repeat_interleave(F, 0), w.pos.repeat_interleave(F, 0)])
    lcm = name == "lcm"
    gen = torch.Generator().manual_seed(seed)
    ts = [float(t) for t in sch.timesteps.tolist()]
    for t in ts:
        noise = torch.randn(x.shape, generator=gen) if lcm and t != ts[-1] else None
        xin = sch.scale_model_input(torch.cat([x] * 2), t)
        out = motion_oracle.forward(w.ucfg, w.usd, w.mcfg, w.msd, xin, t, ehs, F)
        u, c = out.chunk(2)
        eps = g_scale * (c - u) + u
        x = sch.step(eps, t, x, noise=noise, return_dict=False)[0] if lcm else sch.step(eps, t, x, return_dict=False)[0]
    return x.reshape(V, F, 4, HW, HW)


@pytest.mark.parametrize("name", ("DDIM", "euler", "lcm"))
def test_animate_equals_the_host_loop(world, name):
    w = world
    want = host_loop(w, name, 11, 3, 4.0)
    w.model.set_scheduler(name)
    w.unet.calls.clear()
    got = animatediff.animate(w.pipe, w.model, None, prompt_embeds=w.pos, negative_prompt_embeds=w.neg, num_frames=F, height=64,
                              width=64, num_inference_steps=3, guidance_scale=4.0, seed=11, output_type="latents")
    assert got.shape == (V, F, 4, HW, HW)
    assert w.unet.calls == [((2 * V * F, 4, HW, HW), F)] * 3
    e = rel_l2(got, want)
    print("%s: rel-L2 %.2e against the host loop" % (name, e))
    assert e <= 1e-5                                     # the same float operations in the same order


def test_seed_and_noise_layout(world):
    w = world
    w.model.set_scheduler("DDIM")
    kw = dict(prompt_embeds=w.pos, negative_prompt_embeds=w.neg, num_frames=F, height=64, width=64, num_inference_steps=2,
              guidance_scale=3.0, output_type="latents")
    a, b, c = (animatediff.animate(w.pipe, w.model, None, seed=s, **kw) for s in (5, 5, 6))
    assert torch.equal(a, b) and rel_l2(c, a) > 0.1
    # the seed's noise is the [V, 4, F, h, w] draw: handing that tensor over is the same call
    z = torch.randn((V, 4, F, HW, HW), generator=torch.Generator().manual_seed(5))
    assert torch.equal(animatediff.animate(w.pipe, w.model, None, latents=z, **kw), a)
    x = animatediff.video_noise(V, 4, F, HW, HW, 5, "cpu", torch.float32)
    assert torch.equal(x.reshape(V, F, 4, HW, HW), z.permute(0, 2, 1, 3, 4))
    with pytest.raises(ValueError, match="latents"):
        animatediff.animate(w.pipe, w.model, None, latents=z.permute(0, 2, 1, 3, 4), **kw)


def test_decode_chunk_size_does_not_change_the_frames(world):
    w = world
    w.model.set_scheduler("DDIM")
    kw = dict(prompt_embeds=w.pos, negative_prompt_embeds=w.neg, num_frames=F, height=64, width=64, num_inference_steps=1,
              guidance_scale=3.0, seed=2)
    frames = [animatediff.animate(w.pipe, w.model, None, decode_chunk_size=n, **kw) for n in (1, 4, 8)]
    assert frames[0].shape == (V, F, 3, 64, 64) and torch.isfinite(frames[0]).all()
    # (float32 on the CPU: the convolutions of a batch of 1, 4 or 6 frames may sum in another order -- 2^-24 per operation
    # through the decoder's thirty-odd layers stays below 1e-5; a frame in the wrong place is O(1))
    assert rel_l2(frames[1], frames[0]) <= 1e-5 and rel_l2(frames[2], frames[0]) <= 1e-5
    lat = animatediff.animate(w.pipe, w.model, None, output_type="latents", **kw)
    one = w.model.vae.decode(lat[1, 2:3] / w.model.vae.config.scaling_factor)[0]
    assert rel_l2(frames[0][1, 2:3], one) <= 1e-5


def test_refusals_leave_the_wrapper_untouched(world):
    w = world
    kw = dict(prompt_embeds=w.pos, negative_prompt_embeds=w.neg, num_frames=F, height=64, width=64, num_inference_steps=1, seed=2)
    state = (w.pipe.model, w.pipe.is_inpaint, w.pipe._use_refiner, w.model.scheduler)
    w.unet.calls.clear()

    def refused(exc, match, **over):
        with pytest.raises(exc, match=match):
            animatediff.animate(w.pipe, w.model, None, **{**kw, **over})
        assert w.unet.calls == [] and (w.pipe.model, w.pipe.is_inpaint, w.pipe._use_refiner, w.model.scheduler) == state

    refused(ValueError, "num_frames", num_frames=33)
    refused(ValueError, "num_frames", num_frames=0)
    refused(ValueError, "output_type", output_type="pil")
    for attr, value, match in (("deepcache", (3, 1), "DeepCache"), ("tome", (0.5,), "token merging"),
                               ("hypertile", (32, 2, 0, 0), "HyperTile"), ("_graph_on", True, "graph replay")):
        setattr(w.unet, attr, value)
        try:
            refused(NotImplementedError, match)
        finally:
            delattr(w.unet, attr)
    w.model._cn = (None, None)
    try:
        refused(NotImplementedError, "ControlNet")
    finally:
        w.model._cn = None
    w.model._ip = ({}, 4, 4)
    try:
        refused(NotImplementedError, "IP-Adapter")
    finally:
        w.model._ip = None
    adapter, w.unet.motion_adapter = w.unet.motion_adapter, None
    try:
        refused(ValueError, "load_motion_adapter")
    finally:
        w.unet.motion_adapter = adapter
    w.unet.config.in_channels = 9
    try:
        refused(NotImplementedError, "4 latent channels")
    finally:
        w.unet.config.in_channels = 4
    w.model.type = "sdxl"
    try:
        refused(NotImplementedError, "SDXL")
    finally:
        w.model.type = "sd15"
    assert math.isfinite(animatediff.animate(w.pipe, w.model, None, output_type="latents", **kw).sum().item())
