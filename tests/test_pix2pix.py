"""InstructPix2Pix without a GPU: the combine against the float64 oracle (sigma-space round trip included), the host loop
on a recording double of an 8-channel UNet, the refused combinations, checkpoint loading of an 8-channel conv_in, and the
new C entries' presence and argument validation."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p2p_oracle  # noqa: E402
from oracle import schedulers_ref  # noqa: E402
from stablediffusion_amd import _lib, checkpoints as ck, config, pix2pix, schedulers, weights  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sd_unet_forward_concat", "sd_ip2p_linear_step", "sd_ip2p_combine", "sd_op_unet_conv_in2")
# The pipeline runs the loop in fp32, the oracle in float64.  A step is about ten fp32 operations (2^-24 relative each);
# the combine's weights magnify a row's error by at most g_t + g_i + |1 - g_i| < 10 for the scales used here; the errors
# of the three steps add: 3 * 10 * 10 * 2^-24 = 1.8e-5.
LOOP_TOL = 2e-5


def edit_cfg(**kw):
    return config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=8, **kw))


# ------------------------------------------------------------------------------------------------ the combine
def test_combine_is_the_formula_and_the_round_trip_is_the_identity():
    g = torch.Generator().manual_seed(1)
    out = torch.randn(6, 4, 8, 8, generator=g, dtype=torch.float64)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * 14.6
    t, i, u = out.chunk(3)
    for g_t, g_i in ((7.5, 1.5), (1.0, 1.0), (5.0, 2.5), (3.0, 0.0)):
        want = p2p_oracle.combine(out, g_t, g_i)
        assert torch.equal(want, u + g_t * (t - i) + g_i * (i - u))
        got = pix2pix.combine(out, g_t, g_i)
        # the same three products and three sums in the same order: float64 rounding
        assert (got - want).abs().max().item() <= 4 * 2.0 ** -52 * (g_t + g_i + 1) * out.abs().max().item()
        for sigma in (14.6, 1.0, 0.03):
            rt = p2p_oracle.combine_sigma_space(out, x, sigma, g_t, g_i)
            # x0 = x - sigma eps carries |x| 2^-53; the way back divides by sigma
            tol = 2.0 ** -50 * (g_t + g_i + 1) * (x.abs().max().item() / sigma + out.abs().max().item())
            assert (rt - want).abs().max().item() <= tol, (g_t, g_i, sigma)
    # with i == u: plain classifier-free guidance on [u ; t]
    same = torch.cat([t, u, u])
    assert torch.allclose(pix2pix.combine(same, 7.5, 1.5), u + 7.5 * (t - u), rtol=0, atol=1e-13)


def test_row_helpers():
    pe, ne = torch.ones(2, 3, 4), torch.zeros(2, 3, 4) - 1
    rows = pix2pix.embed_rows(pe, ne)
    assert rows.shape[0] == 6 and torch.equal(rows[:2], pe) and torch.equal(rows[2:4], ne) and torch.equal(rows[4:], ne)
    im = torch.full((2, 4, 2, 2), 3.0)
    ir = pix2pix.image_rows(im)
    assert torch.equal(ir[:2], im) and torch.equal(ir[2:4], im) and not ir[4:].any()
    assert pix2pix.is_edit_unet(SimpleNamespace(in_channels=8))
    assert not pix2pix.is_edit_unet(SimpleNamespace(in_channels=4)) and not pix2pix.is_edit_unet(SimpleNamespace(in_channels=9))
    assert not pix2pix.is_edit_unet(None)
    assert pix2pix.DEFAULT_IMAGE_GUIDANCE_SCALE == 1.5


# ------------------------------------------------------------------------------------------------ host loop
def edit_fn(sample, t, ehs):
    """A stand-in for an 8-channel UNet that tells every group apart: the latent channels, the image channels, the
    embedding and the timestep all enter.  Works in the dtype it is given (the oracle calls it in float64)."""
    e = ehs.mean(dim=(1, 2)).view(-1, 1, 1, 1)
    return 0.1 * sample[:, :4] + 0.05 * sample[:, 4:] + 0.02 * e + 1e-5 * float(t)


class RecordingEditUNet:
    """A UNet-shaped double without forward_concat: it gets the 8-channel sample, and keeps what it was given."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.deepcache = None
        self.calls = []

    def to(self, *a, **k):
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False, **kw):
        self.calls.append(SimpleNamespace(sample=sample.clone(), t=float(t), ehs=ehs.clone(), kw=tuple(sorted(kw)),
                                          added=added_cond_kwargs))
        return (edit_fn(sample, t, ehs),)


SCALING = 0.5


def _mode(image):
    """The fake VAE's posterior mode: 8x average pooling of the three colour channels and of their mean."""
    x = torch.cat([image, image.mean(dim=1, keepdim=True)], dim=1)
    return torch.nn.functional.avg_pool2d(x, 8) * 3.0


class FakeVAE:
    def __init__(self):
        self.config = SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=SCALING, latent_channels=4)
        self.encoded = 0

    def to(self, *a, **k):
        return self

    def encode(self, x):
        self.encoded += 1

        def no_sample(generator=None):
            raise AssertionError("InstructPix2Pix reads the mode, not a sample")
        return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: _mode(x), sample=no_sample))


def _model(sched="DDIM", cfg=None):
    m = SDModelWrapper(base=RecordingEditUNet(cfg or edit_cfg()), vae=FakeVAE(), scheduler=schedulers.DDIMScheduler(),
                       device="cpu")
    m.set_scheduler(sched)
    return m


def _inputs(B=2):
    g = torch.Generator().manual_seed(9)
    d = config.tiny_unet().cross_attention_dim
    return SimpleNamespace(noise=torch.randn(B, 4, 8, 8, generator=g), pe=torch.randn(B, 7, d, generator=g),
                           ne=torch.randn(B, 7, d, generator=g), image=torch.rand(B, 3, 64, 64, generator=g) * 2 - 1)


def _run(m, do_cfg=True, steps=3, inp=None, **kw):
    inp = inp or _inputs()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cpu", output_type="latents")
    emb = dict(prompt_embeds=inp.pe, negative_prompt_embeds=inp.ne) if do_cfg else dict(prompt_embeds=inp.pe)
    kw.setdefault("image", inp.image)
    return pipe(m, latents=inp.noise, num_inference_steps=steps, guidance_scale=7.5, **emb, **kw)


REFS = {"DDIM": schedulers_ref.DDIMRef, "euler": schedulers_ref.EulerRef}


@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("sched", ["DDIM", "euler"])
def test_host_loop_builds_the_batch_and_matches_the_oracle_loop(sched, do_cfg):
    m, inp = _model(sched), _inputs()
    got = _run(m, do_cfg, image_guidance_scale=2.0, inp=inp)
    B, G = 2, 3 if do_cfg else 1
    calls = m.base.calls
    assert len(calls) == 3 and m.vae.encoded == 1                    # the image is encoded once, before the loop
    z = _mode(inp.image)
    ref = REFS[sched]()
    ref.set_timesteps(3)
    assert [c.t for c in calls] == [float(t) for t in ref.timesteps]
    for k, c in enumerate(calls):
        assert tuple(c.sample.shape) == (G * B, 8, 8, 8) and c.added is None and c.kw == ()
        # rows and their order: [prompt ; negative ; negative] against [image ; image ; 0]
        want_ehs = torch.cat([inp.pe, inp.ne, inp.ne]) if do_cfg else inp.pe
        assert torch.equal(c.ehs, want_ehs)
        # the image latents are the mode, NOT multiplied by the scaling factor, the same on every step
        for gi in range(min(G, 2)):
            assert torch.equal(c.sample[gi * B:(gi + 1) * B, 4:], z)
        if do_cfg:
            assert not c.sample[2 * B:, 4:].any()                    # the uncond group's image channels are zero
            assert torch.equal(c.sample[:B, :4], c.sample[B:2 * B, :4]) and torch.equal(c.sample[:B, :4], c.sample[2 * B:, :4])
    # the first step's latent channels: noise x init_noise_sigma through scale_model_input, the image channels not
    first = calls[0].sample
    if sched == "euler":
        s0 = float(ref.sigmas[0])
        assert ref.init_noise_sigma > 2                              # (the scaling is far from the identity)
        assert torch.allclose(first[:B, :4], inp.noise * ref.init_noise_sigma / (s0 * s0 + 1) ** 0.5, rtol=1e-5, atol=1e-6)
    else:
        assert torch.equal(first[:B, :4], inp.noise)
    want = p2p_oracle.loop(edit_fn, ref, inp.noise, z, inp.pe, inp.ne, 3, 7.5, 2.0, do_cfg)
    err = (torch.linalg.vector_norm(got.double() - want) / torch.linalg.vector_norm(want)).item()
    print(f"pix2pix host loop {sched} cfg={do_cfg}: rel-L2 against the float64 oracle loop {err:.2e}")
    assert err < LOOP_TOL


def test_image_guidance_scale_defaults_to_one_and_a_half_and_matters():
    inp = _inputs()
    default = _run(_model(), inp=inp)
    explicit = _run(_model(), inp=inp, image_guidance_scale=1.5)
    other = _run(_model(), inp=inp, image_guidance_scale=2.5)
    assert torch.equal(default, explicit)
    assert (default - other).abs().max().item() > 1e-3


def test_image_latents_may_be_given_and_are_repeated_per_prompt():
    inp = _inputs()
    z = _mode(inp.image)
    m = _model()
    from_latents = _run(m, inp=inp, image=z)
    assert m.vae.encoded == 0
    assert torch.equal(from_latents, _run(_model(), inp=inp))
    one = _model()
    _run(one, inp=inp, image=inp.image[:1])                          # one picture for both prompts
    assert torch.equal(one.base.calls[0].sample[:2, 4:], _mode(inp.image[:1]).repeat(2, 1, 1, 1))


def test_four_channel_call_is_unchanged_when_the_kwarg_is_left_out():
    """A 4-channel model: the call with image_guidance_scale=None is the call without it, forward by forward."""
    from test_pag import _model as plain_model, _run as plain_run
    a, b = plain_model(), plain_model()
    x = plain_run(a, True)
    y = plain_run(b, True, image_guidance_scale=None)
    assert torch.equal(x, y) and a.base.calls == b.base.calls and len(a.base.calls) == 3
    assert [c[0] for c in a.base.calls] == [4, 4, 4]                 # [uncond ; text], as before


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_combinations_raise():
    inp = _inputs()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    kw = dict(prompt_embeds=inp.pe, negative_prompt_embeds=inp.ne, latents=inp.noise, num_inference_steps=2, image=inp.image)
    value_errors = [
        (dict(mask_image=torch.ones(1, 1, 64, 64)), "mask_image"),
        (dict(strength=0.8), "strength"),
        (dict(guidance_rescale=0.7), "guidance_rescale"),
        (dict(image=None), "image="),
        (dict(image_guidance_scale=float("nan")), "image_guidance_scale"),
    ]
    for extra, what in value_errors:
        with pytest.raises(ValueError, match=what):
            pipe(_model(), **{**kw, **extra})
    # image_guidance_scale on a UNet that is not 8-channel
    from test_pag import _model as plain_model
    for cfg in (None, config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=9))):
        with pytest.raises(ValueError, match="in_channels == 8"):
            pipe(plain_model(cfg=cfg), prompt_embeds=inp.pe, negative_prompt_embeds=inp.ne, latents=inp.noise,
                 num_inference_steps=2, height=64, width=64, image_guidance_scale=1.5)
    not_implemented = [
        (dict(ip_adapter_image_embeds=[torch.zeros(4, 1, 8)]), "IP-Adapter"),
        (dict(ip_adapter_image=torch.zeros(1, 3, 8, 8)), "IP-Adapter"),
        (dict(pag_scale=3.0), "perturbed-attention"),
        (dict(use_refiner=True), "refiner"),
        (dict(refiner_start=0.8), "refiner"),
    ]
    for extra, what in not_implemented:
        with pytest.raises(NotImplementedError, match=what):
            pipe(_model(), **{**kw, **extra})
    m = _model()
    m.base.deepcache = (3, 1)
    with pytest.raises(NotImplementedError, match="DeepCache"):
        pipe(m, **kw)
    with pytest.raises(NotImplementedError, match="text_time"):
        pipe(_model(cfg=config.UNetConfig(**dict(config.tiny_unet(sdxl_cond=True).to_dict(), in_channels=8))), **kw)
    with pytest.raises(NotImplementedError, match="guidance-embedded"):
        pipe(_model(cfg=config.UNetConfig(**dict(config.tiny_unet(time_cond=32).to_dict(), in_channels=8))), **kw)
    # a ControlNet loaded
    from cn_oracle import synth_cn_state_dict
    from stablediffusion_amd import controlnet
    mc = _model()
    mc.base.make_controlnet = lambda cn_cfg, sd: object()
    mc.base.attach_controlnet = lambda cn: mc.base
    mc.load_controlnet(synth_cn_state_dict(controlnet.encoder_config(edit_cfg()), seed=3, zero_scale=0.5))
    with pytest.raises(NotImplementedError, match="ControlNet"):
        pipe(mc, control_image=torch.rand(1, 3, 64, 64), **kw)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        pipe(mc, **kw)
    # and the plain call goes through
    assert torch.isfinite(pipe(_model(), **kw)).all()


# ------------------------------------------------------------------------------------------------ loading
def test_eight_channel_unets_load_from_a_folder_and_a_single_file(tmp_path):
    from safetensors.torch import save_file
    from test_checkpoints import diffusers_to_ldm_unet, diffusers_to_ldm_vae
    ucfg, vcfg = edit_cfg(), config.tiny_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=1, dtype=torch.float16)
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=2, dtype=torch.float16)
    assert tuple(usd["conv_in.weight"].shape) == (ucfg.block_out_channels[0], 8, 3, 3)
    (tmp_path / "unet").mkdir()
    d = ucfg.to_dict()
    d["attention_head_dim"] = list(d["attention_head_dim"])
    json.dump(d, open(tmp_path / "unet" / "config.json", "w"))
    save_file(usd, str(tmp_path / "unet" / "diffusion_pytorch_model.safetensors"))
    got_cfg, got_sd = ck.load_unet_folder(str(tmp_path))
    assert got_cfg.in_channels == 8 and got_cfg == ucfg
    assert torch.equal(got_sd["conv_in.weight"], usd["conv_in.weight"])
    hub = {"in_channels": 8, "out_channels": 4, "down_block_types": list(config.sd15_unet().down_block_types),
           "up_block_types": list(config.sd15_unet().up_block_types), "block_out_channels": [320, 640, 1280, 1280],
           "layers_per_block": 2, "cross_attention_dim": 768, "attention_head_dim": 8, "sample_size": 64}
    assert ck.unet_config_from_json(hub) == config.UNetConfig(**dict(config.sd15_unet().to_dict(), in_channels=8))
    ldm = {**diffusers_to_ldm_unet(usd, ucfg), **diffusers_to_ldm_vae(vsd, vcfg)}
    assert tuple(ldm["model.diffusion_model.input_blocks.0.0.weight"].shape)[1] == 8
    path = str(tmp_path / "edit.safetensors")
    save_file({k: v.contiguous() for k, v in ldm.items()}, path)
    u2, _ = ck.load_ldm_single_file(path, ucfg, vcfg)
    assert sorted(u2) == sorted(usd) and all(torch.equal(u2[k], usd[k]) for k in usd)


# ------------------------------------------------------------------------------------------------ the C entries
def test_new_symbols_are_declared_bound_and_exported(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sd_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", src))
    so = os.path.join(ROOT, "stablediffusion_amd", "libsd_engine.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(engine_lib, name) is not None
        assert re.search(r"\bT %s\b" % name, exported), name
    assert len(_lib.SIGNATURES["sd_unet_forward_concat"][1]) == 18
    assert len(_lib.SIGNATURES["sd_ip2p_linear_step"][1]) == 12 and len(_lib.SIGNATURES["sd_ip2p_combine"][1]) == 6
    assert len(_lib.SIGNATURES["sd_op_unet_conv_in2"][1]) == 21


def invalid_step_calls():
    """(label, entry, args with 1 standing for a valid pointer): every one is SD_ERR_INVALID before anything launches."""
    inf, nan = float("inf"), float("nan")
    lin = lambda mo=1, lat=1, n=8, g=7.5, s=1.5: ("sd_ip2p_linear_step", (mo, lat, 0, n, g, s, 1.0, 0.1, 0.0, 0.0, 0.0))
    com = lambda mo=1, out=1, n=8, g=7.5, s=1.5: ("sd_ip2p_combine", (mo, out, n, g, s))
    table = []
    for make, what in ((lin, "linear"), (com, "combine")):
        table += [(f"{what}: n = {n}", *make(n=n)) for n in (0, -8)]
        table += [(f"{what}: null model_out", *make(mo=0))]
        table += [(f"{what}: non-finite guidance_scale {v}", *make(g=v)) for v in (inf, -inf, nan)]
        table += [(f"{what}: non-finite image_guidance_scale {v}", *make(s=v)) for v in (inf, nan)]
    table += [("linear: null latents", *lin(lat=0)), ("combine: null out", *com(out=0))]
    return table


def call_step(lib, entry, args, ptrs, stream=None):
    """args: invalid_step_calls' tuple; ptrs: what 1 becomes per pointer position (model_out, latents / out)."""
    a = list(args)
    a[0] = C.c_void_p(ptrs[0]) if a[0] else None
    a[1] = C.c_void_p(ptrs[1]) if a[1] else None
    if entry == "sd_ip2p_linear_step":
        a[2] = None
    return getattr(lib, entry)(*a, stream)


def test_invalid_step_arguments_are_refused(engine_lib):
    """Without a device: the refusal comes before any launch, so host memory stands in for the pointers."""
    mo = (C.c_uint16 * 24)()
    lat = (C.c_uint16 * 8)()
    for label, entry, args in invalid_step_calls():
        rc = call_step(engine_lib, entry, args, (C.addressof(mo), C.addressof(lat)))
        assert rc == 1, label
        assert entry.encode() in engine_lib.sd_last_error(), label
    assert not any(mo) and not any(lat)


def conv_in2_refusals():
    """(label, (Na, Ca, Nb, Cb, zero_from, ldy, N, H, W, Cout)): shapes sd_op_unet_conv_in2 does not take."""
    return [("9 (Ca + Cb) > 128", (1, 8, 1, 7, 1, 320, 1, 16, 16, 320)),
            ("Cout = 256", (1, 4, 1, 4, 1, 256, 1, 16, 16, 256)),
            ("H W = 96", (1, 4, 1, 4, 1, 320, 1, 8, 12, 320)),
            ("N % Na", (2, 4, 1, 4, 3, 320, 3, 16, 16, 320)),
            ("ldy % 8", (1, 4, 1, 4, 1, 324, 1, 16, 16, 320)),
            ("ldy < 320", (1, 4, 1, 4, 1, 312, 1, 16, 16, 320)),
            ("Cb = 0", (1, 4, 1, 0, 1, 320, 1, 16, 16, 320)),
            ("zero_from < 0", (1, 4, 1, 4, -1, 320, 1, 16, 16, 320))]


def call_conv_in2(lib, shape, ptr, stream=None, null=None):
    Na, Ca, Nb, Cb, zero_from, ldy, N, H, W, Cout = shape
    p = [C.c_void_p(ptr)] * 5
    if null is not None:
        p[null] = None
    return lib.sd_op_unet_conv_in2(p[0], Na, Ca, 1.0, p[1], Nb, Cb, zero_from, p[2], p[3], p[4], ldy, None, 0, N, H, W, Cout,
                                   0, None, stream)


def test_conv_in2_refuses_other_shapes_before_anything_runs(engine_lib):
    buf = (C.c_uint16 * 64)()
    for label, shape in conv_in2_refusals():
        assert call_conv_in2(engine_lib, shape, C.addressof(buf)) == 1, label
        assert b"sd_op_unet_conv_in2" in engine_lib.sd_last_error(), label
    for null in range(5):
        assert call_conv_in2(engine_lib, (1, 4, 1, 4, 1, 320, 1, 16, 16, 320), C.addressof(buf), null=null) == 1
    assert not any(buf)


def test_null_arguments_of_the_forward_are_refused(engine_lib):
    assert engine_lib.sd_unet_forward_concat(None, None, 1, 1.0, None, 4, 1, 1, None, None, 7, None, None, None, 1, 16, 16,
                                             None) == 1
    assert b"null" in engine_lib.sd_last_error()
