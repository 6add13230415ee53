"""Which step entry of the engine a denoising loop ends up on, per scheduler name and CFG state (the table in DESIGN.md,
"Which step entry runs"), counted at the library boundary: the UNet's `_lib` is replaced by a proxy that counts the
step entries and forwards everything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stablediffusion_amd import config, schedulers, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402
from stablediffusion_amd.schedulers import DDIMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 3
ENTRIES = ("sd_cfg_linear_step", "sd_cfg_rescale_linear_step", "sd_lcm_step", "sd_sched_affine_step", "sd_inpaint_blend")
LINEAR = ("DDIM", "euler", "DPM++ 2M", "DPM++ 2M Karras")
AFFINE = ("euler_a", "DPM++ 2M SDE Karras", "PNDM", "uni_pc")
NAMES = LINEAR + ("lcm",) + AFFINE


class CountingLib:
    """The engine library with the calls to ENTRIES recorded as (name, arguments)."""

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


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def model():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    return SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                          vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")


def _run(model, name, do_cfg, **extra):
    """One 3-step loop of scheduler `name` -> {entry: [arguments of each call]}."""
    model.set_scheduler(name)
    B, g = 2, torch.Generator().manual_seed(3)
    dim = config.tiny_unet().cross_attention_dim
    pos = torch.randn(B, 7, dim, generator=g).half().cuda()
    neg = torch.randn(B, 7, dim, generator=g).half().cuda()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half().cuda()
    kw = dict(prompt_embeds=pos, latents=lat0, num_inference_steps=STEPS, guidance_scale=5.0, height=128, width=128, **extra)
    if do_cfg:
        kw["negative_prompt_embeds"] = neg
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    real = model.base._lib
    proxy = model.base._lib = CountingLib(real)
    try:
        torch.manual_seed(3)
        out = pipe(model, **kw)
    finally:
        model.base._lib = real
    assert torch.isfinite(out.float()).all()
    calls = {}
    for entry, args in proxy.calls:
        calls.setdefault(entry, []).append(args)
    return calls


def _iterations(name):
    return STEPS + 1 if name == "PNDM" else STEPS          # PNDM's schedule repeats its second timestep


def test_the_table_names_every_scheduler():
    assert sorted(NAMES) == sorted(list(schedulers.REGISTRY) + list(schedulers.EXTRA_SCHEDULERS))


@pytest.mark.parametrize("do_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("name", NAMES)
def test_step_entry_per_scheduler(engine_lib, model, name, do_cfg):
    calls = _run(model, name, do_cfg)
    if name in LINEAR:
        # the linear step is the CFG combine and the update in one: without CFG these schedulers run scheduler.step
        want = "sd_cfg_linear_step" if do_cfg else None
    else:
        want = "sd_lcm_step" if name == "lcm" else "sd_sched_affine_step"
    assert sorted(calls) == ([want] if want else []), (name, do_cfg, sorted(calls))
    if want:
        assert len(calls[want]) == _iterations(name), (name, do_cfg, len(calls[want]))
    if want in ("sd_lcm_step", "sd_sched_affine_step"):
        assert {args[1] for args in calls[want]} == {2 if do_cfg else 1}, (name, do_cfg)       # rows


@pytest.mark.parametrize("name", NAMES)
def test_step_entry_under_guidance_rescale(engine_lib, model, name):
    """guidance_rescale is a per-sample statistic: the linear group has its own entry, the others run scheduler.step."""
    calls = _run(model, name, True, guidance_rescale=0.7)
    if name in LINEAR:
        assert sorted(calls) == ["sd_cfg_rescale_linear_step"], (name, sorted(calls))
        assert len(calls["sd_cfg_rescale_linear_step"]) == STEPS
    else:
        assert not calls, (name, sorted(calls))


def test_inpaint_blend_follows_every_step(engine_lib, model):
    g = torch.Generator().manual_seed(5)
    image = torch.randn(2, 4, 16, 16, generator=g).half().cuda()          # the image as latents: nothing is sampled
    mask = torch.zeros(1, 1, 128, 128)
    mask[:, :, :, 64:] = 1.0
    calls = _run(model, "DDIM", True, image=image, mask_image=mask.cuda(), seed=2)
    assert sorted(calls) == ["sd_cfg_linear_step", "sd_inpaint_blend"], sorted(calls)
    assert len(calls["sd_cfg_linear_step"]) == STEPS and len(calls["sd_inpaint_blend"]) == STEPS
