"""LCM few-step sampling, host side: the scheduler and its device-step coefficients against a float64 restatement
(tests/lcm_oracle.py), the guidance-scale embedding, the weight bookkeeping of `time_cond_proj_dim` and the pipeline's
loop on the oracle-backed doubles.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import lcm_oracle
from conftest import rel_l2
from doubles import OracleUNet, OracleVAE
from stablediffusion_amd import _lib, config, schedulers, weights
from stablediffusion_amd.models import HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline, guidance_scale_embedding

# the cap of test_lcm_gpu.py::test_lcm_step on elements that may differ (by one fp16 ulp) from the rounded float64 result
GPU_STEP_CAP = 0.01
STEP_NS = (1, 7, 8, 2047, 4 * 4 * 16 * 16, 3 * 4 * 24 * 40)


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n,strength,want", [
    (4, 1.0, [999, 759, 499, 259]), (1, 1.0, [999]), (2, 1.0, [999, 499]),
    (8, 1.0, [999, 879, 759, 639, 499, 379, 259, 139]), (50, 1.0, list(range(999, 0, -20))),
    (4, 0.5, [499, 379, 259, 139])])
def test_schedule(n, strength, want):
    s = schedulers.LCMScheduler()
    s.set_timesteps(n, strength=strength)
    assert s.timesteps.tolist() == want
    assert lcm_oracle.LCMOracle().timesteps(n, strength) == want
    assert s.num_inference_steps == n and s.init_noise_sigma == 1.0
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 999) is x


def test_schedule_errors_and_config():
    s = schedulers.LCMScheduler()
    with pytest.raises(ValueError, match="original_inference_steps"):
        s.set_timesteps(51)
    with pytest.raises(ValueError, match="fewer"):
        s.set_timesteps(8, strength=0.1)               # 5 distillation timesteps for 8 steps
    s.set_timesteps(4, original_inference_steps=100)    # k = 10
    assert s.timesteps.tolist() == [999, 749, 499, 249]
    assert s.final_alpha_cumprod == 1.0 and s.sigma_data == 0.5
    assert (s.config.original_inference_steps, s.config.timestep_scaling, s.config.set_alpha_to_one) == (50, 10.0, True)
    for bad in (dict(prediction_type="sample"), dict(rescale_betas_zero_snr=True), dict(timestep_spacing="trailing")):
        with pytest.raises(ValueError):
            schedulers.LCMScheduler(**bad)
    back = schedulers.LCMScheduler.from_config(schedulers.LCMScheduler(original_inference_steps=25, timestep_scaling=5.0,
                                                                       prediction_type="v_prediction").config)
    assert (back.config.original_inference_steps, back.config.timestep_scaling, back.v_prediction) == (25, 5.0, True)


# ------------------------------------------------------------------------------------------------ step
def _loop_data(n_steps, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (2, 4, 8, 8)
    x = torch.randn(shape, generator=g)
    outs = [torch.randn(shape, generator=g) for _ in range(n_steps)]
    noises = [torch.randn(shape, generator=g) for _ in range(n_steps)]
    return x, outs, noises


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_step_matches_float64_oracle(pred):
    """fp32 tensors through `step` with injected noise against the float64 restatement: 1e-6 relative (rel-L2) on every
    step's prev_sample and denoised; the last step adds no noise and returns prev == denoised."""
    s = schedulers.LCMScheduler(prediction_type=pred)
    s.set_timesteps(4)
    ref = lcm_oracle.LCMOracle(prediction_type=pred)
    ts = ref.timesteps(4)
    x, outs, noises = _loop_data(4, 3)
    x64 = x.double().numpy()
    for i, t in enumerate(s.timesteps.tolist()):
        prev, den = s.step(outs[i], t, x, noise=noises[i])
        p64, d64 = ref.step(outs[i].double().numpy(), i, ts, x64, noises[i].double().numpy())
        assert prev.dtype == torch.float32
        assert rel_l2(prev.double(), torch.from_numpy(p64)) < 1e-6 and rel_l2(den.double(), torch.from_numpy(d64)) < 1e-6
        if i == 3:
            assert torch.equal(prev, den)
        else:
            assert not torch.equal(prev, den)
        x, x64 = prev, prev.double().numpy()


def test_step_draws_its_own_noise_and_casts_once():
    s = schedulers.LCMScheduler()
    s.set_timesteps(2)
    x, outs, _ = _loop_data(2, 4)
    a = s.step(outs[0].half(), 999, x.half(), generator=torch.Generator().manual_seed(1))
    s.set_timesteps(2)
    b = s.step(outs[0].half(), 999, x.half(), generator=torch.Generator().manual_seed(1))
    s.set_timesteps(2)
    c = s.step(outs[0].half(), 999, x.half(), generator=torch.Generator().manual_seed(2))
    assert a[0].dtype == torch.float16 and torch.equal(a[0], b[0]) and not torch.equal(a[0], c[0])
    assert torch.equal(a[1], c[1])                      # denoised does not depend on the noise


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n_steps", [4, 8])
def test_fused_plan_equals_step(pred, n_steps):
    """The coefficients handed to sd_lcm_step, applied in float64, are `step` on every step.  `step` computes in fp32
    like every scheduler here, so the two agree as `step` agrees with the float64 oracle: 1e-6 rel-L2."""
    a = schedulers.LCMScheduler(prediction_type=pred)
    b = schedulers.LCMScheduler(prediction_type=pred)
    a.set_timesteps(n_steps)
    b.set_timesteps(n_steps)
    x, outs, noises = _loop_data(n_steps, 5)
    for i, t in enumerate(a.timesteps.tolist()):
        prev, den = a.step(outs[i], t, x, noise=noises[i])
        plan = b.fused_plan(t)
        assert plan.in_scale == 1.0 and plan.needs_noise == (i < n_steps - 1)
        d = plan.d_x * x.double() + plan.d_out * outs[i].double()
        p = plan.p_den * d + plan.p_noise * noises[i].double()
        if not plan.needs_noise:
            assert (plan.p_den, plan.p_noise) == (1.0, 0.0)
        b.fused_commit()
        assert rel_l2(den.double(), d) < 1e-6 and rel_l2(prev.double(), p) < 1e-6
        x = prev


def test_img2img_slice_and_add_noise():
    """A loop that starts mid-schedule (get_timesteps slices `timesteps`) resolves its position from the timestep."""
    s = schedulers.LCMScheduler()
    s.set_timesteps(4)
    assert s.fused_plan(499).p_den == pytest.approx(float(s.ac[259] ** 0.5))
    s.set_timesteps(4)
    s.set_begin_index(3)
    assert not s.fused_plan(259).needs_noise
    a, b = s.add_noise_coefficients(499)
    assert a == pytest.approx(float(s.ac[499] ** 0.5)) and a * a + b * b == pytest.approx(1.0)
    x, n = torch.ones(1, 2), torch.full((1, 2), 2.0)
    assert torch.allclose(s.add_noise(x, n, torch.tensor([499])), torch.full((1, 2), a + 2 * b))


# ------------------------------------------------------------------------------------------------ registry
@pytest.mark.parametrize("name", list(schedulers.REGISTRY))
def test_set_scheduler_lcm_from_any(name):
    from types import SimpleNamespace
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    m = SDModelWrapper(base=None, vae=vae, scheduler=schedulers.DDIMScheduler(prediction_type="v_prediction"), device="cpu")
    m.set_scheduler(name)
    m.set_scheduler("lcm")
    assert type(m.scheduler) is schedulers.LCMScheduler and m.scheduler.v_prediction and m.scheduler_name == "lcm"
    m.scheduler.set_timesteps(4)
    assert m.scheduler.timesteps.tolist() == [999, 759, 499, 259]
    m.set_scheduler(name)
    assert type(m.scheduler) is type(schedulers.REGISTRY[name](schedulers.DDIMScheduler().config))
    with pytest.raises(ValueError):
        m.set_scheduler("lcm2")


def test_registry_keeps_the_eight_names():
    assert sorted(schedulers.REGISTRY) == sorted(["DDIM", "euler", "euler_a", "DPM++ 2M", "DPM++ 2M Karras",
                                                  "DPM++ 2M SDE Karras", "PNDM", "uni_pc"])
    assert list(schedulers.EXTRA_SCHEDULERS) == ["lcm"]
    from stablediffusion_amd import checkpoints
    assert {"original_inference_steps", "timestep_scaling"} <= set(checkpoints.SCHEDULER_FIELDS)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dim", [256, 32, 33])
def test_guidance_scale_embedding(dim):
    w = torch.tensor([7.5 - 1.0, 0.0, 1.5 - 1.0])
    got = guidance_scale_embedding(w, dim)
    ref = lcm_oracle.guidance_scale_embedding(w.double().numpy(), dim)
    assert got.shape == (3, dim) and got.dtype == torch.float32
    # arguments reach 6500 rad: fp32 range reduction, as for the timestep sinusoid (test_ops_gpu.py: 5e-4)
    assert np.abs(got.double().numpy() - ref).max() < 5e-4
    if dim % 2:
        assert (got[:, -1] == 0).all()


# ------------------------------------------------------------------------------------------------ weights
def _engine_manifest(handle, lib):
    out = []
    for i in range(lib.sd_unet_num_weights(handle)):
        key, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert lib.sd_unet_weight_info(handle, i, C.byref(key), shape, C.byref(ndim)) == 0
        out.append((key.value.decode(), tuple(shape[j] for j in range(ndim.value))))
    return out


def test_manifest_and_engine_weight_list(engine_lib):
    for kw in (dict(), dict(linear=True, sdxl_cond=True)):
        plain = config.tiny_unet(**kw)
        tc = config.tiny_unet(time_cond=32, **kw)
        assert plain.time_cond_proj_dim is None and tc.time_cond_proj_dim == 32
        mp, mt = weights.unet_manifest(plain), weights.unet_manifest(tc)
        extra = [k for k in mt if k not in mp]
        assert extra == ["time_embedding.cond_proj.weight"] and mt[extra[0]] == (64, 32)
        assert [(k, v) for k, v in mt.items() if k != extra[0]] == list(mp.items())
        assert list(mt).index(extra[0]) == list(mt).index("time_embedding.linear_2.bias") + 1
        assert _engine_manifest(HipUNet2DConditionModel(tc)._h, engine_lib) == list(mt.items())
        assert _engine_manifest(HipUNet2DConditionModel(plain)._h, engine_lib) == list(mp.items())
    assert "time_embedding.cond_proj.bias" not in weights.unet_manifest(config.tiny_unet(time_cond=32))


def test_config_json_and_create_validation(engine_lib):
    from stablediffusion_amd import checkpoints
    from stablediffusion_amd.models import _unet_config_struct
    d = dict(config.sd15_unet().to_dict(), time_cond_proj_dim=256)
    assert checkpoints.unet_config_from_json(d).time_cond_proj_dim == 256
    d.pop("time_cond_proj_dim")
    assert checkpoints.unet_config_from_json(d).time_cond_proj_dim is None
    assert _lib.SdUNetConfig._fields_[-1][0] == "time_cond_proj_dim"
    for bad in (-1, 1025):
        c = _unet_config_struct(config.tiny_unet())
        c.time_cond_proj_dim = bad
        h = C.c_void_p()
        assert engine_lib.sd_unet_create(C.byref(c), C.byref(h)) == 1
        assert b"time_cond_proj_dim" in engine_lib.sd_last_error()
    c = _unet_config_struct(config.tiny_unet())
    c.time_cond_proj_dim = 1024
    h = C.c_void_p()
    assert engine_lib.sd_unet_create(C.byref(c), C.byref(h)) == 0
    engine_lib.sd_unet_destroy(h)


def test_step_entry_rejects_bad_arguments(engine_lib):
    """sd_lcm_step validates before it launches: no device needed."""
    p = C.c_void_p(64)
    assert engine_lib.sd_lcm_step(p, 3, p, None, None, 8, 1.0, 1.0, 1.0, 1.0, 0.0, None) == 1
    assert engine_lib.sd_lcm_step(p, 1, p, None, None, 0, 1.0, 1.0, 1.0, 1.0, 0.0, None) == 1
    assert engine_lib.sd_lcm_step(p, 1, p, None, None, 8, 1.0, 1.0, 1.0, 1.0, 0.5, None) == 1
    assert b"noise" in engine_lib.sd_last_error()
    assert engine_lib.sd_lcm_step(None, 1, p, None, None, 8, 1.0, 1.0, 1.0, 1.0, 0.0, None) == 1


# ------------------------------------------------------------------------------------------------ pipeline
class _RecordingUNet(OracleUNet):
    """OracleUNet that takes timestep_cond (lcm_oracle.unet_forward) and records what it was called with."""

    def __init__(self, cfg, sd):
        super().__init__(cfg, sd)
        self.calls = []

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                 timestep_cond=None):
        self.calls.append((tuple(sample.shape), None if timestep_cond is None else timestep_cond.clone()))
        return (lcm_oracle.unet_forward(self.cfg, self.sd, sample.float(), t, ehs.float(), timestep_cond,
                                        added_cond_kwargs),)


def test_pipeline_guidance_embedded_unet_runs_without_cfg():
    ucfg, vcfg = config.tiny_unet(time_cond=32), config.tiny_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), 1, perturb=0.1)
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), 2, perturb=0.1)
    unet = _RecordingUNet(ucfg, usd)
    model = SDModelWrapper(base=unet, vae=OracleVAE(vcfg, vsd), device="cpu")
    model.set_scheduler("lcm")
    g = torch.Generator().manual_seed(0)
    pos = torch.randn(2, 7, ucfg.cross_attention_dim, generator=g)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")     # CFG asked for: unused
    kw = dict(prompt_embeds=pos, num_inference_steps=4, guidance_scale=8.0, height=64, width=64, seed=11)
    a = pipe(model, **kw)
    assert len(unet.calls) == 4
    want = guidance_scale_embedding(torch.full((2,), 7.0), 32)
    for shape, tc in unet.calls:
        assert shape == (2, 4, 8, 8)                   # batch B, not 2B
        assert tc.shape == (2, 32) and tc.dtype == torch.float32 and torch.equal(tc, want)
    b = pipe(model, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)                     # same seed: same noise draws
    c = pipe(model, **dict(kw, seed=12))
    assert rel_l2(c, a) > 0.1
    assert pipe.do_classifier_free_guidance is False
    # the same pipeline object on an ordinary UNet is back to CFG
    plain = SDModelWrapper(base=OracleUNet(config.tiny_unet(), weights.synth_state_dict(
        weights.unet_manifest(config.tiny_unet()), 1)), vae=OracleVAE(vcfg, vsd), device="cpu")
    with pytest.raises(ValueError, match="negative_prompt_embeds"):
        pipe(plain, **kw)


def test_pipeline_lcm_on_ordinary_unet_draws_seeded_noise():
    """LCM-LoRA case on the host path: CFG stays on, one seeded noise draw per non-final step."""
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = weights.synth_state_dict(weights.unet_manifest(ucfg), 1, perturb=0.1)
    vsd = weights.synth_state_dict(weights.vae_manifest(vcfg), 2, perturb=0.1)
    model = SDModelWrapper(base=OracleUNet(ucfg, usd), vae=OracleVAE(vcfg, vsd), device="cpu")
    model.set_scheduler("lcm")
    g = torch.Generator().manual_seed(0)
    pos, neg = (torch.randn(1, 7, ucfg.cross_attention_dim, generator=g) for _ in range(2))
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, num_inference_steps=2, guidance_scale=1.5, height=64, width=64)
    a, b, c = pipe(model, seed=5, **kw), pipe(model, seed=5, **kw), pipe(model, seed=6, **kw)
    assert torch.equal(a, b) and rel_l2(c, a) > 0.1
    assert not pipe._fused_step_available(model, a)    # never the deterministic schedulers' CFG step


# ------------------------------------------------------------------------------------------------ yardstick
def test_step_reference_flips_stay_under_a_quarter_of_the_gpu_cap():
    """The GPU step test compares against fp16(float64 result) and lets at most 1 % of the elements differ, by one ulp.
    An fp32 evaluation of the same formula on the same inputs -- the least a device step can be expected to do -- must
    itself differ from that reference in at most a quarter of that share, or the cap would be measuring the reference.
    (Only the share is checked here.  Where d_x x and d_out m cancel to almost nothing this fp32 evaluation is several
    fp16 ulps off -- 5 at n = 11520 -- which is why the kernel forms den in fp64.)"""
    s = schedulers.LCMScheduler()
    s.set_timesteps(4)
    plans = []
    for t in s.timesteps.tolist():
        plans.append(s.fused_plan(t))
        s.fused_commit()
    g = 1.5
    differ_total = elements = 0
    for n in STEP_NS:
        mo, lat, noise = lcm_oracle.step_inputs(n, seed=n)
        for rows in (1, 2):
            for plan in (plans[0], plans[1], plans[3]):
                nz = noise if plan.needs_noise else None
                den64, out64 = lcm_oracle.step_reference(mo, rows, lat, nz, n, g, plan.d_x, plan.d_out, plan.p_den,
                                                         plan.p_noise)
                m = (lcm_oracle.cfg_combine_f16(mo, n, g) if rows == 2 else mo[:n]).float()
                den32 = np.float32(plan.d_x) * lat.float() + np.float32(plan.d_out) * m
                out32 = np.float32(plan.p_den) * den32
                if nz is not None:
                    out32 = out32 + np.float32(plan.p_noise) * nz.float()
                for got, ref in ((den32, den64), (out32, out64)):
                    differ = (got.half() != lcm_oracle.to_f16(ref)).sum().item()
                    if n >= 2047:                       # (below, a quarter of 1 % is less than one element)
                        assert differ <= 0.25 * GPU_STEP_CAP * n, (n, rows, differ)
                    differ_total += differ
                    elements += n
    assert differ_total <= 0.25 * GPU_STEP_CAP * elements, (differ_total, elements)
