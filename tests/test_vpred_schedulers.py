"""v-prediction, zero terminal SNR and trailing timesteps in the host schedulers.  CPU only.

v-prediction is pinned to the existing epsilon oracle (oracle/schedulers_ref.py): a scheduler that is handed v must do
what the oracle does when it is handed eps(v, x, t), with
    eps = a v + s x,  a = sqrt(alpha-bar_t), s = sqrt(1 - alpha-bar_t)                (alpha-space samples)
    eps = v / sqrt(sigma^2 + 1) + sigma x / (sigma^2 + 1)                             (Euler family, unscaled samples)
restated here from the schedules of the oracle, not from the product.  Tolerances are those of tests/test_oracle.py for
the same scheduler (1e-5 for DDIM / DPM++ 2M / euler, 5e-5 for the other five)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import schedulers_ref
from stablediffusion_amd import checkpoints, schedulers
from stablediffusion_amd.pipeline import SDModelWrapper

CASES = [("DDIM", schedulers_ref.DDIMRef, 7, 1e-5), ("DPM++ 2M", schedulers_ref.DPMpp2MRef, 6, 1e-5),
         ("euler", schedulers_ref.EulerRef, 6, 1e-5), ("euler_a", schedulers_ref.EulerAncestralRef, 6, 5e-5),
         ("DPM++ 2M Karras", schedulers_ref.DPMpp2MKarrasRef, 8, 5e-5),
         ("DPM++ 2M SDE Karras", schedulers_ref.DPMpp2MSDERef, 7, 5e-5), ("PNDM", schedulers_ref.PNDMRef, 8, 5e-5),
         ("uni_pc", schedulers_ref.UniPCRef, 7, 5e-5)]
STOCHASTIC = ("euler_a", "DPM++ 2M SDE Karras")
ALPHA_SPACE = ("DDIM", "PNDM")
EULER_FAMILY = ("euler", "euler_a")


def make(name, **kw):
    return schedulers.REGISTRY[name](schedulers.DDIMScheduler(timestep_spacing="leading", **kw).config)


def eps_of_v(name, ref, v, x, t):
    """The identities of the module docstring, from the ORACLE's schedule at the step it is about to take."""
    if name in ALPHA_SPACE:
        ab = schedulers_ref.alphas_cumprod()[int(t)]
        return np.sqrt(ab) * v + np.sqrt(1.0 - ab) * x
    sg = ref.sigmas[ref.i]
    if name in EULER_FAMILY:
        return v / np.sqrt(sg * sg + 1.0) + sg * x / (sg * sg + 1.0)
    a = 1.0 / np.sqrt(sg * sg + 1.0)
    return a * v + sg * a * x


@pytest.mark.parametrize("name,ref_cls,n,atol", CASES)
def test_v_prediction_step_equals_oracle_on_converted_eps(name, ref_cls, n, atol):
    prod, ref = make(name, prediction_type="v_prediction"), ref_cls()
    prod.set_timesteps(n)
    ts = ref.set_timesteps(n)
    assert np.allclose(prod.timesteps.double().numpy(), np.asarray(ts, dtype=np.float64))
    g = torch.Generator().manual_seed(100 + n)
    for t in prod.timesteps:
        x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * float(ref.init_noise_sigma)
        v = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        eps = eps_of_v(name, ref, v.numpy(), x.numpy(), float(t))
        if name in STOCHASTIC:
            z = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
            got = prod.step(v, t, x, noise=z)[0]
            want = ref.step(eps, float(t), x.numpy(), z.numpy())
        else:
            got = prod.step(v, t, x)[0]
            want = ref.step(eps, float(t), x.numpy())
        assert np.allclose(got.numpy(), want, atol=atol), (name, float(t), np.abs(got.numpy() - want).max())


def _model(x, t):
    """A deterministic stand-in for a v-predicting UNet."""
    return 0.6 * np.tanh(x) + 0.2 * np.cos(float(t) / 150.0) - 0.1 * x


@pytest.mark.parametrize("name,ref_cls,n,atol", CASES)
def test_v_prediction_whole_loop_equals_oracle(name, ref_cls, n, atol):
    """Each side on its own trajectory, the model evaluated on its own (scaled) input: multistep histories, PLMS warm-up
    and UniPC's corrector all see v-prediction."""
    prod, ref = make(name, prediction_type="v_prediction"), ref_cls()
    prod.set_timesteps(n)
    ref.set_timesteps(n)
    g = torch.Generator().manual_seed(7 * n)
    x = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * float(ref.init_noise_sigma)
    xr = x.numpy().copy()
    for t in prod.timesteps:
        z = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
        v = torch.from_numpy(_model(prod.scale_model_input(x, t).numpy(), t))
        vr = _model(ref.scale_model_input(xr, float(t)), t)
        er = eps_of_v(name, ref, vr, xr, float(t))
        if name in STOCHASTIC:
            x = prod.step(v, t, x, noise=z)[0]
            xr = ref.step(er, float(t), xr, z.numpy())
        else:
            x = prod.step(v, t, x)[0]
            xr = ref.step(er, float(t), xr)
        assert np.allclose(x.numpy(), xr, atol=atol), (name, float(t), np.abs(x.numpy() - xr).max())


@pytest.mark.parametrize("start", [0, 3])
@pytest.mark.parametrize("name,n,kw", [("DDIM", 10, {}), ("DPM++ 2M", 8, {}), ("euler", 7, {}),
                                       ("DDIM", 6, {"rescale_betas_zero_snr": True, "timestep_spacing": "trailing"}),
                                       ("euler", 6, {"rescale_betas_zero_snr": True, "timestep_spacing": "trailing"}),
                                       ("DPM++ 2M", 6, {"timestep_spacing": "trailing"})])
def test_fused_plan_equals_step_under_v_prediction(name, n, kw, start):
    """As test_oracle.py::test_fused_plan_equals_step: the coefficients handed to the device step reproduce
    scheduler.step (fp32 emulation of the kernel), from the first step and from a mid-schedule start."""
    cfg = schedulers.DDIMScheduler(prediction_type="v_prediction").config
    a, b = (schedulers.REGISTRY[name](cfg).from_config(cfg, **kw) for _ in range(2))
    a.set_timesteps(n)
    b.set_timesteps(n)
    g = torch.Generator().manual_seed(n)
    xa = torch.randn(2, 4, 8, 8, generator=g) * float(a.init_noise_sigma)
    xb = xa.clone()
    hist = torch.zeros_like(xb)
    for t in a.timesteps.tolist()[start:]:
        v = torch.randn(2, 4, 8, 8, generator=g)
        plan = b.fused_plan(t)
        assert rel_l2(plan.in_scale * xb, b.scale_model_input(xb, t)) < 1e-6
        xa = a.step(v, t, xa)[0]
        x0 = plan.h_x * xb + plan.h_eps * v
        xb = plan.c_x * xb + plan.c_eps * v + (plan.c_hist * hist if plan.use_hist else 0.0)
        hist = x0
        b.fused_commit()
        assert all(np.isfinite(c) for c in (plan.c_x, plan.c_eps, plan.c_hist, plan.h_x, plan.h_eps))
        assert rel_l2(xb, xa) < 1e-5, (name, t)


def test_zero_terminal_snr_schedules():
    plain = schedulers.DDIMScheduler()
    d = schedulers.DDIMScheduler(rescale_betas_zero_snr=True)
    assert abs(d.ac[0] - plain.ac[0]) < 1e-15 and d.ac[-1] == 0.0
    assert np.all(np.diff(d.ac) < 0)
    r = np.sqrt(plain.ac)                                   # Lin et al., Alg. 1, restated
    want = ((r - r[-1]) * r[0] / (r[0] - r[-1])) ** 2
    assert np.allclose(d.ac, want, atol=1e-15)
    assert d.final_alpha_cumprod == d.ac[0]
    assert d.add_noise_coefficients(999) == (0.0, 1.0)      # add_noise follows the rescaled schedule
    x0, nz = torch.ones(1, 4, 2, 2), torch.full((1, 4, 2, 2), 3.0)
    assert torch.equal(d.add_noise(x0, nz, torch.tensor([999])), nz)
    e = schedulers.EulerDiscreteScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    assert e.ac[-1] == 2.0 ** -24 and abs(e.ac[0] - plain.ac[0]) < 1e-15      # the documented clamp
    assert np.allclose(e.ac[:-1], want[:-1], atol=1e-15)
    e.set_timesteps(10)
    assert abs(e.sigmas[0] - np.sqrt(2.0 ** 24 - 1.0)) < 1e-6
    assert abs(e.init_noise_sigma - np.sqrt(e.sigmas.max() ** 2 + 1.0)) < 1e-9     # sqrt(sigma_max^2 + 1), as before
    assert e.add_noise_coefficients(999.0) == (1.0, float(e.sigmas[0]))


@pytest.mark.parametrize("name", ["DDIM", "euler", "DPM++ 2M", "DPM++ 2M SDE Karras"])
def test_trailing_timesteps(name):
    s = make(name).from_config(schedulers.DDIMScheduler(timestep_spacing="trailing").config)
    s.set_timesteps(10)
    assert s.timesteps.tolist() == [999 - 100 * k for k in range(10)]
    s.set_timesteps(6)
    assert s.timesteps.tolist() == [999, 832, 666, 499, 332, 166]       # round(arange(1000, 0, -1000 / 6)) - 1


def test_ddim_zero_snr_first_step_closed_form():
    """alpha-bar_999 = 0: the sample is pure noise, x0 = -v, eps = x, so x_prev = sqrt(ab_prev) (-v) + sqrt(1 - ab_prev) x."""
    s = schedulers.DDIMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
    s.set_timesteps(10)
    g = torch.Generator().manual_seed(1)
    x, v = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(2))
    ab_prev = s.ac[899]
    got = s.step(v, 999, x)[0]
    assert torch.allclose(got, np.sqrt(ab_prev) * (-v) + np.sqrt(1.0 - ab_prev) * x, atol=1e-12)
    plan = s.fused_plan(999)
    assert abs(plan.c_x - np.sqrt(1.0 - ab_prev)) < 1e-12 and abs(plan.c_eps + np.sqrt(ab_prev)) < 1e-12


def test_value_errors():
    with pytest.raises(ValueError, match="prediction_type"):
        schedulers.DDIMScheduler(prediction_type="sample")
    for name in ("euler_a", "DPM++ 2M", "DPM++ 2M Karras", "DPM++ 2M SDE Karras", "PNDM", "uni_pc"):
        with pytest.raises(ValueError, match="rescale_betas_zero_snr"):
            schedulers.REGISTRY[name](schedulers.DDIMScheduler(rescale_betas_zero_snr=True).config)
    s = schedulers.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")      # epsilon-prediction
    s.set_timesteps(10)
    with pytest.raises(ValueError, match="alpha-bar is 0"):
        s.step(torch.zeros(1, 4, 2, 2), 999, torch.zeros(1, 4, 2, 2))
    assert torch.isfinite(s.step(torch.zeros(1, 4, 2, 2), 899, torch.ones(1, 4, 2, 2))[0]).all()
    for name in ("PNDM", "uni_pc"):
        t = schedulers.REGISTRY[name](schedulers.DDIMScheduler(timestep_spacing="trailing").config)
        with pytest.raises(ValueError, match="trailing"):
            t.set_timesteps(10)


@pytest.mark.parametrize("name", sorted(schedulers.REGISTRY))
def test_from_config_and_set_scheduler_carry_the_fields(name):
    zero = name in ("DDIM", "euler")
    src = schedulers.DDIMScheduler(prediction_type="v_prediction", timestep_spacing="trailing",
                                   rescale_betas_zero_snr=zero, beta_end=0.011)
    s = schedulers.REGISTRY[name](src.config)
    back = schedulers.DDIMScheduler.from_config(s.config)
    for c in (s.config, back.config):
        assert (c.prediction_type, c.timestep_spacing, c.rescale_betas_zero_snr, c.beta_end) == \
            ("v_prediction", "trailing", zero, 0.011)
    assert s.v_prediction and (s.ac[-1] < 1e-6) == zero
    from types import SimpleNamespace
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    m = SDModelWrapper(base=None, vae=vae, scheduler=schedulers.PNDMScheduler(), device="cpu", prediction_type="v_prediction")
    assert isinstance(m.scheduler, schedulers.PNDMScheduler) and m.scheduler.v_prediction
    m.configure_scheduler(timestep_spacing="trailing", rescale_betas_zero_snr=False)
    m.set_scheduler(name)
    c = m.scheduler.config
    assert (c.prediction_type, c.timestep_spacing, c.rescale_betas_zero_snr) == ("v_prediction", "trailing", False)
    assert type(m.scheduler) is type(s)
    # the default stays what it was
    assert schedulers.REGISTRY[name](schedulers.DDIMScheduler().config).config.prediction_type == "epsilon"


def test_read_scheduler_config(tmp_path):
    os.makedirs(tmp_path / "scheduler")
    cfg = {"_class_name": "EulerDiscreteScheduler", "_diffusers_version": "0.27.2", "beta_schedule": "scaled_linear",
           "beta_start": 0.00085, "beta_end": 0.012, "num_train_timesteps": 1000, "prediction_type": "v_prediction",
           "rescale_betas_zero_snr": True, "timestep_spacing": "trailing", "steps_offset": 1, "clip_sample": False,
           "interpolation_type": "linear", "use_karras_sigmas": False}
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    got = checkpoints.read_scheduler_config(str(tmp_path))
    assert got == {"num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "steps_offset": 1,
                   "timestep_spacing": "trailing", "prediction_type": "v_prediction", "rescale_betas_zero_snr": True}
    from types import SimpleNamespace
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 2, 3, 4)))
    m = SDModelWrapper(base=None, vae=vae, device="cpu")                       # the default Euler scheduler
    m.load_scheduler_config(str(tmp_path))
    assert isinstance(m.scheduler, schedulers.EulerDiscreteScheduler) and m.scheduler.v_prediction
    assert m.scheduler.config.timestep_spacing == "trailing" and m.scheduler.ac[-1] == 2.0 ** -24
    m.set_scheduler("DDIM")
    assert m.scheduler.v_prediction and m.scheduler.ac[-1] == 0.0
    cfg["beta_schedule"] = "squaredcos_cap_v2"
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="beta_schedule"):
        checkpoints.read_scheduler_config(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        checkpoints.read_scheduler_config(str(tmp_path / "scheduler"))
