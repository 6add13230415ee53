"""Host-side (PyTorch) schedulers with the diffusers call surface the reference pipeline uses.

`north_star` keeps the scheduler step on PyTorch-ROCm host code; in the reference these objects come
from diffusers (`/root/reference/models/stable_diffusion.py:199-227`) and are driven at
`/root/reference/pipelines/sd_unified_pipeline.py:203-207` (set_timesteps), `:472`
(scale_model_input), `:489` (step), `:502,:841` (add_noise), `:735` (.order / .timesteps),
`:785` (.init_noise_sigma), `:398` (.config.num_train_timesteps).
Constants follow `/root/reference/scripts/convert_from_A1111.py:947-959` (scaled_linear betas
0.00085..0.012, T=1000, steps_offset=1, set_alpha_to_one=False, clip_sample=False, epsilon).
Coefficients are evaluated in float64 on the host; tensors are updated in fp32 and cast back.

Beyond the reference's constants: `prediction_type="v_prediction"` (every scheduler: the model output is converted with
eps = a v + s x at the step it was made for, then the epsilon update runs), `rescale_betas_zero_snr` (Lin et al., "Common
Diffusion Noise Schedules and Sample Steps are Flawed", Alg. 1; DDIM and Euler) and `timestep_spacing="trailing"` (DDIM,
Euler, the DPM++ 2M family) -- what SD 2.x-768 and zero-terminal-SNR checkpoints are sampled with.  The fields live in
`.config` and travel through `from_config`.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch


class FusedPlan(SimpleNamespace):
    """One denoise step as the affine update the engine applies on the device (`sd_cfg_linear_step`):
        x0 = h_x x + h_eps eps;   x <- c_x x + c_eps eps + c_hist hist;   hist <- x0
    `in_scale` multiplies the UNet input (scale_model_input), `use_hist` says whether the scheduler
    carries an x0 history.  Coefficients are float64 host values."""


class AffinePlan(SimpleNamespace):
    """One denoise step as rows of float64 coefficients over v = (x, m, z, h_0 .. h_3) -- the sample, the model output,
    fresh noise and the fp32 history slots the scheduler keeps on the device (`sd_sched_affine_step`):
        x <- out . v;   h[slot] <- row . v  for (slot, row) in writes, every row from the old values
    `in_scale` multiplies the UNet input, `n_slots` is how many slots exist, `needs_noise` whether z has a non-zero
    coefficient.  The scheduler's `affine_plan` runs the arithmetic of its `step` on unit vectors in place of tensors, so
    a slot the step does not read has the coefficient 0 exactly; which slot holds which history entry is the scheduler's
    bookkeeping (a ring rotates by renaming), advanced by `affine_commit` once the step has been applied."""


AFFINE_COLS = 7


def _unit(k):
    v = np.zeros(AFFINE_COLS)
    v[k] = 1.0
    return v


def _slot(k):
    return _unit(3 + k)


def _affine_plan(in_scale, n_slots, out, writes):
    rows = [out] + [r for _, r in writes]
    return AffinePlan(in_scale=float(in_scale), n_slots=int(n_slots), out=[float(c) for c in out],
                      writes=[(int(k), [float(c) for c in r]) for k, r in writes],
                      needs_noise=any(r[2] != 0.0 for r in rows))


def _alphas_cumprod(T, beta_start, beta_end):
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def _rescale_zero_terminal_snr(ac):
    """Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", Alg. 1, on sqrt(alpha-bar):
    shifted so that the last value is 0 and scaled so that the first keeps its value."""
    r = ac ** 0.5
    r0, rT = r[0], r[-1]
    r = (r - rT) * r0 / (r0 - rT)
    return r ** 2


PREDICTION_TYPES = ("epsilon", "v_prediction")


class _Base:
    order = 1
    zero_snr = False              # rescale_betas_zero_snr is implemented (DDIM, Euler)
    zero_snr_floor = 0.0          # what alpha-bar_T becomes under it (a sigma-space scheduler cannot take 0)
    trailing = False              # timestep_spacing="trailing" is implemented (DDIM, Euler, the DPM++ 2M family)

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 timestep_spacing="leading", prediction_type="epsilon", rescale_betas_zero_snr=False, **extra):
        if prediction_type not in PREDICTION_TYPES:
            raise ValueError(f"prediction_type must be one of {PREDICTION_TYPES}, got {prediction_type!r}")
        if rescale_betas_zero_snr and not self.zero_snr:
            raise ValueError(f"{type(self).__name__} does not implement rescale_betas_zero_snr (DDIM and euler do)")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                      beta_end=beta_end, beta_schedule="scaled_linear",
                                      steps_offset=steps_offset, timestep_spacing=timestep_spacing,
                                      prediction_type=prediction_type,
                                      rescale_betas_zero_snr=bool(rescale_betas_zero_snr), **extra)
        self.ac = _alphas_cumprod(num_train_timesteps, beta_start, beta_end)
        if rescale_betas_zero_snr:
            self.ac = _rescale_zero_terminal_snr(self.ac)
            self.ac[-1] = self.zero_snr_floor
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, config, **kw):
        d = dict(vars(config)) if not isinstance(config, dict) else dict(config)
        keep = {k: d[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "steps_offset",
                                  "timestep_spacing", "prediction_type", "rescale_betas_zero_snr") if k in d}
        keep.update(kw)
        return cls(**keep)

    @property
    def v_prediction(self):
        return self.config.prediction_type == "v_prediction"

    def _leading(self, n, extra=0):
        if self.config.timestep_spacing == "trailing":
            raise ValueError(f"{type(self).__name__} does not implement timestep_spacing='trailing' "
                             "(DDIM, euler and the DPM++ 2M family do)")
        T = self.config.num_train_timesteps
        ratio = T // (n + extra)
        ts = (np.arange(0, n + extra) * ratio).round()[::-1].copy().astype(np.int64)
        return ts + self.config.steps_offset

    def _trailing(self, n):
        T = self.config.num_train_timesteps
        return np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1

    @staticmethod
    def _eps_from_v(v, x, a, s):
        """v-prediction -> epsilon in the space where x = a x0 + s eps (a^2 + s^2 = 1): eps = a v + s x."""
        return float(a) * v.float() + float(s) * x.float()

    @staticmethod
    def _plan_from_v(plan, a, s):
        """The same affine update written for a model that predicts v: eps = a v + s x substituted."""
        return FusedPlan(in_scale=plan.in_scale, c_x=float(plan.c_x + plan.c_eps * s), c_eps=float(plan.c_eps * a),
                         c_hist=plan.c_hist, h_x=float(plan.h_x + plan.h_eps * s), h_eps=float(plan.h_eps * a),
                         use_hist=plan.use_hist)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _begin(self, timestep):
        """Position in the sigma schedule of the step being taken.  The first call after
        set_timesteps resolves it from the timestep (diffusers `_init_step_index` /
        `index_for_timestep`: with duplicates the second match, so that a loop started mid-schedule
        -- img2img with strength < 1, denoising_start; sd_unified_pipeline.py:722-761 slices
        `timesteps[t_start * order:]` -- does not skip a sigma); later calls just count."""
        if self._i is None:
            if timestep is None:
                self._i = 0
            else:
                ts = self.timesteps.double().cpu().numpy()
                hit = np.nonzero(np.isclose(ts, float(timestep)))[0]
                if len(hit) == 0:
                    raise ValueError(f"timestep {float(timestep)} is not in the schedule set by set_timesteps")
                self._i = int(hit[1] if len(hit) > 1 else hit[0])
        return self._i

    def set_begin_index(self, begin_index=0):
        self._i = int(begin_index)

    def add_noise_coefficients(self, timestep):
        """(a, b) of add_noise(x0, noise, t) = a x0 + b noise for one timestep (host floats)."""
        t = int(timestep)
        return float(self.ac[t] ** 0.5), float((1 - self.ac[t]) ** 0.5)

    def add_noise(self, original, noise, timesteps):
        t = torch.as_tensor(timesteps).reshape(-1).long().cpu().numpy()
        a = torch.tensor(self.ac[t] ** 0.5, dtype=torch.float32, device=original.device)
        s = torch.tensor((1 - self.ac[t]) ** 0.5, dtype=torch.float32, device=original.device)
        while a.ndim < original.ndim:
            a, s = a.unsqueeze(-1), s.unsqueeze(-1)
        return (a * original.float() + s * noise.float()).to(original.dtype)


class DDIMScheduler(_Base):
    """eta = 0 DDIM."""
    zero_snr = True
    trailing = True

    def __init__(self, **kw):
        kw.setdefault("timestep_spacing", "leading")
        super().__init__(**kw)
        self.final_alpha_cumprod = self.ac[0]  # set_alpha_to_one=False

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        self.num_inference_steps = num_inference_steps
        trailing = self.config.timestep_spacing == "trailing"
        ts = self._trailing(num_inference_steps) if trailing else self._leading(num_inference_steps)
        self.timesteps = torch.from_numpy(ts).to(device)

    def step_coefficients(self, timestep):
        """x_prev = c_x * x + c_eps * model_output (DDIM eta=0 as one affine update), for the configured
        prediction type.  v-prediction: x0 = a x - s v, eps = a v + s x (a = sqrt(alpha-bar_t), s = sqrt(1 - alpha-bar_t)),
        which stays finite at alpha-bar_t = 0 (zero terminal SNR) where epsilon-prediction does not."""
        t = int(timestep)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.ac[t]
        a_prev = self.ac[prev] if prev >= 0 else self.final_alpha_cumprod
        if self.v_prediction:
            a, s_ = a_t ** 0.5, (1 - a_t) ** 0.5
            ap, sp = a_prev ** 0.5, (1 - a_prev) ** 0.5
            return float(ap * a + sp * s_), float(sp * a - ap * s_)
        if a_t <= 0.0:
            raise ValueError(f"epsilon-prediction cannot step from timestep {t}: alpha-bar is 0 there (zero terminal SNR "
                             "needs prediction_type='v_prediction')")
        c_x = (a_prev / a_t) ** 0.5
        c_eps = (1 - a_prev) ** 0.5 - (a_prev * (1 - a_t) / a_t) ** 0.5
        return float(c_x), float(c_eps)

    def fused_plan(self, timestep):
        c_x, c_eps = self.step_coefficients(timestep)
        return FusedPlan(in_scale=1.0, c_x=c_x, c_eps=c_eps, c_hist=0.0, h_x=0.0, h_eps=0.0, use_hist=False)

    def fused_commit(self):
        pass

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        c_x, c_eps = self.step_coefficients(timestep)
        prev = (c_x * sample.float() + c_eps * model_output.float()).to(sample.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)


class DPMSolverMultistepScheduler(_Base):
    """DPM-Solver++(2M), midpoint, lower_order_final, final sigma 0 ("DPM++ 2M" in the registry)."""
    trailing = True

    def __init__(self, **kw):
        kw.setdefault("timestep_spacing", "linspace")
        super().__init__(**kw)

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        n = num_inference_steps
        T = self.config.num_train_timesteps
        if self.config.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.config.timestep_spacing == "trailing":
            ts = self._trailing(n)
        else:
            ts = self._leading(n, extra=1)[:-1]
        sig_all = ((1 - self.ac) / self.ac) ** 0.5
        sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        self.sigmas = np.concatenate([sig, [0.0]])
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts).to(device)
        self._i = None
        self._m_prev = None
        self._fused_hist = False

    @staticmethod
    def _alpha_sigma(s):
        a = 1.0 / (s * s + 1.0) ** 0.5
        return a, s * a

    def fused_plan(self, timestep=None):
        """The arithmetic of `step` below, collected into coefficients of (x, eps, previous x0)."""
        i, n = self._begin(timestep), self.num_inference_steps
        a0, sg0 = self._alpha_sigma(self.sigmas[i])
        a_t, sg_t = self._alpha_sigma(self.sigmas[i + 1])
        lam0 = np.log(a0) - np.log(sg0)
        lam_t = np.log(a_t) - np.log(sg_t) if sg_t > 0 else np.inf
        h = lam_t - lam0
        em1 = float(np.exp(-h) - 1.0)
        h_x, h_eps = 1.0 / a0, -sg0 / a0
        first_order = i == n - 1 or not getattr(self, "_fused_hist", False)
        b, c_hist = -a_t * em1, 0.0
        if not first_order:
            a1, sg1 = self._alpha_sigma(self.sigmas[i - 1])
            r0 = (lam0 - (np.log(a1) - np.log(sg1))) / h
            b = -a_t * em1 * (1.0 + 0.5 / r0)
            c_hist = 0.5 * a_t * em1 / r0
        plan = FusedPlan(in_scale=1.0, c_x=float(sg_t / sg0 + b * h_x), c_eps=float(b * h_eps), c_hist=float(c_hist),
                         h_x=float(h_x), h_eps=float(h_eps), use_hist=True)
        return self._plan_from_v(plan, a0, sg0) if self.v_prediction else plan

    def fused_commit(self):
        self._fused_hist = True
        self._i += 1

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        i = self._begin(timestep)
        n = self.num_inference_steps
        a0, sg0 = self._alpha_sigma(self.sigmas[i])
        a_t, sg_t = self._alpha_sigma(self.sigmas[i + 1])
        x = sample.float()
        if self.v_prediction:
            model_output = self._eps_from_v(model_output, sample, a0, sg0)
        m0 = (x - sg0 * model_output.float()) / a0
        lam0 = np.log(a0) - np.log(sg0)
        lam_t = np.log(a_t) - np.log(sg_t) if sg_t > 0 else np.inf
        h = lam_t - lam0
        em1 = float(np.exp(-h) - 1.0)
        first_order = i == n - 1 or self._m_prev is None
        out = float(sg_t / sg0) * x - float(a_t) * em1 * m0
        if not first_order:
            a1, sg1 = self._alpha_sigma(self.sigmas[i - 1])
            lam1 = np.log(a1) - np.log(sg1)
            r0 = (lam0 - lam1) / h
            d1 = (m0 - self._m_prev) * float(1.0 / r0)
            out = out - 0.5 * float(a_t) * em1 * d1
        self._m_prev = m0
        self._i += 1
        prev = out.to(sample.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)


class EulerDiscreteScheduler(_Base):
    """The reference's default scheduler (stable_diffusion.py:135-138)."""
    zero_snr = True
    zero_snr_floor = 2.0 ** -24   # sigma_T = sqrt(1 / floor - 1) ~ 4096 (recalled from diffusers, unpinned: DESIGN.md section 8)
    trailing = True

    def __init__(self, **kw):
        kw.setdefault("timestep_spacing", "leading")
        super().__init__(**kw)

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        n = num_inference_steps
        trailing = self.config.timestep_spacing == "trailing"
        ts = (self._trailing(n) if trailing else self._leading(n)).astype(np.float64)
        sig_all = ((1 - self.ac) / self.ac) ** 0.5
        sig = np.interp(ts, np.arange(0, len(sig_all)), sig_all)
        self.sigmas = np.concatenate([sig, [0.0]])
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts.astype(np.float32)).to(device)
        self._i = None

    def scale_model_input(self, sample, timestep=None):
        s = self.sigmas[self._begin(timestep)]
        return (sample.float() / float((s * s + 1) ** 0.5)).to(sample.dtype)

    def add_noise_coefficients(self, timestep):
        ts = self.timesteps.double().cpu().numpy()
        return 1.0, float(self.sigmas[int(np.abs(ts - float(timestep)).argmin())])

    def add_noise(self, original, noise, timesteps):
        """sigma-space noising (diffusers EulerDiscreteScheduler.add_noise): x0 + sigma(t) * noise with
        sigma taken at the schedule position of each timestep (first match, else the nearest)."""
        ts = self.timesteps.double().cpu().numpy()
        want = torch.as_tensor(timesteps).reshape(-1).double().cpu().numpy()
        idx = [int(np.abs(ts - w).argmin()) for w in want]
        s = torch.tensor(self.sigmas[idx], dtype=torch.float32, device=original.device)
        while s.ndim < original.ndim:
            s = s.unsqueeze(-1)
        return (original.float() + s * noise.float()).to(original.dtype)

    @staticmethod
    def _v_terms(s):
        """(a, b) of eps = a v + b x for the UNSCALED sample x (the model saw x / sqrt(sigma^2 + 1)):
        eps = v / sqrt(sigma^2 + 1) + sigma x / (sigma^2 + 1)."""
        return 1.0 / (s * s + 1) ** 0.5, s / (s * s + 1)

    def fused_plan(self, timestep=None):
        i = self._begin(timestep)
        s, s_next = self.sigmas[i], self.sigmas[i + 1]
        plan = FusedPlan(in_scale=float(1.0 / (s * s + 1) ** 0.5), c_x=1.0, c_eps=float(s_next - s), c_hist=0.0,
                         h_x=0.0, h_eps=0.0, use_hist=False)
        return self._plan_from_v(plan, *self._v_terms(s)) if self.v_prediction else plan

    def fused_commit(self):
        self._i += 1

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        i = self._begin(timestep)
        s, s_next = self.sigmas[i], self.sigmas[i + 1]
        if self.v_prediction:
            # x + eps (s_next - s) with eps = a v + b x, collected on the host in float64: at a zero-terminal-SNR sigma
            # (~4096) the two x terms cancel to 1 part in 300, which fp32 tensors would pay for
            a, b = self._v_terms(s)
            prev = (float(1.0 + b * (s_next - s)) * sample.float() + float(a * (s_next - s)) * model_output.float())
            prev = prev.to(sample.dtype)
        else:
            prev = (sample.float() + model_output.float() * float(s_next - s)).to(sample.dtype)
        self._i += 1
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)


class EulerAncestralDiscreteScheduler(EulerDiscreteScheduler):
    """"euler_a" of the registry: Euler step to sigma_down plus fresh noise scaled by sigma_up.  The reference
    calls `step(noise_pred, t, latents)` without a generator (`sd_unified_pipeline.py:489`), so the noise comes
    from torch's global generator on the sample's device; `generator=` / `noise=` are accepted for tests."""

    supports_fused = False                    # stochastic: no affine device step
    zero_snr = False

    def step(self, model_output, timestep, sample, return_dict=False, generator=None, noise=None, **kw):
        i = self._begin(timestep)
        s, s_to = self.sigmas[i], self.sigmas[i + 1]
        s_up = (s_to ** 2 * (s ** 2 - s_to ** 2) / s ** 2) ** 0.5
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        x = sample.float()
        if self.v_prediction:
            a, b = self._v_terms(s)                              # as in EulerDiscreteScheduler.step
            prev = float(1.0 + b * (s_down - s)) * x + float(a * (s_down - s)) * model_output.float()
        else:
            prev = x + model_output.float() * float(s_down - s)  # derivative (x - x0) / sigma = eps
        if noise is None:
            noise = torch.randn(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype)
        prev = prev + noise.float() * float(s_up)
        self._i += 1
        prev = prev.to(sample.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)

    affine_slots = 0
    affine_noise = True                       # `step` draws noise on every step: the device loop draws it the same way

    def affine_plan(self, timestep=None):
        """The arithmetic of `step` on (x, m, z): no history.  The last step has sigma_up = 0: no noise term."""
        i = self._begin(timestep)
        s, s_to = self.sigmas[i], self.sigmas[i + 1]
        s_up = (s_to ** 2 * (s ** 2 - s_to ** 2) / s ** 2) ** 0.5
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        x, eps, z = _unit(0), _unit(1), _unit(2)
        if self.v_prediction:
            a, b = self._v_terms(s)
            eps = a * eps + b * x
        out = x + eps * (s_down - s) + z * s_up
        return _affine_plan(1.0 / (s * s + 1) ** 0.5, 0, out, [])

    def affine_commit(self):
        self._i += 1


def _karras_sigmas(sig_all, n, rho=7.0):
    """diffusers `_convert_to_karras` on the flipped training sigmas: n values from sigma_max down to sigma_min."""
    s_min, s_max = float(sig_all[0]), float(sig_all[-1])
    ramp = np.linspace(0, 1, n)
    lo, hi = s_min ** (1 / rho), s_max ** (1 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def _sigma_to_t(sigma, log_sigmas):
    """diffusers `_sigma_to_t`: fractional training timestep whose log-sigma interpolates to log(sigma)."""
    ls = np.log(np.maximum(sigma, 1e-10))
    dists = ls - log_sigmas[:, None]
    low = np.cumsum(dists >= 0, axis=0).argmax(axis=0).clip(max=len(log_sigmas) - 2)
    high = low + 1
    w = np.clip((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[high]), 0, 1)
    return (1 - w) * low + w * high


class DPMSolverKarrasScheduler(DPMSolverMultistepScheduler):
    """"DPM++ 2M Karras": DPMSolverMultistepScheduler.from_config(config, use_karras_sigmas=True)
    (`models/stable_diffusion.py:213-214`): Karras rho = 7 sigma ladder, timesteps = rounded sigma -> t."""

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        n = num_inference_steps
        sig_all = ((1 - self.ac) / self.ac) ** 0.5
        sig = _karras_sigmas(sig_all, n)
        ts = _sigma_to_t(sig, np.log(sig_all)).round().astype(np.int64)
        self.sigmas = np.concatenate([sig, [0.0]])
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts).to(device)
        self._i = None
        self._m_prev = None
        self._fused_hist = False


class DPMSolverSDEScheduler(DPMSolverMultistepScheduler):
    """"DPM++ 2M SDE Karras" of the registry: `from_config(config, se_karras_sigmas=True,
    algorithm_type="sde-dpmsolver++")` (`models/stable_diffusion.py:215-218`).  The keyword is misspelt in the
    reference (`se_karras_sigmas`), so diffusers keeps `use_karras_sigmas=False`: what actually runs is
    sde-dpmsolver++ (2M, midpoint) on the ordinary sigma schedule -- reproduced as it runs, not as it is named."""

    supports_fused = False                    # stochastic

    def step(self, model_output, timestep, sample, return_dict=False, generator=None, noise=None, **kw):
        i = self._begin(timestep)
        n = self.num_inference_steps
        a0, sg0 = self._alpha_sigma(self.sigmas[i])
        a_t, sg_t = self._alpha_sigma(self.sigmas[i + 1])
        x = sample.float()
        if self.v_prediction:
            model_output = self._eps_from_v(model_output, sample, a0, sg0)
        m0 = (x - sg0 * model_output.float()) / a0
        lam0 = np.log(a0) - np.log(sg0)
        lam_t = np.log(a_t) - np.log(sg_t) if sg_t > 0 else np.inf
        h = lam_t - lam0
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=sample.device, dtype=model_output.dtype)
        e1, e2 = float(np.exp(-h)), float(1.0 - np.exp(-2.0 * h))
        out = float(sg_t / sg0 * e1) * x + float(a_t * e2) * m0 + float(sg_t * e2 ** 0.5) * noise.float()
        if not (i == n - 1 or self._m_prev is None):
            a1, sg1 = self._alpha_sigma(self.sigmas[i - 1])
            r0 = (lam0 - (np.log(a1) - np.log(sg1))) / h
            out = out + float(0.5 * a_t * e2 / r0) * (m0 - self._m_prev)
        self._m_prev = m0
        self._i += 1
        prev = out.to(sample.dtype)
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)

    affine_slots = 1                          # the previous x0 prediction
    affine_noise = True

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        super().set_timesteps(num_inference_steps, device=device, **kw)
        self._aff_hist = False                # affine_plan: slot 0 has been written

    def affine_plan(self, timestep=None):
        """The arithmetic of `step` on (x, m, z, previous x0).  The last step goes to sigma 0: its noise coefficient
        is 0."""
        i, n = self._begin(timestep), self.num_inference_steps
        a0, sg0 = self._alpha_sigma(self.sigmas[i])
        a_t, sg_t = self._alpha_sigma(self.sigmas[i + 1])
        x, eps, z = _unit(0), _unit(1), _unit(2)
        if self.v_prediction:
            eps = a0 * eps + sg0 * x
        m0 = (x - sg0 * eps) / a0
        lam0 = np.log(a0) - np.log(sg0)
        lam_t = np.log(a_t) - np.log(sg_t) if sg_t > 0 else np.inf
        h = lam_t - lam0
        e1, e2 = float(np.exp(-h)), float(1.0 - np.exp(-2.0 * h))
        out = (sg_t / sg0 * e1) * x + (a_t * e2) * m0 + (sg_t * e2 ** 0.5) * z
        if not (i == n - 1 or not self._aff_hist):
            a1, sg1 = self._alpha_sigma(self.sigmas[i - 1])
            r0 = (lam0 - (np.log(a1) - np.log(sg1))) / h
            out = out + (0.5 * a_t * e2 / r0) * (m0 - _slot(0))
        return _affine_plan(1.0, 1, out, [(0, m0)])

    def affine_commit(self):
        self._aff_hist = True
        self._i += 1


class PNDMScheduler(_Base):
    """PLMS (PNDM with skip_prk_steps=True, as every SD scheduler config has it): 4th-order linear multistep
    on epsilon; the schedule has num_inference_steps + 1 entries (the second value is visited twice)."""

    def __init__(self, **kw):
        kw.setdefault("timestep_spacing", "leading")
        super().__init__(**kw)
        self.final_alpha_cumprod = self.ac[0]  # set_alpha_to_one=False

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        n = num_inference_steps
        self.num_inference_steps = n
        base = self._leading(n)[::-1]                                   # ascending
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(plms.astype(np.int64)).to(device)
        self.ets = []
        self.counter = 0
        self.cur_sample = None
        self._aff_ets = []                    # affine_plan: the slots of the kept epsilons, oldest first
        self._aff_cur = None                  # ... and the slot of the saved sample
        self._aff_next = None

    def _prev_sample(self, sample, t, prev_t, eps):
        a_t = self.ac[t]
        a_p = self.ac[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_p = 1 - a_t, 1 - a_p
        coeff = (a_p / a_t) ** 0.5
        denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
        return float(coeff) * sample - float((a_p - a_t) / denom) * eps

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        t = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev_t = t - ratio
        if self.v_prediction:                 # converted at the timestep and sample the model saw, then PLMS on eps
            model_output = self._eps_from_v(model_output, sample, self.ac[t] ** 0.5, (1 - self.ac[t]) ** 0.5)
        eps = model_output.float()
        x = sample.float()
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(eps)
        else:
            prev_t = t
            t = t + ratio
        if len(self.ets) == 1 and self.counter == 0:
            self.cur_sample = x
        elif len(self.ets) == 1 and self.counter == 1:
            eps = (eps + self.ets[-1]) / 2
            x = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            eps = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            eps = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            eps = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        prev = self._prev_sample(x, t, prev_t, eps).to(sample.dtype)
        self.counter += 1
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)

    affine_slots = 3                          # three earlier epsilons; the saved sample borrows one on the first two steps

    def affine_plan(self, timestep):
        """The arithmetic of `step` on (x, m, kept epsilons, saved sample).  `step` keeps four epsilons, the newest being
        this step's own: three slots hold the earlier ones and the new one overwrites the oldest (read in the same step).
        The sample saved by the first step is read by the second only, before the ring needs its slot."""
        t = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev_t = t - ratio
        x, eps = _unit(0), _unit(1)
        if self.v_prediction:
            eps = self.ac[t] ** 0.5 * eps + (1 - self.ac[t]) ** 0.5 * x
        slots, cur, writes = list(self._aff_ets), self._aff_cur, []
        ets = [_slot(k) for k in slots]
        if self.counter != 1:
            ets = ets[-3:] + [eps]
            free = [k for k in range(self.affine_slots) if k not in slots]
            new = free[0] if free else slots.pop(0)
            writes.append((new, eps))
            slots.append(new)
        else:
            prev_t = t
            t = t + ratio
        if len(ets) == 1 and self.counter == 0:
            cur = next(k for k in range(self.affine_slots) if k not in slots)
            writes.append((cur, x))
        elif len(ets) == 1 and self.counter == 1:
            eps = (eps + ets[-1]) / 2
            x, cur = _slot(cur), None
        elif len(ets) == 2:
            eps = (3 * ets[-1] - ets[-2]) / 2
        elif len(ets) == 3:
            eps = (23 * ets[-1] - 16 * ets[-2] + 5 * ets[-3]) / 12
        else:
            eps = (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4]) / 24
        self._aff_next = (slots, cur)
        return _affine_plan(1.0, self.affine_slots, self._prev_sample(x, t, prev_t, eps), writes)

    def affine_commit(self):
        self._aff_ets, self._aff_cur = self._aff_next
        self.counter += 1


class UniPCMultistepScheduler(_Base):
    """UniPC (order 2, bh2, predict_x0, lower_order_final): UniP predictor + UniC corrector on the data
    prediction; sigma schedule by linear interpolation, last sigma = the training schedule's smallest."""
    solver_order = 2

    def __init__(self, **kw):
        kw.setdefault("timestep_spacing", "linspace")
        super().__init__(**kw)

    def set_timesteps(self, num_inference_steps, device=None, **kw):
        n = num_inference_steps
        T = self.config.num_train_timesteps
        if self.config.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        else:
            ts = self._leading(n, extra=1)[:-1]
        sig_all = ((1 - self.ac) / self.ac) ** 0.5
        self.sigmas = np.concatenate([np.interp(ts, np.arange(0, len(sig_all)), sig_all), [sig_all[0]]])
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(ts).to(device)
        self._i = None
        self.model_outputs = [None] * self.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self.this_order = 1
        self._aff_x0 = []                     # affine_plan: the slots (0, 1) of the x0 predictions, oldest first
        self._aff_last = False                # ... and whether slot 2 holds the corrected sample
        self._aff_next = None

    @staticmethod
    def _al(s):
        a = 1.0 / (s * s + 1.0) ** 0.5
        return a, s * a, np.log(a) - np.log(s * a)

    def _bh_terms(self, h, order):
        hh = -h
        h_phi_1 = np.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = np.expm1(hh)
        fact, b = 1, []
        for k in range(1, order + 1):
            b.append(h_phi_k * fact / B_h)
            fact *= k + 1
            h_phi_k = h_phi_k / hh - 1 / fact
        return h_phi_1, B_h, np.array(b)

    def _predict(self, sample, order, outputs=None):
        i = self._i
        outputs = self.model_outputs if outputs is None else outputs
        m0 = outputs[-1]
        a_t, sg_t, lam_t = self._al(self.sigmas[i + 1])
        a_0, sg_0, lam_0 = self._al(self.sigmas[i])
        h = lam_t - lam_0
        h_phi_1, B_h, _ = self._bh_terms(h, order)
        x_t = float(sg_t / sg_0) * sample - float(a_t * h_phi_1) * m0
        if order == 2:
            _, _, lam_1 = self._al(self.sigmas[i - 1])
            rk = (lam_1 - lam_0) / h
            d1 = (outputs[-2] - m0) / float(rk)
            x_t = x_t - float(a_t * B_h * 0.5) * d1
        return x_t

    def _correct(self, model_t, last_sample, order, outputs=None):
        i = self._i
        outputs = self.model_outputs if outputs is None else outputs
        m0 = outputs[-1]
        a_t, sg_t, lam_t = self._al(self.sigmas[i])
        a_0, sg_0, lam_0 = self._al(self.sigmas[i - 1])
        h = lam_t - lam_0
        h_phi_1, B_h, b = self._bh_terms(h, order)
        x_t = float(sg_t / sg_0) * last_sample - float(a_t * h_phi_1) * m0
        if order == 1:
            rhos = np.array([0.5])
            corr = 0.0
        else:
            _, _, lam_1 = self._al(self.sigmas[i - 2])
            rk = (lam_1 - lam_0) / h
            R = np.array([[1.0, 1.0], [rk, 1.0]])
            rhos = np.linalg.solve(R, b)
            corr = float(rhos[0]) * ((outputs[-2] - m0) / float(rk))
        return x_t - float(a_t * B_h) * (corr + float(rhos[-1]) * (model_t - m0))

    def step(self, model_output, timestep, sample, return_dict=False, **kw):
        i = self._begin(timestep)
        n = len(self.timesteps)
        x = sample.float()
        a_i, sg_i, _ = self._al(self.sigmas[i])
        if self.v_prediction:
            model_output = self._eps_from_v(model_output, sample, a_i, sg_i)
        x0 = (x - float(sg_i) * model_output.float()) / float(a_i)
        if i > 0 and self.last_sample is not None:
            x = self._correct(x0, self.last_sample, self.this_order)
        self.model_outputs = self.model_outputs[1:] + [x0]
        order = min(self.solver_order, n - i)                    # lower_order_final
        self.this_order = min(order, self.lower_order_nums + 1)
        self.last_sample = x
        prev = self._predict(x, self.this_order).to(sample.dtype)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self._i += 1
        return (prev,) if not return_dict else SimpleNamespace(prev_sample=prev)

    affine_slots = 3                          # two x0 predictions and the corrected sample

    def affine_plan(self, timestep=None):
        """The arithmetic of `step` on (x, m, the two kept x0 predictions, the corrected sample of the previous step):
        `_correct` and `_predict` themselves, on unit vectors.  Every step writes its x0 over the older of the two
        (which the corrector still reads) and its corrected sample to slot 2."""
        i = self._begin(timestep)
        n = len(self.timesteps)
        x, eps = _unit(0), _unit(1)
        a_i, sg_i, _ = self._al(self.sigmas[i])
        if self.v_prediction:
            eps = a_i * eps + sg_i * x
        x0 = (x - sg_i * eps) / a_i
        slots = list(self._aff_x0)
        outputs = [None] * (self.solver_order - len(slots)) + [_slot(k) for k in slots]
        if i > 0 and self._aff_last:
            x = self._correct(x0, _slot(2), self.this_order, outputs)
        outputs = outputs[1:] + [x0]
        order = min(self.solver_order, n - i)                    # lower_order_final
        this_order = min(order, self.lower_order_nums + 1)
        out = self._predict(x, this_order, outputs)
        free = [k for k in range(self.solver_order) if k not in slots]
        new = free[0] if free else slots.pop(0)
        self._aff_next = (slots + [new], this_order)
        return _affine_plan(1.0, self.affine_slots, out, [(new, x0), (2, x)])

    def affine_commit(self):
        self._aff_x0, self.this_order = self._aff_next
        self._aff_last = True
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self._i += 1


class LCMScheduler(_Base):
    """Latent Consistency Model sampling (Luo et al. 2023; diffusers 0.27.2 `LCMScheduler`, recalled and unpinned:
    DESIGN.md section 8): the model output becomes an x0 prediction, the consistency boundary condition mixes it with the
    sample (c_skip, c_out), and every step but the last re-noises the result to the NEXT timestep of the schedule.
    2-8 steps, taken from the `original_inference_steps` the model was distilled on.  For guidance-embedded UNets
    (`time_cond_proj_dim`) and for ordinary checkpoints with an LCM-LoRA fused in.

    Stochastic, and not affine in (x, eps) alone: its device step is `sd_lcm_step` (`fused_plan` returns that kernel's
    coefficients), not the CFG step of the deterministic schedulers (`supports_fused = False` keeps it off that path)."""

    supports_fused = False
    sigma_data = 0.5

    def __init__(self, original_inference_steps=50, timestep_scaling=10.0, set_alpha_to_one=True, **kw):
        if kw.get("timestep_spacing", "leading") == "trailing":
            raise ValueError("LCMScheduler does not implement timestep_spacing='trailing'")
        kw["timestep_spacing"] = "leading"         # (unused: the schedule is a subset of the distillation's)
        super().__init__(original_inference_steps=int(original_inference_steps), timestep_scaling=float(timestep_scaling),
                         set_alpha_to_one=bool(set_alpha_to_one), **kw)
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else self.ac[0]
        self._i = None

    @classmethod
    def from_config(cls, config, **kw):
        d = dict(vars(config)) if not isinstance(config, dict) else dict(config)
        keep = {k: d[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "steps_offset", "prediction_type",
                                  "rescale_betas_zero_snr", "original_inference_steps", "timestep_scaling",
                                  "set_alpha_to_one") if k in d}
        if d.get("timestep_spacing") == "trailing":      # another scheduler's linspace / leading says nothing here
            keep["timestep_spacing"] = "trailing"
        keep.update(kw)
        return cls(**keep)

    def set_timesteps(self, num_inference_steps, device=None, original_inference_steps=None, strength=1.0, **kw):
        n = int(num_inference_steps)
        T = self.config.num_train_timesteps
        original = int(original_inference_steps or self.config.original_inference_steps)
        if original > T:
            raise ValueError(f"original_inference_steps {original} cannot exceed num_train_timesteps {T}")
        if n > original:
            raise ValueError(f"num_inference_steps {n} cannot exceed original_inference_steps {original}")
        k = T // original
        origin = np.arange(1, int(original * strength) + 1) * k - 1
        if n < 1 or len(origin) // n < 1:
            raise ValueError(f"{len(origin)} distillation timesteps (original_inference_steps {original} x strength "
                             f"{strength}) are fewer than num_inference_steps {n}")
        origin = origin[::-1].copy()
        idx = np.floor(np.linspace(0, len(origin), n, endpoint=False)).astype(np.int64)
        self.num_inference_steps = n
        self.timesteps = torch.from_numpy(origin[idx].astype(np.int64)).to(device)
        self._ts = [int(v) for v in origin[idx]]
        self._i = None

    def _boundary(self, t):
        s = float(t) * self.config.timestep_scaling
        sd2 = self.sigma_data ** 2
        return sd2 / (s * s + sd2), s / (s * s + sd2) ** 0.5          # c_skip, c_out

    def _coefficients(self, timestep):
        """(d_x, d_out, p_den, p_noise, last) of the step at this position, float64:
            denoised = d_x x + d_out model_output;   prev = p_den denoised + p_noise noise"""
        i = self._begin(timestep)
        t = self._ts[i]
        last = i == len(self._ts) - 1
        a = self.ac[t]
        ra, rb = a ** 0.5, (1 - a) ** 0.5
        c_skip, c_out = self._boundary(t)
        if self.v_prediction:                      # x0 = ra x - rb v
            d_x, d_out = c_skip + c_out * ra, -c_out * rb
        else:                                      # x0 = (x - rb eps) / ra
            if a <= 0.0:
                raise ValueError(f"epsilon-prediction cannot step from timestep {t}: alpha-bar is 0 there")
            d_x, d_out = c_skip + c_out / ra, -c_out * rb / ra
        if last:
            return float(d_x), float(d_out), 1.0, 0.0, True
        a_prev = self.ac[self._ts[i + 1]]
        return float(d_x), float(d_out), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5), False

    def fused_plan(self, timestep=None):
        """The step as `sd_lcm_step` applies it; v-prediction is eps = a v + s x substituted into d_x / d_out (what
        `_plan_from_v` does for the affine schedulers -- `_coefficients` writes both forms out)."""
        d_x, d_out, p_den, p_noise, last = self._coefficients(timestep)
        return FusedPlan(in_scale=1.0, d_x=d_x, d_out=d_out, p_den=p_den, p_noise=p_noise, needs_noise=not last)

    def fused_commit(self):
        self._i += 1

    def step(self, model_output, timestep, sample, generator=None, noise=None, return_dict=False, **kw):
        """-> (prev_sample, denoised).  The last step adds no noise: prev_sample is denoised."""
        d_x, d_out, p_den, p_noise, last = self._coefficients(timestep)
        denoised = d_x * sample.float() + d_out * model_output.float()
        prev = denoised
        if not last:
            if noise is None:
                noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                    dtype=model_output.dtype)
            prev = p_den * denoised + p_noise * noise.float()
        self._i += 1
        prev, denoised = prev.to(sample.dtype), denoised.to(sample.dtype)
        return (prev, denoised) if not return_dict else SimpleNamespace(prev_sample=prev, denoised=denoised)


REGISTRY = {
    # names of /root/reference/models/stable_diffusion.py:199-227 (all eight)
    "DDIM": lambda cfg: DDIMScheduler.from_config(cfg),
    "euler": lambda cfg: EulerDiscreteScheduler.from_config(cfg),
    "euler_a": lambda cfg: EulerAncestralDiscreteScheduler.from_config(cfg),
    "DPM++ 2M": lambda cfg: DPMSolverMultistepScheduler.from_config(cfg),
    "DPM++ 2M Karras": lambda cfg: DPMSolverKarrasScheduler.from_config(cfg),
    "DPM++ 2M SDE Karras": lambda cfg: DPMSolverSDEScheduler.from_config(cfg),
    "PNDM": lambda cfg: PNDMScheduler.from_config(cfg),
    "uni_pc": lambda cfg: UniPCMultistepScheduler.from_config(cfg),
}

# Schedulers beyond the reference's eight (REGISTRY stays the reference's list); SDModelWrapper.set_scheduler looks here next.
EXTRA_SCHEDULERS = {
    "lcm": lambda cfg: LCMScheduler.from_config(cfg),
}
