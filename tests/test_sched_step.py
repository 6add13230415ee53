"""The device step of euler_a, DPM++ 2M SDE, PNDM and UniPC, host side: the schedulers' `affine_plan` rows against the
oracle's float64 classes and against their own `step`, the slot bookkeeping, the ABI of sd_sched_affine_step and the
reference the GPU test compares with.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sched_step_oracle as sso
from stablediffusion_amd import _lib, schedulers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 4, 8, 8)


def _data(n_draws, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(SHAPE, generator=g).double()
    outs = [torch.randn(SHAPE, generator=g).double() for _ in range(n_draws)]
    noises = [torch.randn(SHAPE, generator=g).double() for _ in range(n_draws)]
    return x, outs, noises


class PlanLoop:
    """A scheduler driven through affine_plan / affine_commit, the rows applied in float64 (sso.apply_plan)."""

    def __init__(self, sched, x):
        self.s, self.x = sched, x.copy()
        self.bank = np.full((4,) + x.shape, np.nan)             # nothing may be read before it was written
        self.max_slots = self.max_writes = 0

    def step(self, t, m, z):
        plan = self.s.affine_plan(t)
        self.max_slots, self.max_writes = max(self.max_slots, plan.n_slots), max(self.max_writes, len(plan.writes))
        assert len({k for k, _ in plan.writes}) == len(plan.writes) and all(0 <= k < plan.n_slots for k, _ in plan.writes)
        scaled = plan.in_scale * self.x
        self.x, writes = sso.apply_plan(plan, self.x, m, z if plan.needs_noise else None, self.bank)
        for k, v in writes.items():
            self.bank[k] = v
        self.s.affine_commit()
        return scaled


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("n", [2, 3, 7, 30])
@pytest.mark.parametrize("name", list(sso.NAMES))
def test_plans_match_oracle_trajectories(name, n):
    """Whole trajectories with random model outputs and shared noise: the plan rows applied in float64 against the
    oracle's class (atol 1e-9: only the order of float64 sums differs), and the plan loop started at timesteps[2:]
    against the scheduler's own `step` loop started there (atol 5e-5: `step` computes in fp32)."""
    ref_cls, stochastic = sso.NAMES[name]
    prod, ref = sso.make(name), ref_cls()
    prod.set_timesteps(n)
    ts_ref = ref.set_timesteps(n)
    ts = prod.timesteps.tolist()
    assert np.allclose(ts, np.asarray(ts_ref, dtype=np.float64))
    x, outs, noises = _data(len(ts), n)
    x = x * float(ref.init_noise_sigma)
    xr = x.numpy().copy()
    loop = PlanLoop(prod, xr)
    worst = 0.0
    for i, t in enumerate(ts):
        m, z = outs[i].numpy(), noises[i].numpy()
        want_in = ref.scale_model_input(xr, float(t))
        xr = ref.step(m, float(t), xr, z) if stochastic else ref.step(m, float(t), xr)
        assert np.allclose(loop.step(t, m, z), want_in, atol=1e-9)
        worst = max(worst, np.abs(loop.x - xr).max())
        assert np.allclose(loop.x, xr, atol=1e-9, rtol=0), (name, n, i, worst)
    print(f"{name} n={n}: max |plan - oracle| {worst:.2e}, max |x| {np.abs(xr).max():.1f}")
    assert loop.max_slots <= prod.affine_slots <= 4 and loop.max_writes <= 2
    # a loop entered in the middle of the schedule (img2img strength < 1, denoising_start)
    host, dev = sso.make(name), sso.make(name)
    host.set_timesteps(n)
    dev.set_timesteps(n)
    xh = x.clone()
    loop = PlanLoop(dev, x.numpy())
    for i, t in list(enumerate(ts))[2:]:
        kw = dict(noise=noises[i]) if stochastic else {}
        want_in = host.scale_model_input(xh, t).numpy()
        xh = host.step(outs[i], t, xh, **kw)[0]
        assert np.allclose(loop.step(t, outs[i].numpy(), noises[i].numpy()), want_in, atol=5e-5)
        assert np.allclose(loop.x, xh.numpy(), atol=5e-5, rtol=0), (name, n, i, np.abs(loop.x - xh.numpy()).max())


# ------------------------------------------------------------------------------------------------ 2. against `step`
@pytest.mark.parametrize("n", [3, 7])
@pytest.mark.parametrize("pred", sso.PREDICTIONS)
@pytest.mark.parametrize("name", list(sso.NAMES))
def test_plans_match_step_both_prediction_types(name, pred, n):
    """The class's own `step` on float64 tensors (it computes in fp32: atol 5e-5, as
    test_remaining_registry_schedulers_match_oracle compares it with the oracle)."""
    stochastic = sso.NAMES[name][1]
    host, dev = sso.make(name, pred), sso.make(name, pred)
    host.set_timesteps(n)
    dev.set_timesteps(n)
    ts = host.timesteps.tolist()
    x, outs, noises = _data(len(ts), 10 * n + len(pred))
    x = x * float(host.init_noise_sigma)
    loop = PlanLoop(dev, x.numpy())
    for i, t in enumerate(ts):
        kw = dict(noise=noises[i]) if stochastic else {}
        want_in = host.scale_model_input(x, t).numpy()
        x = host.step(outs[i], t, x, **kw)[0]
        assert np.allclose(loop.step(t, outs[i].numpy(), noises[i].numpy()), want_in, atol=5e-5)
        assert np.allclose(loop.x, x.numpy(), atol=5e-5, rtol=0), (name, pred, i, np.abs(loop.x - x.numpy()).max())


# ------------------------------------------------------------------------------------------------ 3. bookkeeping
@pytest.mark.parametrize("name", list(sso.NAMES))
def test_bookkeeping(name):
    s = sso.make(name)
    assert 0 <= s.affine_slots <= 4
    assert s.affine_slots == {"euler_a": 0, "DPM++ 2M SDE Karras": 1, "PNDM": 3, "uni_pc": 3}[name]
    assert bool(getattr(s, "affine_noise", False)) == sso.NAMES[name][1]

    def run():
        s.set_timesteps(7)
        rows = []
        for t in s.timesteps.tolist():
            p = s.affine_plan(t)
            assert p.n_slots <= s.affine_slots and len(p.writes) <= 2
            assert len(p.out) == sso.COLS and all(len(r) == sso.COLS for _, r in p.writes)
            rows.append((p.in_scale, p.n_slots, p.out, p.writes, p.needs_noise))
            s.affine_commit()
        return rows

    first = run()
    assert run() == first                                       # set_timesteps resets the slots, counters and orders
    writes = [len(r[3]) for r in first]
    noise = [r[4] for r in first]
    if name == "euler_a":
        assert writes == [0] * 7 and noise == [True] * 6 + [False]
    elif name == "DPM++ 2M SDE Karras":
        assert writes == [1] * 7 and noise == [True] * 6 + [False]
    elif name == "PNDM":
        assert writes == [2, 0] + [1] * 6 and not any(noise)    # two writes on the first step only
    else:
        assert writes == [2] * 7 and not any(noise)
    # a plan that is not committed changes nothing
    s.set_timesteps(7)
    t0 = s.timesteps.tolist()[0]
    a = s.affine_plan(t0)
    b = s.affine_plan(t0)
    assert (a.out, a.writes) == (b.out, b.writes)
    # the deterministic CFG step stays closed to all four, as before
    assert not (hasattr(s, "fused_plan") and getattr(s, "supports_fused", True))
    assert hasattr(s, "fused_plan") == (name in ("euler_a", "DPM++ 2M SDE Karras"))       # (inherited, switched off)
    assert getattr(s, "supports_fused", True) == (name in ("PNDM", "uni_pc"))


def test_unread_slots_have_exact_zero_coefficients():
    """PNDM's early steps and UniPC's first steps must not read slots nobody has written."""
    for name in ("PNDM", "uni_pc", "DPM++ 2M SDE Karras"):
        s = sso.make(name)
        s.set_timesteps(7)
        written = set()
        for t in s.timesteps.tolist():
            p = s.affine_plan(t)
            for k in range(4):
                if k not in written:
                    assert p.out[3 + k] == 0.0 and all(r[3 + k] == 0.0 for _, r in p.writes), (name, t, k)
            written |= {k for k, _ in p.writes}
            s.affine_commit()


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_step_plan_struct_matches_header():
    src = open(os.path.join(ROOT, "include", "sd_engine.h")).read()
    body = re.search(r"typedef struct sd_step_plan \{(.*?)\} sd_step_plan;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.SdStepPlan._fields_]
    assert (_lib.SD_STEP_MAX_SLOTS, _lib.SD_STEP_MAX_WRITES) == (4, 2)
    assert re.search(r"#define SD_STEP_MAX_SLOTS 4\b", src) and re.search(r"#define SD_STEP_MAX_WRITES 2\b", src)
    assert C.sizeof(_lib.SdStepPlan) == 4 * 4 + 8 * 7 * 3 and _lib.SdStepPlan.out.offset == 16
    p = _lib.step_plan(sso.dense_plan())
    assert (p.n_slots, p.n_writes, list(p.write_slot)) == (4, 2, [3, 1])
    assert list(p.out) == sso.dense_plan().out and list(p.write[1]) == sso.dense_plan().writes[1][1]


def _plan(n_slots=0, writes=(), out=(1.0, 0.5, 0.0, 0, 0, 0, 0)):
    p = _lib.SdStepPlan(n_slots=n_slots, n_writes=len(writes))
    p.out[:] = out
    for j, (slot, row) in enumerate(writes):
        p.write_slot[j] = slot
        p.write[j][:] = row
    return p


def invalid_calls():
    """(label, args of sd_sched_affine_step without the stream) for every SD_ERR_INVALID case; 64 stands for a pointer."""
    p, n = 64, 8
    row = (1.0, 1.0, 0.0, 0, 0, 0, 0)
    nan, inf = float("nan"), float("inf")
    ok = _plan()
    return [
        ("rows 0", (p, 0, p, None, None, 0, n, 1.0, ok)), ("rows 3", (p, 3, p, None, None, 0, n, 1.0, ok)),
        ("n 0", (p, 1, p, None, None, 0, 0, 1.0, ok)), ("n < 0", (p, 1, p, None, None, 0, -8, 1.0, ok)),
        ("null model_out", (None, 1, p, None, None, 0, n, 1.0, ok)), ("null latents", (p, 1, None, None, None, 0, n, 1.0, ok)),
        ("null plan", (p, 1, p, None, None, 0, n, 1.0, None)),
        ("n_slots 5", (p, 1, p, None, p, n, n, 1.0, _plan(5))), ("n_slots -1", (p, 1, p, None, p, n, n, 1.0, _plan(-1))),
        ("n_writes 3", (p, 1, p, None, p, n, n, 1.0, _lib.SdStepPlan(n_slots=4, n_writes=3))),
        ("n_writes -1", (p, 1, p, None, p, n, n, 1.0, _lib.SdStepPlan(n_slots=4, n_writes=-1))),
        ("write_slot >= n_slots", (p, 1, p, None, p, n, n, 1.0, _plan(2, [(2, row)]))),
        ("write_slot < 0", (p, 1, p, None, p, n, n, 1.0, _plan(2, [(-1, row)]))),
        ("write_slot repeated", (p, 1, p, None, p, n, n, 1.0, _plan(2, [(1, row), (1, row)]))),
        ("null bank", (p, 1, p, None, None, n, n, 1.0, _plan(1))),
        ("bank_stride < n", (p, 1, p, None, p, n - 1, n, 1.0, _plan(1))),
        ("null noise, z in out", (p, 1, p, None, None, 0, n, 1.0, _plan(out=(1.0, 1.0, 0.5, 0, 0, 0, 0)))),
        ("null noise, z in a write", (p, 1, p, None, p, n, n, 1.0, _plan(1, [(0, (1.0, 0, 0.5, 0, 0, 0, 0))]))),
        ("nan in out", (p, 1, p, None, None, 0, n, 1.0, _plan(out=(nan, 1.0, 0, 0, 0, 0, 0)))),
        ("inf in a write", (p, 1, p, None, p, n, n, 1.0, _plan(1, [(0, (1.0, inf, 0, 0, 0, 0, 0))]))),
        ("nan in a used slot column", (p, 1, p, None, p, n, n, 1.0, _plan(1, out=(1.0, 1.0, 0, nan, 0, 0, 0)))),
    ]


def call(lib, args, stream=None):
    *head, plan = args
    ptr = lambda v: None if v is None else C.c_void_p(v) if isinstance(v, int) else v
    mo, rows, lat, nz, bank, stride, n, g = head
    return lib.sd_sched_affine_step(ptr(mo), rows, ptr(lat), ptr(nz), ptr(bank), stride, n, g,
                                    None if plan is None else C.byref(plan), stream)


def test_entry_rejects_bad_arguments(engine_lib):
    """sd_sched_affine_step validates before it launches: no device needed."""
    for label, args in invalid_calls():
        assert call(engine_lib, args) == 1, label
        assert b"sd_sched_affine_step" in engine_lib.sd_last_error(), label


# ------------------------------------------------------------------------------------------------ 5. the GPU test's cap
def test_reference_flips_stay_under_a_quarter_of_the_gpu_cap():
    """The GPU test compares with the single rounding of a float64 evaluation and lets at most 1e-4 of the elements of a
    large case be one ulp off.  Two float64 evaluations of the same rows in different summation orders must themselves
    round alike on all but a quarter of that share, or the cap would be measuring the reference."""
    orders = (list(range(sso.COLS)), list(reversed(range(sso.COLS))))
    flips16 = flips32 = n16 = n32 = 0
    for n in sso.GPU_NS:
        mo, lat, noise, bank = sso.step_inputs(n, seed=n)
        for label, plan in sso.gpu_plans():
            for rows in (1, 2):
                (xa, wa), (xb, wb) = (sso.reference(plan, mo, rows, lat, noise, bank, n, sso.GPU_GUIDANCE, o) for o in orders)
                d16 = (sso.to_f16(xa) != sso.to_f16(xb)).sum().item()
                d32 = sum((sso.to_f32(wa[k]) != sso.to_f32(wb[k])).sum().item() for k in wa)
                if n >= sso.GPU_LARGE_N:
                    assert d16 <= 0.25 * sso.GPU_CAP * n and d32 <= 0.25 * sso.GPU_CAP * n * max(len(wa), 1), (label, n, rows)
                flips16, flips32, n16, n32 = flips16 + d16, flips32 + d32, n16 + n, n32 + n * len(wa)
    print(f"reference: {flips16} of {n16} fp16 roundings and {flips32} of {n32} fp32 roundings depend on the summation order")
    assert flips16 <= 0.25 * sso.GPU_CAP * n16 and flips32 <= 0.25 * sso.GPU_CAP * n32
