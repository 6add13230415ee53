"""The affine scheduler step (`sd_sched_affine_step`, schedulers.py `affine_plan`) restated for the tests (not a test
module): a float64 numpy evaluation of a plan's rows, and the plans and inputs that the CPU and the GPU tests share."""
from types import SimpleNamespace

import numpy as np
import torch

import lcm_oracle
from oracle import schedulers_ref
from stablediffusion_amd import schedulers

COLS = 7
# registry name -> (oracle class, its step takes noise)
NAMES = {"euler_a": (schedulers_ref.EulerAncestralRef, True), "DPM++ 2M SDE Karras": (schedulers_ref.DPMpp2MSDERef, True),
         "PNDM": (schedulers_ref.PNDMRef, False), "uni_pc": (schedulers_ref.UniPCRef, False)}
PREDICTIONS = ("epsilon", "v_prediction")
GPU_NS = (1, 7, 8, 2047, 4096, 3 * 4 * 24 * 40)
GPU_GUIDANCE = 5.0
GPU_LARGE_N = 10 ** 4         # below: bit for bit; from here on at most GPU_CAP of the elements may be one ulp off
GPU_CAP = 1e-4


def make(name, pred="epsilon"):
    """The registry's scheduler with the spacing the oracle classes have (as test_oracle.py builds them)."""
    return schedulers.REGISTRY[name](schedulers.DDIMScheduler(timestep_spacing="leading", prediction_type=pred).config)


def _row(coef, v, order):
    acc = None
    for k in order:
        if coef[k] != 0.0:                    # an exact 0 contributes nothing, whatever the operand holds
            term = coef[k] * v[k]
            acc = term if acc is None else acc + term
    return np.zeros_like(v[0]) if acc is None else acc


def apply_plan(plan, x, m, z, bank, order=None):
    """float64: (out . v, {slot: row . v}) for v = (x, m, z, bank[0], ..), every row from the given (old) values.  z may
    be None and bank rows may hold anything where the coefficients are 0.  `order`: the columns' summation order."""
    order = range(COLS) if order is None else order
    zero = np.zeros_like(x)
    v = [x, m, zero if z is None else z] + [bank[k] if k < plan.n_slots else zero for k in range(COLS - 3)]
    assert z is not None or not plan.needs_noise
    return _row(plan.out, v, order), {slot: _row(row, v, order) for slot, row in plan.writes}


def step_plans(name, pred, n_steps=7):
    """[(label, plan)] of the first, the second, a middle and the last step of an n_steps schedule."""
    s = make(name, pred)
    s.set_timesteps(n_steps)
    ts = s.timesteps.tolist()
    plans = []
    for t in ts:
        plans.append(s.affine_plan(t))
        s.affine_commit()
    picks = {"first": 0, "second": 1, "middle": len(ts) // 2 + 1, "last": len(ts) - 1}
    return [(f"{name} {pred} {k}", plans[i]) for k, i in picks.items()]


def dense_plan():
    """All seven columns non-zero in all three rows, two writes; slots 1 and 3 are read and written."""
    r = np.random.default_rng(7)
    rows = r.uniform(0.25, 2.0, size=(3, COLS)) * r.choice([-1.0, 1.0], size=(3, COLS))
    return SimpleNamespace(in_scale=1.0, n_slots=4, out=rows[0].tolist(), writes=[(3, rows[1].tolist()), (1, rows[2].tolist())],
                           needs_noise=True)


def gpu_plans():
    out = [(lab, p) for name in NAMES for pred in PREDICTIONS for lab, p in step_plans(name, pred)]
    return out + [("dense", dense_plan())]


def used_columns(plan):
    rows = [plan.out] + [r for _, r in plan.writes]
    return [any(r[k] != 0.0 for r in rows) for k in range(COLS)]


def step_inputs(n, seed):
    """One case's inputs: fp16 model output [2n] (rows = 1 reads the first n), latents [n], noise [n]; fp32 bank [4, n]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2 * n, generator=g).half(), torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half(),
            torch.randn(4, n, generator=g))


def reference(plan, mo, rows, lat, noise, bank, n, g, order=None):
    """float64, unrounded: (latents, {slot: values}) of the step on these inputs, m rounded as the kernel rounds it."""
    m = (lcm_oracle.cfg_combine_f16(mo, n, g) if rows == 2 else mo[:n]).double().numpy()
    z = noise.double().numpy() if plan.needs_noise else None
    return apply_plan(plan, lat.double().numpy(), m, z, bank.double().numpy(), order)


def to_f16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float16))


def to_f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float32))


def ulp_diff_f32(a, b):
    def key(x):
        i = x.view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()
