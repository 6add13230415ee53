"""float64 restatement of MultiDiffusion's denoising loop (Bar-Tal et al. 2023) the way diffusers 0.27.2's
StableDiffusionPanoramaPipeline runs it, for the tests (not a test module).  Recalled, not pinned: diffusers is not
installed where this was written.

What is restated (`loop_per_view`): per step, for every view, the view's slice of the canvas latents (columns modulo the
width under circular padding), the scheduler state COPIED per view and restored in front of its step, the CFG batch and
combine per view, the scheduler's step on the view, value += stepped view, count += 1 (here: the window weights), and
latents = value / count.  `loop_merged` is what the engine runs instead: the views' model outputs are averaged into one
canvas-shaped model output and ONE scheduler steps the canvas.  Every update is affine in (sample, model output, noise,
history) with coefficients of the step alone, so the two agree; tests/test_views.py shows it numerically.

Where this differs from diffusers on purpose: the view list covers every pixel (a final start L - win; diffusers leaves
such edges to where(count > 0)), and a scheduler that adds noise gets the canvas noise's slice in every view instead of
an independent draw per view.  The schedulers are oracle/schedulers_ref.py's and lcm_oracle's (numpy float64)."""
import copy

import numpy as np
import torch

import lcm_oracle
from oracle import schedulers_ref


def axis_starts(L, win, s, wrap=False):
    """The plan's rule, written independently of stablediffusion_amd.views (a stride above the window is the window)."""
    s = min(s, win)
    if wrap:
        assert win <= L
        return [k * s for k in range((L + s - 1) // s)]
    if L <= win:
        return [0]
    starts = [k * s for k in range((L - win) // s + 1)]
    if starts[-1] != L - win:
        starts.append(L - win)
    return starts


def diffusers_get_views(H, W, window=64, stride=8):
    """StableDiffusionPanoramaPipeline.get_views without circular padding, in latent pixels: (h0, h1, w0, w1)."""
    nby = (H - window) // stride + 1 if H > window else 1
    nbx = (W - window) // stride + 1 if W > window else 1
    return [((i // nbx) * stride, (i // nbx) * stride + window, (i % nbx) * stride, (i % nbx) * stride + window)
            for i in range(nby * nbx)]


class Plan:
    def __init__(self, Hc, Wc, h, w, stride, wrap=False):
        self.Hc, self.Wc, self.h, self.w, self.wrap = Hc, Wc, min(h, Hc), w if wrap else min(w, Wc), wrap
        self.ys = axis_starts(Hc, self.h, stride)
        self.xs = axis_starts(Wc, self.w, stride, wrap)

    def views(self):
        return [(y, x) for y in self.ys for x in self.xs]

    def cols(self, x):
        return (torch.arange(self.w) + x) % self.Wc

    def cut(self, canvas, y, x):
        return canvas[:, :, y:y + self.h, :][:, :, :, self.cols(x)]


class Stepper:
    """One interface over the float64 schedulers: timesteps, init_noise_sigma, scale(x, k), step(eps, k, x, noise); the
    state is whatever the wrapped object holds, so copy.deepcopy is diffusers' per-view copy of the scheduler state."""

    def __init__(self, name, steps):
        self.name = name
        if name == "lcm":
            self.ref = lcm_oracle.LCMOracle()
            self.timesteps = self.ref.timesteps(steps)
            self.init_noise_sigma = 1.0
        else:
            self.ref = {"DDIM": schedulers_ref.DDIMRef, "euler": schedulers_ref.EulerRef,
                        "dpmpp_2m": schedulers_ref.DPMpp2MRef, "PNDM": schedulers_ref.PNDMRef,
                        "euler_a": schedulers_ref.EulerAncestralRef}[name]()
            self.ref.set_timesteps(steps)
            self.timesteps = list(self.ref.timesteps)
            self.init_noise_sigma = float(self.ref.init_noise_sigma)
        self.noisy = name in ("euler_a", "lcm")

    def scale(self, x, k):
        if self.name == "lcm":
            return x
        return torch.from_numpy(np.asarray(self.ref.scale_model_input(x.numpy(), self.timesteps[k])))

    def step(self, eps, k, x, noise):
        t = self.timesteps[k]
        if self.name == "lcm":
            return torch.from_numpy(np.asarray(self.ref.step(eps.numpy(), k, self.timesteps, x.numpy(), noise.numpy())[0]))
        if self.name == "euler_a":
            return torch.from_numpy(np.asarray(self.ref.step(eps.numpy(), t, x.numpy(), noise.numpy())))
        return torch.from_numpy(np.asarray(self.ref.step(eps.numpy(), t, x.numpy())))


def _eps(unet, x, t, ehs, g, do_cfg):
    """One view's (or the canvas's) guided model output from its already scaled latents."""
    if not do_cfg:
        return unet(x, float(t), ehs).double()
    u, c = unet(torch.cat([x] * 2), float(t), ehs).double().chunk(2)
    return u + g * (c - u)


def _ehs(pe, ne, do_cfg):
    return torch.cat([ne.double(), pe.double()]) if do_cfg else pe.double()


def _weights(plan, weights):
    return torch.ones(plan.h, plan.w, dtype=torch.float64) if weights is None else weights.double()


def loop_per_view(unet, name, plan, noise, pe, ne, steps, g, do_cfg=True, weights=None, step_noise=None):
    """diffusers' loop: step every view with its own copy of the scheduler state, then value / count.  `step_noise`:
    one canvas-shaped noise per step for the schedulers that add some."""
    first = Stepper(name, steps)
    x = noise.double() * first.init_noise_sigma
    ehs, wt = _ehs(pe, ne, do_cfg), _weights(plan, weights)
    state = [copy.deepcopy(first) for _ in plan.views()]
    for k, t in enumerate(first.timesteps):
        value, count = torch.zeros_like(x), torch.zeros(plan.Hc, plan.Wc, dtype=torch.float64)
        for v, (y0, x0) in enumerate(plan.views()):
            sched = state[v]
            xv = plan.cut(x, y0, x0)
            eps = _eps(unet, sched.scale(xv, k), t, ehs, g, do_cfg)
            nz = plan.cut(step_noise[k].double(), y0, x0) if first.noisy else None
            stepped = sched.step(eps, k, xv, nz)
            cols = plan.cols(x0)
            value[:, :, y0:y0 + plan.h, :] = value[:, :, y0:y0 + plan.h, :].index_add(3, cols, stepped * wt)
            count[y0:y0 + plan.h, :] = count[y0:y0 + plan.h, :].index_add(1, cols, wt)
        assert (count > 0).all()
        x = value / count
    return x


def merge(outs, plan, weights=None):
    """Weighted mean of the views' tensors [V][rows, C, h, w] -> [rows, C, Hc, Wc], float64."""
    wt = _weights(plan, weights)
    value = torch.zeros(outs[0].shape[0], outs[0].shape[1], plan.Hc, plan.Wc, dtype=torch.float64)
    count = torch.zeros(plan.Hc, plan.Wc, dtype=torch.float64)
    for (y0, x0), e in zip(plan.views(), outs):
        cols = plan.cols(x0)
        value[:, :, y0:y0 + plan.h, :] = value[:, :, y0:y0 + plan.h, :].index_add(3, cols, e.double() * wt)
        count[y0:y0 + plan.h, :] = count[y0:y0 + plan.h, :].index_add(1, cols, wt)
    return value / count


def loop_merged(unet, name, plan, noise, pe, ne, steps, g, do_cfg=True, weights=None, step_noise=None):
    """The engine's loop: merge the views' guided model outputs, then ONE scheduler steps the canvas."""
    sched = Stepper(name, steps)
    x = noise.double() * sched.init_noise_sigma
    ehs = _ehs(pe, ne, do_cfg)
    for k, t in enumerate(sched.timesteps):
        scaled = sched.scale(x, k)
        outs = [_eps(unet, plan.cut(scaled, y0, x0), t, ehs, g, do_cfg) for y0, x0 in plan.views()]
        x = sched.step(merge(outs, plan, weights), k, x, step_noise[k].double() if sched.noisy else None)
    return x


class AffineUNet:
    """A random affine "UNet" of the window's shape that tells views apart: a 3x3 convolution with zero padding (so a
    pixel's output depends on where the window's border is), a bias map over the window, the embedding and the timestep."""

    def __init__(self, h, w, seed=0, channels=4):
        g = torch.Generator().manual_seed(seed)
        self.k = torch.randn(channels, channels, 3, 3, generator=g, dtype=torch.float64) * 0.08
        self.bias = torch.randn(1, channels, h, w, generator=g, dtype=torch.float64) * 0.3
        self.calls = 0

    def __call__(self, sample, t, ehs, **kw):
        self.calls += 1
        k, bias = self.k.to(sample.dtype), self.bias.to(sample.dtype)
        e = ehs.to(sample.dtype).mean(dim=(1, 2)).view(-1, 1, 1, 1)
        return torch.nn.functional.conv2d(sample, k, padding=1) + bias + 0.05 * e + 1e-4 * float(t)


# ------------------------------------------------------------------------------------------------ the kernels' cases
# (Hc, Wc, h, w, stride, wrap): the smallest shapes at which each branch of the gather / merge kernels can go wrong --
# the vector path with overlaps on both axes; the scalar path with ragged final starts; one view; a wrapped x axis; a
# window that is not square.  Shared by the CPU test of the reference and the GPU test of the kernels.
KERNEL_SHAPES = [(24, 40, 16, 16, 8, 0), (20, 37, 16, 16, 8, 0), (16, 16, 16, 16, 8, 0), (24, 40, 16, 16, 8, 1),
                 (24, 24, 16, 8, 8, 0)]
KERNEL_GROUPS, KERNEL_BATCHES, KERNEL_CHANNELS = (1, 2, 3), (1, 2), 4
MAGNITUDES = (1e-3, 1.0, 30.0)


def kernel_plan(shape):
    Hc, Wc, h, w, s, wrap = shape
    return Plan(Hc, Wc, h, w, s, bool(wrap))


def chunk_lists(V, vpc):
    return [list(range(lo, min(lo + vpc, V))) for lo in range(0, V, vpc)]


def kernel_weights(kind, h, w, seed=0):
    """None, the package's Gaussian profile, or random values in [0.05, 1]: fp32 [h, w]."""
    if kind == "none":
        return None
    if kind == "gaussian":
        from stablediffusion_amd import views
        return views.window_weights("gaussian", h, w)
    return (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) * 0.95 + 0.05).float()


def view_outputs(plan, G, B, seed):
    """Random fp16 model outputs per view, [V][G, B, C, h, w], every view at a magnitude of its own."""
    g = torch.Generator().manual_seed(seed)
    outs = []
    for v in range(len(plan.views())):
        mag = MAGNITUDES[int(torch.randint(0, 3, (1,), generator=g))]
        outs.append((torch.randn(G, B, KERNEL_CHANNELS, plan.h, plan.w, generator=g) * mag).half())
    return outs


def chunked_buffer(outs, vpc):
    """The UNet outputs as the forwards leave them: per chunk [G, size, B, C, h, w], chunks one after another."""
    parts = [torch.stack([outs[v] for v in chunk], dim=1).reshape(-1, *outs[0].shape[2:])
             for chunk in chunk_lists(len(outs), vpc)]
    return torch.cat(parts)


def merge_reference(outs, plan, weights):
    """float64 merge of the fp16 values -> (O, A, n): the weighted mean, the weighted mean of |e|, the number of covering
    views, each [G * B, C, Hc, Wc] (n: [Hc, Wc])."""
    flat = [e.reshape(-1, *e.shape[2:]) for e in outs]
    wt = _weights(plan, weights)
    O = merge(flat, plan, weights)
    A = merge([e.double().abs() for e in flat], plan, weights)
    n = torch.zeros(plan.Hc, plan.Wc, dtype=torch.float64)
    for y0, x0 in plan.views():
        n[y0:y0 + plan.h, :] = n[y0:y0 + plan.h, :].index_add(1, plan.cols(x0), torch.ones_like(wt))
    return O, A, n


def merge_bound(O, A, n):
    """|out - O| <= 2^-11 |O| + (2 n + 5) 2^-24 A + 2^-25: one round-to-nearest to fp16; one rounding per product, the
    two fp32 sums, the reciprocal and its multiply, each relative to the weighted mean of |e|; the subnormal floor."""
    return 2.0 ** -11 * O.abs() + (2 * n + 5) * 2.0 ** -24 * A + 2.0 ** -25


def merge_fp32_emulation(outs, plan, weights, reciprocal=True):
    """The kernel's arithmetic in torch fp32: views in ascending order, acc += w * e and ws += w in fp32, then
    acc * (1 / ws) (or acc / ws), one rounding to fp16."""
    flat = [e.reshape(-1, *e.shape[2:]).float() for e in outs]
    wt = torch.ones(plan.h, plan.w) if weights is None else weights.float()
    acc = torch.zeros(flat[0].shape[0], flat[0].shape[1], plan.Hc, plan.Wc)
    ws = torch.zeros(plan.Hc, plan.Wc)
    for (y0, x0), e in zip(plan.views(), flat):
        cols = plan.cols(x0)
        acc[:, :, y0:y0 + plan.h, :] = acc[:, :, y0:y0 + plan.h, :].index_add(3, cols, e * wt)
        ws[y0:y0 + plan.h, :] = ws[y0:y0 + plan.h, :].index_add(1, cols, wt)
    return (acc * (1.0 / ws) if reciprocal else acc / ws).half()


def invalid_view_calls():
    """(label, entry, kwargs over the valid call below): every one is SD_ERR_INVALID before anything launches."""
    base = dict(canvas=1, out=1, G=2, B=1, C=4, Hc=24, Wc=40, h=16, w=16, ys=[0, 8], xs=[0, 8, 16, 24], wrap=0, vpc=3)
    table = []
    for entry in ("sd_views_gather", "sd_views_merge"):
        t = [("null input", dict(canvas=0)), ("null output", dict(out=0)), ("null ys", dict(ys=None)),
             ("null xs", dict(xs=None)), ("B = 0", dict(B=0)), ("C = -4", dict(C=-4)), ("Hc = 0", dict(Hc=0)),
             ("Wc = 0", dict(Wc=0)), ("h = 0", dict(h=0)), ("w = 0", dict(w=0)),
             ("65 starts", dict(xs=list(range(65)), w=16)), ("no starts", dict(xs=[])),
             ("a negative start", dict(ys=[-1, 8])), ("a start past the canvas", dict(xs=[0, 8, 16, 40], wrap=1)),
             ("a window that ends outside", dict(xs=[0, 8, 16, 25])), ("h > Hc", dict(h=32, ys=[0])),
             ("w > Wc", dict(w=48, xs=[0])), ("w > Wc wrapped", dict(w=48, xs=[0], wrap=1)),
             ("an uncovered column", dict(xs=[0, 24], w=16)), ("an uncovered row", dict(ys=[8])),
             ("an uncovered column, wrapped", dict(xs=[0, 16], w=8, wrap=1))]
        if entry == "sd_views_merge":
            t += [("G = 0", dict(G=0)), ("views_per_chunk = 0", dict(vpc=0)), ("views_per_chunk = -1", dict(vpc=-1))]
        table += [(f"{entry}: {label}", entry, dict(base, **kw)) for label, kw in t]
    return table


def call_view_entry(lib, entry, a, ptrs, stream=None, weights=None):
    """One call of invalid_view_calls' table (or a valid one): ptrs = (input, output) stand in for the 1s."""
    import ctypes as C
    arr = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
    p_in = C.c_void_p(ptrs[0]) if a["canvas"] else None
    p_out = C.c_void_p(ptrs[1]) if a["out"] else None
    ny, nx = len(a["ys"] or []), len(a["xs"] or [])
    if entry == "sd_views_gather":
        return lib.sd_views_gather(p_in, p_out, a["B"], a["C"], a["Hc"], a["Wc"], a["h"], a["w"], arr(a["ys"]), ny,
                                   arr(a["xs"]), nx, a["wrap"], stream)
    return lib.sd_views_merge(p_in, p_out, weights, a["G"], a["B"], a["C"], a["Hc"], a["Wc"], a["h"], a["w"], arr(a["ys"]),
                              ny, arr(a["xs"]), nx, a["wrap"], a["vpc"], stream)
