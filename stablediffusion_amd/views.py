"""MultiDiffusion (Bar-Tal et al. 2023; diffusers' StableDiffusionPanoramaPipeline, A1111's "Tiled Diffusion"): a latent
canvas larger than the UNet's training size is denoised as overlapping fixed-size windows ("views").  Every step gathers
the windows, runs the UNet on them in chunks, and merges the windows' model outputs into ONE canvas-shaped model output --
a weighted mean where views overlap -- on which the scheduler's step then runs as it runs on a plain forward's.

diffusers steps every view with a copy of the scheduler state and averages the stepped latents.  Every update in the
registry is affine in (sample, model output, noise, history) with coefficients that depend on the step only, so the
weighted mean of the per-view updates IS the update of the weighted-mean model output (tests/views_oracle.py shows it in
float64); merging epsilon keeps one scheduler state and lets every device step entry run unchanged.  Schedulers that add
noise get one canvas noise instead of diffusers' independent per-view draws, which lose variance where views overlap.

Recalled, not pinned: diffusers is not installed where this was written.

The layout: view v = iy * nx + ix sits at (ys[iy], xs[ix]); windows are [V * B, C, h, w] with row v * B + b; the UNet's
outputs of a chunk of `size` views are [G, size, B, C, h, w] (G guidance groups), chunks one after another in one buffer.
On the engine the gather and the merge are sd_views_gather / sd_views_merge (csrc/views.hip); the torch restatements
below serve UNets without the engine library and the tests.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

MAX_STARTS = 64            # per axis: the starts travel in the kernels' launch parameters (sd_engine.h)
GAUSSIAN_SIGMA = 0.3       # of the window's extent, per axis.  A free choice: the centre of a window, where the UNet sees
#                            the most context, weighs e^(1 / (2 * 0.09)) ~ 260 times its corner, and no weight underflows


def axis_starts(L: int, win: int, stride: int, wrap: bool = False) -> List[int]:
    """The starts of one axis (sd_view_plan's rule): 0, s, 2s, .. <= L - win plus a final L - win when the last one is not
    already there; the single start 0 when L <= win; wrapped: 0, s, .. < L, which needs win <= L.  A stride above the window
    counts as the window, so every position is covered whatever the arguments."""
    if L < 1 or win < 1:
        raise ValueError("plan_views: sizes must be positive")
    if stride < 1:
        raise ValueError("view_stride must be at least 1")
    stride = min(stride, win)                # (a larger stride would leave gaps between windows: they abut instead)
    if wrap:
        if win > L:
            raise ValueError(f"a window of {win} is larger than the wrapped axis of {L}")
        starts = list(range(0, L, stride))
    elif L <= win:
        starts = [0]
    else:
        starts = list(range(0, L - win + 1, stride))
        if starts[-1] != L - win:
            starts.append(L - win)
    if len(starts) > MAX_STARTS:
        raise ValueError(f"{len(starts)} window starts on one axis: at most {MAX_STARTS} (use a larger stride)")
    return starts


@dataclass(frozen=True)
class ViewPlan:
    Hc: int
    Wc: int
    h: int
    w: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    wrap: bool

    @property
    def num_views(self) -> int:
        return len(self.ys) * len(self.xs)

    def views(self) -> List[Tuple[int, int]]:
        """(y, x) of every view in order v = iy * nx + ix."""
        return [(y, x) for y in self.ys for x in self.xs]


def as_pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"expected an int or a pair, got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def plan_views(Hc: int, Wc: int, window, stride, circular: bool = False) -> ViewPlan:
    """The views of an [Hc, Wc] canvas: `window` and `stride` are ints or (y, x) pairs in latent pixels.  A window larger
    than an unwrapped axis is clamped to it; `circular` wraps the x axis (diffusers' circular_padding) and then refuses a
    window wider than the canvas."""
    wh, ww = as_pair(window)
    if wh < 1 or ww < 1:
        raise ValueError("view_window must be positive")
    sy, sx = (max(1, wh // 2), max(1, ww // 2)) if stride is None else as_pair(stride)     # None: half the window
    if sy < 1 or sx < 1:
        raise ValueError("view_stride must be at least 1")
    if circular and ww > Wc:
        raise ValueError(f"view_window {ww} is wider than the canvas ({Wc}) on the wrapped axis")
    h, w = min(wh, Hc), min(ww, Wc)
    return ViewPlan(Hc, Wc, h, w, tuple(axis_starts(Hc, h, sy)), tuple(axis_starts(Wc, w, sx, circular)), bool(circular))


def window_weights(kind: str, h: int, w: int) -> Optional[torch.Tensor]:
    """The [h, w] fp32 profile a window's output is weighted with in the merge: "uniform" -> None (all ones, MultiDiffusion
    as published), "gaussian" -> the separable exp(-(d / sigma)^2 / 2), d the distance from the window's centre and
    sigma = GAUSSIAN_SIGMA * extent per axis (peak 1)."""
    if kind == "uniform":
        return None
    if kind != "gaussian":
        raise ValueError(f"view_blend must be 'uniform' or 'gaussian', got {kind!r}")

    def axis(n):
        d = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
        return torch.exp(-0.5 * (d / (GAUSSIAN_SIGMA * n)) ** 2)
    return (axis(h)[:, None] * axis(w)[None, :]).to(torch.float32).contiguous()


def chunk_sizes(V: int, views_per_chunk: int) -> List[int]:
    return [min(views_per_chunk, V - lo) for lo in range(0, V, views_per_chunk)]


def view_row(v: int, g: int, b: int, V: int, views_per_chunk: int, G: int, B: int) -> int:
    """The row of (group g, view v, sample b) in the chunked output buffer (the kernel's closed form)."""
    ch, k = divmod(v, views_per_chunk)
    size = min(views_per_chunk, V - ch * views_per_chunk)
    return ch * views_per_chunk * G * B + (g * size + k) * B + b


def _cols(plan: ViewPlan, x: int, device) -> torch.Tensor:
    return (torch.arange(plan.w, device=device) + x) % plan.Wc


def gather(canvas: torch.Tensor, plan: ViewPlan) -> torch.Tensor:
    """torch restatement of sd_views_gather: [B, C, Hc, Wc] -> [V * B, C, h, w]."""
    wins = [canvas[:, :, y:y + plan.h, :].index_select(3, _cols(plan, x, canvas.device)) for y, x in plan.views()]
    return torch.cat(wins, dim=0)


def merge(model_out: torch.Tensor, plan: ViewPlan, G: int, B: int, views_per_chunk: int,
          weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch restatement of sd_views_merge: the chunked buffer [G * V * B, C, h, w] -> [G * B, C, Hc, Wc], views in ascending
    order, sums in fp32 (in the buffer's own dtype when that is wider), one rounding to the buffer's dtype."""
    V, Cc = plan.num_views, model_out.shape[1]
    acc_t = torch.float64 if model_out.dtype == torch.float64 else torch.float32
    dev = model_out.device
    wt = torch.ones(plan.h, plan.w, dtype=acc_t, device=dev) if weights is None else weights.to(device=dev, dtype=acc_t)
    num = torch.zeros(G * B, Cc, plan.Hc, plan.Wc, dtype=acc_t, device=dev)
    den = torch.zeros(plan.Hc, plan.Wc, dtype=acc_t, device=dev)
    for v, (y, x) in enumerate(plan.views()):
        cols = _cols(plan, x, dev)
        rows = [view_row(v, g, b, V, views_per_chunk, G, B) for g in range(G) for b in range(B)]
        e = model_out[rows].to(acc_t) * wt
        num[:, :, y:y + plan.h, :] = num[:, :, y:y + plan.h, :].index_add(3, cols, e)
        den[y:y + plan.h, :] = den[y:y + plan.h, :].index_add(1, cols, wt)
    return (num * (1.0 / den)).to(model_out.dtype)


def _int_array(values):
    return (C.c_int * len(values))(*values)


class ViewRunner:
    """The windows of one denoising loop: the plan, the window and output buffers, the merge weights and the prompt
    embeddings repeated to every chunk size (one tensor per size, alive for the whole loop: the engine's text K/V cache is
    keyed by the buffer's address).  `forward` turns canvas latents into the canvas-shaped model output.

    `lib` is the engine library when the UNet is the engine's (the gather and the merge are then its kernels, on fp16 CUDA
    tensors), None for any other UNet (the torch restatements)."""

    def __init__(self, plan: ViewPlan, B: int, G: int, view_batch_size: int, blend: str, prompt_embeds: torch.Tensor,
                 lib=None):
        if view_batch_size < 1:
            raise ValueError("view_batch_size must be at least 1")
        if prompt_embeds.shape[0] != G * B:
            raise ValueError(f"prompt_embeds must hold {G} x {B} rows, got {prompt_embeds.shape[0]}")
        self.plan, self.B, self.G, self.lib = plan, B, G, lib
        self.vpc = min(int(view_batch_size), plan.num_views)
        self.sizes = chunk_sizes(plan.num_views, self.vpc)
        self.weights = window_weights(blend, plan.h, plan.w)
        if self.weights is not None:
            self.weights = self.weights.to(prompt_embeds.device)
        # rows [group][view in chunk][b], the order of a chunk's forward
        pe = prompt_embeds.reshape(G, 1, B, *prompt_embeds.shape[1:])
        self.embeds: Dict[int, torch.Tensor] = {
            k: pe.expand(G, k, B, *prompt_embeds.shape[1:]).reshape(G * k * B, *prompt_embeds.shape[1:]).contiguous()
            for k in sorted(set(self.sizes))}
        self._ys, self._xs = _int_array(plan.ys), _int_array(plan.xs)
        self._windows = self._out = None

    def _buffers(self, like: torch.Tensor):
        p, V = self.plan, self.plan.num_views
        if self._windows is None or self._windows.dtype != like.dtype or self._windows.device != like.device:
            Cc = like.shape[1]
            self._windows = torch.empty(V * self.B, Cc, p.h, p.w, dtype=like.dtype, device=like.device)
            self._out = torch.empty(self.G * V * self.B, Cc, p.h, p.w, dtype=like.dtype, device=like.device)
        return self._windows, self._out

    def forward(self, latents: torch.Tensor, run: Callable[[torch.Tensor, torch.Tensor, torch.Tensor], Optional[torch.Tensor]]):
        """latents [B, C, Hc, Wc] -> [G * B, C, Hc, Wc].  `run(windows, embeds, out)` is one UNet forward of a chunk:
        `windows` [size * B, C, h, w], `embeds` the prompt embeddings of its G * size * B output rows, `out` the
        [G * size * B, C, h, w] slice of the output buffer; it writes there and returns None, or returns the tensor."""
        p, B, G = self.plan, self.B, self.G
        if tuple(latents.shape[0:1] + latents.shape[2:]) != (B, p.Hc, p.Wc):
            raise ValueError(f"latents {tuple(latents.shape)} do not match the view plan ({B}, C, {p.Hc}, {p.Wc})")
        engine = self.lib is not None and latents.is_cuda and latents.dtype == torch.float16
        latents = latents.contiguous()
        Cc = latents.shape[1]
        windows, out = self._buffers(latents)
        if engine:
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _check(self.lib, self.lib.sd_views_gather(
                C.c_void_p(latents.data_ptr()), C.c_void_p(windows.data_ptr()), B, Cc, p.Hc, p.Wc, p.h, p.w, self._ys,
                len(p.ys), self._xs, len(p.xs), int(p.wrap), stream))
        else:
            windows.copy_(gather(latents, p))
        lo = 0
        for size in self.sizes:
            dst = out[G * lo * B:G * (lo + size) * B]
            got = run(windows[lo * B:(lo + size) * B], self.embeds[size], dst)
            if got is not None:
                dst.copy_(got)
            lo += size
        if not engine:
            return merge(out, p, G, B, self.vpc, self.weights)
        eps = torch.empty(G * B, Cc, p.Hc, p.Wc, dtype=latents.dtype, device=latents.device)
        _check(self.lib, self.lib.sd_views_merge(
            C.c_void_p(out.data_ptr()), C.c_void_p(eps.data_ptr()),
            C.c_void_p(self.weights.data_ptr()) if self.weights is not None else None, G, B, Cc, p.Hc, p.Wc, p.h, p.w,
            self._ys, len(p.ys), self._xs, len(p.xs), int(p.wrap), self.vpc, stream))
        return eps


def _check(lib, rc):
    if rc:
        raise RuntimeError(lib.sd_last_error().decode())
