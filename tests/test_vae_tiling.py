"""Tiled / sliced VAE without a GPU: the engine's tile plan against the oracle's loop, the plan's refusals, the closed
form of the merge against diffusers' sequential in-place blend (float64: this guards the derivation the merge kernel
rests on), and the routing of HipAutoencoderKL.decode / .encode on a recording double."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_tile_oracle as vt  # noqa: E402
from stablediffusion_amd import _lib, config, vae_tiles  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper  # noqa: E402

# the grids the merge is checked on (rows x columns of tiles)
GRIDS = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 3), (4, 2)]


def canvases(n: int, tile: int, stride: int):
    """Lengths of an axis that give n tiles: the last tile one pixel, a last tile that leaves the one before it
    truncated too, and the longest (the last tile as large as a crop)."""
    lo, hi = (n - 1) * stride + 1, n * stride
    mid = min(hi, max(lo, (n - 2) * stride + tile - 1)) if n > 1 else max(1, tile // 2)
    return sorted({lo, mid, hi} if n > 1 else {1, mid, stride})


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("f", [0.0, 0.25, 0.5])
@pytest.mark.parametrize("encode", [False, True])
def test_plan_equals_the_oracles_loop(engine_lib, f, encode):
    ts, tl = 512, 64
    tin, stride, tout, blend, limit = vt.plan_ints(encode, ts, tl, f)
    unit = 8 if encode else 1                    # an image canvas is a multiple of the VAE's scale
    sizes = {1 * unit, tin - unit, tin, tin + unit}
    for m in (1, 2, 3):
        sizes |= {m * stride - unit, m * stride, m * stride + unit, m * stride + tin - unit}
    sizes = sorted(s for s in sizes if s >= unit)
    for h in sizes:
        for w in (sizes[0], sizes[len(sizes) // 2], h, sizes[-1]):          # square and non-square
            want = vt.plan(encode, h, w, ts, tl, f)
            p = vae_tiles.plan(encode, h, w, ts, tl, f)
            assert (p.tile_in, p.stride_in, p.tile_out, p.blend, p.limit) == (tin, stride, tout, blend, limit)
            assert list(p.size_y[:p.ny]) == want["size_y"] and list(p.size_x[:p.nx]) == want["size_x"], (h, w)
            assert [k * p.stride_in for k in range(p.ny)] == want["ys"] and [k * p.stride_in for k in range(p.nx)] == want["xs"]
            got = {(c["h"], c["w"]): c["tiles"] for c in vae_tiles.classes(p)}
            assert got == want["classes"], (h, w)
            assert p.n_classes == len(want["classes"]) <= 9
            assert (p.out_h, p.out_w) == ((h // 8, w // 8) if encode else (h * 8, w * 8))
            # the crops tile the output canvas
            s = (lambda v: v // 8) if encode else (lambda v: v * 8)
            assert sum(min(s(v), limit) for v in want["size_y"]) == p.out_h
            assert sum(min(s(v), limit) for v in want["size_x"]) == p.out_w


def test_plan_last_tile_one_pixel_wide_and_four_classes(engine_lib):
    p = vae_tiles.plan(False, 96 + 1, 48 + 1, 512, 64, 0.25)          # tiles at 0, 48, 96 | 0, 48
    assert list(p.size_y[:p.ny]) == [64, 49, 1] and list(p.size_x[:p.nx]) == [49, 1]
    p = vae_tiles.plan(False, 128, 256, 512, 64, 0.25)                # the 512 x 2048 panorama's latents: 3 x 6 tiles
    assert (p.ny, p.nx) == (3, 6)
    assert [(c["h"], c["w"], len(c["tiles"])) for c in vae_tiles.classes(p)] == [
        (64, 64, 10), (64, 16, 2), (32, 64, 5), (32, 16, 1)]          # interior, last column, last row, corner


def test_stack_offsets_follow_the_classes(engine_lib):
    p = vae_tiles.plan(False, 9, 14, 64, 8, 0.25)
    B, Cc = 2, 3
    offs, total = vae_tiles.stack_offsets(p, B, Cc)
    want, off = {}, 0
    for c in vae_tiles.classes(p):
        for t in c["tiles"]:
            want[t] = off
            off += B * Cc * c["h"] * 8 * c["w"] * 8
    assert total == off and offs == [want[(k // p.nx, k % p.nx)] for k in range(p.ny * p.nx)]


@pytest.mark.parametrize("args,why", [
    ((False, 64, 64, 512, 64, 0.51), "outside [0, 0.5]"),
    ((False, 64, 64, 512, 64, -0.01), "outside [0, 0.5]"),
    ((False, 64, 64, 512, 64, float("nan")), "outside [0, 0.5]"),
    ((False, 65 * 48, 64, 512, 64, 0.25), "more than 64 tiles"),
    ((False, 64, 65 * 48, 512, 64, 0.25), "more than 64 tiles"),
    ((False, 64, 64, 512, 64, 0.3), "do not tile the canvas"),        # int(44.8) * 8 != 512 - int(153.6)
    ((True, 100, 64, 512, 64, 0.25), "do not tile the canvas"),       # an image height that is no multiple of 8
    ((False, 64, 64, 500, 64, 0.25), "multiple of tile_latent_min_size"),
    ((False, 0, 64, 512, 64, 0.25), "non-positive"),
])
def test_plan_refusals(engine_lib, args, why):
    with pytest.raises(_lib.EngineError, match=why.replace("[", r"\[")):
        vae_tiles.plan(*args)
    assert vae_tiles.plan(False, 64 * 48, 64, 512, 64, 0.25).ny == 64          # the bound itself is accepted


def test_plan_refuses_a_blend_above_half_a_tile(engine_lib):
    """No overlap factor in [0, 0.5] gives int(tile f) > tile / 2, so the bound is reached only through a hand-made plan:
    the merge entry rebuilds the plan from its integers and refuses one that breaks it, before anything is launched."""
    p = vae_tiles.plan(False, 40, 40, 32, 32, 0.25)
    p.blend, p.limit = 17, 15
    rc = engine_lib.sd_op_vae_tiles_merge(C.c_void_p(16), 1 << 40, C.c_void_p(16), 64, C.byref(p), 1, 1, 0, None, None)
    assert rc == 1                                  # SD_ERR_INVALID
    assert b"not a plan" in engine_lib.sd_last_error()


# ------------------------------------------------------------------- the closed form against the sequential blend
@pytest.mark.parametrize("tile,f", [(32, 0.25), (16, 0.5), (32, 0.0), (24, 0.25)])
@pytest.mark.parametrize("grid", GRIDS)
def test_closed_form_equals_the_sequential_blend(grid, tile, f):
    ny, nx = grid
    tin, stride, tout, blend, limit = vt.plan_ints(False, tile, tile, f)
    assert 2 * blend <= tout
    seen = 0
    for h in canvases(ny, tile, stride):
        for w in canvases(nx, tile, stride):
            p = vt.plan(False, h, w, tile, tile, f)
            assert (len(p["ys"]), len(p["xs"])) == grid
            rows = vt.raw_tiles(p, 2, 3, seed=h * 1000 + w)
            seq = vt.merge_sequential(rows, blend, limit)
            closed, reads = vt.merge_closed(rows, blend, limit, return_reads=True)
            assert seq.shape == closed.shape == (2, 3, h, w)
            assert (seq - closed).abs().max().item() <= 1e-12, (h, w)
            # what the closed form never read does not matter to the sequential result either
            poisoned = [[torch.where(m, t, torch.full_like(t, float("nan"))) for t, m in zip(tr, mr)]
                        for tr, mr in zip(rows, reads)]
            assert torch.equal(vt.merge_sequential(poisoned, blend, limit), seq)
            seen += 1
    assert seen >= 1


def test_tiled_apply_is_the_identity_on_the_identity():
    """Tiles cut from one canvas and merged again give the canvas: every lerp mixes equal values only when the lent rows
    line up, which is the untruncated case (f = 0.25, canvas = a whole number of strides plus a tile)."""
    x = torch.randn(1, 2, 32 + 24, 32 + 48, dtype=torch.float64)
    assert (vt.tiled_apply(lambda t: t.clone(), x, False, 32, 32, 0.25) - x).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------- the Python surface
class Recorder:
    """Stands in for HipAutoencoderKL._call: records (entry, src shape, dst shape, args) and fills dst."""

    def __init__(self, fill=lambda n: 0.0):
        self.calls, self.fill = [], fill

    def __call__(self, name, src, dst, *args):
        self.calls.append((name, tuple(src.shape), tuple(dst.shape), args))
        dst.fill_(self.fill(len(self.calls)))

    def names(self):
        return [c[0] for c in self.calls]


def double(cfg=None, **kw):
    vae = HipAutoencoderKL(cfg or config.tiny_vae(), device="cpu")
    vae._finalized = True
    vae._call = Recorder(**kw)
    return vae


def test_attributes_default_and_round_trip(engine_lib):
    vae = double()
    assert (vae.use_tiling, vae.use_slicing) == (False, False)
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor) == (64, 8, 0.25)
    sd15 = HipAutoencoderKL(config.sd15_vae(), device="cpu")
    assert (sd15.tile_sample_min_size, sd15.tile_latent_min_size) == (512, 64)
    vae.enable_tiling()
    assert vae.use_tiling
    vae.enable_tiling(False)
    assert not vae.use_tiling
    vae.enable_tiling()
    vae.disable_tiling()
    assert not vae.use_tiling
    vae.enable_slicing()
    assert vae.use_slicing
    vae.disable_slicing()
    assert not vae.use_slicing
    vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor = 32, 4, 0.5
    vae.enable_tiling()
    vae.decode(torch.zeros(1, 4, 5, 4))
    assert vae._call.calls[-1] == ("sd_vae_decode_tiled", (1, 4, 5, 4), (1, 3, 40, 32), (1, 5, 4, 4, 0.5, 4))
    vae.tile_sample_min_size = 64                   # no longer tile_latent times the scale
    with pytest.raises(_lib.EngineError, match="tile_sample_min_size"):
        vae.decode(torch.zeros(1, 4, 5, 4))


def test_decode_routing(engine_lib):
    vae = double()
    small, tall, wide = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 9, 8), torch.zeros(2, 4, 8, 9)
    for z in (small, tall, wide):
        vae.decode(z)
    assert vae._call.names() == ["sd_vae_decode"] * 3                 # tiling off: the plain entry whatever the size
    vae._call.calls.clear()
    vae.enable_tiling()
    for z in (small, tall, wide):
        vae.decode(z)
    assert vae._call.names() == ["sd_vae_decode", "sd_vae_decode_tiled", "sd_vae_decode_tiled"]     # h > tl or w > tl
    assert vae._call.calls[1][3] == (2, 9, 8, 8, 0.25, 4)
    vae._call.calls.clear()
    vae.enable_slicing()
    out = vae.decode(tall)[0]
    assert out.shape == (2, 3, 72, 64)
    assert [(c[0], c[1], c[2]) for c in vae._call.calls] == [("sd_vae_decode_tiled", (1, 4, 9, 8), (1, 3, 72, 64))] * 2
    vae._call.calls.clear()
    vae.disable_tiling()
    vae.decode(tall)
    vae.decode(tall[:1])                                             # one image: nothing to slice
    assert [(c[0], c[1][0]) for c in vae._call.calls] == [("sd_vae_decode", 1)] * 3
    vae._call.calls.clear()
    vae.disable_slicing()
    vae.decode(tall)
    assert [(c[0], c[1][0]) for c in vae._call.calls] == [("sd_vae_decode", 2)]


def test_encode_routing(engine_lib):
    vae = double()
    small, big = torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 72)
    vae.encode_moments(small), vae.encode_moments(big)
    assert vae._call.names() == ["sd_vae_encode"] * 2
    vae._call.calls.clear()
    vae.enable_tiling()
    vae.encode_moments(small)
    mom = vae.encode(big).latent_dist.mean
    assert mom.shape == (2, 4, 8, 9)
    assert [(c[0], c[3]) for c in vae._call.calls] == [("sd_vae_encode", (2, 64, 64)),
                                                       ("sd_vae_encode_tiled", (2, 64, 72, 8, 0.25, 4))]   # H > ts or W > ts
    vae._call.calls.clear()
    vae.enable_slicing()
    vae.encode_moments(big)
    assert [(c[0], c[1][0]) for c in vae._call.calls] == [("sd_vae_encode_tiled", 1)] * 2


def test_force_upcast_retry_reruns_every_tile_and_slice(engine_lib):
    """Non-finite moments of a force_upcast VAE: the WHOLE routed encode runs again at the raised shift -- both slices,
    each through the tiled entry -- and the shift is set on the handle in between."""
    cfg = config.VAEConfig(block_out_channels=(64, 64, 128, 128), sample_size=64, force_upcast=True)
    vae = double(cfg, fill=lambda n: float("inf") if n <= 2 else 1.0)          # the first pass (two slices) overflows
    vae.enable_tiling()
    vae.enable_slicing()
    shifts = []
    real = vae._lib.sd_vae_encode_range_shift

    class Lib:
        def __getattr__(self, name):
            return getattr(real_lib, name)

        def sd_vae_encode_range_shift(self, h, shift):
            shifts.append((len(vae._call.calls), shift))
            return real(h, shift)

    real_lib = vae._lib
    vae._lib = Lib()
    try:
        mom = vae.encode_moments(torch.zeros(2, 3, 72, 64))
    finally:
        vae._lib = real_lib
    assert bool(torch.isfinite(mom).all())
    assert vae._call.names() == ["sd_vae_encode_tiled"] * 4 and [c[1][0] for c in vae._call.calls] == [1, 1, 1, 1]
    assert shifts == [(2, 4)] and vae._enc_shift == 4


def test_wrapper_forwards_the_switches(engine_lib):
    vae = double()
    m = SDModelWrapper.__new__(SDModelWrapper)
    m.vae = vae
    m.enable_vae_tiling()
    m.enable_vae_slicing()
    assert vae.use_tiling and vae.use_slicing
    m.disable_vae_tiling()
    m.disable_vae_slicing()
    assert not vae.use_tiling and not vae.use_slicing


def test_header_declares_what_the_library_exports(engine_lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sd_engine.h")).read()
    for name in ("sd_vae_tile_plan", "sd_vae_tile_stack", "sd_vae_decode_tiled", "sd_vae_encode_tiled",
                 "sd_vae_memory_tiled", "sd_op_vae_tiles_gather", "sd_op_vae_tiles_merge"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(engine_lib, name)
    assert C.sizeof(_lib.SdVAETiles) == 4 * (12 + 2 * 64 + 1 + 7 * 9)
