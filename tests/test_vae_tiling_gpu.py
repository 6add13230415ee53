"""Tiled / sliced VAE on the device: the merge kernel element by element against the float64 closed form
(tests/vae_tile_oracle.py; tests/test_vae_tiling.py shows that form equal to diffusers' sequential blend), the gather
bit for bit, sd_vae_decode_tiled / sd_vae_encode_tiled against the oracle's sequential tiling over oracle/vae_ref.py,
and the bit-for-bit equivalences of the switches.

No real-size case is kept here: decoding 96 x 96 latents at the SD1.5 configuration through 2 x 2 tiles against the
oracle's tiling (tile decodes in fp32 on the device) measured rel-L2 1.30e-3 once, but the test took 59 s, nearly all
of it synthesising the weights and the oracle's four tile decodes, so the tiny case stands alone.

The merge's element bound, from the arithmetic alone.  An output is three nested fp32 lerps p (1 - t) + q t of fp16
operands, then one rounding to fp16.  A lerp rounds t (one division), 1 - t, two products and a sum -- contracted or not,
at most five roundings of relative size u32 = 2^-24 on quantities no larger than the largest operand A of the pixel's
tiles -- and passes the error of its own inputs on with weight at most 1 (the weights are non-negative and sum to 1 but
for their own roundings).  Three levels: delta = 16 u32 A covers 15 roundings and the weights' slack.  The rounding to
fp16 adds half an ulp of the fp32 value, which lies within delta of the reference r: u16 (|r| + delta) with u16 = 2^-11,
or 2^-25 (half the smallest subnormal) below the normal range:
    |err| <= u16 (|r| + delta) + 2^-25 + delta,   delta = 16 * 2^-24 * A.
"""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_tile_oracle as vt  # noqa: E402
from conftest import rel_l2  # noqa: E402
from oracle import vae_ref  # noqa: E402
from stablediffusion_amd import _lib, config, vae_tiles, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL  # noqa: E402
from test_vae_tiling import GRIDS, canvases  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-2                      # the project's stated relative L2 against the fp32 oracle (README)
U16, U32 = 2.0 ** -11, 2.0 ** -24
SENTINEL = 77.0
GUARD = 512


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ the merge kernel
def _merge_case(lib, tile, f, Cc, h, w, ld_pad, B=2):
    """Two launches on canvas [h, w] (a toy VAE of scale 1), the canvas inside a sentinel-filled buffer with row stride
    w + ld_pad: (kernel output, float64 reference, bound) after checking the guards and that the runs agree bit for bit."""
    p = vae_tiles.plan(False, h, w, tile, tile, f)
    want = vt.plan(False, h, w, tile, tile, f)
    rows = vt.raw_tiles(want, B, Cc, seed=tile * 100000 + h * 100 + w, dtype=torch.float16)
    ref, reads = vt.merge_closed(rows, p.blend, p.limit, return_reads=True)
    offs, total = vae_tiles.stack_offsets(p, B, Cc)
    # NaN wherever the closed form does not read: a stray read shows in the output
    stack = torch.full((total + 2 * GUARD,), float("nan"), dtype=torch.float16)
    for iy, row in enumerate(rows):
        for ix, t in enumerate(row):
            t = torch.where(reads[iy][ix], t, torch.full_like(t, float("nan")))
            o = GUARD + offs[iy * p.nx + ix]
            stack[o:o + t.numel()] = t.reshape(-1)
    A = max(t.abs().max().item() for row in rows for t in row)
    delta = 16 * U32 * A
    bound = U16 * (ref.abs() + delta) + 2.0 ** -25 + delta
    ld = w + ld_pad
    nrows = B * Cc * h
    buf = torch.full((GUARD + nrows * ld + GUARD,), SENTINEL, dtype=torch.float16).cuda()
    dstack = stack.cuda()
    outs = []
    for _ in range(2):
        buf.fill_(SENTINEL)
        rc = lib.sd_op_vae_tiles_merge(C.c_void_p(dstack.data_ptr() + 2 * GUARD), total, C.c_void_p(buf.data_ptr() + 2 * GUARD), ld,
                                       C.byref(p), B, Cc, 0, None, None)
        _lib.check(rc, "sd_op_vae_tiles_merge")
        outs.append(buf.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))          # the second run bit-equal
    got = outs[0]
    body = got[GUARD:GUARD + nrows * ld].view(nrows, ld)
    assert bool((got[:GUARD] == SENTINEL).all()) and bool((got[GUARD + nrows * ld:] == SENTINEL).all())
    assert bool((body[:, w:] == SENTINEL).all())                                     # nothing outside the canvas written
    out = body[:, :w].reshape(B, Cc, h, w).double()
    return out, ref, bound


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("Cc", [3, 8])
@pytest.mark.parametrize("tile,f", [(32, 0.25), (16, 0.5)])
def test_merge_kernel_per_element(engine_lib, tile, f, Cc, grid):
    ny, nx = grid
    stride = int(tile * (1 - f))
    worst = 0.0
    for h in canvases(ny, tile, stride):
        for w in canvases(nx, tile, stride):
            # a row stride that keeps 16-byte rows where the widths allow the vector kernel, and an odd one
            for ld_pad in ((8, 3) if w % 8 == 0 else (3,)):
                out, ref, bound = _merge_case(engine_lib, tile, f, Cc, h, w, ld_pad)
                assert bool(torch.isfinite(out).all()), (h, w, ld_pad)
                ratio = ((out - ref).abs() / bound).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (h, w, ld_pad, ratio)
    print("merge tile %d f %.2f C %d grid %dx%d: worst |err| / bound %.3f" % (tile, f, Cc, ny, nx, worst))


# ------------------------------------------------------------------------------------------------ the gather kernel
@pytest.mark.parametrize("case", [
    # (B, C, Hc, Wc, ld, th, tw, [(b, y, x)])
    (2, 4, 40, 48, 48, 16, 16, [(0, 0, 0), (1, 0, 0), (0, 24, 32), (1, 24, 32), (1, 8, 16)]),          # 16-byte path
    (2, 4, 40, 48, 56, 16, 16, [(0, 0, 0), (1, 24, 32)]),                                               # padded rows
    (2, 3, 37, 45, 45, 5, 7, [(0, 0, 0), (1, 32, 38), (0, 11, 3), (1, 1, 2)]),                          # odd everything
    (2, 4, 40, 48, 48, 16, 16, [(0, 0, 4), (1, 24, 32)]),                                               # a start off 8
    (3, 8, 9, 14, 14, 3, 1, [(b, 6, 13) for b in range(3)] + [(b, 0, 0) for b in range(3)]),            # one pixel wide
    (1, 4, 64, 64, 64, 64, 64, [(0, 0, 0)] * 32),                                                       # the full list
])
def test_gather_kernel_is_exact(engine_lib, case):
    B, Cc, Hc, Wc, ld, th, tw, tiles = case
    g = torch.Generator().manual_seed(Hc * Wc)
    canvas = torch.full((B, Cc, Hc, ld), SENTINEL, dtype=torch.float16)
    canvas[..., :Wc] = torch.randn(B, Cc, Hc, Wc, generator=g).half()
    n = len(tiles)
    numel = n * Cc * th * tw
    stack = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.float16).cuda()
    arr = lambda k: (C.c_int * n)(*[t[k] for t in tiles])                                    # noqa: E731
    dcanvas = canvas.cuda()
    _lib.check(engine_lib.sd_op_vae_tiles_gather(_ptr(dcanvas), ld, C.c_void_p(stack.data_ptr() + 2 * GUARD), arr(0), arr(1),
                                                 arr(2), n, B, Cc, Hc, Wc, th, tw, 0, None, None), "sd_op_vae_tiles_gather")
    got = stack.cpu()
    want = torch.stack([canvas[b, :, y:y + th, x:x + tw] for b, y, x in tiles])
    assert torch.equal(got[GUARD:GUARD + numel].view(n, Cc, th, tw).view(torch.int16), want.contiguous().view(torch.int16))
    assert bool((got[:GUARD] == SENTINEL).all()) and bool((got[GUARD + numel:] == SENTINEL).all())


def test_gather_refuses_a_tile_outside_the_canvas(engine_lib):
    x = torch.zeros(1, 1, 8, 8, dtype=torch.float16).cuda()
    out = torch.zeros(1, 1, 4, 4, dtype=torch.float16).cuda()
    for b, y, xx in [(1, 0, 0), (0, 5, 0), (0, 0, 5), (0, -1, 0)]:
        rc = engine_lib.sd_op_vae_tiles_gather(_ptr(x), 8, _ptr(out), (C.c_int * 1)(b), (C.c_int * 1)(y), (C.c_int * 1)(xx), 1,
                                               1, 1, 8, 8, 4, 4, 0, None, None)
        assert rc == 1 and b"outside the canvas" in engine_lib.sd_last_error()


# ------------------------------------------------------------------------------------------------ end to end, tiny VAE
TL, TS = 4, 32                  # the smallest tile of the tiny VAE (scale 8) whose crops tile the canvas at f = 0.25:
#                                 int(4 * 0.75) * 8 == 32 - int(32 * 0.25); tile_latent 2 and 3 are refused by the plan


@pytest.fixture(scope="module")
def tiny():
    cfg = config.tiny_vae()
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(cfg), seed=31, perturb=0.1).items()}
    vae = HipAutoencoderKL(cfg).load_state_dict(sd)
    vae.tile_latent_min_size, vae.tile_sample_min_size = TL, TS
    g = torch.Generator().manual_seed(7)
    # 2 x 3 tiles with truncated edges: rows of 4 and 2 latents, columns of 4, 4 and 1
    z = torch.randn(2, 4, 5, 7, generator=g).half()
    img = torch.randn(2, 3, 40, 56, generator=g).clamp(-1, 1).half()
    return cfg, sd, vae, z, img


def test_plan_refuses_the_smaller_tiny_tiles(engine_lib):
    for tl in (2, 3):
        with pytest.raises(_lib.EngineError, match="do not tile the canvas"):
            vae_tiles.plan(False, 5, 7, tl * 8, tl, 0.25)


def test_tiled_decode_matches_the_oracles_tiling(engine_lib, tiny):
    cfg, sd, vae, z, _ = tiny
    p = vae_tiles.plan(False, 5, 7, TS, TL, 0.25)
    assert (p.ny, p.nx) == (2, 3) and [(c["h"], c["w"]) for c in vae_tiles.classes(p)] == [(4, 4), (4, 1), (2, 4), (2, 1)]
    with torch.no_grad():
        ref = vt.tiled_decode(lambda t: vae_ref.vae_decode(cfg, sd, t.float()), z, TS, TL, 0.25)
    vae.enable_tiling()
    try:
        got = vae.decode(z.cuda())[0]
    finally:
        vae.disable_tiling()
    assert got.shape == ref.shape == (2, 3, 40, 56)
    e = rel_l2(got, ref)
    print("tiny tiled decode, 2 x 3 tiles, B = 2: rel-L2 %.3e (bound %.0e)" % (e, TOL))
    assert e < TOL
    w, s, t = vae.memory_tiled()
    assert t > 0 and (w, s) == vae.memory()


def test_tiled_encode_matches_the_oracles_tiling(engine_lib, tiny):
    cfg, sd, vae, _, img = tiny
    with torch.no_grad():
        ref = vt.tiled_encode(lambda t: vae_ref.vae_encode_moments(cfg, sd, t.float()), img, TS, TL, 0.25)
    vae.enable_tiling()
    try:
        got = vae.encode_moments(img.cuda())
    finally:
        vae.disable_tiling()
    assert got.shape == ref.shape == (2, 8, 5, 7)
    e = rel_l2(got, ref)
    print("tiny tiled encode, 2 x 3 tiles, B = 2: rel-L2 %.3e (bound %.0e)" % (e, TOL))
    assert e < TOL


def test_tiled_calls_refuse_debug_taps(engine_lib, tiny):
    _, _, vae, z, _ = tiny
    out = torch.zeros(2, 3, 40, 56, dtype=torch.float16).cuda()
    _lib.check(engine_lib.sd_vae_tap(vae._h, 1), "sd_vae_tap")
    try:
        rc = engine_lib.sd_vae_decode_tiled(vae._h, _ptr(z.cuda()), _ptr(out), 2, 5, 7, TL, 0.25, 4, None)
        assert rc == 4 and b"debug taps" in engine_lib.sd_last_error()            # SD_ERR_UNSUPPORTED
    finally:
        _lib.check(engine_lib.sd_vae_tap(vae._h, 0), "sd_vae_tap")


# ------------------------------------------------------------------------------------------------ equivalences
def _bits(t):
    return t.cpu().view(torch.int16)


def test_switch_equivalences_bit_for_bit(engine_lib, tiny):
    _, _, vae, z, img = tiny
    zc, ic = z.cuda(), img.cuda()
    one_tile = zc[:, :, :TL, :TL].contiguous()
    one_img = ic[:, :, :TS, :TS].contiguous()
    plain = {k: _bits(v) for k, v in (("z", vae.decode(zc)[0]), ("z1", vae.decode(one_tile)[0]),
                                      ("i", vae.encode_moments(ic)), ("i1", vae.encode_moments(one_img)))}
    vae.enable_tiling()
    try:
        # a canvas no larger than one tile with tiling on is the plain call
        assert torch.equal(_bits(vae.decode(one_tile)[0]), plain["z1"])
        assert torch.equal(_bits(vae.encode_moments(one_img)), plain["i1"])
        tiled = _bits(vae.decode(zc)[0])
        assert not torch.equal(tiled, plain["z"])                    # (the tiled result differs: it has seams)
        assert torch.equal(_bits(vae.decode(zc)[0]), tiled)          # and is the same on every run
        # slicing composes with tiling: one image at a time, the same bits
        vae.enable_slicing()
        assert torch.equal(_bits(vae.decode(zc)[0]), tiled)
        vae.disable_slicing()
    finally:
        vae.disable_tiling()
    # tiling on then off restores the plain result
    assert torch.equal(_bits(vae.decode(zc)[0]), plain["z"])
    assert torch.equal(_bits(vae.encode_moments(ic)), plain["i"])
    # slicing on equals slicing off
    vae.enable_slicing()
    try:
        assert torch.equal(_bits(vae.decode(zc)[0]), plain["z"])
        assert torch.equal(_bits(vae.encode_moments(ic)), plain["i"])
    finally:
        vae.disable_slicing()
