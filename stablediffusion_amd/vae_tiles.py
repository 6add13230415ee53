"""Tiled VAE: the host-side plan of a tiled decode / encode (sd_vae_tile_plan, include/sd_engine.h) and the layout of
the tile stack the merge launch reads (sd_vae_tile_stack).  Both need no device.

The semantics are diffusers 0.27.2 `AutoencoderKL.tiled_decode` / `tiled_encode` (recalled, not pinned: DESIGN.md
section 8); `HipAutoencoderKL.enable_tiling()` is the switch, this module is what tests and tools look the plan up with.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

from . import _lib


def plan(encode: bool, h: int, w: int, tile_sample: int, tile_latent: int, overlap_factor: float = 0.25) -> _lib.SdVAETiles:
    """The plan of a canvas [h, w] in INPUT space (latents for decode, pixels for encode); EngineError where the engine
    refuses it (factor outside [0, 0.5], blend above half a tile, more than 64 tiles on an axis, crops that would not
    tile the canvas)."""
    p = _lib.SdVAETiles()
    lib = _lib.load()
    _lib.check(lib.sd_vae_tile_plan(int(bool(encode)), int(h), int(w), int(tile_sample), int(tile_latent),
                                    float(overlap_factor), C.byref(p)), "sd_vae_tile_plan")
    return p


def classes(p: _lib.SdVAETiles) -> List[dict]:
    """The shape classes: input shape (h, w), and the tiles (iy, ix) of each in the order they are stacked."""
    out = []
    for c in range(p.n_classes):
        tiles = [(p.class_iy0[c] + t // p.class_nx[c], p.class_ix0[c] + t % p.class_nx[c]) for t in range(p.class_count[c])]
        out.append({"h": p.class_h[c], "w": p.class_w[c], "tiles": tiles})
    return out


def stack_offsets(p: _lib.SdVAETiles, B: int, C_: int) -> Tuple[List[int], int]:
    """(element offset of tile iy * nx + ix in the merge's tile stack, total elements) for B images of C_ channels."""
    offs = (C.c_int64 * (p.ny * p.nx))()
    total = C.c_int64()
    _lib.check(_lib.load().sd_vae_tile_stack(C.byref(p), int(B), int(C_), offs, C.byref(total)), "sd_vae_tile_stack")
    return list(offs), total.value
