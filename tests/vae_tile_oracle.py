"""Test helper, not a test: diffusers 0.27.2 `AutoencoderKL.tiled_decode` / `tiled_encode` / `blend_v` / `blend_h`,
restated in float64.

RECALLED, NOT PINNED: diffusers is not installed here and the reference carries no fixture for this path (the same
status as the FreeU and LCM notes).  What is restated:

    tiled_decode(z):  overlap = int(tl (1 - f)); blend = int(ts f); limit = ts - blend
                      rows[i][j] = decoder(post_quant_conv(z[:, :, i:i+tl, j:j+tl]))  for i, j in range(0, h|w, overlap)
                      raster order, IN PLACE: tile = blend_v(rows[i-1][j], tile, blend) if i > 0
                                              tile = blend_h(row[j-1], tile, blend)     if j > 0
                      result = cat of every tile[:, :, :limit, :limit]
    blend_v(a, b, e): e = min(a.shape[2], b.shape[2], e); b[:, :, y, :] = a[:, :, -e + y, :] (1 - y/e) + b[:, :, y, :] (y/e)
    blend_h likewise along x.   tiled_encode: the same in image space with ts / tl exchanged, on the moments.

Three things live here: the plan (the loops above, as lists), the sequential in-place merge, and the closed form the
engine's merge kernel evaluates.  `merge_closed` also reports which raw tile elements it read.
"""
from __future__ import annotations

import torch


def plan_ints(encode: bool, tile_sample: int, tile_latent: int, f: float):
    """(tile_in, stride_in, tile_out, blend, limit) -- diffusers' integers."""
    tin, tout = (tile_sample, tile_latent) if encode else (tile_latent, tile_sample)
    stride = int(tin * (1 - f))
    blend = int(tout * f)
    return tin, stride, tout, blend, tout - blend


def plan(encode: bool, h: int, w: int, tile_sample: int, tile_latent: int, f: float) -> dict:
    """The loop of tiled_decode / tiled_encode over a canvas [h, w] in input space: starts and (truncated) sizes per axis,
    and the tiles grouped by input shape in first-seen raster order."""
    tin, stride, tout, blend, limit = plan_ints(encode, tile_sample, tile_latent, f)
    ys = list(range(0, h, stride))
    xs = list(range(0, w, stride))
    size_y = [min(i + tin, h) - i for i in ys]
    size_x = [min(j + tin, w) - j for j in xs]
    classes = {}
    for iy in range(len(ys)):
        for ix in range(len(xs)):
            classes.setdefault((size_y[iy], size_x[ix]), []).append((iy, ix))
    return {"ys": ys, "xs": xs, "size_y": size_y, "size_x": size_x, "tile_in": tin, "stride_in": stride, "tile_out": tout,
            "blend": blend, "limit": limit, "classes": classes}


def blend_v(a, b, e):
    e = min(a.shape[2], b.shape[2], e)
    for y in range(e):
        b[:, :, y, :] = a[:, :, -e + y, :] * (1 - y / e) + b[:, :, y, :] * (y / e)
    return b


def blend_h(a, b, e):
    e = min(a.shape[3], b.shape[3], e)
    for x in range(e):
        b[:, :, :, x] = a[:, :, :, -e + x] * (1 - x / e) + b[:, :, :, x] * (x / e)
    return b


def merge_sequential(rows, blend: int, limit: int) -> torch.Tensor:
    """diffusers' merge of raw output tiles rows[i][j] ([B, C, th, tw]): in place on float64 copies, raster order."""
    rows = [[t.double().clone() for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, blend)
            if j > 0:
                tile = blend_h(row[j - 1], tile, blend)
            result_row.append(tile[:, :, :limit, :limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def _lerp(p, q, t):
    return p * (1 - t) + q * t


def merge_closed(rows, blend: int, limit: int, return_reads: bool = False):
    """The closed form: every output pixel from at most four RAW tiles,
        out = lerp_x( lerp_y(AL, L), lerp_y( lerp_x(AL, A), b ) ),
    b the tile whose crop holds the pixel, A / L / AL the tiles above / left / above-left read at their bottom-most ev
    rows / right-most eh columns, ty = y / ev inside the top strip, tx = x / eh inside the left strip; outside a strip the
    lerp passes its second operand through and its first is not read.  With return_reads also a boolean mask per tile of
    the elements read."""
    raw = [[t.double() for t in row] for row in rows]
    reads = [[torch.zeros(t.shape, dtype=torch.bool) for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(raw):
        result_row = []
        for j, b in enumerate(row):
            th, tw = b.shape[2], b.shape[3]
            ch, cw = min(th, limit), min(tw, limit)
            out = b[:, :, :ch, :cw].clone()
            reads[i][j][:, :, :ch, :cw] = True
            ev = min(raw[i - 1][j].shape[2], th, blend) if i > 0 else 0
            eh = min(row[j - 1].shape[3], tw, blend) if j > 0 else 0
            ty = (torch.arange(ev, dtype=torch.float64) / max(ev, 1)).view(1, 1, ev, 1)
            tx = (torch.arange(eh, dtype=torch.float64) / max(eh, 1)).view(1, 1, 1, eh)
            if ev:
                A = raw[i - 1][j]
                ah = A.shape[2]
                top = A[:, :, ah - ev:, :cw].clone()
                reads[i - 1][j][:, :, ah - ev:, :cw] = True
            if eh:
                L = row[j - 1]
                lw = L.shape[3]
                left = L[:, :, :ch, lw - eh:].clone()
                reads[i][j - 1][:, :, :ch, lw - eh:] = True
            if ev and eh:
                AL = raw[i - 1][j - 1]
                al = AL[:, :, AL.shape[2] - ev:, AL.shape[3] - eh:]
                reads[i - 1][j - 1][:, :, AL.shape[2] - ev:, AL.shape[3] - eh:] = True
                top[:, :, :, :eh] = _lerp(al, top[:, :, :, :eh], tx)
                left[:, :, :ev, :] = _lerp(al, left[:, :, :ev, :], ty)
            if ev:
                out[:, :, :ev, :] = _lerp(top, out[:, :, :ev, :], ty)
            if eh:
                out[:, :, :, :eh] = _lerp(left, out[:, :, :, :eh], tx)
            result_row.append(out)
        result_rows.append(torch.cat(result_row, dim=3))
    merged = torch.cat(result_rows, dim=2)
    return (merged, reads) if return_reads else merged


def tiled_apply(fn, x: torch.Tensor, encode: bool, tile_sample: int, tile_latent: int, f: float) -> torch.Tensor:
    """tiled_decode (fn = post_quant_conv + decoder) or tiled_encode up to the merged moments (fn = encoder + quant_conv)
    of canvas x, sequential form, float64."""
    tin, stride, _, blend, limit = plan_ints(encode, tile_sample, tile_latent, f)
    rows = []
    for i in range(0, x.shape[2], stride):
        rows.append([fn(x[:, :, i:i + tin, j:j + tin]) for j in range(0, x.shape[3], stride)])
    return merge_sequential(rows, blend, limit)


def tiled_decode(decode_fn, z, tile_sample: int, tile_latent: int, f: float = 0.25):
    return tiled_apply(decode_fn, z, False, tile_sample, tile_latent, f)


def tiled_encode(encode_fn, x, tile_sample: int, tile_latent: int, f: float = 0.25):
    return tiled_apply(encode_fn, x, True, tile_sample, tile_latent, f)


def raw_tiles(p: dict, B: int, C: int, scale_num: int = 1, scale_den: int = 1, seed: int = 0, dtype=torch.float64):
    """Random raw OUTPUT tiles rows[i][j] for plan p (output size = input size * scale_num / scale_den)."""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(B, C, sy * scale_num // scale_den, sx * scale_num // scale_den, generator=g, dtype=torch.float64).to(dtype)
             for sx in p["size_x"]] for sy in p["size_y"]]
