"""HyperTile's division rule (sd_unet_set_hypertile): which tile counts an axis offers and which one a site draws at a step.

One axis of `n` tokens offers the first `swap_size` divisors of `n` that are at least min(tile_size, n) as tile extents;
a self-attention site draws one candidate per axis from the counter hash token merging's plan uses.  The engine's
`sd_hypertile_plan` is the same arithmetic; tools and tests use this copy."""
from __future__ import annotations

from typing import List, Tuple

_M32 = 0xFFFFFFFF


def mix32(seed: int, step: int, site: int, cell: int) -> int:
    h = (seed ^ (step * 0x9E3779B9) ^ (site * 0x85EBCA6B) ^ (cell * 0xC2B2AE35)) & _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    h ^= h >> 16
    return h


def counts(n: int, tile_size: int, swap_size: int) -> List[int]:
    """Tile counts of one axis, most tiles first; never empty (the whole axis always divides)."""
    if n < 1 or tile_size < 1 or not 1 <= swap_size <= 8:
        raise ValueError(f"hypertile.counts: n >= 1, tile_size >= 1 and swap_size in 1..8 required, got {(n, tile_size, swap_size)}")
    m = min(tile_size, n)
    extents = [e for e in range(m, n + 1) if n % e == 0][:swap_size]
    return [n // e for e in extents]


def plan(Hs: int, Ws: int, tile_size: int, swap_size: int, seed: int, step: int, site: int) -> Tuple[int, int, int, int]:
    """(nh, nw, th, tw) of the site on an Hs x Ws map at this step."""
    ch, cw = counts(Hs, tile_size, swap_size), counts(Ws, tile_size, swap_size)
    nh = ch[mix32(seed, step, site, 0) % len(ch)]
    nw = cw[mix32(seed, step, site, 1) % len(cw)]
    return nh, nw, Hs // nh, Ws // nw
