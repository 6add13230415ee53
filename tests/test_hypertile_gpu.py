"""HyperTile on the GPU: the gather / scatter kernels bit for bit against torch indexing with guard rows and columns, the
tiled attention (gather, the unchanged attention kernel on batch B nh nw, scatter) per element against the float64
tiled attention under tests/test_attention_gpu.py's bound, the UNet forward against the float64 oracle run with the
divisions the engine reported, off == plain bit for bit, steps, forward_cfg, DeepCache store + reuse, the engine's
refusals and a forward on NaN-filled scratch."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
import hypertile_oracle  # noqa: E402
from conftest import rel_l2  # noqa: E402
from stablediffusion_amd import _lib, config, hypertile, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-2                     # tests/test_tome_gpu.py: TOL
SENTINEL = 0x7E5A              # an fp16 NaN pattern, compared as int16
GUARD = 8                      # guard rows in front of and behind dst


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ gather / scatter
def tile_order(B, Hs, Ws, nh, nw):
    """perm [B Hs Ws]: the raster-order row that tile-order row r holds."""
    rows = torch.arange(B * Hs * Ws).view(B, Hs * Ws, 1)
    return hypertile_oracle.to_tiles(rows, Hs, Ws, nh, nw).reshape(-1)


def run_copy(lib, fn, src_rows, cols, lds, ldd, B, Hs, Ws, nh, nw):
    """One launch of `fn` from an int16 source [M, cols] placed in a row of stride lds into a sentinel-filled dst of
    stride ldd with guard rows around it; returns dst's [M, cols] after checking the guards."""
    M = B * Hs * Ws
    g = torch.Generator().manual_seed(5)
    src = torch.randint(-2 ** 15, 2 ** 15, (M, lds), generator=g, dtype=torch.int16).cuda()
    src[:, :cols] = src_rows.cuda()
    dst = torch.full((M + 2 * GUARD, ldd), SENTINEL, dtype=torch.int16, device="cuda")
    rc = getattr(lib, fn)(P(src), lds, cols, B, Hs, Ws, nh, nw, P(dst[GUARD:]), ldd, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    out = dst.cpu()
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + M:] == SENTINEL).all(), "guard rows were written"
    assert (out[:, cols:] == SENTINEL).all(), "guard columns were written"
    return out[GUARD:GUARD + M, :cols]


@pytest.mark.parametrize("B,Hs,Ws,nh,nw,cols", [(2, 16, 16, 2, 2, 192), (1, 12, 20, 2, 2, 960), (3, 8, 24, 1, 3, 64),
                                                (2, 24, 8, 3, 1, 128)])
def test_gather_scatter_bit_for_bit(engine_lib, B, Hs, Ws, nh, nw, cols):
    M = B * Hs * Ws
    g = torch.Generator().manual_seed(B * 1000 + cols)
    data = torch.randint(-2 ** 15, 2 ** 15, (M, cols), generator=g, dtype=torch.int16)      # every bit pattern, NaNs included
    perm = tile_order(B, Hs, Ws, nh, nw)
    geom = (B, Hs, Ws, nh, nw)
    gathered = run_copy(engine_lib, "sd_op_hypertile_gather", data, cols, cols + 24, cols + 8, *geom)
    assert torch.equal(gathered, data[perm])
    want = torch.empty_like(data)
    want[perm] = data
    scattered = run_copy(engine_lib, "sd_op_hypertile_scatter", data, cols, cols + 8, cols + 16, *geom)
    assert torch.equal(scattered, want)
    back = run_copy(engine_lib, "sd_op_hypertile_scatter", gathered, cols, cols + 8, cols + 8, *geom)
    assert torch.equal(back, data)                      # the round trip is the identity


def test_gather_scatter_rejections(engine_lib):
    lib = engine_lib
    src = torch.zeros(256 + 1, 64, dtype=torch.int16, device="cuda")
    dst = torch.full((256 + 1, 64), SENTINEL, dtype=torch.int16, device="cuda")
    ok = dict(src=src.data_ptr(), lds=64, cols=32, B=1, Hs=16, Ws=16, nh=2, nw=2, dst=dst.data_ptr(), ldd=64)
    bad = [dict(cols=12), dict(cols=0), dict(lds=60), dict(ldd=52), dict(lds=24), dict(ldd=24), dict(src=src.data_ptr() + 8),
           dict(dst=dst.data_ptr() + 2), dict(nh=3), dict(nw=5), dict(B=0), dict(nh=0), dict(nw=0), dict(src=None), dict(dst=None)]
    for fn in ("sd_op_hypertile_gather", "sd_op_hypertile_scatter"):
        for change in bad:
            a = dict(ok, **change)
            rc = getattr(lib, fn)(a["src"], a["lds"], a["cols"], a["B"], a["Hs"], a["Ws"], a["nh"], a["nw"], a["dst"], a["ldd"],
                                  stream())
            assert rc == 1, (fn, change)
            assert b"hypertile" in lib.sd_last_error()
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all(), "a refused launch wrote"
    a = ok
    assert lib.sd_op_hypertile_gather(a["src"], a["lds"], a["cols"], a["B"], a["Hs"], a["Ws"], a["nh"], a["nw"], a["dst"], a["ldd"],
                                      stream()) == 0
    torch.cuda.synchronize()
    assert (dst[:256, :32] == 0).all() and (dst[:256, 32:] == SENTINEL).all() and (dst[256:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------ tiled attention
# (Hs, Ws, nh, nw): tiles of 64 tokens (exactly one key tile), 60 (ragged), 72 (one tile plus 8) and 16
TILINGS = [(16, 16, 2, 2), (12, 20, 2, 2), (12, 24, 2, 2), (8, 8, 2, 2)]


@pytest.mark.parametrize("d", [32, 40, 160])
@pytest.mark.parametrize("Hs,Ws,nh,nw", TILINGS)
def test_tiled_attention_against_float64(engine_lib, d, Hs, Ws, nh, nw):
    """gather -> sd_op_attention_ex (pre-scaled queries, as the UNet's) -> scatter on one q|k|v buffer, against the
    float64 attention of every tile; the bound and rel-L2 limit are tests/test_attention_gpu.py's."""
    lib = engine_lib
    B, heads = 2, 2
    Cw, T, tt = heads * d, Hs * Ws, (Hs // nh) * (Ws // nw)
    assert tt in (64, 60, 72, 16)
    g = torch.Generator().manual_seed(d * 100 + tt)
    q = (torch.randn(B, T, Cw, generator=g) * ac.LOG2E / math.sqrt(d)).half()
    k, v = torch.randn(B, T, Cw, generator=g).half(), torch.randn(B, T, Cw, generator=g).half()
    # float64 per tile, through attn_cases.reference on the tile-ordered operands
    case = ac.Case("hypertile", B * nh * nw, heads, tt, tt, d, 0, 1, "randn", ("qkv",), None)
    O, A = ac.reference(case, *(hypertile_oracle.to_tiles(t, Hs, Ws, nh, nw) for t in (q, k, v)))
    O, A = hypertile_oracle.from_tiles(O, Hs, Ws, nh, nw), hypertile_oracle.from_tiles(A, Hs, Ws, nh, nw)
    # and the same through the oracle's own tiled attention (the two float64 forms agree)
    unscale = math.sqrt(d) / ac.LOG2E
    O2 = hypertile_oracle.tiled_attention(q.double() * unscale, k.double(), v.double(), heads, Hs, Ws, nh, nw)
    assert (O - O2).abs().max() < 1e-12
    M = B * T
    qkv = torch.cat([q, k, v], dim=-1).reshape(M, 3 * Cw).cuda()
    qg = torch.full((M, 3 * Cw), float("nan"), dtype=torch.float16, device="cuda")
    og = torch.full((M, Cw), float("nan"), dtype=torch.float16, device="cuda")
    out = torch.full((M, Cw), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.sd_op_hypertile_gather(P(qkv), 3 * Cw, 3 * Cw, B, Hs, Ws, nh, nw, P(qg), 3 * Cw, stream()) == 0, lib.sd_last_error()
    rc = lib.sd_op_attention_ex(P(qg[:, :Cw]), P(qg[:, Cw:2 * Cw]), P(qg[:, 2 * Cw:]), P(og), B * nh * nw, tt, tt, heads, d,
                                3 * Cw, 3 * Cw, 3 * Cw, Cw, 0, 1, stream())
    assert rc == 0, lib.sd_last_error()
    assert lib.sd_op_hypertile_scatter(P(og), Cw, Cw, B, Hs, Ws, nh, nw, P(out), Cw, stream()) == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    o = out.cpu().view(B, T, Cw).double()
    assert torch.isfinite(o).all()
    err = (o - O).abs()
    bound = ac.elementwise_bound(O, A, tt, v.abs().max().double())
    r, ratio = rel_l2(o, O), (err / bound).max().item()
    print(f"tiled attention d {d}, {Hs}x{Ws} in {nh}x{nw} ({tt} tokens): rel-L2 {r:.2e}, worst |err| / bound {ratio:.3f}")
    assert r < 3e-3
    assert ratio <= 1.0
    # band form: nw == 1 needs no copy, the attention runs on the raster-order rows with batch B nh
    band = torch.full((M, Cw), float("nan"), dtype=torch.float16, device="cuda")
    rc = lib.sd_op_attention_ex(P(qkv[:, :Cw]), P(qkv[:, Cw:2 * Cw]), P(qkv[:, 2 * Cw:]), P(band), B * nh, T // nh, T // nh, heads, d,
                                3 * Cw, 3 * Cw, 3 * Cw, Cw, 0, 1, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    Ob = hypertile_oracle.tiled_attention(q.double() * unscale, k.double(), v.double(), heads, Hs, Ws, nh, 1)
    assert rel_l2(band.cpu().view(B, T, Cw), Ob) < 3e-3


# ---------------------------------------------------------------------------------------------------- UNet
def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


_NETS = {}


def _build(kind):
    cfg = config.tiny_unet() if kind == "sd15" else config.tiny_unet(linear=True, sdxl_cond=True)
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    added = None
    if kind == "sdxl":
        added = {"text_embeds": torch.randn(2, 64, generator=g).half(), "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)}
    xw = torch.randn(2, 4, 16, 24, generator=g).half()
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd), x, ehs, added, xw


def _make(kind):
    if kind not in _NETS:
        _NETS[kind] = _build(kind)
    return _NETS[kind]


@pytest.fixture(scope="module", params=["sd15", "sdxl"])
def tiny(request):
    return _make(request.param)


@pytest.fixture(scope="module")
def tiny15():
    return _make("sd15")


def _run(net, x, ehs, added):
    return net(x.cuda(), torch.tensor(501.0), ehs.cuda(), added_cond_kwargs=added)[0].float().cpu()


_PLAIN = {}


def _plain(tiny, x):
    """The never-enabled forward of the fixture's network on x, computed once per (network, input)."""
    cfg, sd, net, _, ehs, added, _ = tiny
    key = (id(net), tuple(x.shape))
    if key not in _PLAIN:
        assert net.hypertile is None
        _PLAIN[key] = _run(net, x, ehs, added)
    return _PLAIN[key]


def _oracle(cfg, sd, x, ehs, added, ht):
    w = {k: v.double() for k, v in sd.items()}
    a = None if added is None else {"text_embeds": added["text_embeds"].double(), "time_ids": added["time_ids"].double()}
    with torch.no_grad():
        return hypertile_oracle.unet_forward(cfg, w, x.double(), torch.tensor(501.0, dtype=torch.float64), ehs.double(), a, ht)


L0, L1 = [0, 1, 13, 14, 15], [2, 3, 10, 11, 12]       # tiny_unet's level-0 and level-1 blocks, by ordinal


def _check_forward(tiny, x, tile, depth, step, want_sites, site0=None):
    cfg, sd, net, _, ehs, added, _ = tiny
    H, W = x.shape[2:]
    plain = _plain(tiny, x)
    net.enable_hypertile(tile, 2, depth, 0).hypertile_step(step)
    try:
        got = _run(net, x, ehs, added)
        sites = net.hypertile_sites()
    finally:
        net.disable_hypertile()
    assert [s["site"] for s in sites] == want_sites
    for s in sites:
        lvl = 0 if s["site"] in L0 else 1
        assert (s["H"], s["W"], s["level"], s["images"]) == (H >> lvl, W >> lvl, lvl, 2), s
        assert (s["nh"], s["nw"]) == hypertile.plan(s["H"], s["W"], tile, 2, 0, step, s["site"])[:2], s
        assert s["copied"] == (s["nw"] > 1), s
    if site0 is not None:
        assert (sites[0]["nh"], sites[0]["nw"]) == site0
    ref = _oracle(cfg, sd, x, ehs, added,
                  hypertile_oracle.HyperTile(tile, 2, depth, 0, step, divisions={s["site"]: (s["nh"], s["nw"]) for s in sites}))
    err, moved = rel_l2(got, ref), rel_l2(plain, ref)
    print(f"unet hypertile {H}x{W} tile {tile} depth {depth} step {step}: rel-L2 vs oracle on the engine's divisions {err:.2e}; "
          f"plain forward vs that oracle {moved:.2e}")
    assert err < TOL
    assert moved > err                                  # the plain forward is farther from that oracle than the engine's
    # off again: the never-enabled forward, bit for bit
    assert torch.equal(_run(net, x, ehs, added), plain)
    assert net.hypertile_sites() == []
    return got, sites


@pytest.mark.parametrize("step,site0", [(0, (2, 2)), (2, (1, 2)), (3, (2, 1))])
def test_unet_with_hypertile_matches_oracle(engine_lib, tiny, step, site0):
    """tile_size 8 on 16 x 16 latents, level 0 only: site 0 draws 2 x 2 (copied), 1 x 2 (copied), 2 x 1 (a band, not copied)."""
    _check_forward(tiny, tiny[3], 8, 0, step, L0, site0)


@pytest.mark.parametrize("step", [0, 2, 3])
def test_unet_with_hypertile_two_levels(engine_lib, tiny, step):
    _check_forward(tiny, tiny[3], 4, 1, step, [0, 1, 2, 3, 10, 11, 12, 13, 14, 15])


@pytest.mark.parametrize("tile,depth,want", [(8, 0, L0), (4, 1, [0, 1, 2, 3, 10, 11, 12, 13, 14, 15])])
def test_unet_with_hypertile_on_a_wide_map(engine_lib, tiny, tile, depth, want):
    for step in (0, 2, 3):
        _check_forward(tiny, tiny[6], tile, depth, step, want)


def _profile(lib, net, x, ehs, added):
    lib.sd_prof_enable(1)
    try:
        _run(net, x, ehs, added)
        ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {ents[i].kernel.decode(): (int(ents[i].launches), float(ents[i].flops), float(ents[i].bytes)) for i in range(n.value)}


def test_off_equals_plain(engine_lib, tiny):
    """Step 4 draws (1, 1) at site 0: that site runs the plain launches.  tile_size >= max(H, W) and disable_hypertile()
    give the never-enabled output bit for bit and the never-enabled launch list."""
    cfg, sd, net, x, ehs, added, _ = tiny
    lib = engine_lib
    plain = _plain(tiny, x)
    off = _profile(lib, net, x, ehs, added)
    assert not any(k.startswith("hypertile_") for k in off)
    net.enable_hypertile(8, 2, 0, 0).hypertile_step(4)
    try:
        on = _profile(lib, net, x, ehs, added)
        sites = net.hypertile_sites()
    finally:
        net.disable_hypertile()
    assert (sites[0]["site"], sites[0]["nh"], sites[0]["nw"], sites[0]["copied"]) == (0, 1, 1, False)
    copied = [s for s in sites if s["copied"]]
    assert len(copied) >= 1
    for k in ("hypertile_gather_kernel", "hypertile_scatter_kernel"):
        assert on[k][0] == len(copied), (k, on.get(k))
    Cw = 64                                             # level 0 of tiny_unet: heads x d
    assert on["hypertile_gather_kernel"][2] == sum(2.0 * 2 * 256 * 3 * Cw * 2 for _ in copied)
    assert on["hypertile_scatter_kernel"][2] == sum(2.0 * 2 * 256 * Cw * 2 for _ in copied)
    # every launch but the copies as before, and the attention FLOPs of a site fall by nh nw (site 0: not at all)
    assert {k: v[0] for k, v in on.items() if not k.startswith("hypertile_")} == {k: v[0] for k, v in off.items()}
    full = 4.0 * 2 * Cw * 256 * 256
    attn = lambda prof: sum(v[1] for k, v in prof.items() if k.startswith("attn_kernel"))
    assert attn(on) == attn(off) - sum(full - full / (s["nh"] * s["nw"]) for s in sites)
    # a tile as large as the map, and off: the plain forward
    net.enable_hypertile(16, 2, 0, 0).hypertile_step(0)
    try:
        whole = _run(net, x, ehs, added)
        ws = net.hypertile_sites()
        prof = _profile(lib, net, x, ehs, added)
    finally:
        net.disable_hypertile()
    assert torch.equal(whole, plain)
    assert [s["site"] for s in ws] == L0 and all((s["nh"], s["nw"], s["copied"]) == (1, 1, False) for s in ws)
    assert {k: v[:2] for k, v in prof.items()} == {k: v[:2] for k, v in off.items()}
    assert torch.equal(_run(net, x, ehs, added), plain)
    assert net.hypertile_sites() == [] and net.hypertile is None
    assert {k: v[0] for k, v in _profile(lib, net, x, ehs, added).items()} == {k: v[0] for k, v in off.items()}


def test_steps_and_reproducibility(engine_lib, tiny):
    cfg, sd, net, x, ehs, added, _ = tiny
    net.enable_hypertile(8, 2, 0, 0)
    try:
        a = _run(net.hypertile_step(0), x, ehs, added)
        sa = net.hypertile_sites()
        b = _run(net.hypertile_step(3), x, ehs, added)
        sb = net.hypertile_sites()
        a2 = _run(net.hypertile_step(0), x, ehs, added)
        sa2 = net.hypertile_sites()
        b2 = _run(net.hypertile_step(3), x, ehs, added)
    finally:
        net.disable_hypertile()
    assert torch.equal(a, a2) and sa == sa2 and torch.equal(b, b2)
    assert sa != sb and not torch.equal(a, b)


def test_forward_cfg(engine_lib, tiny15):
    """forward_cfg (shared prefix: the first block runs on half the batch) against the plain forward on duplicated latents,
    with the comparison of tests/test_cfg_share_gpu.py: the shared prefix computes the same values once."""
    cfg, sd, net, x, ehs, added, _ = tiny15
    lat = x[:1]
    net.enable_hypertile(8, 2, 0, 0).hypertile_step(0)
    try:
        two = net(torch.cat([lat, lat]).cuda(), torch.tensor(501.0), ehs.cuda())[0].float().cpu()
        s2 = net.hypertile_sites()
        one = net.forward_cfg(lat.cuda(), torch.tensor(501.0), ehs.cuda())
        one = (one[0] if isinstance(one, (tuple, list)) else one).float().cpu()
        s1 = net.hypertile_sites()
    finally:
        net.disable_hypertile()
    assert [s["images"] for s in s1] == [1, 2, 2, 2, 2] and [s["images"] for s in s2] == [2] * 5
    assert [(s["site"], s["nh"], s["nw"]) for s in s1] == [(s["site"], s["nh"], s["nw"]) for s in s2]
    e = rel_l2(one, two)
    print(f"forward_cfg vs forward on duplicated latents with HyperTile: rel-L2 {e:.2e}")
    assert e < 1e-3                                     # tests/test_cfg_share_gpu.py: SAME


def test_with_deepcache_store_and_reuse(engine_lib, tiny):
    """One store + reuse pair with HyperTile on against deepcache_oracle's forms composed with the HyperTile oracle, each
    run with the engine's divisions; a reuse step's blocks keep the ordinals of the full forward."""
    cfg, sd, net, x, ehs, added, _ = tiny
    g = torch.Generator().manual_seed(77)
    x1 = torch.randn(2, 4, 16, 16, generator=g).half()
    net.enable_deepcache(2, 1)
    net.enable_hypertile(8, 2, 0, 0)
    try:
        net.deep_cache_mode(net.DC_STORE).hypertile_step(0)
        got0 = _run(net, x, ehs, added)
        s0 = net.hypertile_sites()
        net.deep_cache_mode(net.DC_REUSE).hypertile_step(2)
        got1 = _run(net, x1, ehs, added)
        s1 = net.hypertile_sites()
    finally:
        net.deep_cache_mode(net.DC_PLAIN)
        net.disable_hypertile()
        net.disable_deepcache()
    assert [s["site"] for s in s0] == L0 and [s["site"] for s in s1] == [0, 14, 15]
    for step, ss in ((0, s0), (2, s1)):
        for s in ss:
            assert (s["nh"], s["nw"]) == hypertile.plan(16, 16, 8, 2, 0, step, s["site"])[:2]
    w = {k: v.double() for k, v in sd.items()}
    a = None if added is None else {"text_embeds": added["text_embeds"].double(), "time_ids": added["time_ids"].double()}
    t = torch.tensor(501.0, dtype=torch.float64)
    div = lambda ss: {s["site"]: (s["nh"], s["nw"]) for s in ss}
    with torch.no_grad():
        h0 = hypertile_oracle.HyperTile(8, 2, 0, 0, 0, divisions=div(s0))
        ref0, feat = hypertile_oracle.deepcache_forward(cfg, w, x.double(), t, ehs.double(), a, 1, h0)
        h1 = hypertile_oracle.HyperTile(8, 2, 0, 0, 2, divisions=div(s1))
        ref1, _ = hypertile_oracle.deepcache_forward(cfg, w, x1.double(), t, ehs.double(), a, 1, h1, cached=feat)
    e0, e1 = rel_l2(got0, ref0), rel_l2(got1, ref1)
    print(f"deepcache + hypertile: store rel-L2 {e0:.2e}, reuse rel-L2 {e1:.2e}")
    assert e0 < TOL and e1 < TOL
    assert torch.equal(_run(net, x, ehs, added), _plain(tiny, x))


def test_engine_refusals(engine_lib, tiny):
    cfg, sd, net, x, ehs, added, _ = tiny
    lib, h = engine_lib, net._h
    plain = _plain(tiny, x)
    for bad in ((-1, 2, 0), (8, 0, 0), (8, 9, 0), (8, 2, -1), (8, 2, 4)):
        assert lib.sd_unet_set_hypertile(h, bad[0], bad[1], bad[2], 0) == 1, bad
    assert net.hypertile_sites() == [] and torch.equal(_run(net, x, ehs, added), plain)
    info = (C.c_int32 * 8)()
    assert lib.sd_unet_hypertile_read(h, 0, info) == 1 and lib.sd_unet_hypertile_read(h, -1, info) == 1
    try:
        # token merging on, then HyperTile: refused, token merging stays what it was
        net.enable_tome(0.5)
        with pytest.raises(_lib.EngineError) as e:
            net.enable_hypertile(8)
        assert "error 4" in str(e.value) and net.hypertile is None
        net.disable_tome()
        assert torch.equal(_run(net, x, ehs, added), plain)
        # HyperTile on, then token merging
        net.enable_hypertile(8)
        with pytest.raises(_lib.EngineError) as e:
            net.enable_tome(0.5)
        assert "error 4" in str(e.value) and net.tome is None
        net.disable_tome()                               # (turning it off while HyperTile is on is no error)
        net.disable_hypertile()
        assert torch.equal(_run(net, x, ehs, added), plain)
        # graph replay
        net.enable_hypertile(8)
        net.use_graph(True)
        with pytest.raises(_lib.EngineError) as e:
            _run(net, x, ehs, added)
        assert "error 4" in str(e.value)
        net.use_graph(False)
        net.disable_hypertile()
        assert torch.equal(_run(net, x, ehs, added), plain)
        # forward_pag
        if added is None:
            net.set_pag_layers(["mid"])
            net.enable_hypertile(8)
            with pytest.raises(_lib.EngineError) as e:
                net.forward_pag(x[:1].cuda(), torch.tensor(501.0), ehs.cuda())
            assert "error 4" in str(e.value)
            net.disable_hypertile()
            net.set_pag_layers([])
            assert torch.equal(_run(net, x, ehs, added), plain)
    finally:
        net.use_graph(False)
        net.set_pag_layers([])
        net.disable_tome()
        net.disable_hypertile()


def test_forward_on_poisoned_scratch(engine_lib, tiny):
    """The gather buffers are new scratch: a forward after the workspace was filled with NaN (or fp16 +Inf) bytes is the
    forward before it, bit for bit, for a copied step and for a band step."""
    cfg, sd, net, x, ehs, added, _ = tiny
    net.enable_hypertile(8, 2, 0, 0)
    try:
        for step in (0, 3):
            net.hypertile_step(step)
            first = _run(net, x, ehs, added)
            assert torch.isfinite(first).all()
            for pattern in (0, 1):
                assert net._poison_workspace(pattern) > 0
                assert torch.equal(_run(net, x, ehs, added), first), (step, pattern)
    finally:
        net.disable_hypertile()
