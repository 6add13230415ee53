"""Token merging on the GPU: the match, merge and unmerge operators against tests/tome_oracle.py on the same fp16 inputs,
and the UNet with token merging on against the oracle's forward run with the engine's own maps.

Match bound.  node_max is held to tau / 2 of the float64 scores, tau = 2 (C + 8) 2^-24: exact fp16 products, fp32 sums
of C of them, two fp32 reciprocal norms, and Cauchy-Schwarz on sum |x y|.  A source is ambiguous when its reference
node_max lies within tau of the midpoint between the r-th and (r + 1)-th largest, or its two best destinations lie within
tau; everywhere else the engine's choice must be the oracle's exactly, and at most 2 % of a case's sources may be
ambiguous (asserted from the reference before the engine is consulted).

Merge bound, per element of a row with n members: 2^-11 |m| + (n + 1) 2^-24 mean |x_i| (one fp16 rounding of the mean, n
fp32 additions and a divide)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import tome_oracle  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipControlNetModel, HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-2


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tau(Cc):
    return 2.0 * (Cc + 8) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ match
def engine_match(lib, xdev, ldx, B, H, W, Cc, ratio, key=(3, 1, 2), sx=2, sy=2, use_rand=1):
    T = H * W
    Nd, Ns, r, Tm, dst, src = tome_oracle.plan(H, W, sx, sy, ratio, use_rand, *key)
    plan = torch.zeros(lib.sd_tome_plan_bytes(B, T), dtype=torch.uint8, device="cuda")
    mp = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    nmax = torch.full((B, max(Ns, 1)), float("nan"), dtype=torch.float32, device="cuda")
    nidx = torch.full((B, max(Ns, 1)), -1, dtype=torch.int32, device="cuda")
    rc = lib.sd_op_tome_match(xdev.data_ptr(), ldx, B, H, W, Cc, sx, sy, ratio, use_rand, key[0], key[1], key[2],
                              plan.data_ptr(), mp.data_ptr(), nmax.data_ptr(), nidx.data_ptr(), stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    return mp.cpu().long(), nmax.cpu()[:, :Ns], nidx.cpu().long()[:, :Ns], (Nd, Ns, r, Tm, dst, src), plan


def reference(x, geom):
    """Per image: scores, node_max, node_idx, merged, ambiguity masks (all from float64)."""
    Nd, Ns, r, Tm, dst, src = geom
    out = []
    for b in range(x.shape[0]):
        s = tome_oracle.scores(x[b], src, dst)
        mp, nmax, nidx, merged = tome_oracle.match_from_scores(s, r, src, dst, x.shape[1])
        t = tau(x.shape[2])
        amb_thr = torch.zeros(Ns, dtype=torch.bool)
        if r < Ns:
            v = torch.sort(nmax, descending=True).values
            amb_thr = (nmax - (v[r - 1] + v[r]) / 2).abs() <= t
        amb_dst = torch.zeros(Ns, dtype=torch.bool)
        if Nd > 1:
            top = s.topk(2, dim=1).values
            amb_dst = (top[:, 0] - top[:, 1]) <= t
        out.append(dict(s=s, map=mp, nmax=nmax, nidx=nidx, merged=merged, amb_thr=amb_thr, amb_dst=amb_dst))
    return out


def check_map_shape(mp, geom):
    """A surjection onto [0, T'): unmerged sources 0.. in source-rank order, then the destinations in rank order."""
    Nd, Ns, r, Tm, dst, src = geom
    U = Ns - r
    assert mp.min() >= 0 and mp.max() < Tm
    assert sorted(set(mp.tolist())) == list(range(Tm))
    assert mp[dst].tolist() == list(range(U, U + Nd))
    un = [int(mp[t]) for t in src if mp[t] < U]
    assert un == list(range(U))
    assert sum(1 for t in src if mp[t] >= U) == r


def check_match(x, got, geom, what):
    mp_all, nmax_all, nidx_all = got
    Nd, Ns, r, Tm, dst, src = geom
    U = Ns - r
    t = tau(x.shape[2])
    refs = reference(x, geom)
    for b, ref in enumerate(refs):          # the cap comes from the reference alone
        amb = int((ref["amb_thr"] | ref["amb_dst"]).sum())
        assert amb <= 0.02 * Ns, (what, b, amb)
    for b, ref in enumerate(refs):
        mp, nmax, nidx = mp_all[b], nmax_all[b].double(), nidx_all[b]
        err = (nmax - ref["nmax"]).abs().max().item()
        print(f"{what} image {b}: max |node_max - float64| {err:.2e} (tau / 2 = {t / 2:.2e}), "
              f"ambiguous {int((ref['amb_thr'] | ref['amb_dst']).sum())} of {Ns}")
        assert err <= t / 2, (what, b)
        check_map_shape(mp, geom)
        for i, tk in enumerate(src):
            merged = bool(mp[tk] >= U)
            j = int(mp[tk]) - U
            if not ref["amb_thr"][i]:
                assert merged == bool(ref["merged"][i]), (what, b, i)
            if not ref["amb_dst"][i]:
                assert int(nidx[i]) == int(ref["nidx"][i]), (what, b, i)
                if merged:
                    assert j == int(ref["nidx"][i]), (what, b, i)
            else:
                assert ref["s"][i, int(nidx[i])] >= ref["nmax"][i] - t, (what, b, i)
                if merged:
                    assert j == int(nidx[i])


MATCH_CASES = [(2, 16, 16, 64, 0.5), (1, 8, 8, 128, 0.5), (1, 6, 10, 64, 0.5), (1, 5, 7, 64, 0.25), (1, 16, 16, 64, 0.75),
               (1, 4, 4, 1280, 0.5), (1, 8, 8, 320, 0.5), (1, 8, 8, 640, 0.5)]     # (the last two: every staged width)


@pytest.mark.parametrize("B,H,W,Cc,ratio", MATCH_CASES)
@pytest.mark.parametrize("scale", [1.0, 64.0, 1.0 / 64])
def test_match_against_oracle(engine_lib, B, H, W, Cc, ratio, scale):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, H * W, Cc, generator=g) * scale).half()
    zero = None
    if B == 2:      # one image has a zero row (a source): its scores are all 0, an exact tie that goes to destination 0
        zero = tome_oracle.plan(H, W, 2, 2, ratio, 1, 3, 1, 2)[5][5]
        x[1, zero] = 0
    got = engine_match(engine_lib, x.cuda(), Cc, B, H, W, Cc, ratio)
    check_match(x, got[:3], got[3], f"match {B}x{H}x{W}x{Cc} r{ratio} x{scale:g}")
    if zero is not None:
        assert got[1][1][5].item() == 0.0 and got[2][1][5].item() == 0
    if ratio == 0.75:
        assert got[3][2] == got[3][1]                   # every source merges
    again = engine_match(engine_lib, x.cuda(), Cc, B, H, W, Cc, ratio)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and torch.equal(got[2], again[2])
    assert torch.equal(got[4], again[4])                # the whole plan, byte for byte


def test_match_reads_only_its_view(engine_lib):
    B, H, W, Cc, ld = 2, 8, 8, 64, 88
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H * W, Cc, generator=g).half()
    buf = torch.full((B * H * W + 64, ld), float("nan"), dtype=torch.float16)
    buf[:B * H * W, :Cc] = x.reshape(-1, Cc)
    got = engine_match(engine_lib, buf.cuda(), ld, B, H, W, Cc, 0.5)
    check_match(x, got[:3], got[3], "match strided")


def test_match_exact_ties(engine_lib):
    """Duplicated source rows whose equal node_max straddles the threshold, two identical destination rows, and sources
    identical to them: the lower-rank rules hold exactly."""
    H = W = 8
    Cc = 64
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, H * W, Cc, generator=g).half()
    Nd, Ns, _, _, dst, src = tome_oracle.plan(H, W, 2, 2, 0.5, 1, 3, 1, 2)
    x[0, dst[7]] = x[0, dst[2]]                          # two identical destinations
    for i in (1, 31):
        x[0, src[i]] = x[0, dst[2]]                      # sources that tie between them (score 1 with both)
    dup = [i for i in range(Ns) if i % 2 == 0][:22]
    for i in dup[1:]:
        x[0, src[i]] = x[0, src[dup[0]]]
    s = tome_oracle.scores(x[0], src, dst)
    nm = s.max(dim=1).values
    above = int((nm > nm[dup[0]]).sum())
    ratio = next((q for q in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7) if above < int(H * W * q) < above + len(dup)), None)
    assert ratio is not None
    mp, nmax, nidx, geom, _ = engine_match(engine_lib, x.cuda(), Cc, 1, H, W, Cc, ratio)
    r = geom[2]
    ref_map, ref_max, ref_idx, ref_merged = tome_oracle.match_from_scores(s, r, src, dst, H * W)
    assert 0 < int(ref_merged[dup].sum()) < len(dup)     # the tie really straddles the threshold
    assert int(nidx[0][1]) == 2 and int(nidx[0][31]) == 2
    assert len(set(nmax[0][dup].tolist())) == 1
    assert torch.equal(mp[0], ref_map)
    assert torch.equal(nidx[0][dup], ref_idx[dup])


def test_match_rejections(engine_lib):
    lib = engine_lib
    x = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    plan = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    args = lambda H, W, Cc, ratio, ld=64: (x.data_ptr(), ld, 1, H, W, Cc, 2, 2, ratio, 1, 0, 0, 0, plan.data_ptr(), None, None,
                                            None, stream())
    assert lib.sd_op_tome_match(*args(129, 128, 64, 0.5)) == 4          # T > 16384: before anything is read
    assert lib.sd_op_tome_match(*args(1, 9, 64, 0.5)) == 4              # no whole cell
    assert lib.sd_op_tome_match(*args(8, 8, 64, 0.9)) == 1
    assert lib.sd_op_tome_match(*args(8, 8, 48, 0.5)) == 1              # C % 32
    assert lib.sd_op_tome_match(*args(8, 8, 64, 0.5, ld=68)) == 1       # ldx % 8
    assert lib.sd_op_tome_match(*args(8, 8, 64, 0.0)) == 1              # nothing to merge
    assert lib.sd_op_tome_match(None, 64, 1, 8, 8, 64, 2, 2, 0.5, 1, 0, 0, 0, plan.data_ptr(), None, None, None, stream()) == 1


# ------------------------------------------------------------------------------------------------ merge / unmerge
def _maps(kind, B, T, g):
    Nd = T // 4
    Ns = T - Nd
    if kind == "perm":
        return torch.stack([torch.randperm(T, generator=g) for _ in range(B)]), T
    if kind == "all_in_one":                            # r = Ns, one destination holds every source
        mp = torch.empty(B, T, dtype=torch.long)
        for b in range(B):
            mp[b, :Ns] = 3
            mp[b, Ns:] = torch.arange(Nd)
        return mp, Nd
    if kind == "one":                                   # r = 1
        mp = torch.stack([torch.arange(T) for _ in range(B)])
        mp[:, T - 1] = 5
        return mp, T - 1
    Tm = T // 2                                         # random groups, every row used
    mp = torch.stack([torch.cat([torch.randperm(Tm, generator=g), torch.randint(0, Tm, (T - Tm,), generator=g)])
                      [torch.randperm(T, generator=g)] for _ in range(B)])
    return mp, Tm


MERGE_CASES = [("perm", 8, 0), ("all_in_one", 24, 0), ("one", 192, 0), ("rand", 960, 8), ("rand", 8, 8), ("rand", 7, 1),
               ("all_in_one", 7, 1), ("rand", 192, 0)]


@pytest.mark.parametrize("kind,cols,pad", MERGE_CASES)
def test_merge_unmerge(engine_lib, kind, cols, pad):
    lib = engine_lib
    B, T = 2, 64
    g = torch.Generator().manual_seed(cols * 7 + len(kind))
    mp, Tm = _maps(kind, B, T, g)
    plan = torch.zeros(lib.sd_tome_plan_bytes(B, T), dtype=torch.uint8, device="cuda")
    mp32 = mp.to(torch.int32).contiguous()
    rc = lib.sd_op_tome_plan_from_map(C.cast(mp32.data_ptr(), C.POINTER(C.c_int32)), B, T, Tm, plan.data_ptr(), stream())
    assert rc == 0, lib.sd_last_error()
    off = 1 if cols == 7 else 0                         # an unaligned base for the scalar path
    lds, ldd = cols + pad, cols + pad + (8 if pad else 0)
    SENT = 777.0
    cnt = torch.stack([torch.bincount(mp[b], minlength=Tm) for b in range(B)])
    for exact in (True, False):
        if exact:   # x_i = (members of its row) * small integer: every group mean is a small integer
            x = torch.randint(-8, 9, (B, T, cols), generator=g).double() * torch.gather(cnt, 1, mp)[..., None]
        else:
            x = torch.randn(B, T, cols, generator=g).double()
        x = x.half()
        src = torch.full((B * T * lds + 16,), float("nan"), dtype=torch.float16)
        src[off:off + B * T * lds].view(B * T, lds)[:, :cols] = x.reshape(-1, cols)
        dst = torch.full(((B * Tm + 4) * ldd + 16,), SENT, dtype=torch.float16)
        srcd, dstd = src.cuda(), dst.cuda()
        rc = lib.sd_op_tome_merge(srcd.data_ptr() + 2 * off, lds, cols, plan.data_ptr(), B, T, dstd.data_ptr() + 2 * (off + 2 * ldd),
                                  ldd, stream())
        assert rc == 0, lib.sd_last_error()
        out = dstd.cpu()
        body = out[off + 2 * ldd:off + 2 * ldd + B * Tm * ldd].view(B * Tm, ldd)
        got = body[:, :cols].reshape(B, Tm, cols)
        # guards: two rows in front, two behind, the pad columns
        assert (out[:off + 2 * ldd] == SENT).all() and (out[off + 2 * ldd + (B * Tm - 1) * ldd + cols:] == SENT).all()
        assert (body[:-1, cols:] == SENT).all()
        ref = torch.stack([tome_oracle.merge(x[b], mp[b], Tm) for b in range(B)])
        if exact:
            assert torch.equal(got, ref.half()), (kind, cols)
        else:
            mabs = torch.stack([tome_oracle.merge(x[b].abs(), mp[b], Tm) for b in range(B)])
            lim = 2.0 ** -11 * ref.abs() + (cnt[..., None].double() + 1) * 2.0 ** -24 * mabs
            err = (got.double() - ref).abs()
            print(f"merge {kind} cols {cols}: worst error / bound {(err / lim.clamp_min(1e-30)).max().item():.2f}")
            assert (err <= lim).all(), (kind, cols)
        if kind == "perm":                              # groups of one: a permutation, bit for bit
            for b in range(B):
                assert torch.equal(got[b][mp[b]], x[b])
        # unmerge of what merge wrote: a pure copy through the map, with its own guards
        back = torch.full(((B * T + 4) * lds + 16,), SENT, dtype=torch.float16).cuda()
        rc = lib.sd_op_tome_unmerge(dstd.data_ptr() + 2 * (off + 2 * ldd), ldd, cols, plan.data_ptr(), B, T,
                                    back.data_ptr() + 2 * (off + 2 * lds), lds, stream())
        assert rc == 0, lib.sd_last_error()
        bo = back.cpu()
        bb = bo[off + 2 * lds:off + 2 * lds + B * T * lds].view(B * T, lds)
        assert (bo[:off + 2 * lds] == SENT).all() and (bo[off + 2 * lds + (B * T - 1) * lds + cols:] == SENT).all()
        assert (bb[:-1, cols:] == SENT).all()
        want = torch.stack([got[b][mp[b]] for b in range(B)])
        assert torch.equal(bb[:, :cols].reshape(B, T, cols), want), (kind, cols)


def test_plan_from_map_rejects(engine_lib):
    lib = engine_lib
    plan = torch.zeros(lib.sd_tome_plan_bytes(1, 8), dtype=torch.uint8, device="cuda")
    bad = (C.c_int32 * 8)(0, 1, 2, 3, 3, 3, 3, 9)
    assert lib.sd_op_tome_plan_from_map(bad, 1, 8, 5, plan.data_ptr(), stream()) == 1      # an entry outside [0, T')
    gap = (C.c_int32 * 8)(0, 1, 2, 4, 4, 4, 4, 4)
    assert lib.sd_op_tome_plan_from_map(gap, 1, 8, 5, plan.data_ptr(), stream()) == 1      # row 3 without a member


# ---------------------------------------------------------------------------------------------------- UNet
def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


_NETS = {}


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


def _build(kind):
    cfg = config.tiny_unet() if kind == "sd15" else config.tiny_unet(linear=True, sdxl_cond=True)
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    added = None
    if kind == "sdxl":
        added = {"text_embeds": torch.randn(2, 64, generator=g).half(), "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)}
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd), x, ehs, added


def _run(net, x, ehs, added):
    return net(x.cuda(), torch.tensor(501.0), ehs.cuda(), added_cond_kwargs=added)[0].float().cpu()


def _oracle(cfg, sd, x, ehs, added, tome):
    w = {k: v.double() for k, v in sd.items()}
    a = None if added is None else {"text_embeds": added["text_embeds"].double(), "time_ids": added["time_ids"].double()}
    with torch.no_grad():
        return tome_oracle.unet_forward(cfg, w, x.double(), torch.tensor(501.0, dtype=torch.float64), ehs.double(), a, tome)


@pytest.mark.parametrize("max_ds", [1, 2])
def test_unet_with_tome_matches_oracle(engine_lib, tiny, max_ds):
    cfg, sd, net, x, ehs, added = tiny
    net.disable_tome()
    plain = _run(net, x, ehs, added)
    net.enable_tome(0.5, max_downsample=max_ds, seed=3).tome_step(2)
    try:
        got = _run(net, x, ehs, added)
        sites = net.tome_sites()
    finally:
        net.disable_tome()
    # the blocks the level rule selects, in execution order (tiny_unet: two blocks per down level, three per up level)
    want = {1: [0, 1, 13, 14, 15], 2: [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]}[max_ds]
    assert [s["site"] for s in sites] == want
    for s in sites:
        assert (s["H"], s["W"]) == ((16, 16) if s["site"] in (0, 1, 13, 14, 15) else (8, 8))
        T = s["H"] * s["W"]
        geom = tome_oracle.plan(s["H"], s["W"], 2, 2, 0.5, 1, 3, 2, s["site"])
        assert (s["r"], s["T_merged"]) == (geom[2], geom[3]) == (T // 2, T // 2)
        assert s["maps"].shape == (2, T)
        for b in range(2):
            check_map_shape(s["maps"][b].long(), geom[:4] + (geom[4], geom[5]))
    maps = {s["site"]: s["maps"] for s in sites}
    ref = _oracle(cfg, sd, x, ehs, added, tome_oracle.Tome(0.5, max_ds, seed=3, step=2, maps=maps, order="pre"))
    post = _oracle(cfg, sd, x, ehs, added, tome_oracle.Tome(0.5, max_ds, seed=3, step=2, maps=maps, order="post"))
    # the identity the design rests on: merging before or after the projections is the same function
    assert rel_l2(post.float(), ref.float()) < 1e-6 and (post - ref).abs().max().item() < 1e-9 * ref.abs().max().item() + 1e-12
    err, moved = rel_l2(got, ref), rel_l2(plain, ref)
    print(f"unet tome max_ds {max_ds}: rel-L2 vs oracle with the engine's maps {err:.2e}; plain forward vs that {moved:.2e}")
    assert err < TOL
    # off again: the never-enabled forward, bit for bit
    assert torch.equal(_run(net, x, ehs, added), plain)
    assert net.tome_sites() == []


def test_unet_tome_step_and_reproducibility(engine_lib, tiny):
    cfg, sd, net, x, ehs, added = tiny
    net.enable_tome(0.5, seed=3)
    try:
        a = _run(net.tome_step(0), x, ehs, added)
        ma = [s["maps"] for s in net.tome_sites()]
        b = _run(net.tome_step(1), x, ehs, added)
        mb = [s["maps"] for s in net.tome_sites()]
        a2 = _run(net.tome_step(0), x, ehs, added)
        ma2 = [s["maps"] for s in net.tome_sites()]
    finally:
        net.disable_tome()
    assert any(not torch.equal(p, q) for p, q in zip(ma, mb))
    assert all(torch.equal(p, q) for p, q in zip(ma, ma2))
    assert torch.equal(a, a2) and not torch.equal(a, b)


def test_unet_tome_profile_and_off_launches(engine_lib, tiny):
    """With token merging on the level-0 self-attention runs on T' rows (the profile's attention launches change and the
    four new kernels appear); ratio 0 after ratio 0.5 gives the never-enabled launch list."""
    cfg, sd, net, x, ehs, added = tiny
    lib = engine_lib

    def profile():
        lib.sd_prof_enable(1)
        try:
            _run(net, x, ehs, added)
            ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
            _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
        finally:
            lib.sd_prof_enable(0)
        return {ents[i].kernel.decode(): (int(ents[i].launches), float(ents[i].flops)) for i in range(n.value)}

    off = profile()
    net.enable_tome(0.5, seed=3)
    try:
        on = profile()
    finally:
        net.disable_tome()
    again = profile()
    assert {k: v[0] for k, v in again.items()} == {k: v[0] for k, v in off.items()}
    assert not any(k.startswith("tome_") for k in off)
    for k in ("tome_prep_kernel", "tome_match_kernel", "tome_select_kernel", "tome_merge_kernel", "tome_unmerge_kernel"):
        assert on[k][0] == 5, (k, on.get(k))
    attn_off = sum(v[1] for k, v in off.items() if k.startswith("attn_kernel"))
    attn_on = sum(v[1] for k, v in on.items() if k.startswith("attn_kernel"))
    print(f"attention FLOPs off {attn_off:.3e}, on {attn_on:.3e}")
    # the five level-0 self-attentions (B 2, T 256, heads x d = 64) run at T' = 128, every other launch as before
    full = 4.0 * 2 * 64 * 256 * 256
    assert attn_on == attn_off - 5 * full + 5 * 4.0 * 2 * 64 * 128 * 128
    assert sum(v[0] for k, v in on.items() if k.startswith("attn_kernel")) == \
        sum(v[0] for k, v in off.items() if k.startswith("attn_kernel"))


def test_unet_tome_cfg_share(engine_lib, tiny15):
    """forward_cfg (shared prefix: the first block matches on half the batch) against the plain forward on duplicated
    latents, with the comparison of tests/test_cfg_share_gpu.py: the shared prefix computes the same values once."""
    cfg, sd, net, x, ehs, added = tiny15
    lat = x[:1]
    net.enable_tome(0.5, seed=3).tome_step(4)
    try:
        two = net(torch.cat([lat, lat]).cuda(), torch.tensor(501.0), ehs.cuda())[0].float().cpu()
        one = net.forward_cfg(lat.cuda(), torch.tensor(501.0), ehs.cuda())
        one = (one[0] if isinstance(one, (tuple, list)) else one).float().cpu()
        sites = net.tome_sites()
    finally:
        net.disable_tome()
    assert sites[0]["maps"].shape[0] == 1 and sites[1]["maps"].shape[0] == 2
    e = rel_l2(one, two)
    print(f"forward_cfg vs forward on duplicated latents with token merging: rel-L2 {e:.2e}")
    assert e < 1e-3                                     # tests/test_cfg_share_gpu.py: SAME


def test_unet_tome_rejections(engine_lib, tiny):
    cfg, sd, net, x, ehs, added = tiny
    lib, h = engine_lib, net._h
    for bad in ((0.8, 1, 2, 2), (float("nan"), 1, 2, 2), (0.5, 3, 2, 2), (0.5, 1, 0, 2), (0.5, 1, 2, 9)):
        assert lib.sd_unet_set_tome(h, bad[0], bad[1], bad[2], bad[3], 1, 0) == 1, bad
    assert lib.sd_unet_set_tome(None, 0.5, 1, 2, 2, 1, 0) == 1
    net.enable_tome(0.5)
    try:
        net.use_graph(True)
        with pytest.raises(_lib.EngineError):
            _run(net, x, ehs, added)
        net.use_graph(False)
        if added is None:
            net.set_pag_layers(["mid"])
            with pytest.raises(_lib.EngineError):
                net.forward_pag(x[:1].cuda(), torch.tensor(501.0), ehs.cuda())
    finally:
        net.use_graph(False)
        net.set_pag_layers([])
        net.disable_tome()
    assert torch.isfinite(_run(net, x, ehs, added)).all()


def check_maps(x, maps, geom, what):
    """check_match's criteria for maps alone (what the UNet hands back): the cap from the reference first, then on the
    unambiguous sources the oracle's merged status and destination exactly, on the others a choice its scores allow."""
    Nd, Ns, r, Tm, dst, src = geom
    U = Ns - r
    t = tau(x.shape[2])
    refs = reference(x, geom)
    for b, ref in enumerate(refs):
        amb = int((ref["amb_thr"] | ref["amb_dst"]).sum())
        assert amb <= 0.02 * Ns, (what, b, amb)
    for b, ref in enumerate(refs):
        mp = maps[b].long()
        check_map_shape(mp, geom)
        for i, tk in enumerate(src):
            merged, j = bool(mp[tk] >= U), int(mp[tk]) - U
            if not ref["amb_thr"][i]:
                assert merged == bool(ref["merged"][i]), (what, b, i)
            if merged:
                if not ref["amb_dst"][i]:
                    assert j == int(ref["nidx"][i]), (what, b, i)
                else:
                    assert ref["s"][i, j] >= ref["nmax"][i] - t, (what, b, i)


def test_unet_maps_are_the_match_of_the_engines_own_block_inputs(engine_lib, tiny):
    """Every map read back against the oracle's scores of the very fp16 view the engine's match read (the debug tap
    "tome.<site>"): the right tensor, stride and image count reach the matcher, and the selection is the oracle's."""
    cfg, sd, net, x, ehs, added = tiny
    net.enable_tome(0.5, max_downsample=2, seed=3).tome_step(2)
    try:
        kw = {} if added is None else {"added_cond_kwargs": added}
        out, taps = net.forward_tapped(x.cuda(), torch.tensor(501.0), ehs.cuda(), **kw)
        sites = net.tome_sites()
        again = _run(net, x, ehs, added)
    finally:
        net.disable_tome()
    assert torch.equal(out.float().cpu(), again)        # taps change nothing
    assert [s["site"] for s in sites] == [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]
    for s in sites:
        xin = taps[f"tome.{s['site']}"]["in"]           # [B, C, H, W] fp16
        assert xin.shape[0] == 2 and xin.shape[2:] == (s["H"], s["W"])
        rows = xin.permute(0, 2, 3, 1).reshape(2, s["H"] * s["W"], xin.shape[1])
        geom = tome_oracle.plan(s["H"], s["W"], 2, 2, 0.5, 1, 3, 2, s["site"])
        check_maps(rows, s["maps"], geom, f"unet site {s['site']}")


def test_unet_tome_with_deepcache_store_and_reuse(engine_lib, tiny):
    """One store + reuse pair with token merging on against deepcache_oracle's forms composed with the token-merging
    oracle, each run with the engine's maps; a reuse step's blocks keep the ordinals of the full forward."""
    cfg, sd, net, x, ehs, added = tiny
    g = torch.Generator().manual_seed(77)
    x1 = torch.randn(2, 4, 16, 16, generator=g).half()
    net.enable_deepcache(2, 1)
    net.enable_tome(0.5, seed=3)
    try:
        net.deep_cache_mode(net.DC_STORE).tome_step(0)
        got0 = _run(net, x, ehs, added)
        s0 = net.tome_sites()
        net.deep_cache_mode(net.DC_REUSE).tome_step(1)
        got1 = _run(net, x1, ehs, added)
        s1 = net.tome_sites()
    finally:
        net.deep_cache_mode(net.DC_PLAIN)
        net.disable_tome()
        net.disable_deepcache()
    assert [s["site"] for s in s0] == [0, 1, 13, 14, 15] and [s["site"] for s in s1] == [0, 14, 15]
    w = {k: v.double() for k, v in sd.items()}
    a = None if added is None else {"text_embeds": added["text_embeds"].double(), "time_ids": added["time_ids"].double()}
    t = torch.tensor(501.0, dtype=torch.float64)
    with torch.no_grad():
        t0 = tome_oracle.Tome(0.5, 1, seed=3, step=0, maps={s["site"]: s["maps"] for s in s0})
        ref0, feat = tome_oracle.deepcache_forward(cfg, w, x.double(), t, ehs.double(), a, 1, t0)
        t1 = tome_oracle.Tome(0.5, 1, seed=3, step=1, maps={s["site"]: s["maps"] for s in s1})
        ref1, _ = tome_oracle.deepcache_forward(cfg, w, x1.double(), t, ehs.double(), a, 1, t1, cached=feat)
    for s in s1:                                        # the reuse step drew with step 1 at the full forward's ordinals
        geom = tome_oracle.plan(s["H"], s["W"], 2, 2, 0.5, 1, 3, 1, s["site"])
        for b in range(2):
            check_map_shape(s["maps"][b].long(), geom)
    e0, e1 = rel_l2(got0, ref0), rel_l2(got1, ref1)
    print(f"deepcache + tome: store rel-L2 {e0:.2e}, reuse rel-L2 {e1:.2e}")
    assert e0 < TOL and e1 < TOL


def test_unet_tome_refuses_what_no_test_composes(engine_lib, tiny15):
    """forward_concat, FreeU, an attached ControlNet and an attached IP-Adapter with token merging on: refused by the
    forward with nothing launched, never silently run."""
    cfg, sd, net, x, ehs, added = tiny15
    t = torch.tensor(501.0)
    net.enable_tome(0.5)
    try:
        net.enable_freeu(0.9, 0.2, 1.5, 1.6)
        with pytest.raises(_lib.EngineError, match="FreeU"):
            _run(net, x, ehs, None)
        net.disable_freeu()
        ccfg = controlnet.encoder_config(cfg)
        net.attach_controlnet(HipControlNetModel(net, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=4)))
        with pytest.raises(_lib.EngineError, match="ControlNet"):
            net(x.cuda(), t, ehs.cuda(), controlnet_cond=torch.zeros(1, 3, 128, 128).half().cuda(),
                controlnet_conditioning_scale=0.8)
        net.attach_controlnet(None)
        net.attach_ip_adapter(HipIPAdapter(net, 128, 4).load_state_dict(synth_ip_state_dict(cfg, 128, 4, seed=3)))
        with pytest.raises(_lib.EngineError, match="IP-Adapter"):
            net(x.cuda(), t, ehs.cuda(), added_cond_kwargs={"image_embeds": [torch.zeros(2, 1, 128).half().cuda()]})
    finally:
        net.disable_freeu()
        net.attach_controlnet(None)
        net.attach_ip_adapter(None)
        net.disable_tome()
    assert torch.isfinite(_run(net, x, ehs, None)).all()
    cfg8 = config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=8))
    sd8 = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg8), seed=5, perturb=0.1))
    net8 = HipUNet2DConditionModel(cfg8).load_state_dict(sd8)
    lat, img = x[:1].cuda(), torch.zeros(1, 4, 16, 16).half().cuda()
    ok = net8.forward_concat(lat, t, ehs.cuda(), img)
    net8.enable_tome(0.5)
    with pytest.raises(_lib.EngineError, match="forward_concat"):
        net8.forward_concat(lat, t, ehs.cuda(), img)
    net8.disable_tome()
    again = net8.forward_concat(lat, t, ehs.cuda(), img)
    assert torch.equal(ok[0] if isinstance(ok, (tuple, list)) else ok, again[0] if isinstance(again, (tuple, list)) else again)
