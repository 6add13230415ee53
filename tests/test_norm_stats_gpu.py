"""Norm statistics left by GEMM epilogues, at rows / groups whose mean is large next to their spread.

The transformer blocks fold their three LayerNorms into the next linear: the GEMM that produces the residual stream
leaves per-row statistics (igemm2 / igemm3 / wsgemm epilogues, or row_stats_kernel behind a split-K launch) and the
consumer (igemm2 / igemm3 / wsgemm / the persistent GEGLU kernel / ffn_fused_kernel) turns them into mean and rstd.
Computed as E[x^2] - mean^2 in fp32 those fall apart at rows like 50 +- 0.1.  The reference is fp32 torch fed the
engine's own stored fp16 y1, so each check isolates the statistics and the fold."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


LN_CASES = [
    # M, K, C, residual, site, forced producer (variant, splits), forced consumer
    (32768, 320, 320, False, "qkv", None, None),       # SD1.5 64 x 64 level: wsgemm producer (80-column parts) -> wsgemm LN
    (32768, 320, 320, True, "ff1", None, None),        # residual producer (streamed tile) -> wsgemm GEGLU with the LN
    (32768, 320, 320, True, "q2", (18, 1), (18, 1)),   # igemm3 on both sides
    (8192, 640, 640, True, "qkv", None, None),         # 32 x 32 level
    (8192, 640, 640, False, "ff1", None, None),        # GEGLU projection at C = 640
    (2048, 1280, 1280, True, "q2", None, None),        # 16 x 16 level
    (2048, 1280, 1280, True, "ff1", (1, 3), (1, 1)),   # split-K producer -> row_stats_kernel; igemm2's GEGLU epilogue
    (4096, 640, 640, True, "q2", (3, 1), (2, 1)),      # 64-column producer tiles (10 parts) -> 160-column consumer tiles
    (1000, 640, 640, True, "qkv", None, None),         # ragged M
    (2880, 1280, 1280, False, "q2", None, None),       # ragged M, SDXL width
    (8192, 1280, 1280, True, "ff1", None, None),       # SDXL 32 x 32 level
]
PROFILES = ["normal", "offset:50", "offset:-30", "spikes"]

_kinds = {}     # case -> (producer, consumer) kernel ids seen


def _operands(case, profile, g):
    M, K, Cc, with_res, site, _, _ = case
    x = torch.randn(M, K, generator=g).half()
    if profile == "normal" or profile == "spikes":
        w0 = (torch.randn(Cc, K, generator=g) / K ** 0.5).half()
        b0 = 0.2 * torch.randn(Cc, generator=g)
        res = torch.randn(M, Cc, generator=g).half() if with_res else None
        if profile == "spikes":          # a few channels of +-300 on N(0, 1) rows
            for i, c in enumerate((3, Cc // 3, Cc // 2 + 5, Cc - 2)):
                b0[c] = 300.0 if i % 2 == 0 else -300.0
    else:                                # rows v +- 0.1: the offset in the bias, or in the residual stream when there is one
        v = float(profile.split(":")[1])
        w0 = (0.07 * torch.randn(Cc, K, generator=g) / K ** 0.5).half()
        b0 = (0.0 if with_res else v) + 0.05 * torch.randn(Cc, generator=g)
        res = (v + 0.07 * torch.randn(M, Cc, generator=g)).half() if with_res else None
    return x, w0, b0, res


def _run_chain(engine_lib, case, profile):
    M, K, Cc, with_res, site, fp, fc = case
    g = torch.Generator().manual_seed(M + 7 * Cc + len(site) + PROFILES.index(profile))
    x, w0, b0, res = _operands(case, profile, g)
    geglu = site == "ff1"
    O = 4 * Cc if geglu else (3 * Cc if site == "qkv" else Cc)
    w1 = (torch.randn(2 * O if geglu else O, Cc, generator=g) / Cc ** 0.5).half()
    b1 = 0.2 * torch.randn(2 * O if geglu else O, generator=g)
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    rows_scaled, row_scale = (0, 1.0) if geglu else (Cc, (Cc // 8) ** -0.5)

    dev = dict(device="cuda")
    xd, w0d, b0d = x.cuda(), w0.cuda(), b0.cuda()
    rd = res.cuda() if res is not None else None
    w1d, b1d, gd, bd = w1.cuda(), b1.cuda(), gamma.cuda(), beta.cuda()
    nstat = M * ((Cc + 63) // 64) * 2

    def once():
        y1 = torch.empty(M, Cc, dtype=torch.float16, **dev)
        stat = torch.zeros(nstat, dtype=torch.float32, **dev)
        y2 = torch.empty(M, O, dtype=torch.float16, **dev)
        parts, part_w, prod, cons = C.c_int(-9), C.c_int(-9), C.c_int(-9), C.c_int(-9)
        try:
            if fp:
                engine_lib.sd_igemm_force(*fp)
            rc = engine_lib.sd_op_linear_rowstats(P(xd), P(w0d), P(b0d), P(rd), P(y1), P(stat), M, K, Cc, C.byref(parts),
                                                  C.byref(part_w), C.byref(prod), stream())
            assert rc == 0, engine_lib.sd_last_error()
            engine_lib.sd_igemm_force(*(fc if fc else (-1, 0)))
            rc = engine_lib.sd_op_ln_linear(P(y1), P(stat), parts.value, part_w.value, P(gd), P(bd), 1e-5, P(w1d), P(b1d),
                                            P(y2), M, Cc, O, int(geglu), rows_scaled, row_scale, C.byref(cons), stream())
            assert rc == 0, engine_lib.sd_last_error()
        finally:
            engine_lib.sd_igemm_force(-1, 0)
        torch.cuda.synchronize()
        return y1, stat, y2, (prod.value, cons.value, parts.value, part_w.value)

    y1, stat, y2, info = once()
    _kinds[case] = info[:2]
    print("LN chain", case, profile, "producer", info[0], "consumer", info[1], "parts", info[2], "x", info[3])

    with torch.no_grad():
        y1_ref = (xd.float() @ w0d.float().t() + b0d).half()
        if rd is not None:
            y1_ref = (y1_ref.float() + rd.float()).half()
        proj = F.linear(F.layer_norm(y1.float(), (Cc,), gd, bd, 1e-5), w1d.float(), b1d)
        if geglu:
            hid, gate = proj.chunk(2, dim=-1)
            ref = hid * F.gelu(gate)
        else:
            ref = proj
            ref[:, :rows_scaled] *= row_scale
    assert rel_l2(y1, y1_ref) < 2e-3
    assert torch.isfinite(y2.float()).all()
    err = rel_l2(y2, ref)
    print("  y2 rel-L2 %.3e" % err)
    assert err < 3e-3, err
    return y1, stat, y2, info, once


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("case", LN_CASES)
def test_folded_layernorm_chain(engine_lib, case, profile):
    """Producer epilogue statistics -> folded LayerNorm consumer, at the UNet's transformer sites; a second run on fresh
    buffers is bitwise identical (statistics merged in a fixed order)."""
    y1, stat, y2, info, once = _run_chain(engine_lib, case, profile)
    y1b, statb, y2b, infob = once()
    assert infob == info
    assert torch.equal(y1, y1b) and torch.equal(stat, statb) and torch.equal(y2, y2b)


def test_folded_layernorm_chain_covers_every_producer_and_consumer(engine_lib):
    """The cases above reach every producer (igemm2 tile epilogue, wsgemm, igemm3, row_stats_kernel) and every consumer
    (igemm2 plain and GEGLU epilogues, wsgemm plain / GEGLU, igemm3, the persistent GEGLU kernel) of the statistics."""
    for case in LN_CASES:
        if case not in _kinds:
            _run_chain(engine_lib, case, "normal")
    prods = {k[0] for k in _kinds.values()}
    cons_plain = {k[1] for c, k in _kinds.items() if c[4] != "ff1"}
    cons_geglu = {k[1] for c, k in _kinds.items() if c[4] == "ff1"}
    igemm2_tiles = set(range(13)) - {10}
    assert {-1, 13, 18} <= prods, prods
    assert prods & igemm2_tiles, prods
    assert {13, 18} <= cons_plain and cons_plain & igemm2_tiles, cons_plain
    assert {14, 100} <= cons_geglu and cons_geglu & igemm2_tiles, cons_geglu


@pytest.mark.parametrize("M,with_res,profile", [(8192, True, "offset:50"), (8192, False, "offset:50"),
                                                (32768, True, "offset:-30"), (8192, True, "normal")])
def test_ffn_fused_on_producer_statistics(engine_lib, M, with_res, profile):
    """ffn_fused_kernel (C = 320) fed the multi-part row statistics of a real producer, as in the UNet: igemm2's tile
    epilogue behind a residual (two 160-column parts), wsgemm without one (four 80-column parts).  W2 is scaled up so the
    feed-forward branch y - x, where an rstd error shows, stands well above y's fp16 step at |y| ~ offset."""
    Cc = 320
    case = (M, Cc, Cc, with_res, "ff1", None, None)
    g = torch.Generator().manual_seed(M + int(with_res) + PROFILES.index(profile))
    x0, w0, b0, res = _operands(case, profile, g)
    w1 = (torch.randn(8 * Cc, Cc, generator=g) / Cc ** 0.5).half()
    b1 = torch.randn(8 * Cc, generator=g) * 0.2
    w2 = (30.0 * torch.randn(Cc, 4 * Cc, generator=g) / (4 * Cc) ** 0.5).half()
    b2 = torch.randn(Cc, generator=g) * 0.2
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    xd, w0d, b0d = x0.cuda(), w0.cuda(), b0.cuda()
    rd = res.cuda() if res is not None else None
    w1d, w2d, b1d, b2d, gd, bd = w1.cuda(), w2.cuda(), b1.cuda(), b2.cuda(), gamma.cuda(), beta.cuda()
    x = torch.empty(M, Cc, dtype=torch.float16, device="cuda")
    stat = torch.zeros(M * ((Cc + 63) // 64) * 2, dtype=torch.float32, device="cuda")
    parts, part_w, prod = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    rc = engine_lib.sd_op_linear_rowstats(P(xd), P(w0d), P(b0d), P(rd), P(x), P(stat), M, Cc, Cc, C.byref(parts),
                                          C.byref(part_w), C.byref(prod), stream())
    assert rc == 0, engine_lib.sd_last_error()
    print("ffn on producer statistics", M, with_res, profile, "producer", prod.value, "parts", parts.value, "x", part_w.value)
    assert parts.value > 1 and prod.value != -1
    ys = []
    for _ in range(2):
        y = torch.zeros(M, Cc, dtype=torch.float16, device="cuda")
        fused = C.c_int(-1)
        rc = engine_lib.sd_op_ln_ffn_geglu(P(x), P(stat), parts.value, part_w.value, P(gd), P(bd), 1e-5, P(w1d), P(b1d),
                                           P(w2d), P(b2d), P(y), M, Cc, C.byref(fused), stream())
        assert rc == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        assert fused.value == 1
        ys.append(y)
    with torch.no_grad():
        xf = x.double()
        proj = F.linear(F.layer_norm(xf, (Cc,), gd.double(), bd.double(), 1e-5), w1d.double(), b1d.double())
        hid, gate = proj.chunk(2, dim=-1)
        branch = F.linear(hid * F.gelu(gate), w2d.double(), b2d.double())
    assert torch.isfinite(ys[0].float()).all()
    assert rel_l2(ys[0], xf + branch) < 3e-3
    err = rel_l2(ys[0].double() - xf, branch)
    print("  branch rel-L2 %.3e" % err)
    assert err < 3e-3, err
    assert torch.equal(ys[0], ys[1])
