"""MultiControlNet on the GPU: the scale fold bit for bit, the residual stage of n nets element by element in both forms
(chained per-net GEMMs, one K-concatenated GEMM on the folded weights), the UNet with a list of nets against the fp32
oracle composition (tests/mcn_oracle.py), the identities that tie a list to the single-net path, the fold cache, the
workspace and the rejections."""
import ctypes as C

import pytest
import torch

from cn_oracle import synth_cn_state_dict
from conftest import rel_l2
from mcn_oracle import unet_mcn_forward
from stablediffusion_amd import _lib, config, controlnet, weights
from stablediffusion_amd.models import HipControlNetModel, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu
TOL = 1e-2                  # tests/test_controlnet_gpu.py's
U16, U32 = 2.0 ** -11, 2.0 ** -23
ALL_SCALES = [1.0, 0.37, -0.5, 1e-4]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(autouse=True)
def _default_form(engine_lib):
    yield
    engine_lib.sd_cn_kcat_force(-1)


def f32(v):
    """The value the engine receives for a Python float scale."""
    return C.c_float(v).value


# ------------------------------------------------------------------------------------------------ 1. the fold
@pytest.mark.parametrize("C_", [64, 320])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fold_bit_for_bit(engine_lib, n, C_):
    g = torch.Generator().manual_seed(100 * n + C_)
    scales = (ALL_SCALES[n % 4:] + ALL_SCALES[:n % 4])[:n]
    ws = [(torch.randn(C_, C_, generator=g) / C_ ** 0.5).half().cuda() for _ in range(n)]
    bs = [(0.1 * torch.randn(C_, generator=g)).cuda() for _ in range(n)]
    G = 3
    wbuf = torch.full((C_ + 2 * G, n * C_), float("nan"), dtype=torch.float16, device="cuda")
    bbuf = torch.full((C_ + 16,), float("nan"), dtype=torch.float32, device="cuda")
    wp = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
    bp = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
    sp = (C.c_float * n)(*scales)
    rc = engine_lib.sd_op_cn_fold_scales(wp, bp, sp, n, C_, C.c_void_p(wbuf[G:].data_ptr()), C.c_void_p(bbuf[8:].data_ptr()),
                                         0, None, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    want = torch.cat([(w.float() * f32(s)).half() for w, s in zip(ws, scales)], dim=1)
    assert torch.equal(wbuf[G:G + C_], want)
    assert torch.isnan(wbuf[:G]).all() and torch.isnan(wbuf[G + C_:]).all()
    assert torch.isnan(bbuf[:8]).all() and torch.isnan(bbuf[8 + C_:]).all()
    terms = torch.stack([f32(s) * b.double().cpu() for s, b in zip(scales, bs)])
    err = (bbuf[8:8 + C_].double().cpu() - terms.sum(0)).abs()
    assert (err <= n * 2.0 ** -24 * terms.abs().sum(0)).all(), err.max().item()


# ------------------------------------------------------------------------------------ 2. the residual stage
OP_SCALES = [0.8, 0.6, 1.0, 0.37]
GR, GC = 2, 24              # guard rows above and below y, guard columns to its right


def _op_case(M, C_, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, n * C_, generator=g).half()
    ws = [(torch.randn(C_, C_, generator=g) / C_ ** 0.5).half() for _ in range(n)]
    bs = [0.1 * torch.randn(C_, generator=g) for _ in range(n)]
    y0 = torch.randn(M, C_, generator=g).half()
    return x, ws, bs, y0


def _run_op(lib, x, ws, bs, y0, scales, mode):
    M, C_, n = y0.shape[0], y0.shape[1], len(ws)
    xd = x.cuda()
    wd = [w.cuda() for w in ws]
    bd = [b.cuda() for b in bs]
    buf = torch.full((M + 2 * GR, C_ + GC), float("nan"), dtype=torch.float16, device="cuda")
    buf[GR:GR + M, :C_] = y0.cuda()
    q = _lib.SdCnMultiProblem()
    for j in range(n):
        q.x[j] = xd.data_ptr() + 2 * j * C_
        q.ldx[j] = n * C_
        q.w[j] = wd[j].data_ptr()
        q.bias[j] = bd[j].data_ptr()
    q.y, q.ldy, q.M, q.C = buf[GR:].data_ptr(), buf.stride(0), M, C_
    arr = (_lib.SdCnMultiProblem * 1)(q)
    rc = lib.sd_op_controlnet_residuals_multi(arr, 1, (C.c_float * n)(*scales), n, mode, 0, None, stream())
    assert rc == 0, lib.sd_last_error()
    torch.cuda.synchronize()
    got = buf[GR:GR + M, :C_].double().cpu()
    guards_ok = bool(torch.isnan(buf[:GR]).all() and torch.isnan(buf[GR + M:]).all() and torch.isnan(buf[GR:GR + M, C_:]).all())
    return got, guards_ok


@pytest.mark.parametrize("M,C_,n", [(33, 64, 2), (130, 128, 3), (128, 1280, 4), (1, 64, 2)])
def test_residual_op_element_by_element(engine_lib, M, C_, n):
    """The bounds are tests/conv_cases.py's for a GEMM with a residual epilogue, |err| <= u16 (|p| + |p + res|) +
    (K + 3) u32 A + 2^-25 with A the expression on absolute values, restated for these operands:
      (a) the folded form against float64 on the folded fp16 weights: K = n C, plus b_cat's own error
          n 2^-24 sum |s_i b_i| (the fold test's bound), since the reference sums the biases in float64;
      (b) against float64 of the unfolded formula: the same plus 2^-11 sum_i |s_i| sum_k |w| |x|, the fold's one rounding;
      (c) the chained form: n launches, each y_j = fp16(y_{j-1} + s_j (x_j W_j^T + b_j)) with K = C, whose scale is no
          power of two, so the two multiplications by s_j add a rounding each: (C + 5) u32 A_j.  An earlier launch's error
          passes through the later additions unchanged, so the bounds add; each launch rounds a value that is off by the
          errors so far, a second-order term covered by the factor 1 + 2^-10."""
    x, ws, bs, y0 = _op_case(M, C_, n, seed=M + C_ + n)
    scales = [f32(s) for s in OP_SCALES[:n]]
    xs = [x[:, j * C_:(j + 1) * C_].double() for j in range(n)]
    res = y0.double()
    sb_abs = sum(abs(s) * b.double().abs() for s, b in zip(scales, bs))[None, :]
    bcat = sum(s * b.double() for s, b in zip(scales, bs))[None, :]
    K = n * C_
    # (a)
    wf = [(w.float() * s).half().double() for w, s in zip(ws, scales)]
    p = sum(xi @ w.t() for xi, w in zip(xs, wf)) + bcat
    A = sum(xi.abs() @ w.abs().t() for xi, w in zip(xs, wf)) + sb_abs
    bound_a = U16 * (p.abs() + (p + res).abs()) + (K + 3) * U32 * A + 2.0 ** -25 + n * 2.0 ** -24 * sb_abs
    # (b)
    terms = [s * (xi @ w.double().t() + b.double()[None, :]) for s, xi, w, b in zip(scales, xs, ws, bs)]
    prod_abs = [abs(s) * (xi.abs() @ w.double().abs().t()) for s, xi, w in zip(scales, xs, ws)]
    pu = sum(terms)
    Au = sum(prod_abs) + sb_abs
    bound_b = U16 * (pu.abs() + (pu + res).abs()) + (K + 3) * U32 * Au + 2.0 ** -25 + n * 2.0 ** -24 * sb_abs + U16 * sum(prod_abs)
    # (c)
    bound_c = torch.zeros_like(pu)
    run = res.clone()
    for j in range(n):
        Aj = prod_abs[j] + abs(scales[j]) * bs[j].double().abs()[None, :]
        nxt = run + terms[j]
        bound_c += U16 * (terms[j].abs() + nxt.abs()) + (C_ + 5) * U32 * Aj + 2.0 ** -25
        run = nxt
    bound_c *= 1 + 2.0 ** -10

    got1, ok1 = _run_op(engine_lib, x, ws, bs, y0, scales, 1)
    got0, ok0 = _run_op(engine_lib, x, ws, bs, y0, scales, 0)
    ea, eb, ec = (got1 - (p + res)).abs(), (got1 - (pu + res)).abs(), (got0 - (pu + res)).abs()
    print(f"max err / bound: folded vs folded ref {(ea / bound_a).max():.3f}, folded vs unfolded {(eb / bound_b).max():.3f}, "
          f"chained {(ec / bound_c).max():.3f}")
    assert ok1 and ok0
    assert (ea <= bound_a).all()
    assert (eb <= bound_b).all()
    assert (ec <= bound_c).all()


# --------------------------------------------------------------------------------------- UNet + list of nets
def _f16(sd):
    return {k: v.half().float() for k, v in sd.items()}


def _inputs(cfg, B, H, W, n_ctrls, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half()
    imgs = [torch.rand(n, 3, 8 * H, 8 * W, generator=g).half() for n in n_ctrls]
    return x, ehs, imgs


def _sdxl_kwargs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    tdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    return {"text_embeds": torch.randn(B, tdim, generator=g).half(),
            "time_ids": torch.tensor([[64.0, 64.0, 0.0, 0.0, 64.0, 64.0]] * B)}


def _build(ucfg, seed, n_nets):
    usd = _f16(weights.synth_state_dict(weights.unet_manifest(ucfg), seed=seed, perturb=0.1))
    ccfg = controlnet.encoder_config(ucfg)
    csds = [synth_cn_state_dict(ccfg, seed=seed + 1 + i) for i in range(n_nets)]
    net = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    cns = [HipControlNetModel(net, ccfg).load_state_dict(csd) for csd in csds]
    return usd, ccfg, csds, net, cns


@pytest.mark.parametrize("variant", ["plain", "linear", "sdxl"])
@pytest.mark.parametrize("B,H,W,n_ctrls", [(2, 16, 16, (1, 2)), (3, 24, 16, (3, 1, 1)), (1, 8, 24, (1, 1))])
def test_unet_with_controlnets_matches_oracle(engine_lib, variant, B, H, W, n_ctrls):
    N = len(n_ctrls)
    scales = [0.8, 0.6, 1.0][:N]
    ucfg = config.tiny_unet(linear=variant == "linear", sdxl_cond=variant == "sdxl")
    usd, ccfg, csds, net, cns = _build(ucfg, seed=31, n_nets=N)
    x, ehs, imgs = _inputs(ucfg, B, H, W, n_ctrls, B * 100 + H + N)
    add = _sdxl_kwargs(ucfg, B, 3) if variant == "sdxl" else None
    add_dev = {k: v.cuda() for k, v in add.items()} if add else None
    add_ref = {k: v.float() for k, v in add.items()} if add else None
    nets = [(ccfg, csd) for csd in csds]
    t = torch.tensor(500.0)
    with torch.no_grad():
        ref = unet_mcn_forward(ucfg, usd, nets, x, t, ehs, imgs, scales, add_ref)
        first = unet_mcn_forward(ucfg, usd, nets[:1], x, t, ehs, imgs[:1], scales[:1], add_ref)
    assert rel_l2(first, ref) > 5 * TOL                       # (of the reference alone) the further nets matter
    net.attach_controlnets(cns)
    for form in (1, 0):
        engine_lib.sd_cn_kcat_force(form)
        a = net(x.cuda(), t, ehs.cuda(), added_cond_kwargs=add_dev, controlnet_cond=[i.cuda() for i in imgs],
                controlnet_conditioning_scale=scales)[0]
        err = rel_l2(a, ref)
        print(f"form {form}: rel_l2 {err:.3e}")
        assert err < TOL, form


@pytest.fixture(scope="module")
def tiny():
    ucfg = config.tiny_unet()
    usd, ccfg, csds, net, cns = _build(ucfg, seed=21, n_nets=3)
    x, ehs, imgs = _inputs(ucfg, 2, 16, 16, (1, 2, 1), 8)
    return dict(ucfg=ucfg, usd=usd, ccfg=ccfg, csds=csds, net=net, cns=cns, x=x.cuda(), ehs=ehs.cuda(),
                imgs=[i.cuda() for i in imgs])


def _fresh(tn):
    return HipUNet2DConditionModel(tn["ucfg"]).load_state_dict(tn["usd"])


def _fwd(net, tn, imgs, scales):
    return net(tn["x"], 401.0, tn["ehs"], controlnet_cond=imgs, controlnet_conditioning_scale=scales)[0]


# ----------------------------------------------------------------------------------------------- 4. identities
def test_identities(engine_lib, tiny):
    net, cns, imgs = tiny["net"], tiny["cns"], tiny["imgs"]
    never = _fresh(tiny)(tiny["x"], 401.0, tiny["ehs"])[0]
    try:
        alone = []
        for k in (0, 1):
            net.attach_controlnet(cns[k])
            alone.append(_fwd(net, tiny, imgs[k], 0.7))
        net.attach_controlnets([cns[0]])
        assert torch.equal(_fwd(net, tiny, [imgs[0]], [0.7]), alone[0])
        assert torch.equal(_fwd(net, tiny, [imgs[0]], 0.7), alone[0])            # a float scale broadcasts
        net.attach_controlnets(cns[:2])
        assert torch.equal(_fwd(net, tiny, [imgs[0], None], [0.7, 0.0]), alone[0])  # (a null pointer at the C level)
        assert torch.equal(_fwd(net, tiny, [None, imgs[1]], [0.0, 0.7]), alone[1])
        assert torch.equal(_fwd(net, tiny, [None, None], [0.0, 0.0]), never)
        assert torch.equal(_fwd(net, tiny, imgs[:2], 0.0), never)
        both = _fwd(net, tiny, imgs[:2], [0.7, 0.7])
        assert not torch.equal(both, alone[0]) and not torch.equal(both, alone[1])
        net.attach_controlnet(cns[1])                                            # after a list: exactly that one net
        assert net.controlnets == [cns[1]]
        assert torch.equal(_fwd(net, tiny, imgs[1], 0.7), alone[1])
        net.attach_controlnets(cns[:2])
        net.attach_controlnets([])
        assert net.controlnet is None
        assert torch.equal(net(tiny["x"], 401.0, tiny["ehs"])[0], never)
    finally:
        net.attach_controlnets([])


# ----------------------------------------------------------------------------------------------- 5. fold cache
def test_fold_cache(engine_lib, tiny):
    cns, imgs = tiny["cns"], tiny["imgs"]
    engine_lib.sd_cn_kcat_force(1)
    net = _fresh(tiny).attach_controlnets(cns)
    try:
        assert net.cn_fold_count() == 0
        a = _fwd(net, tiny, imgs, [0.8, 0.6, 1.0])
        b = _fwd(net, tiny, imgs, [0.8, 0.6, 1.0])
        assert net.cn_fold_count() == 1 and torch.equal(a, b)
        c = _fwd(net, tiny, imgs, [0.8, 0.5, 1.0])                 # one scale changed
        assert net.cn_fold_count() == 2 and not torch.equal(c, a)
        d = _fwd(net, tiny, imgs, [0.8, 0.0, 1.0])                 # a net switched off
        assert net.cn_fold_count() == 3
        e = _fwd(net, tiny, imgs, [0.8, 0.0, 0.0])                 # one running net: the single-net path, no fold
        assert net.cn_fold_count() == 3
        for scales, got in (([0.8, 0.5, 1.0], c), ([0.8, 0.0, 1.0], d), ([0.8, 0.0, 0.0], e)):
            new = _fresh(tiny).attach_controlnets(cns)
            assert torch.equal(_fwd(new, tiny, imgs, scales), got), scales
            new.attach_controlnets([])
    finally:
        net.attach_controlnets([])


def test_caches_per_net(engine_lib, tiny):
    """tests/test_controlnet_gpu.py's test_cache_reuse_and_invalidation, on net 1 of two."""
    net, cns = tiny["net"], tiny["cns"][:2]
    im0, im1 = tiny["imgs"][0].clone(), tiny["imgs"][1].clone()
    new1 = torch.rand_like(im1.float()).half()
    sc = [0.8, 0.6]
    net.attach_controlnets(cns)
    try:
        ref = _fwd(net, tiny, [im0, im1], sc)
        ref2 = _fwd(net, tiny, [im0, new1], sc)
        net.text_kv_cache(True)
        a = _fwd(net, tiny, [im0, im1], sc)
        b = _fwd(net, tiny, [im0, im1], sc)
        im1.copy_(new1)                         # same pointer, new contents: stale until the cache is toggled
        stale = _fwd(net, tiny, [im0, im1], sc)
        net.text_kv_cache(True)
        fresh = _fwd(net, tiny, [im0, im1], sc)
        other = torch.rand_like(im1.float()).half()
        c = _fwd(net, tiny, [im0, other], sc)   # a new pointer: recomputed
        net.text_kv_cache(False)
        c_ref = _fwd(net, tiny, [im0, other], sc)
    finally:
        net.text_kv_cache(False)
        net.attach_controlnets([])
    assert torch.equal(a, ref) and torch.equal(b, ref)
    assert torch.equal(stale, ref) and torch.equal(fresh, ref2) and not torch.equal(ref, ref2)
    assert torch.equal(c, c_ref)


# ------------------------------------------------------------------------------------------------ 6. workspace
@pytest.mark.parametrize("form", [1, 0])
def test_poisoned_workspace(engine_lib, tiny, form):
    net, cns, imgs = tiny["net"], tiny["cns"][:2], tiny["imgs"][:2]
    engine_lib.sd_cn_kcat_force(form)
    net.attach_controlnets(cns)
    try:
        ref = _fwd(net, tiny, imgs, [0.8, 0.6])
        for pattern in (0, 1):
            assert net._poison_workspace(pattern) > 0
            assert torch.equal(_fwd(net, tiny, imgs, [0.8, 0.6]), ref), pattern
    finally:
        net.attach_controlnets([])


# ----------------------------------------------------------------------------------------------- 7. rejections
def _raw(lib, tn, net, imgs, counts, scales, n_nets, entry="mcn"):
    """One raw forward call; returns (rc, whether the output buffer was left alone)."""
    x, ehs = tn["x"], tn["ehs"]
    B, _, H, W = x.shape
    t = torch.full((B,), 401.0, device="cuda")
    out = torch.full((B, 4, H, W), 7.0, dtype=torch.float16, device="cuda")
    head = (net._h, C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(ehs.data_ptr()), ehs.shape[1], None, None,
            None, 0)
    tail = (C.c_void_p(out.data_ptr()), B, H, W, stream())
    if entry == "mcn":
        n = len(imgs)
        rc = lib.sd_unet_forward_mcn(*head, (C.c_void_p * n)(*[i.data_ptr() if i is not None else None for i in imgs]),
                                     (C.c_int * n)(*counts), (C.c_float * n)(*scales), n_nets, *tail)
    else:
        rc = lib.sd_unet_forward_cn(*head, C.c_void_p(imgs[0].data_ptr()), counts[0], scales[0], *tail)
    torch.cuda.synchronize()
    return rc, bool((out == 7.0).all())


def test_rejections(engine_lib, tiny):
    net, cns, imgs = tiny["net"], tiny["cns"], tiny["imgs"]
    ccfg = tiny["ccfg"]
    h = lambda ns: (C.c_void_p * len(ns))(*[n._h for n in ns])
    extra = [HipControlNetModel(net, ccfg).load_state_dict(tiny["csds"][0]) for _ in range(2)]
    ocfg = config.tiny_unet(sdxl_cond=True)
    other = HipUNet2DConditionModel(ocfg)
    foreign = HipControlNetModel(other, controlnet.encoder_config(ocfg)).load_state_dict(
        synth_cn_state_dict(controlnet.encoder_config(ocfg), seed=2))
    try:
        net.attach_controlnets(cns[:2])
        assert engine_lib.sd_unet_set_controlnets(net._h, h(cns + extra), 5) == 1           # five nets
        assert engine_lib.sd_unet_set_controlnets(net._h, h([cns[0], foreign]), 2) == 1     # created for another UNet
        assert engine_lib.sd_unet_set_controlnets(net._h, h([cns[0], cns[0]]), 2) == 1      # the same net twice
        with pytest.raises(ValueError):
            net.attach_controlnets(cns + extra)
        assert net.controlnets == cns[:2]                                                   # nothing changed
        ok = _raw(engine_lib, tiny, net, imgs[:2], (1, 2), (0.8, 0.6), 2)
        assert ok[0] == 0 and not ok[1]
        bad = [_raw(engine_lib, tiny, net, imgs[:2], (1, 2), (0.8, 0.6), 1),                # n_nets != attached
               _raw(engine_lib, tiny, net, imgs[:3], (1, 2, 1), (0.8, 0.6, 1.0), 3),
               _raw(engine_lib, tiny, net, [imgs[0], None], (1, 2), (0.8, 0.6), 2),         # a null image, net running
               _raw(engine_lib, tiny, net, [imgs[0], imgs[0]], (1, 3), (0.8, 0.6), 2),      # n_ctrl does not divide B
               _raw(engine_lib, tiny, net, imgs[:1], (1,), (0.8,), 1, entry="cn")]          # forward_cn with two nets
        assert bad == [(1, True)] * 5, bad
        net.use_graph(True)
        assert _raw(engine_lib, tiny, net, imgs[:2], (1, 2), (0.8, 0.6), 2) == (4, True)
        assert _raw(engine_lib, tiny, net, [None, None], (0, 0), (0.0, 0.0), 2) == (4, True)  # attached is enough
        net.use_graph(False)
        with pytest.raises(ValueError):
            _fwd(net, tiny, imgs[:3], [0.8, 0.6, 1.0])                                      # three images, two nets
        with pytest.raises(ValueError):
            _fwd(net, tiny, imgs[:2], [0.8])
        with pytest.raises(ValueError):
            _fwd(net, tiny, imgs[0], 0.8)                                                   # a list is attached
        net.attach_controlnet(cns[0])
        with pytest.raises(NotImplementedError):                                            # a single net: lists refused
            _fwd(net, tiny, [imgs[0]], [0.8])
    finally:
        net.use_graph(False)
        net.attach_controlnets([])


# -------------------------------------------------------------------------------------------------- 8. pipeline
@pytest.fixture(scope="module")
def loop_case():
    """The model, the inputs and the oracle loop of the pipeline test, computed once for both step paths."""
    from oracle import pipeline_ref
    from stablediffusion_amd.models import HipAutoencoderKL
    from stablediffusion_amd.pipeline import SDModelWrapper
    from stablediffusion_amd.schedulers import DDIMScheduler
    from test_controlnet import _to_original
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16(weights.synth_state_dict(weights.unet_manifest(ucfg), seed=11, perturb=0.1))
    vsd = _f16(weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1))
    ccfg = controlnet.encoder_config(ucfg)
    csds = [synth_cn_state_dict(ccfg, seed=6), synth_cn_state_dict(ccfg, seed=7)]
    model = SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                           vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler("DDIM")
    model.load_controlnets([_to_original(csds[0], ccfg, "control_model."), csds[1]])      # an original file and a dict
    g = torch.Generator().manual_seed(4)
    B = 2
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    ctrls = [torch.rand(1, 3, 128, 128, generator=g), torch.rand(1, 3, 128, 128, generator=g)]
    scales, starts, ends = [0.9, 0.7], [0.0, 0.25], [0.5, 1.0]
    rows = controlnet.keep_schedule(10, scales, starts, ends)
    assert [[s != 0 for s in r] for r in rows] == [[True, False]] * 3 + [[True, True]] * 2 + [[False, True]] * 5
    step = [0]

    def mcn_unet(cfg, w, x, t, ehs, added):
        row = rows[step[0]]
        step[0] += 1
        return unet_mcn_forward(cfg, w, [(ccfg, c) for c in csds], x, t, ehs, [c.half() for c in ctrls], row, added)

    ref_ctx = torch.cat([neg, pos]).float()
    plain = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), ref_ctx, steps=10, guidance_scale=5.0, scheduler="DDIM")
    saved = pipeline_ref.unet_forward
    pipeline_ref.unet_forward = mcn_unet
    try:
        ref = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), ref_ctx, steps=10, guidance_scale=5.0, scheduler="DDIM")
    finally:
        pipeline_ref.unet_forward = saved
    assert step[0] == 10
    assert rel_l2(plain, ref) > 5 * TOL
    yield dict(model=model, pos=pos, neg=neg, lat0=lat0, ctrls=ctrls, ref=ref, windows=(scales, starts, ends))
    model.unload_controlnet()


@pytest.mark.parametrize("path", ["device_step", "host_step"])
def test_tiny_txt2img_with_two_control_images_matches_oracle_loop(engine_lib, monkeypatch, loop_case, path):
    """tests/test_controlnet_gpu.py's 10-step DDIM loop with two nets whose guidance windows leave steps with the first
    net alone, both, and the second alone."""
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    lc = loop_case
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    assert pipe._fused_step_available(lc["model"], lc["lat0"].cuda())
    if path == "host_step":
        monkeypatch.setattr(pipe, "_device_step_kind", lambda *a, **k: None)
    scales, starts, ends = lc["windows"]
    folds = lc["model"].base.cn_fold_count()
    got = pipe(lc["model"], prompt_embeds=lc["pos"].cuda(), negative_prompt_embeds=lc["neg"].cuda(), latents=lc["lat0"].cuda(),
               num_inference_steps=10, guidance_scale=5.0, height=128, width=128, control_image=lc["ctrls"],
               controlnet_conditioning_scale=scales, control_guidance_start=starts, control_guidance_end=ends)
    assert torch.isfinite(got.float()).all()
    err = rel_l2(got, lc["ref"])
    print(f"{path}: rel_l2 {err:.3e}")
    assert err < TOL
    assert lc["model"].base.cn_fold_count() - folds <= 1       # both nets run with one pair of scales: at most one fold
