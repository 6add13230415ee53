"""The UNet with an AnimateDiff motion adapter attached, against tests/motion_oracle.py: every module alone on the engine's
own block input (debug taps), the whole forward, forward_cfg shared and unshared, a zero proj_out, detaching, the
refusals and poisoned scratch.

Tiny UNet (config.tiny_unet) with the tiny adapter: heads (2, 4, 8, 8), max_seq_length 32, a mid module, random weights
with a non-zero proj_out.  V = 2 videos of F in {3, 16} frames of 16 x 16 latents whose frames differ in level and spread:
GroupNorm statistics taken per frame instead of per video, or a resnet normalising with the summaries of the tensor in
front of the module, move the output far beyond the tolerances."""
import ctypes as C

import pytest
import torch

import motion_oracle
from conftest import rel_l2
from stablediffusion_amd import _lib, config, controlnet, motion, weights
from stablediffusion_amd.models import HipMotionAdapter, HipUNet2DConditionModel

pytestmark = pytest.mark.gpu

V = 2
L_TXT = 77
UNET_TOL = 1e-2         # the project's bound for a UNet forward (rel-L2 of the last tensor of ~800 launches)
# One module alone, on what it ADDS to its input (out - x): twelve tensors stored in fp16 between its launches (2^-11
# each, about 2^-12.8 rms) and two attention launches (2^-9 A per element, tests/tattn_cases.py) add in quadrature to
# about 2e-3 of the contribution; 5e-3 leaves a factor of two to three.
MODULE_TOL = 5e-3


@pytest.fixture(scope="module")
def tiny():
    ucfg = config.tiny_unet()
    usd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(ucfg), 1, perturb=0.1).items()}
    mcfg = motion.tiny_motion_adapter(ucfg)
    msd = motion.synth_state_dict(mcfg, seed=5)
    net = HipUNet2DConditionModel(ucfg, "cuda").load_state_dict(usd)
    ad = HipMotionAdapter(net, mcfg).load_state_dict(msd)
    net.attach_motion_adapter(ad)
    return ucfg, usd, mcfg, msd, net, ad


_INPUTS = {}


def inputs(F):
    """x [V F, 4, 16, 16] with per-frame level and spread, ehs [V F, L, D] repeated per frame, and the oracle's output and
    module inputs, computed once per frame count."""
    if F not in _INPUTS:
        g = torch.Generator().manual_seed(100 + F)
        ucfg = config.tiny_unet()
        level = torch.linspace(-1.5, 1.5, V * F)[torch.randperm(V * F, generator=g)]
        spread = 0.3 + 1.4 * torch.rand(V * F, generator=g)
        x = (torch.randn(V * F, 4, 16, 16, generator=g) * spread[:, None, None, None] + level[:, None, None, None]).half()
        ehs = torch.randn(V, 1, L_TXT, ucfg.cross_attention_dim, generator=g).expand(V, F, -1, -1).reshape(V * F, L_TXT, -1).half()
        _INPUTS[F] = (x, ehs.contiguous())
    return _INPUTS[F]


_ORACLE = {}


def oracle(tiny, F):
    if F not in _ORACLE:
        ucfg, usd, mcfg, msd = tiny[:4]
        x, ehs = inputs(F)
        taps = {}
        with torch.no_grad():
            y = motion_oracle.forward(ucfg, usd, mcfg, msd, x.float(), torch.tensor(501.0), ehs.float(), F, taps)
        _ORACLE[F] = (y, taps)
    return _ORACLE[F]


def run(net, x, ehs, F):
    return net(x.cuda(), torch.tensor(501.0), ehs.cuda(), num_frames=F)[0].float().cpu()


def plain(net, x, ehs):
    return net(x.cuda(), torch.tensor(501.0), ehs.cuda())[0].float().cpu()


def _launches(lib, fn):
    lib.sd_prof_enable(1)
    try:
        out = fn()
        ents, n = (_lib.SdProfEntry * 512)(), C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return out, {ents[i].kernel.decode(): int(ents[i].launches) for i in range(n.value)}


@pytest.mark.parametrize("F", (3, 16))
def test_whole_forward_matches_oracle(engine_lib, tiny, F):
    net = tiny[4]
    x, ehs = inputs(F)
    y_ref, _ = oracle(tiny, F)
    y = run(net, x, ehs, F)
    assert torch.isfinite(y).all()
    e = rel_l2(y, y_ref)
    moved = rel_l2(plain(net, x, ehs), y_ref)
    print("F = %d: rel-L2 %.2e against the oracle (tolerance %.0e); the plain forward is %.2e away" % (F, e, UNET_TOL, moved))
    assert moved > 10 * UNET_TOL          # the modules matter at these weights
    assert e <= UNET_TOL


@pytest.mark.parametrize("F", (3, 16))
def test_every_module_alone(engine_lib, tiny, F):
    """Each of the 21 modules through the taps: the oracle's module on the ENGINE's input of that module."""
    ucfg, usd, mcfg, msd, net, _ = tiny
    x, ehs = inputs(F)
    _, taps = net.forward_tapped(x.cuda(), torch.tensor(501.0), ehs.cuda(), num_frames=F)
    mods = motion.module_prefixes(mcfg)
    assert len(mods) == 21
    worst = 0.0
    for p, c, heads in mods:
        rec = taps[p]
        xin = rec["in"].float()
        with torch.no_grad():
            ref = motion_oracle.motion_module(xin, msd, p, heads, F)
        got = rec["out"].float()
        e = rel_l2(got - xin, ref - xin)
        whole = rel_l2(got, ref)
        worst = max(worst, e)
        print("%s (C %d, %d heads): rel-L2 of the contribution %.2e, of the output %.2e" % (p, c, heads, e, whole))
        assert e <= MODULE_TOL, p
    print("F = %d: worst module %.2e (tolerance %.0e)" % (F, worst, MODULE_TOL))


@pytest.mark.parametrize("F", (3, 16))
@pytest.mark.parametrize("share", (True, False))
def test_forward_cfg(engine_lib, tiny, share, F):
    """CFG on 2V videos from V F latents: the shared prefix ends before the first module."""
    ucfg, usd, mcfg, msd, net, _ = tiny
    x, ehs = inputs(F)
    g = torch.Generator().manual_seed(7)
    neg = torch.randn(V, 1, L_TXT, ucfg.cross_attention_dim, generator=g).expand(V, F, -1, -1).reshape(V * F, L_TXT, -1).half()
    ehs2 = torch.cat([neg, ehs])
    t = torch.full((V * F,), 501.0)
    y = net.forward_cfg(x.cuda(), t, ehs2.cuda(), in_scale=0.75, share=share, num_frames=F)[0].float().cpu()
    xs = (x.float() * 0.75).half().float()
    with torch.no_grad():
        ref = motion_oracle.forward(ucfg, usd, mcfg, msd, torch.cat([xs, xs]), torch.tensor(501.0), ehs2.float(), F)
    e = rel_l2(y, ref)
    print("forward_cfg share=%s, F = %d: rel-L2 %.2e (tolerance %.0e)" % (share, F, e, UNET_TOL))
    assert e <= UNET_TOL
    two_step = run(net, torch.cat([xs, xs]).half(), ehs2, F)
    if not share:
        assert torch.equal(y, two_step)
    else:
        assert rel_l2(y, two_step) <= 2e-3


def test_zero_proj_out_and_detach(engine_lib, tiny):
    """An adapter whose proj_out is all zero adds exactly nothing; detaching restores the plain launches."""
    ucfg, usd, mcfg, msd, net, ad = tiny
    F = 3
    x, ehs = inputs(F)
    try:
        net.attach_motion_adapter(None)
        base, l_plain = _launches(engine_lib, lambda: plain(net, x, ehs))
        zsd = {k: (torch.zeros_like(v) if ".proj_out." in k else v) for k, v in msd.items()}
        zero = HipMotionAdapter(net, mcfg).load_state_dict(zsd)
        net.attach_motion_adapter(zero)
        y, l_motion = _launches(engine_lib, lambda: run(net, x, ehs, F))
        assert torch.equal(y, base)
        n_attn = sum(n for k, n in l_motion.items() if k.startswith("temporal_attn_kernel"))
        assert n_attn == 42
        assert sum(l_motion.values()) > sum(l_plain.values())
        # attached but without frames: the plain launches
        y0, l_noframes = _launches(engine_lib, lambda: plain(net, x, ehs))
        assert torch.equal(y0, base) and l_noframes == l_plain
        net.attach_motion_adapter(None)
        y1, l_detached = _launches(engine_lib, lambda: plain(net, x, ehs))
        assert torch.equal(y1, base) and l_detached == l_plain
        with pytest.raises(_lib.EngineError) as e:
            run(net, x, ehs, F)
        assert "error 1" in str(e.value)
        print("launches: plain %d, with 21 modules %d" % (sum(l_plain.values()), sum(l_motion.values())))
    finally:
        net.attach_motion_adapter(ad)


def test_invalid_frames(engine_lib, tiny):
    net = tiny[4]
    x, ehs = inputs(3)
    for F in (4, 5):                                   # 6 frames are no multiple
        with pytest.raises(_lib.EngineError) as e:
            run(net, x, ehs, F)
        assert "error 1" in str(e.value)
    x33 = torch.zeros(33, 4, 16, 16).half()
    with pytest.raises(_lib.EngineError) as e:
        run(net, x33, ehs[:1].expand(33, -1, -1).contiguous(), 33)
    assert "error 1" in str(e.value) and "max_seq_length" in str(e.value)


def test_refused_combinations(engine_lib, tiny):
    """Everything that is not composed with frames returns SD_ERR_UNSUPPORTED before anything is launched, and the plain
    and the motion forward after it are what they were."""
    ucfg, usd, mcfg, msd, net, ad = tiny
    F = 3
    x, ehs = inputs(F)
    first = run(net, x, ehs, F)
    base = plain(net, x, ehs)

    def refused(fn=None):
        with pytest.raises(_lib.EngineError) as e:
            (fn or (lambda: run(net, x, ehs, F)))()
        assert "error 4" in str(e.value), str(e.value)

    states = [
        ("graph replay", lambda: net.use_graph(True), lambda: net.use_graph(False)),
        ("token merging", lambda: net.enable_tome(0.5), net.disable_tome),
        ("HyperTile", lambda: net.enable_hypertile(8), net.disable_hypertile),
        ("FreeU", lambda: net.enable_freeu(0.9, 0.2, 1.2, 1.4), net.disable_freeu),
    ]
    try:
        for name, on, off in states:
            on()
            try:
                refused()
                refused(lambda: net.forward_cfg(x.cuda(), torch.full((V * F,), 501.0), torch.cat([ehs, ehs]).cuda(), num_frames=F))
            finally:
                off()
            assert torch.equal(plain(net, x, ehs), base), name
        # DeepCache store and reuse
        net.enable_deepcache(2, 1)
        try:
            for mode in (1, 2):
                net.deep_cache_mode(mode)
                refused()
                refused(lambda: net.forward_cfg(x.cuda(), torch.full((V * F,), 501.0), torch.cat([ehs, ehs]).cuda(), num_frames=F))
            net.deep_cache_mode(0)
        finally:
            net.disable_deepcache()
        assert torch.equal(plain(net, x, ehs), base) and torch.equal(run(net, x, ehs, F), first)
        # regional prompts
        w = torch.rand(1, 2, 16, 16)
        net.set_regions(w / w.sum(1, keepdim=True))
        try:
            refused(lambda: run(net, x, torch.cat([ehs, ehs], dim=1), F))
        finally:
            net.clear_regions()
        # forward_pag / forward_concat cannot name frames: refused while an adapter is attached
        net.set_pag_layers(["mid"])
        try:
            refused(lambda: net.forward_pag(x[:1].cuda(), torch.tensor(501.0), ehs[:2].cuda()))
        finally:
            net.set_pag_layers([])
        assert torch.equal(plain(net, x, ehs), base)
        assert torch.equal(run(net, x, ehs, F), first)
        # forward_concat, through the C entry (the Python method checks the channel counts of an edit UNet first)
        lat, img_lat, e3 = x[:2].cuda(), x[:2].cuda(), ehs[:6].cuda()
        t2 = torch.full((2,), 501.0, device="cuda")
        out = torch.empty(6, 4, 16, 16, dtype=torch.float16, device="cuda")
        rc = engine_lib.sd_unet_forward_concat(net._h, P(lat), 2, 1.0, P(img_lat), 4, 2, 4, P(t2), P(e3), L_TXT, None, None, P(out),
                                               6, 16, 16, stream())
        assert rc == 4 and b"motion adapter" in engine_lib.sd_last_error()
        assert torch.equal(plain(net, x, ehs), base)
        assert torch.equal(run(net, x, ehs, F), first)
    finally:
        net.use_graph(False)
        net.disable_tome()
        net.disable_hypertile()
        net.disable_freeu()


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def c_forward_motion(lib, h, x, ehs, F):
    """sd_unet_forward_motion on handle h -> (rc, out)."""
    xc, ec = x.cuda(), ehs.cuda()
    t = torch.full((x.shape[0],), 501.0, device="cuda")
    out = torch.empty(x.shape[0], 4, 16, 16, dtype=torch.float16, device="cuda")
    rc = lib.sd_unet_forward_motion(h, P(xc), P(t), P(ec), ehs.shape[1], F, P(out), x.shape[0], 16, 16, stream())
    torch.cuda.synchronize()
    return rc, out


def test_refused_ip_adapter_and_timestep_cond(engine_lib, tiny):
    """An IP-Adapter at a non-zero scale is refused by the engine (error 4), at scale 0 the text attention runs alone and
    the forward is the one without the adapter, bit for bit; timestep_cond cannot be combined with frames at all."""
    from ip_oracle import synth_ip_state_dict
    from stablediffusion_amd.models import HipIPAdapter
    ucfg, usd, mcfg, msd, net, ad = tiny
    F = 3
    x, ehs = inputs(F)
    first = run(net, x, ehs, F)
    base = plain(net, x, ehs)
    ipad = HipIPAdapter(net, 128, 4).load_state_dict(synth_ip_state_dict(ucfg, 128, 4, seed=3))
    net.attach_ip_adapter(ipad)
    try:
        net.set_ip_adapter_scale(0.7)
        rc, _ = c_forward_motion(engine_lib, net._h, x, ehs, F)
        assert rc == 4 and b"IP-Adapter" in engine_lib.sd_last_error()
        img = torch.randn(2 * V * F, 1, 128, generator=torch.Generator().manual_seed(1)).half().cuda()
        with pytest.raises(_lib.EngineError) as e:
            net.forward_cfg(x.cuda(), torch.full((V * F,), 501.0), torch.cat([ehs, ehs]).cuda(),
                            added_cond_kwargs={"image_embeds": [img]}, num_frames=F)
        assert "error 4" in str(e.value) and "IP-Adapter" in str(e.value)
        net.set_ip_adapter_scale(0.0)
        rc, out = c_forward_motion(engine_lib, net._h, x, ehs, F)
        assert rc == 0, engine_lib.sd_last_error()
        assert torch.equal(out.float().cpu(), first)
        assert torch.equal(run(net, x, ehs, F), first)
    finally:
        net.set_ip_adapter_scale(1.0)
        net.attach_ip_adapter(None)
    assert torch.equal(plain(net, x, ehs), base) and torch.equal(run(net, x, ehs, F), first)
    # timestep_cond: no engine entry takes it together with frames, and the Python call says so before anything runs
    with pytest.raises(NotImplementedError, match="timestep_cond"):
        net(x.cuda(), torch.tensor(501.0), ehs.cuda(), timestep_cond=torch.zeros(V * F, 32), num_frames=F)
    assert torch.equal(run(net, x, ehs, F), first)


def test_refused_text_time_unet(engine_lib, tiny):
    """UNet::motion_refuse on a text_time UNet, through both C entries that name frames (the Python adapter class
    refuses the configuration itself, so the tiny adapter is moved over at the C level and back)."""
    ucfg, usd, mcfg, msd, net, ad = tiny
    F = 3
    x, ehs = inputs(F)
    first = run(net, x, ehs, F)
    xcfg = config.tiny_unet(sdxl_cond=True)
    with pytest.raises(NotImplementedError):
        mcfg.check(xcfg)
    xsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(xcfg), 1, perturb=0.1).items()}
    xnet = HipUNet2DConditionModel(xcfg, "cuda").load_state_dict(xsd)
    lib = engine_lib
    assert lib.sd_unet_set_motion(xnet._h, ad._h) == 0, lib.sd_last_error()
    try:
        rc, _ = c_forward_motion(lib, xnet._h, x, ehs, F)
        assert rc == 4 and b"text_time" in lib.sd_last_error()
        xc, e2 = x.cuda(), torch.cat([ehs, ehs]).cuda()
        t = torch.full((V * F,), 501.0, device="cuda")
        out = torch.empty(2 * V * F, 4, 16, 16, dtype=torch.float16, device="cuda")
        rc = lib.sd_unet_forward_cfg_ex(xnet._h, P(xc), P(t), P(e2), L_TXT, None, None, None, 0, 1.0, 1, F, P(out), V * F, 16, 16,
                                        stream())
        assert rc == 4 and b"text_time" in lib.sd_last_error()
    finally:
        assert lib.sd_unet_set_motion(net._h, ad._h) == 0, lib.sd_last_error()
    assert torch.equal(run(net, x, ehs, F), first)


def test_refused_models(engine_lib, tiny):
    """An attached ControlNet."""
    ucfg, usd, mcfg, msd, net, ad = tiny
    F = 3
    x, ehs = inputs(F)
    first = run(net, x, ehs, F)
    from stablediffusion_amd.models import HipControlNetModel
    cn_sd = {k: v.half().float() for k, v in weights.synth_state_dict(controlnet.controlnet_manifest(ucfg), 3, perturb=0.1).items()}
    cn = HipControlNetModel(net, ucfg).load_state_dict(cn_sd)
    net.attach_controlnet(cn)
    try:
        rc = engine_lib.sd_unet_forward_motion(net._h, C.c_void_p(x.cuda().data_ptr()), None, None, L_TXT, F, None, V * F, 16, 16, None)
        assert rc in (1, 4)
        t = torch.full((V * F,), 501.0, device="cuda")
        xc, ec = x.cuda(), ehs.cuda()
        out = torch.empty(V * F, 4, 16, 16, dtype=torch.float16, device="cuda")
        rc = engine_lib.sd_unet_forward_motion(net._h, C.c_void_p(xc.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(ec.data_ptr()),
                                               L_TXT, F, C.c_void_p(out.data_ptr()), V * F, 16, 16,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 4 and b"ControlNet" in engine_lib.sd_last_error()
    finally:
        net.attach_controlnet(None)
    assert torch.equal(run(net, x, ehs, F), first)


def test_forward_on_poisoned_scratch(engine_lib, tiny):
    net = tiny[4]
    for F in (3, 16):
        x, ehs = inputs(F)
        first = run(net, x, ehs, F)
        assert torch.isfinite(first).all()
        for pattern in (0, 1):
            assert net._poison_workspace(pattern) > 0
            assert torch.equal(run(net, x, ehs, F), first), (F, pattern)
