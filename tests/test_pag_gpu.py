"""Perturbed-attention guidance on the GPU: HipUNet2DConditionModel.forward_pag (sd_unet_forward_pag) against
tests/pag_oracle.py, late widening against up-front duplication, the device step entries sd_pag_linear_step /
sd_pag_combine against the float64 formula, and the pipeline's loops.

Bounds are the project's own: TOL = 1e-2 rel-L2 against the oracle, SAME = 1e-3 for "same sample, other batch size".

Power condition.  A perturbed branch that silently equals the text branch must not pass, so every oracle case asserts
the ORACLE's own rel_l2(perturbed, text) >= 5 TOL.  With the synthetic weights as they come the mid block alone (a 2 x 2
map at 16 x 16 latents) gives 2.3e-2 .. 3.2e-2, so `mid_block.attentions.0.transformer_blocks.0.attn1.to_out.0.weight`
is scaled by MID_BOOST = 4 in the state dict of both networks.  The oracle then measures, with CFG at t = 501 over the
three shapes: mid 7.4e-2 .. 1.0e-1 (tiny) and 8.8e-2 .. 9.5e-2 (linear + text_time); down_blocks.1.attentions.0
3.1e-1 .. 3.7e-1; up_blocks.1.attentions.2 1.6e-1 .. 1.7e-1; down_blocks.0.attentions.0 5.8e-1 .. 6.5e-1;
mid + up_blocks.2.attentions.0 1.9e-1 .. 2.2e-1 (those four measured without the boost, which only adds to them)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import pag_oracle  # noqa: E402
from test_pag import call_step, invalid_step_calls  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import (HipAutoencoderKL, HipControlNetModel, HipIPAdapter,  # noqa: E402
                                        HipUNet2DConditionModel)

pytestmark = pytest.mark.gpu

TOL = 1e-2
SAME = 1e-3
MID_BOOST = 4.0
CASES = [(2, 16, 16), (1, 8, 24), (3, 16, 16)]
MID = "mid_block.attentions.0"
SITES = [(MID,), ("down_blocks.1.attentions.0",), ("up_blocks.1.attentions.2",), ("down_blocks.0.attentions.0",),
         (MID, "up_blocks.2.attentions.0")]
FREEU = (0.9, 0.2, 1.5, 1.6)
GUARD = 16


def _state_dict(cfg, seed):
    sd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=seed, perturb=0.1).items()}
    k = MID + ".transformer_blocks.0.attn1.to_out.0.weight"
    sd[k] = (sd[k] * MID_BOOST).half().float()
    return sd


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, cfg, seed in (("tiny", config.tiny_unet(), 11), ("xl", config.tiny_unet(linear=True, sdxl_cond=True), 13)):
        sd = _state_dict(cfg, seed)
        out[name] = (cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd))
    return out


def _inputs(cfg, B, H, W, cfg_on, seed=None):
    g = torch.Generator().manual_seed(B * 100 + H if seed is None else seed)
    G = 2 if cfg_on else 1
    x = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(G * B, 77, cfg.cross_attention_dim, generator=g).half()
    added = None
    if cfg.addition_embed_type == "text_time":
        added = {"text_embeds": torch.randn(G * B, 64, generator=g).half(),
                 "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * (G * B))}
    return x, ehs, added


def _cuda(added):
    return None if added is None else {k: v.cuda() for k, v in added.items()}


def _f32(added):
    return None if added is None else {k: v.float() for k, v in added.items()}


# ------------------------------------------------------------------------------------------------ the forward
@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("sites", SITES, ids=["mid", "down1", "up1", "first", "mid+up2"])
@pytest.mark.parametrize("B,H,W", CASES)
@pytest.mark.parametrize("name", ["tiny", "xl"])
def test_forward_pag_matches_oracle_and_its_own_forms(engine_lib, nets, name, B, H, W, sites, cfg_on):
    """Every group within TOL of the oracle; the un-perturbed groups within SAME of forward_cfg / the plain forward; late
    widening within SAME of up-front duplication; the oracle's own perturbed group at least 5 TOL off its text group."""
    cfg, sd, net = nets[name]
    x, ehs, added = _inputs(cfg, B, H, W, cfg_on)
    G = 2 if cfg_on else 1
    t, s = 501.0, 0.5          # (exact in fp16: the test scales the reference latents itself)
    xs = (x.float() * s).half()
    net.set_pag_layers(sites)
    assert net.pag_layers == sites
    late = net.forward_pag(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), in_scale=s, cfg=cfg_on, share=True)[0]
    front = net.forward_pag(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), in_scale=s, cfg=cfg_on, share=False)[0]
    assert late.shape == front.shape == ((G + 1) * B, cfg.out_channels, H, W) and late.dtype == torch.float16
    with torch.no_grad():
        ref = pag_oracle.forward_pag(cfg, sd, xs.float(), torch.tensor(t), ehs.float(), sites, cfg_on, _f32(added))
    power = rel_l2(ref[G * B:], ref[(G - 1) * B:G * B])
    errs = [rel_l2(late[k * B:(k + 1) * B], ref[k * B:(k + 1) * B]) for k in range(G + 1)]
    errs_front = [rel_l2(front[k * B:(k + 1) * B], ref[k * B:(k + 1) * B]) for k in range(G + 1)]
    if cfg_on:
        plain = net.forward_cfg(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), in_scale=s)[0]
    else:
        plain = net(xs.cuda(), torch.tensor(t), ehs.cuda(), added_cond_kwargs=_cuda(added))[0]
    e_plain, e_share = rel_l2(late[:G * B], plain), rel_l2(late, front)
    print(f"{name} B={B} {H}x{W} {'+'.join(sites)} cfg={cfg_on}: oracle pert-vs-text {power:.2e}; vs oracle late "
          f"{' '.join(f'{e:.2e}' for e in errs)}, up front {' '.join(f'{e:.2e}' for e in errs_front)}; un-perturbed vs plain "
          f"{e_plain:.2e}; late vs up front {e_share:.2e}")
    assert power >= 5 * TOL
    assert max(errs) < TOL and max(errs_front) < TOL
    assert e_plain < SAME
    assert e_share < SAME
    # up-front duplication takes no shared prefix: its un-perturbed groups are bit for bit the un-perturbed forward's
    if cfg_on:
        plain = net.forward_cfg(x.cuda(), t, ehs.cuda(), added_cond_kwargs=_cuda(added), in_scale=s, share=False)[0]
    assert torch.equal(front[:G * B], plain)


@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("sites", SITES, ids=["mid", "down1", "up1", "first", "mid+up2"])
def test_share_off_is_bitwise_the_forward_on_triplicated_latents(engine_lib, nets, sites, cfg_on):
    """share=False against net(cat([latents] * (G + 1)), ...), the plain forward on the whole batch, whose last group is
    a second text group: the un-perturbed groups bit for bit, the perturbed one apart."""
    cfg, sd, net = nets["tiny"]
    B, H, W = 2, 16, 16
    x, ehs, added = _inputs(cfg, B, H, W, cfg_on)
    G = 2 if cfg_on else 1
    net.set_pag_layers(sites)
    front = net.forward_pag(x.cuda(), 501.0, ehs.cuda(), cfg=cfg_on, share=False)[0]
    sample3, ehs3, _ = pag_oracle.pag_batch(x, ehs, cfg_on)
    explicit = net(sample3.cuda(), torch.tensor(501.0), ehs3.cuda())[0]
    small = net(sample3[:G * B].cuda(), torch.tensor(501.0), ehs.cuda())[0]
    print(f"{'+'.join(sites)} cfg={cfg_on}: un-perturbed groups, share=False vs the (G+1)B forward "
          f"{rel_l2(front[:G * B], explicit[:G * B]):.2e}; the GB forward vs the (G+1)B forward's first GB "
          f"{rel_l2(small, explicit[:G * B]):.2e} (bitwise {torch.equal(small, explicit[:G * B])})")
    assert rel_l2(front[G * B:], explicit[G * B:]) > TOL          # (the plain forward's third group is the text group)
    assert torch.equal(front[:G * B], explicit[:G * B])


def _garbage_qk(sd, sites, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    for k in sd:
        if any(k.startswith(s + ".") for s in sites) and (k.endswith("attn1.to_q.weight") or k.endswith("attn1.to_k.weight")):
            out[k] = (torch.randn(sd[k].shape, generator=g) * 0.3).half().float()
    return out


@pytest.mark.parametrize("share", [True, False], ids=["late", "upfront"])
@pytest.mark.parametrize("sites", [(MID,), ("down_blocks.1.attentions.0", "down_blocks.1.attentions.1")], ids=["mid", "down1"])
def test_perturbed_group_never_reads_q_or_k(engine_lib, nets, sites, share):
    """With the flagged transformers' attn1.to_q / to_k replaced by other finite weights the perturbed group's output is
    bit for bit the same (everything it reads upstream is unchanged for these sites), while the text group's moves."""
    cfg, sd, net = nets["tiny"]
    other = HipUNet2DConditionModel(cfg).load_state_dict(_garbage_qk(sd, sites))
    x, ehs, _ = _inputs(cfg, 2, 16, 16, True, seed=31)
    outs = []
    for n in (net, other):
        n.set_pag_layers(sites)
        outs.append(n.forward_pag(x.cuda(), 301.0, ehs.cuda(), share=share)[0])
    a, b = outs
    assert torch.equal(a[4:], b[4:])            # (down1: both transformers of the block are flagged, one after the other)
    assert rel_l2(a[2:4], b[2:4]) > 1e-3


def test_determinism_and_text_kv_cache(engine_lib, nets):
    cfg, sd, net = nets["tiny"]
    net.set_pag_layers((MID,))
    g = torch.Generator().manual_seed(25)
    ehs = torch.randn(4, 77, cfg.cross_attention_dim, generator=g).half().cuda()
    steps = [(torch.randn(2, 4, 16, 16, generator=g).half().cuda(), t) for t in (981.0, 501.0, 21.0)]
    for share in (True, False):
        plain = [net.forward_pag(x, t, ehs, share=share)[0] for x, t in steps]
        again = [net.forward_pag(x, t, ehs, share=share)[0] for x, t in steps]
        try:
            net.text_kv_cache(True)
            cached = [net.forward_pag(x, t, ehs, share=share)[0] for x, t in steps]
            # a CFG forward in between re-projects for its own batch and does not disturb the next perturbed one
            mixed = [net.forward_cfg(steps[0][0], 981.0, ehs)[0], net.forward_pag(*steps[1], ehs, share=share)[0]]
        finally:
            net.text_kv_cache(False)
        assert not torch.equal(plain[0], plain[1])
        for a, b, c in zip(plain, again, cached):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(mixed[1], plain[1])
        assert torch.equal(mixed[0], net.forward_cfg(steps[0][0], 981.0, ehs)[0])


@pytest.mark.parametrize("sites", [(MID,), ("up_blocks.1.attentions.2",), ("down_blocks.1.attentions.0",)], ids=["mid", "up1", "down1"])
def test_freeu_composes(engine_lib, nets, sites):
    cfg, sd, net = nets["tiny"]
    B, H, W = 2, 16, 16
    x, ehs, _ = _inputs(cfg, B, H, W, True, seed=41)
    net.set_pag_layers(sites)
    net.enable_freeu(*FREEU)
    try:
        late = net.forward_pag(x.cuda(), 501.0, ehs.cuda(), share=True)[0]
        front = net.forward_pag(x.cuda(), 501.0, ehs.cuda(), share=False)[0]
    finally:
        net.disable_freeu()
    with torch.no_grad():
        on = pag_oracle.forward_pag(cfg, sd, x.float(), torch.tensor(501.0), ehs.float(), sites, True, freeu=FREEU)
        off = pag_oracle.forward_pag(cfg, sd, x.float(), torch.tensor(501.0), ehs.float(), sites, True)
    e_late, e_front = rel_l2(late, on), rel_l2(front, on)
    print(f"FreeU {'+'.join(sites)}: late {e_late:.2e}, up front {e_front:.2e}; oracle on vs off {rel_l2(on, off):.2e}")
    assert rel_l2(on, off) > 5 * TOL
    assert e_late < TOL and e_front < TOL
    assert rel_l2(late, front) < SAME


def _refused(fn, what):
    with pytest.raises(_lib.EngineError, match=r"error 4: .*" + what):
        fn()


def test_refusals_leave_the_handle_usable(engine_lib, nets):
    cfg, sd, net = nets["tiny"]
    x, ehs, _ = _inputs(cfg, 2, 16, 16, True, seed=51)
    xd, ed = x.cuda(), ehs.cuda()
    net.set_pag_layers((MID,))
    want = net.forward_pag(xd, 501.0, ed)[0]
    plain = net(torch.cat([xd, xd]), torch.tensor(501.0), ed)[0]
    run = lambda: net.forward_pag(xd, 501.0, ed)[0]
    # a ControlNet attached
    ccfg = controlnet.encoder_config(cfg)
    cn = HipControlNetModel(net, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=6))
    net.attach_controlnet(cn)
    try:
        _refused(run, "ControlNet")
    finally:
        net.attach_controlnet(None)
    assert torch.equal(net(torch.cat([xd, xd]), torch.tensor(501.0), ed)[0], plain)
    # an IP-Adapter at a non-zero scale; at scale 0 the text attention runs alone
    ad = HipIPAdapter(net, 128, 4).load_state_dict(synth_ip_state_dict(cfg, 128, 4, seed=3))
    net.attach_ip_adapter(ad).set_ip_adapter_scale(0.7)
    try:
        _refused(run, "IP-Adapter")
        net.set_ip_adapter_scale(0.0)
        assert torch.equal(run(), want)
    finally:
        net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    assert torch.equal(net(torch.cat([xd, xd]), torch.tensor(501.0), ed)[0], plain)
    # DeepCache store / reuse
    net.enable_deepcache(2, 1)
    try:
        for mode in (net.DC_STORE, net.DC_REUSE):
            net.deep_cache_mode(mode)
            _refused(run, "DeepCache")
        net.deep_cache_mode(net.DC_PLAIN)
        assert torch.equal(run(), want)
    finally:
        net.disable_deepcache()
    # graph replay
    net.use_graph(True)
    try:
        _refused(run, "graph")
    finally:
        net.use_graph(False)
    assert torch.equal(net(torch.cat([xd, xd]), torch.tensor(501.0), ed)[0], plain)
    assert torch.equal(run(), want)
    # no flagged transformer, an unknown key
    net.set_pag_layers(None)
    with pytest.raises(_lib.EngineError, match="error 1"):
        run()
    keys = (C.c_char_p * 1)(b"mid_block.attentions.7")
    assert engine_lib.sd_unet_set_pag_layers(net._h, keys, 1) == 1
    net.set_pag_layers("mid")
    assert torch.equal(run(), want)
    # a guidance-embedded UNet
    tcfg = config.tiny_unet(time_cond=32)
    tsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(tcfg), seed=11).items()}
    tnet = HipUNet2DConditionModel(tcfg).load_state_dict(tsd).set_pag_layers("mid")
    _refused(lambda: tnet.forward_pag(xd, 501.0, ed), "timestep_cond")
    tc = torch.zeros(2, 32).cuda()
    assert torch.isfinite(tnet(xd, torch.tensor(501.0), ed[:2], timestep_cond=tc)[0].float()).all()


def test_layers_survive_rebuild(engine_lib, nets):
    cfg, sd, net = nets["tiny"]
    net.set_pag_layers(["mid", "up.block_1.attentions_2"])
    assert net.pag_layers == (MID, "up_blocks.1.attentions.2")
    new = net.rebuild(sd)
    assert new.pag_layers == net.pag_layers
    x, ehs, _ = _inputs(cfg, 1, 16, 16, True, seed=61)
    assert torch.equal(new.forward_pag(x.cuda(), 301.0, ehs.cuda())[0], net.forward_pag(x.cuda(), 301.0, ehs.cuda())[0])
    with pytest.raises(ValueError, match="pag_applied_layers"):
        net.set_pag_layers("up.block_0")


# ------------------------------------------------------------------------------------------------ the device step
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def _guarded(t, fill, shift=0):
    buf = torch.full((GUARD + shift + t.numel() + GUARD,), fill, dtype=t.dtype, device="cuda")
    buf[GUARD + shift:GUARD + shift + t.numel()] = t.cuda()
    return buf, buf[GUARD + shift:GUARD + shift + t.numel()]


def _ulp16(v):
    """Spacing of fp16 at |v| (float64 tensor): 2^-24 below 2^-14, else 2^(floor(log2 |v|) - 10)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def _bounds(mo, rows, x, hist, g, s, c):
    """float64 references and per-element bounds.  The combine: one fp16 ulp of e (its rounding is half of one) plus the
    fp32 evaluation of the two fmas, each within 2^-24 of its result and so within 2^-23 of the sum of the terms'
    magnitudes.  That bound goes through the update's coefficients; the latents add one fp16 ulp of their own and the
    fp32 evaluation of the update (2^-22 of the terms' magnitudes), the fp32 history only the latter."""
    m = mo.double().reshape(rows, -1)
    t, p = m[rows - 2], m[rows - 1]
    mag = (s * (t - p)).abs() + t.abs()
    if rows == 3:
        mag = mag + m[0].abs() + (g * (t - m[0])).abs()
    e = pag_oracle.pag_combine(mo, rows, g, s)
    tol_e = _ulp16(e) + 2.0 ** -23 * mag
    cx, ce, ch, hx, he = c
    out, h_new = pag_oracle.linear_step(e, x, hist, cx, ce, ch, hx, he)
    xd = x.double().reshape(-1)
    mag_out = (cx * xd).abs() + (ce * e).abs() + (0 if hist is None else (ch * hist.double().reshape(-1)).abs())
    tol_out = abs(ce) * tol_e + _ulp16(out) + 2.0 ** -22 * mag_out
    tol_h = abs(he) * tol_e + 2.0 ** -22 * ((hx * xd).abs() + (he * e).abs())
    return e, tol_e, out, tol_out, h_new, tol_h


COEF = tuple(torch.tensor(v, dtype=torch.float32).item() for v in (0.93, -0.41, 0.27, 1.07, -0.38))   # (exact in fp32)


@pytest.mark.parametrize("with_hist", [False, True], ids=["nohist", "hist"])
@pytest.mark.parametrize("n,shift", [(8, 0), (8, 1), (4096 + 8, 0), (37, 0)])
@pytest.mark.parametrize("rows", [2, 3])
def test_pag_step_entries(engine_lib, rows, n, shift, with_hist):
    """sd_pag_linear_step and sd_pag_combine against the float64 formula for g in {1, 7.5} x s in {0, 3}; n = 37 and the
    base one element off the 16-byte alignment take the scalar kernel.  The guards around every buffer and the model
    output stay untouched; with s = 0 three rows are bit for bit sd_cfg_linear_step on the first two."""
    gen = torch.Generator().manual_seed(n * 10 + rows)
    mo = torch.randn(rows * n, generator=gen).half()
    x = (torch.randn(n, generator=gen) * 2).half()
    hist = torch.randn(n, generator=gen) if with_hist else None
    for g in (1.0, 7.5):
        for s in (0.0, 3.0):
            e, tol_e, out, tol_out, h_new, tol_h = _bounds(mo, rows, x, hist, g, s, COEF)
            mo_buf, mo_v = _guarded(mo, 3.0, shift)
            x_buf, x_v = _guarded(x, 5.0, shift)
            e_buf, e_v = _guarded(torch.zeros(n).half(), 7.0, shift)
            h_buf, h_v = _guarded(hist if with_hist else torch.zeros(n), 9.0, shift)
            assert engine_lib.sd_pag_combine(P(mo_v), rows, P(e_v), n, g, s, stream()) == 0, engine_lib.sd_last_error()
            assert engine_lib.sd_pag_linear_step(P(mo_v), rows, P(x_v), P(h_v) if with_hist else None, n, g, s, *COEF,
                                                 stream()) == 0, engine_lib.sd_last_error()
            torch.cuda.synchronize()
            got_e, got_x = e_v.cpu().double(), x_v.cpu().double()
            assert torch.isfinite(got_e).all() and torch.isfinite(got_x).all()
            worst_e = ((got_e - e).abs() / tol_e).max().item()
            worst_x = ((got_x - out).abs() / tol_out).max().item()
            assert worst_e <= 1.0, (rows, n, shift, g, s, worst_e)
            assert worst_x <= 1.0, (rows, n, shift, g, s, worst_x)
            if with_hist:
                worst_h = ((h_v.cpu().double() - h_new).abs() / tol_h).max().item()
                assert worst_h <= 1.0, (rows, n, shift, g, s, worst_h)
            else:
                assert (h_v == 0).all()
            for buf, fill in ((mo_buf, 3.0), (x_buf, 5.0), (e_buf, 7.0)):
                assert (buf[:GUARD + shift] == fill).all() and (buf[-GUARD:] == fill).all()
            assert (h_buf[:GUARD + shift] == 9.0).all() and (h_buf[-GUARD:] == 9.0).all()
            assert torch.equal(mo_v.cpu(), mo)
            if s == 0.0 and rows == 3:
                ref_x = x.cuda().clone()
                ref_h = hist.cuda().clone() if with_hist else None
                assert engine_lib.sd_cfg_linear_step(P(mo_v), P(ref_x), P(ref_h) if with_hist else None, n, g, *COEF,
                                                     stream()) == 0
                torch.cuda.synchronize()
                assert torch.equal(x_v.view(torch.int16), ref_x.view(torch.int16))
                if with_hist:
                    assert torch.equal(h_v.view(torch.int32), ref_h.view(torch.int32))
            if s == 0.0 and rows == 2:
                assert torch.equal(e_v.cpu(), mo[:n])               # t + 0 (t - p) is t


def test_pag_step_invalid_arguments_launch_nothing(engine_lib):
    mo = torch.randn(24).half().cuda()
    lat = torch.randn(8).half().cuda()
    mo0, lat0 = mo.clone(), lat.clone()
    for label, entry, args in invalid_step_calls():
        assert call_step(engine_lib, entry, args, (mo.data_ptr(), lat.data_ptr()), stream()) == 1, label
    torch.cuda.synchronize()
    assert torch.equal(mo, mo0) and torch.equal(lat, lat0)
    assert engine_lib.sd_pag_linear_step(P(mo), 3, P(lat), None, 8, 5.0, 3.0, *COEF, stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(lat, lat0)


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def model(nets):
    from stablediffusion_amd.pipeline import SDModelWrapper
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, usd, _ = nets["tiny"]
    vcfg = config.tiny_vae()
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), seed=12, perturb=0.1).items()}
    return SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                          vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")


def _oracle_loop(cfg, sd, lat0, ehs2b, steps, g, pag_scale, adaptive, sites, scheduler, noises=None):
    """pipeline_ref.denoise_ref with the perturbed third group and PAG's combine; -> (latents, the steps' scales)."""
    import numpy as np
    from oracle import schedulers_ref
    from oracle.pipeline_ref import SCHEDULERS
    from stablediffusion_amd import pag
    sch = schedulers_ref.EulerAncestralRef() if scheduler == "euler_a" else SCHEDULERS[scheduler]()
    ts = sch.set_timesteps(steps)
    x = lat0.double().numpy() * sch.init_noise_sigma
    B = lat0.shape[0]
    scales = []
    for i, t in enumerate(ts):
        s = pag.step_scale(pag_scale, adaptive, float(t))
        scales.append(s)
        xin = torch.from_numpy(sch.scale_model_input(x, t)).float()
        with torch.no_grad():
            if s > 0:
                eps = pag_oracle.forward_pag(cfg, sd, xin, torch.tensor(float(t)), ehs2b, sites, True).double().numpy()
                e_u, e_t, e_p = eps[:B], eps[B:2 * B], eps[2 * B:]
                e = e_u + g * (e_t - e_u) + s * (e_t - e_p)
            else:
                from oracle.unet_ref import unet_forward
                eps = unet_forward(cfg, sd, torch.cat([xin, xin]), torch.tensor(float(t)), ehs2b).double().numpy()
                e = eps[:B] + g * (eps[B:] - eps[:B])
        x = sch.step(e, t, x, noises[i].double().numpy()) if noises is not None else sch.step(e, t, x)
    return torch.from_numpy(np.asarray(x)).float(), scales


@pytest.mark.parametrize("sched", ["DDIM", "euler_a"])
def test_tiny_txt2img_loop_matches_oracle_loop(engine_lib, nets, model, sched):
    """4 steps with pag_scale = 3 and an adaptive scale that switches the last steps back to plain CFG: DDIM runs the
    fused sd_pag_linear_step, euler_a sd_pag_combine + sd_sched_affine_step.  Against the oracle loop at the tiny-loop
    tests' bound (test_tiny_txt2img_with_ip_embeds_matches_oracle_loop: TOL); pag_scale = 0 is bitwise the call without."""
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    ucfg, usd, _ = nets["tiny"]
    model.set_scheduler(sched)
    g = torch.Generator().manual_seed(4)
    B, steps, gs, adaptive = 2, 4, 5.0, 0.005
    pos = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    neg = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).half()
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    kw = dict(prompt_embeds=pos.cuda(), negative_prompt_embeds=neg.cuda(), latents=lat0.cuda(), num_inference_steps=steps,
              guidance_scale=gs, height=128, width=128)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    calls = {}
    lib = model.base._lib

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("sd_"):
                return fn

            def wrapped(*a):
                calls[name] = calls.get(name, 0) + 1
                return fn(*a)
            return wrapped
    model.base._lib = Counting()
    try:
        torch.manual_seed(7)
        got = pipe(model, pag_scale=3.0, pag_adaptive_scale=adaptive, **kw)
    finally:
        model.base._lib = lib
    noises = None
    if sched == "euler_a":
        torch.manual_seed(7)
        noises = [torch.randn(lat0.shape, device="cuda", dtype=torch.float16).cpu().float() for _ in range(steps)]
    ref, scales = _oracle_loop(ucfg, usd, lat0.float(), torch.cat([neg, pos]).float(), steps, gs, 3.0, adaptive, (MID,),
                               sched, noises)
    plain_ref, _ = _oracle_loop(ucfg, usd, lat0.float(), torch.cat([neg, pos]).float(), steps, gs, 0.0, 0.0, (MID,), sched,
                                noises)
    on = sum(1 for s in scales if s > 0)
    assert 0 < on < steps and scales[-1] == 0.0
    assert calls.get("sd_unet_forward_pag") == on and calls.get("sd_unet_forward_cfg") == steps - on
    if sched == "DDIM":
        assert calls.get("sd_pag_linear_step") == on and calls.get("sd_cfg_linear_step") == steps - on
        assert "sd_pag_combine" not in calls
    else:
        assert calls.get("sd_pag_combine") == on and calls.get("sd_sched_affine_step") == steps
        assert "sd_pag_linear_step" not in calls
    e, apart = rel_l2(got, ref), rel_l2(plain_ref, ref)
    print(f"{sched}: PAG loop vs oracle loop {e:.2e}; oracle with vs without PAG {apart:.2e}; scales {scales}")
    assert torch.isfinite(got.float()).all()
    assert e < TOL
    assert apart > 3 * TOL      # (the oracle alone, on the CPU: 4.5e-2 for DDIM, 5.2e-2 for euler_a with other noise)
    torch.manual_seed(7)
    zero = pipe(model, pag_scale=0.0, pag_adaptive_scale=0.0, **kw)
    torch.manual_seed(7)
    without = pipe(model, **kw)
    assert torch.equal(zero, without)
    assert rel_l2(zero, got) > TOL


def test_pipeline_layers_and_rescale_path(engine_lib, model):
    """set_pag_applied_layers reaches the engine; guidance_rescale > 0 with PAG takes scheduler.step; share on vs off."""
    from stablediffusion_amd.pipeline import StableDiffusionUnifiedPipeline
    ucfg = config.tiny_unet()
    model.set_scheduler("DDIM")
    g = torch.Generator().manual_seed(6)
    pos = torch.randn(1, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    neg = torch.randn(1, 77, ucfg.cross_attention_dim, generator=g).half().cuda()
    lat0 = torch.randn(1, 4, 16, 16, generator=g).half().cuda()
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=lat0, num_inference_steps=3, guidance_scale=5.0,
              height=128, width=128, pag_scale=2.0)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    used = []
    real = pipe._device_iteration
    pipe._device_iteration = lambda *a, **k: (used.append(1), real(*a, **k))[1]
    try:
        model.set_pag_applied_layers(["mid", "up.block_1.attentions_2"])
        assert model.base.pag_layers == (MID, "up_blocks.1.attentions.2")
        two = pipe(model, **kw)
        assert len(used) == 3
        pipe.pag_share = False
        front = pipe(model, **kw)
        pipe.pag_share = True
        model.set_pag_applied_layers("mid")
        one = pipe(model, **kw)
        used.clear()
        resc = pipe(model, guidance_rescale=0.7, **kw)
        assert not used
    finally:
        model.set_pag_applied_layers("mid")
    assert rel_l2(two, front) < TOL
    assert rel_l2(two, one) > 1e-3
    assert torch.isfinite(resc.float()).all() and rel_l2(resc, one) > 1e-3
    # without CFG: DDIM has no device step there, the host loop calls forward_pag; euler_a runs combine + the affine entry
    nocfg = StableDiffusionUnifiedPipeline(do_cfg=False, device="cuda", output_type="latents")
    kw2 = {k: v for k, v in kw.items() if k != "negative_prompt_embeds"}
    a = nocfg(model, **kw2)
    b = nocfg(model, **{**kw2, "pag_scale": 0.0})
    assert torch.isfinite(a.float()).all() and rel_l2(a, b) > 1e-3
    model.set_scheduler("euler_a")
    torch.manual_seed(2)
    c = nocfg(model, **kw2)
    torch.manual_seed(2)
    d = nocfg(model, **{**kw2, "pag_scale": 0.0})
    assert torch.isfinite(c.float()).all() and rel_l2(c, d) > 1e-3
