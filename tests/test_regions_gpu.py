"""Regional prompts on the engine: the weight pyramid, the UNet forward with regions against the oracle with the regional
attention (tests/region_oracle.py), forward_cfg, the text-K/V cache, clearing, every refusal, the pipeline, and one
full-width forward per preset."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")   # the full-width checker's fp32 convs: skip MIOpen's kernel search

import pytest  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import region_oracle as ro  # noqa: E402
from conftest import rel_l2  # noqa: E402
from oracle import unet_ref  # noqa: E402
from stablediffusion_amd import _lib, config, regions, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-2
FAR = 5e-2
L = 77
R = 3


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sd(cfg, seed=1):
    return {k: v.half().float() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed, perturb=0.1).items()}


@pytest.fixture(scope="module")
def tiny():
    cfg = config.tiny_unet()
    sd = _sd(cfg)
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


@pytest.fixture(scope="module")
def tiny_xl():
    cfg = config.tiny_unet(linear=True, sdxl_cond=True)
    sd = _sd(cfg)
    return cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd)


@pytest.fixture(autouse=True)
def _leave_no_regions(tiny, tiny_xl):
    yield
    for _, _, net in (tiny, tiny_xl):
        net.clear_regions()
        net.text_kv_cache(False)


# ---------------------------------------------------------------------------------------------------- the pyramid
@pytest.mark.parametrize("Bw,Rr,H,W,levels", [(2, 3, 16, 24, 4), (1, 8, 8, 8, 4), (3, 1, 6, 10, 2), (2, 5, 7, 3, 1)])
def test_pyramid_is_the_average_pool(engine_lib, Bw, Rr, H, W, levels):
    """Every level [Bw, T_l, R] of sd_op_region_pyramid is avg_pool2d of the level above, transposed; nothing is written
    behind the last level."""
    g = torch.Generator().manual_seed(H * W + Rr)
    w = torch.rand(Bw, Rr, H, W, generator=g)
    w = (w / w.sum(1, keepdim=True)).cuda()
    sizes = [Bw * (H >> lvl) * (W >> lvl) * Rr for lvl in range(levels)]
    out = torch.full((sum(sizes) + 64,), float("nan"), device="cuda")
    assert engine_lib.sd_op_region_pyramid(P(w), P(out), Bw, Rr, H, W, levels, stream()) == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out[sum(sizes):]).all()
    at, want = 0, w
    for lvl in range(levels):
        if lvl:
            want = F.avg_pool2d(want, 2)
        got = out[at:at + sizes[lvl]].view(Bw, (H >> lvl) * (W >> lvl), Rr)
        assert torch.allclose(got, want.flatten(2).transpose(1, 2), atol=1e-7, rtol=0), lvl
        assert torch.allclose(got.sum(-1), torch.ones_like(got[..., 0]), atol=1e-6)
        at += sizes[lvl]
    # 0 / 1 stripes: every level exact
    s = ro.stripe_weights(Bw, Rr, 16, 24).cuda() if (H, W) == (16, 24) else None
    if s is not None:
        assert engine_lib.sd_op_region_pyramid(P(s), P(out), Bw, Rr, H, W, levels, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[sizes[0]:sizes[0] + sizes[1]].view(Bw, -1, Rr), F.avg_pool2d(s, 2).flatten(2).transpose(1, 2))


def test_pyramid_rejects(engine_lib):
    w = torch.ones(1, 1, 8, 8, device="cuda")
    out = torch.full((256,), float("nan"), device="cuda")
    for args in [(1, 1, 8, 8, 5), (1, 1, 8, 8, 0), (1, 9, 8, 8, 1), (1, 0, 8, 8, 1), (0, 1, 8, 8, 1), (1, 1, 6, 8, 3)]:
        assert engine_lib.sd_op_region_pyramid(P(w), P(out), *args, stream()) == 1, args
    assert engine_lib.sd_op_region_pyramid(None, P(out), 1, 1, 8, 8, 1, stream()) == 1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------- the UNet
def _forward_ex(net, x, t, ehs, cond):
    """sd_unet_forward_ex without image embeds (the wrapper's __call__ takes the narrower sd_unet_forward)."""
    B, _, H, W = x.shape
    out = torch.empty(B, net.cfg.out_channels, H, W, device="cuda", dtype=torch.float16)
    ts = torch.full((B,), float(t), device="cuda")
    rc = net._lib.sd_unet_forward_ex(net._h, P(x), P(ts), P(ehs), ehs.shape[1], P(cond["text_embeds"]), P(cond["time_ids"]),
                                     None, 0, P(out), B, H, W, stream())
    _lib.check(rc, "sd_unet_forward_ex")
    return out


@pytest.mark.parametrize("h,w", [(16, 16), (8, 24)])
@pytest.mark.parametrize("variant", ["tiny", "tiny-xl"])
def test_tiny_unet_with_regions_matches_the_oracle(engine_lib, tiny, tiny_xl, variant, h, w):
    """B = 2, R = 3, stripes whose edges mix at the coarser levels: within 1e-2 of the oracle with the regional attention,
    and more than 5e-2 away from the plain forward on the base prompt."""
    cfg, sd, net = tiny if variant == "tiny" else tiny_xl
    x, ehs = ro.unet_inputs(cfg, 2, h, w, R, seed=11)
    wts = ro.stripe_weights(2, R, h, w)
    cond = ro.sdxl_cond(cfg, 2, 5) if variant == "tiny-xl" else None
    xd, ed = x.cuda(), ehs.cuda()
    net.set_regions(wts)
    assert net.regions == (2, R, h, w)
    if cond is None:
        got = net(xd, 981.0, ed)[0]
    else:
        cd = {"text_embeds": cond["text_embeds"].cuda(), "time_ids": cond["time_ids"].cuda().float().contiguous()}
        got = _forward_ex(net, xd, 981.0, ed, cd)
    net.clear_regions()
    base = net(xd, 981.0, ehs[:, :L].contiguous().cuda(), added_cond_kwargs=cond)[0]
    ref = ro.forward(cfg, sd, x, torch.tensor(981.0), ehs, wts, None if cond is None else {k: v.float() for k, v in cond.items()})
    err, dist = rel_l2(got, ref), rel_l2(got, base)
    print("%s %dx%d: vs oracle %.2e, vs the base prompt alone %.3f" % (variant, h, w, err, dist))
    assert torch.isfinite(got.float()).all()
    assert err < TOL
    assert dist > FAR


def test_soft_weights_and_a_weight_row_per_sample_pair(engine_lib, tiny):
    """Overlapping weights everywhere (no segment is skipped) and Bw = 2 under a batch of 4."""
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 4, 16, 16, R, seed=12)
    wts = ro.stripe_weights(2, R, 16, 16, soft=True, seed=3)
    got = net.set_regions(wts)(x.cuda(), 500.0, ehs.cuda())[0]
    ref = ro.forward(cfg, sd, x, torch.tensor(500.0), ehs, wts)
    assert rel_l2(got, ref) < TOL


@pytest.mark.parametrize("share", [True, False])
def test_forward_cfg_equals_the_duplicated_call(engine_lib, tiny, share):
    cfg, sd, net = tiny
    B = 2
    lat, _ = ro.unet_inputs(cfg, B, 16, 16, R, seed=13)
    _, ehs = ro.unet_inputs(cfg, 2 * B, 16, 16, R, seed=14)
    wts = regions.batch_weights(ro.stripe_weights(1, R, 16, 16)[0], B, True)          # uncond rows one-hot on region 0
    net.set_regions(wts)
    ed = ehs.cuda()
    two = net(torch.cat([lat, lat]).cuda(), 700.0, ed)[0]
    one = net.forward_cfg(lat.cuda(), 700.0, ed, share=share)[0]
    assert rel_l2(one, two) < 1e-3
    if not share:
        assert torch.equal(one, two)
    ref = ro.forward(cfg, sd, torch.cat([lat, lat]), torch.tensor(700.0), ehs, wts)
    assert rel_l2(one, ref) < TOL
    # the uncond rows attend the first segment only: up to the two kernels' rounding (the parity tolerance) they are the
    # plain forward on it
    net.clear_regions()
    plain = net(torch.cat([lat, lat]).cuda(), 700.0, ehs[:, :L].contiguous().cuda())[0]
    assert rel_l2(two[:B], plain[:B]) < TOL


def test_clearing_restores_the_plain_forward_bit_for_bit(engine_lib, tiny):
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, R, seed=15)
    xd, e1 = x.cuda(), ehs[:, :L].contiguous().cuda()
    before = net(xd, 300.0, e1)[0].clone()
    with_regions = net.set_regions(ro.stripe_weights(2, R, 16, 16))(xd, 300.0, ehs.cuda())[0].clone()
    held = net.memory()[1]
    net.clear_regions()
    # the caller's weights [2, 3, 16, 16] and the four levels [2, T_l, 3] were counted in the workspace and are released
    assert net.regions is None and held - net.memory()[1] == 4 * 2 * 3 * (256 + 256 + 64 + 16 + 4)
    after = net(xd, 300.0, e1)[0]
    assert torch.equal(before, after)
    assert not torch.equal(with_regions, after)
    # setting them again gives the regional result again, bit for bit
    again = net.set_regions(ro.stripe_weights(2, R, 16, 16))(xd, 300.0, ehs.cuda())[0]
    assert torch.equal(again, with_regions)


def test_poisoned_workspace_rebuilds_the_level_weights(engine_lib, tiny):
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, R, seed=16)
    xd, ed = x.cuda(), ehs.cuda()
    net.set_regions(ro.stripe_weights(2, R, 16, 16))
    want = net(xd, 300.0, ed)[0].clone()
    for pattern in (0, 1):
        assert net._poison_workspace(pattern) > 0
        assert torch.equal(net(xd, 300.0, ed)[0], want)


def test_text_kv_cache_is_bitwise_the_uncached_run(engine_lib, tiny):
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, R, seed=17)
    xs = [x.cuda(), (x * 0.5).cuda(), (x * -1.0).cuda()]
    ed = ehs.cuda()
    net.set_regions(ro.stripe_weights(2, R, 16, 16))
    want = [net(xi, 400.0 - 100 * i, ed)[0].clone() for i, xi in enumerate(xs)]
    net.text_kv_cache(True)
    got = [net(xi, 400.0 - 100 * i, ed)[0].clone() for i, xi in enumerate(xs)]
    net.text_kv_cache(False)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def _refused(net, code, fn):
    with pytest.raises(_lib.EngineError, match="error %d" % code):
        fn()


def test_invalid_calls_with_regions_set(engine_lib, tiny):
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, R, seed=18)
    xd, ed = x.cuda(), ehs.cuda()
    net.set_regions(ro.stripe_weights(2, R, 16, 16))
    out = torch.full((2, 4, 16, 16), 7.0, device="cuda", dtype=torch.float16)
    _refused(net, 1, lambda: net(xd, 1.0, ed[:, :R * L - 1].contiguous(), out=out))            # ehs_len % R != 0
    _refused(net, 1, lambda: net(xd[:1], 1.0, ed[:1]))                                         # N % Bw != 0
    _refused(net, 1, lambda: net(torch.zeros(2, 4, 8, 24, device="cuda", dtype=torch.float16), 1.0, ed))   # another H / W
    long = torch.zeros(2, R * 161, cfg.cross_attention_dim, device="cuda", dtype=torch.float16)
    _refused(net, 4, lambda: net(xd, 1.0, long, out=out))                                      # more than 160 tokens per region
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # set_regions itself
    w = torch.ones(1, 9, 16, 16, device="cuda")
    assert engine_lib.sd_unet_set_regions(net._h, P(w), 1, 9, 16, 16, stream()) == 4
    assert engine_lib.sd_unet_set_regions(net._h, P(w), 1, 3, 12, 16, stream()) == 1           # 12 % 8 != 0
    assert engine_lib.sd_unet_set_regions(net._h, P(w), 0, 3, 16, 16, stream()) == 1
    assert net(xd, 1.0, ed)[0].shape == (2, 4, 16, 16)                                         # the regions set before still hold


def test_unsupported_combinations_surface_as_errors(engine_lib, tiny):
    """Everything the forward refuses with regions set returns SD_ERR_UNSUPPORTED before a launch: the output buffer
    keeps its fill."""
    from cn_oracle import synth_cn_state_dict
    from ip_oracle import synth_ip_state_dict
    from stablediffusion_amd import controlnet
    from stablediffusion_amd.models import HipControlNetModel
    cfg, sd, net = tiny
    x, ehs = ro.unet_inputs(cfg, 2, 16, 16, R, seed=19)
    xd, ed = x.cuda(), ehs.cuda()
    wts = ro.stripe_weights(2, R, 16, 16)
    net.set_regions(wts)
    out = torch.full((2, 4, 16, 16), 7.0, device="cuda", dtype=torch.float16)
    run = lambda **kw: net(xd, 1.0, ed, out=out, **kw)  # noqa: E731
    # graph replay
    net.use_graph(True)
    try:
        _refused(net, 4, run)
    finally:
        net.use_graph(False)
    # token merging
    net.enable_tome(0.5)
    try:
        _refused(net, 4, run)
    finally:
        net.disable_tome()
    # a DeepCache store / reuse mode
    net.enable_deepcache(2, 1)
    try:
        net.deep_cache_mode(1)
        _refused(net, 4, run)
        net.deep_cache_mode(0)
        run()                                           # (DeepCache enabled but a plain step: the regional forward)
        out.fill_(7.0)
    finally:
        net.disable_deepcache()
    net.set_regions(wts)
    # forward_pag, forward_concat
    _refused(net, 4, lambda: net.forward_pag(xd[:1], 1.0, ed))
    rc = net._lib.sd_unet_forward_concat(net._h, P(xd), 2, 1.0, P(xd), 4, 2, 2, P(torch.ones(2, device="cuda")), P(ed),
                                         ed.shape[1], None, None, P(out), 2, 16, 16, stream())
    assert rc == 4, engine_lib.sd_last_error()
    # the shared and the duplicating forward_cfg refuse before they launch anything, too
    net.use_graph(True)
    try:
        for share in (True, False):
            _refused(net, 4, lambda: net.forward_cfg(xd[:1], 1.0, ed, share=share))
    finally:
        net.use_graph(False)
    # an IP-Adapter at a non-zero scale (at scale 0 the text attention runs alone: regions apply)
    ad = net.make_ip_adapter(synth_ip_state_dict(cfg, 64, 4, seed=5), 64, 4)
    net.attach_ip_adapter(ad)
    try:
        img = torch.zeros(2, 1, 64, device="cuda", dtype=torch.float16)
        _refused(net, 4, lambda: run(added_cond_kwargs={"image_embeds": [img]}))
        net.set_ip_adapter_scale(0.0)
        got = net(xd, 1.0, ed, added_cond_kwargs={"image_embeds": [img]})[0]
    finally:
        net.attach_ip_adapter(None)
        net.set_ip_adapter_scale(1.0)
    assert torch.equal(got, net(xd, 1.0, ed)[0])
    # an attached ControlNet
    ccfg = controlnet.encoder_config(cfg)
    cn = HipControlNetModel(net, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=4))
    net.attach_controlnet(cn)
    try:
        ctrl = torch.zeros(2, 3, 128, 128, device="cuda", dtype=torch.float16)
        _refused(net, 4, lambda: run(controlnet_cond=ctrl, controlnet_conditioning_scale=1.0))
    finally:
        net.attach_controlnet(None)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # timestep_cond (forward_tc) on a guidance-embedded UNet
    tcfg = config.tiny_unet(time_cond=32)
    tnet = HipUNet2DConditionModel(tcfg).load_state_dict(_sd(tcfg, 2))
    tnet.set_regions(wts)
    _refused(tnet, 4, lambda: tnet(xd, 1.0, ed, timestep_cond=torch.zeros(2, 32, device="cuda")))


def test_head_dims_outside_the_list_are_refused_when_set(engine_lib):
    """A UNet whose cross-attention runs at head dim 128 builds and runs, but takes no regions."""
    cfg = config.UNetConfig(sample_size=16, block_out_channels=(128, 256, 256, 256), cross_attention_dim=64,
                            attention_head_dim=(1, 2, 2, 2))
    net = HipUNet2DConditionModel(cfg).load_state_dict(_sd(cfg, 3))
    with pytest.raises(_lib.EngineError, match="error 4"):
        net.set_regions(torch.ones(1, 1, 16, 16))
    assert net.regions is None


# ---------------------------------------------------------------------------------------------------- the pipeline
@pytest.mark.parametrize("do_cfg", [True, False])
def test_tiny_pipeline_with_regions_matches_the_oracle_loop(engine_lib, do_cfg):
    """4-step DDIM through the pipeline at 16 x 16 latents against pipeline_ref.denoise_ref (CFG) or the same loop
    without guidance, both with the regional attention patched in."""
    from oracle import pipeline_ref
    from stablediffusion_amd.models import HipAutoencoderKL
    from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline
    from stablediffusion_amd.schedulers import DDIMScheduler
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _sd(ucfg, 11)
    vsd = {k: v.half().float() for k, v in weights.synth_state_dict(weights.vae_manifest(vcfg), 12, perturb=0.1).items()}
    base = HipUNet2DConditionModel(ucfg).load_state_dict(usd)
    model = SDModelWrapper(base=base, vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")
    model.set_scheduler("DDIM")
    g = torch.Generator().manual_seed(4)
    B = 2
    pos, neg, r1, r2 = ((torch.randn(B, L, ucfg.cross_attention_dim, generator=g) * s).half() for s in (2.0, 1.0, 2.0, 2.0))
    lat0 = torch.randn(B, 4, 16, 16, generator=g).half()
    masks = torch.zeros(2, 1, 128, 128)
    masks[0, :, :, :40] = 1.0                                # 5 latent columns: the coarser levels mix the regions
    masks[1, :, 72:, 88:] = 1.0
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    kw = dict(prompt_embeds=pos.cuda(), latents=lat0.cuda(), num_inference_steps=4, guidance_scale=5.0, height=128, width=128)
    if do_cfg:
        kw["negative_prompt_embeds"] = neg.cuda()
    got = pipe(model, region_prompt_embeds=[r1.cuda(), r2.cuda()], region_masks=masks, region_base_weight=0.1, **kw)
    assert base.regions is None                              # cleared after the loop
    plain = pipe(model, **kw)
    rw = regions.region_weights(masks, 16, 16, 0.1)
    wts = regions.batch_weights(rw, B, do_cfg)
    ehs_pos = torch.cat([pos, r1, r2], 1).float()
    with ro.patched():
        if do_cfg:
            ehs = torch.cat([torch.cat([neg] * 3, 1).float(), ehs_pos])
            ref = pipeline_ref.denoise_ref(ucfg, usd, lat0.float(), (ehs, wts), steps=4, guidance_scale=5.0, scheduler="DDIM")
        else:
            sch = pipeline_ref.SCHEDULERS["DDIM"]()
            xs = lat0.double().numpy() * sch.init_noise_sigma
            for t in sch.set_timesteps(4):
                with torch.no_grad():
                    eps = unet_ref.unet_forward(ucfg, usd, torch.from_numpy(sch.scale_model_input(xs, t)).float(),
                                                torch.tensor(float(t)), (ehs_pos, wts)).double().numpy()
                xs = sch.step(eps, t, xs)
            ref = torch.from_numpy(xs).float()
    assert torch.isfinite(got.float()).all()
    err, dist = rel_l2(got, ref), rel_l2(got, plain)
    print("pipeline cfg=%s: vs the oracle loop %.2e, vs the call without regions %.3f" % (do_cfg, err, dist))
    assert err < TOL
    assert dist > FAR


# ---------------------------------------------------------------------------------------------------- full width
@pytest.fixture()
def _true_fp32():
    old = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old


def _oracle_on_gpu(cfg, sd16, x, t, ehs, wts, added=None):
    w = {k: v.float().cuda() for k, v in sd16.items()}
    orig = unet_ref.timestep_sinusoid
    unet_ref.timestep_sinusoid = lambda tt, *a, **k: orig(tt.cpu(), *a, **k).cuda()
    try:
        with ro.patched(), torch.no_grad():
            add = {k: v.float().cuda() for k, v in added.items()} if added else None
            kw = {"added_cond_kwargs": add} if add else {}
            return unet_ref.unet_forward(cfg, w, x.float().cuda(), t, (ehs.float().cuda(), wts.float().cuda()), **kw)
    finally:
        unet_ref.timestep_sinusoid = orig


@pytest.mark.parametrize("preset,B", [("sd15", 2), ("sdxl", 1)])
def test_full_width_forward_cfg_with_regions(engine_lib, _true_fp32, preset, B):
    """SD1.5 (head dims 40 / 80 / 160: the grouped form at the two deepest levels) with 2 latents and SDXL (head dim 64)
    with 1, 32 x 32 latents, R = 3, through forward_cfg, against the fp32 oracle evaluated on the GPU."""
    cfg = config.sd15_unet() if preset == "sd15" else config.sdxl_unet()
    sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=41, dtype=torch.float16, perturb=0.1)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    g = torch.Generator().manual_seed(32 + B)
    lat = torch.randn(B, 4, 32, 32, generator=g).half()
    ehs = (torch.randn(2 * B, R * L, cfg.cross_attention_dim, generator=g) * 2).half()
    wts = regions.batch_weights(ro.stripe_weights(1, R, 32, 32)[0], B, True)
    added = None
    if preset == "sdxl":
        added = {"text_embeds": torch.randn(2 * B, 1280, generator=g).half(),
                 "time_ids": torch.tensor([[256.0, 256, 0, 0, 256, 256]] * (2 * B))}
    net.set_regions(wts)
    got = net.forward_cfg(lat.cuda(), 501.0, ehs.cuda(),
                          added_cond_kwargs=None if added is None else {k: v.cuda() for k, v in added.items()})[0]
    net.clear_regions()
    ref = _oracle_on_gpu(cfg, sd, torch.cat([lat, lat]), torch.tensor(501.0), ehs, wts, added)
    err = rel_l2(got, ref)
    print("%s: rel-L2 %.2e" % (preset, err))
    assert torch.isfinite(got.float()).all()
    assert err < TOL
