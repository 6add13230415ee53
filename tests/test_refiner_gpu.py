"""SDXL refiner on the device: the one-launch text_time input kernel bit for bit, the five-id forward against the fp32
CPU oracle (rel-L2 < 1e-2, the project's model tolerance) eager and graph-replayed, the operators at the refiner's
widths (384 / 768 / 1536: GroupNorm groups of 12 / 24 / 48 channels, 24 LayerNorm column parts), and the pipeline's
use_refiner / refiner_start paths on the engine."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_norm_stats_gpu as norm_stats
import test_ops_gpu as ops
from conftest import rel_l2
from oracle import unet_ref
from refiner_doubles import StubTextEncoder, StubTokenizer
from stablediffusion_amd import config, weights
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

pytestmark = pytest.mark.gpu
TOL = 1e-2
P, stream, h = ops.P, ops.stream, ops.h


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


def _synth(cfg, seed):
    return _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=seed, perturb=0.1))


# ------------------------------------------------------------------------------------------------ kernel
ID_VALUES = [1024.0, 0.0, 2.5, 6.0, 128.0, 980.9999, 1.0, 512.5]


@pytest.mark.parametrize("flip,shift", [(1, 0.0), (0, 1.0)])
@pytest.mark.parametrize("Pw,ad,n", [(64, 32, 5), (64, 32, 6), (1280, 256, 5), (1280, 256, 6), (64, 2, 1), (64, 32, 8)])
@pytest.mark.parametrize("B", [1, 3])
def test_text_time_input_is_the_composition_bit_for_bit(engine_lib, B, Pw, ad, n, flip, shift):
    """sd_op_text_time_input == exact f16 -> f32 copy of the pooled text | sd_op_timestep_sinusoid per id column, bitwise;
    sentinel rows in front of and behind `out` stay untouched."""
    g = torch.Generator().manual_seed(B * 1000 + Pw + ad + n)
    text = torch.randn(B, Pw, generator=g).half().cuda()
    ids = torch.tensor([[ID_VALUES[(b * 3 + j) % len(ID_VALUES)] for j in range(n)] for b in range(B)]).cuda()
    assert {0.0, 1024.0, 2.5, 6.0} <= set(ids.flatten().tolist()) or B * n < 4
    width = Pw + n * ad
    want = torch.empty(B, width, device="cuda")
    want[:, :Pw] = text.float()
    for j in range(n):
        col = ids[:, j].contiguous()
        part = torch.zeros(B, ad, device="cuda")
        assert engine_lib.sd_op_timestep_sinusoid(P(col), P(part), B, ad, flip, shift, stream()) == 0
        want[:, Pw + j * ad: Pw + (j + 1) * ad] = part
    SENT = 12345.0
    buf = torch.full((B + 2, width), SENT, device="cuda")
    out = buf[1:B + 1]
    rc = engine_lib.sd_op_text_time_input(P(text), P(ids), C.c_void_p(out.data_ptr()), B, Pw, ad, n, flip, shift, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert (buf[0] == SENT).all() and (buf[B + 1] == SENT).all()


def test_text_time_input_invalid_arguments_launch_nothing(engine_lib):
    text = torch.zeros(2, 64, dtype=torch.float16, device="cuda")
    ids = torch.zeros(2, 8, device="cuda")
    out = torch.full((2, 64 + 8 * 32), 7.0, device="cuda")
    for Pw, ad, n in ((64, 32, 0), (64, 32, 9), (64, 31, 5), (0, 32, 5), (-1, 32, 5)):
        assert engine_lib.sd_op_text_time_input(P(text), P(ids), P(out), 2, Pw, ad, n, 1, 0.0, stream()) == 1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ forward
def _refiner_inputs(cfg, seed, pooled):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, 16, 16, generator=g).half()
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half()
    added = {"text_embeds": torch.randn(2, pooled, generator=g).half(),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 6.0], [128.0, 128, 0, 0, 2.5]])}
    return x, ehs, added


def _oracle(cfg, sd, x, t, ehs, added):
    with torch.no_grad():
        return unet_ref.unet_forward(cfg, sd, x.float(), torch.tensor(t), ehs.float(),
                                     {"text_embeds": added["text_embeds"].float(), "time_ids": added["time_ids"]})


def test_tiny_refiner_forward_eager_and_graph(engine_lib):
    """(a) the refiner topology with five time ids, whose two rows differ in the score column: against the oracle, and the
    graph replay (staging copy of [B, 5] ids) bitwise the eager result.  A [B, 6] id tensor is refused."""
    cfg = config.tiny_refiner_unet()
    sd = _synth(cfg, 21)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    x, ehs, added = _refiner_inputs(cfg, 9, 64)
    ref = _oracle(cfg, sd, x, 741.0, ehs, added)
    eager = net(x.cuda(), torch.tensor(741.0), ehs.cuda(), added_cond_kwargs=added)[0]
    err = rel_l2(eager, ref)
    print("tiny refiner rel-L2 %.3e" % err)
    assert eager.shape == ref.shape and err < TOL
    # the score column reaches the output: swapping the two rows' ids changes it
    swapped = dict(added, time_ids=added["time_ids"].flip(0))
    assert not torch.equal(net(x.cuda(), torch.tensor(741.0), ehs.cuda(), added_cond_kwargs=swapped)[0], eager)
    with pytest.raises(ValueError, match="time_ids"):
        net(x.cuda(), torch.tensor(741.0), ehs.cuda(),
            added_cond_kwargs=dict(added, time_ids=torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)))
    with pytest.raises(ValueError, match="time_ids"):
        net.forward_cfg(x[:1].cuda(), 741.0, ehs.cuda(),
                        added_cond_kwargs=dict(added, time_ids=torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)))
    net.use_graph(True)
    try:
        first = net(x.cuda(), torch.tensor(741.0), ehs.cuda(), added_cond_kwargs=added)[0]      # captures
        replay = net(x.cuda(), torch.tensor(741.0), ehs.cuda(), added_cond_kwargs=added)[0]     # replays
    finally:
        net.use_graph(False)
    assert torch.equal(first, eager) and torch.equal(replay, eager)


def test_tiny_refiner_forward_cfg_takes_the_duplicate_path(engine_lib):
    """forward_cfg with text_time conditioning: 2B rows of five ids, bitwise the duplicate-then-forward result."""
    cfg = config.tiny_refiner_unet()
    net = HipUNet2DConditionModel(cfg).load_state_dict(_synth(cfg, 21))
    x, ehs, added = _refiner_inputs(cfg, 10, 64)
    lat = x[:1].cuda()
    two = net(torch.cat([lat, lat]), torch.tensor(301.0), ehs.cuda(), added_cond_kwargs=added)[0]
    one = net.forward_cfg(lat, 301.0, ehs.cuda(), added_cond_kwargs=added, in_scale=1.0)[0]
    assert torch.equal(one, two)


def test_refiner_widths_forward(engine_lib):
    """(b) 384 / 768 / 1536 channels (groups of 12 / 24 / 48, head dim 64) on three blocks of depth 1."""
    cfg = config.UNetConfig(
        sample_size=16, down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
        up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), block_out_channels=(384, 768, 1536),
        layers_per_block=1, cross_attention_dim=128, attention_head_dim=(6, 12, 24), transformer_layers_per_block=(1, 1, 1),
        use_linear_projection=True, addition_embed_type="text_time", addition_time_embed_dim=32,
        projection_class_embeddings_input_dim=5 * 32 + 128, pooled_projection_dim=128)
    assert cfg.num_time_ids == 5
    sd = _synth(cfg, 22)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    x, ehs, added = _refiner_inputs(cfg, 11, 128)
    ref = _oracle(cfg, sd, x, 501.0, ehs, added)
    got = net(x.cuda(), torch.tensor(501.0), ehs.cuda(), added_cond_kwargs=added)[0]
    err = rel_l2(got, ref)
    print("refiner widths rel-L2 %.3e" % err)
    assert torch.isfinite(got.float()).all() and err < TOL


# ------------------------------------------------------------------------------------------------ operators, new widths
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("Cc", [384, 768, 1536])
def test_groupnorm_at_refiner_widths(engine_lib, Cc, silu):
    """Groups of 12 / 24 / 48 channels around a mean of 100 (float64 reference, test_groupnorm's tolerance)."""
    N, HW = 2, 64
    g = torch.Generator().manual_seed(Cc + silu)
    x = (torch.randn(N, HW, Cc, generator=g) * 1.5 + 0.7 + 100.0).half()
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    ref = F.group_norm(x.double().permute(0, 2, 1).contiguous(), 32, gamma.double(), beta.double(), 1e-5)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1).float()
    y = torch.empty(N, HW, Cc, dtype=torch.float16, device="cuda")
    xd, gd, bd = h(x), gamma.cuda(), beta.cuda()
    rc = engine_lib.sd_op_groupnorm(P(xd), P(gd), P(bd), P(y), N, HW, Cc, 32, 1e-5, silu, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    err = rel_l2(y, ref)
    print("groupnorm C=%d silu=%d rel-L2 %.3e" % (Cc, silu, err))
    assert err < 1.5e-3


@pytest.mark.parametrize("Ca,Cb", [(1536, 1536), (1536, 768), (768, 768), (768, 384), (384, 384)])
def test_groupnorm_concat_at_refiner_widths(engine_lib, Ca, Cb):
    """The up path's norm1 over cat([hidden, skip]) at the refiner's seams (groups of 96 / 72 / 48 / 36 / 24 channels;
    (1536, 768) and (768, 384) have groups that straddle the seam): test_groupnorm_of_a_concatenation's data and
    tolerances, float64 reference."""
    N, HW, G = 2, 256, 32
    Cc = Ca + Cb
    g = torch.Generator().manual_seed(HW + Ca + Cb)
    x = torch.randn(N, HW, Cc, generator=g) * (0.5 + torch.rand(1, 1, Cc, generator=g) * 2) + torch.randn(1, 1, Cc, generator=g) * 3
    x[..., Ca:] += 5.0
    x = x.half()
    gamma = 1 + 0.2 * torch.randn(Cc, generator=g)
    beta = 0.2 * torch.randn(Cc, generator=g)
    ref = F.silu(F.group_norm(x.double().permute(0, 2, 1).contiguous(), G, gamma.double(), beta.double(), 1e-5))
    ref = ref.permute(0, 2, 1).float()
    xd, gd, bd = h(x), gamma.cuda(), beta.cuda()
    y = torch.zeros_like(xd)
    rc = engine_lib.sd_op_groupnorm_concat(P(xd), Ca, Cb, P(gd), P(bd), P(y), N, HW, G, 1e-5, 1, stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    err = rel_l2(y, ref)
    print("groupnorm_concat (%d, %d) rel-L2 %.3e" % (Ca, Cb, err))
    assert err < 1e-3, err
    assert (y.float().cpu() - ref).abs().max() < 2e-2


@pytest.mark.parametrize("offset", [None, 50.0])
def test_conv_groupnorm_384(engine_lib, offset):
    """conv 384 -> 384 3x3 followed by GroupNorm over groups of 12 (which no 128- or 160-column epilogue can summarise):
    test_ops_gpu's conv -> GroupNorm case, its references and tolerances."""
    ops._conv_groupnorm_case(engine_lib, (2, 16, 16, 384, 384, 3, 1, 0, True, None), offset)


@pytest.mark.parametrize("xs,xsh", [(1.0, 0.0), (0.1, 50.0)])
def test_groupnorm_conv_384(engine_lib, xs, xsh):
    """GroupNorm (groups of 12) -> SiLU -> conv 384 -> 384 3x3 with bias, row add and residual: test_groupnorm_conv2d's
    operands, reference and tolerances; whether the norm ran inside the convolution is reported, not required."""
    N, H, W, Cin, Cout, G = 2, 16, 16, 384, 384, 32
    g = torch.Generator().manual_seed(Cin + int(xsh))
    x = (torch.randn(N, Cin, H, W, generator=g) * xs + xsh + 0.3 * torch.randn(1, Cin, 1, 1, generator=g)).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half()
    gamma = 1.0 + 0.3 * torch.randn(Cin, generator=g)
    beta = 0.3 * torch.randn(Cin, generator=g)
    bias = torch.randn(Cout, generator=g) * 0.5
    rowadd = torch.randn(N, Cout, generator=g) * 0.5
    hn = F.silu(F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-5)).float()
    ref = F.conv2d(hn, w.float(), bias, padding=1) + rowadd[:, :, None, None]
    res = torch.randn(ref.shape, generator=g).half()
    ref = ref.half().float() + res.float()
    y = torch.empty(N, H, W, Cout, dtype=torch.float16, device="cuda")
    xd, wd, bd, rd = h(x.permute(0, 2, 3, 1)), h(w), bias.cuda(), rowadd.cuda().contiguous()
    resd, gd, btd = h(res.permute(0, 2, 3, 1)), gamma.cuda(), beta.cuda()
    fused = C.c_int(-1)
    rc = engine_lib.sd_op_groupnorm_conv2d(P(xd), P(gd), P(btd), G, 1e-5, 1, P(wd), P(bd), P(rd), P(resd), P(y), N, H, W,
                                           Cin, Cout, 3, 0, None, C.byref(fused), stream())
    assert rc == 0, engine_lib.sd_last_error()
    torch.cuda.synchronize()
    out = y.float().cpu().permute(0, 3, 1, 2)
    err = rel_l2(out, ref)
    print("GN->conv 384 shift %g: norm inside the conv %d, rel-L2 %.3e" % (xsh, fused.value, err))
    assert err < 3e-3, err
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    assert rel_l2(out[:, :, ring], ref[:, :, ring]) < 4e-3


@pytest.mark.parametrize("profile", ["normal", "offset:50"])
@pytest.mark.parametrize("site", ["q2", "qkv"])
def test_layernorm_fold_at_1536(engine_lib, site, profile):
    """linear + row statistics -> LayerNorm folded into the next linear at C = 1536, M = 128: behind 64-column tiles the row
    would have 24 parts, more than a consumer reads (20), so the planner must hand at most 20 on (or run the stand-alone
    row statistics: one part).  test_norm_stats_gpu's chain, references and tolerances."""
    y1, stat, y2, info, once = norm_stats._run_chain(engine_lib, (128, 1536, 1536, True, site, None, None), profile)
    assert 1 <= info[2] <= 20, info
    y1b, statb, y2b, infob = once()
    assert infob == info and torch.equal(y2, y2b)


# ------------------------------------------------------------------------------------------------ pipeline
def tiny_sdxl_base():
    return config.UNetConfig(**dict(config.tiny_unet(linear=True, sdxl_cond=True).to_dict(), cross_attention_dim=128))


@pytest.fixture(scope="module")
def sdxl_pair():
    bcfg, rcfg, vcfg = tiny_sdxl_base(), config.tiny_refiner_unet(), config.tiny_vae()
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    return SDModelWrapper(base=HipUNet2DConditionModel(bcfg).load_state_dict(_synth(bcfg, 31)),
                          refiner=HipUNet2DConditionModel(rcfg).load_state_dict(_synth(rcfg, 32)),
                          vae=HipAutoencoderKL(vcfg).load_state_dict(vsd),
                          text_encoder=StubTextEncoder(64, 64, 1).to("cuda"), tokenizer=StubTokenizer(),
                          text_encoder_2=StubTextEncoder(64, 64, 2).to("cuda"), tokenizer_2=StubTokenizer(),
                          model_type="sdxl", device="cuda")


@pytest.mark.parametrize("sched", ["DDIM", "euler", "DPM++ 2M"])
def test_refiner_start_is_the_two_call_composition(engine_lib, sdxl_pair, sched):
    model = sdxl_pair
    model.set_scheduler(sched)
    kw = dict(prompt=["a cat", "a dog"], negative_prompt="blurry", num_inference_steps=5, guidance_scale=5.0, seed=3)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    one = pipe(model, refiner_start=0.6, **kw)
    assert one.is_cuda and one.shape == (2, 4, 16, 16) and torch.isfinite(one.float()).all()
    assert pipe._fused_step_available(model, one)
    a = pipe(model, denoising_end=0.6, **kw)
    b = pipe(model, use_refiner=True, image=a, denoising_start=0.6, **kw)
    assert torch.equal(one, b)
    assert not torch.equal(b, a)
    # the same loop with scheduler.scale_model_input / .step on the host
    host_pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    host_pipe._fused_step_available = lambda *a: False
    host = host_pipe(model, refiner_start=0.6, **kw)
    err = rel_l2(one, host)
    print("refiner_start %s: device step vs host loop rel-L2 %.3e" % (sched, err))
    assert err < 3e-3


def test_use_refiner_on_latents_differs_from_the_base(engine_lib, sdxl_pair):
    model = sdxl_pair
    model.set_scheduler("euler")
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 4, 16, 16, generator=g).half().cuda()
    kw = dict(prompt="a cat", negative_prompt="blurry", num_inference_steps=4, guidance_scale=5.0, seed=3, image=lat,
              strength=0.5)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    refined = pipe(model, use_refiner=True, **kw)
    based = pipe(model, **kw)
    assert refined.shape == based.shape == (1, 4, 16, 16)
    assert torch.isfinite(refined.float()).all() and not torch.equal(refined, based)
    # decoded output comes through the same VAE
    img = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda")(model, use_refiner=True, **kw)
    assert img.shape == (1, 3, 128, 128) and torch.isfinite(img.float()).all()
