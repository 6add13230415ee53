"""MultiDiffusion on the GPU: sd_views_gather against indexing, sd_views_merge against the float64 merge of the same fp16
values (tests/views_oracle.py: the cases, the reference and the bound, which tests/test_views.py checks on the CPU), the
exact cases, the refusals, and the pipeline's windowed device loops against the same loops on scheduler.step."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402
import views_oracle as vo  # noqa: E402
from test_sched_step_gpu import LOOP_TOL  # noqa: E402
from stablediffusion_amd import config, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402
from stablediffusion_amd.schedulers import DDIMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on either side of every output


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr())


def ints(v):
    return (C.c_int * len(v))(*v)


def guarded(n, dtype, fill, shift=0):
    """A buffer of n elements between two guards of `fill`; `shift` moves it off the 16-byte alignment."""
    buf = torch.full((GUARD + shift + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n]


def guards_intact(buf, n, fill, shift=0):
    return bool((buf[:GUARD + shift] == fill).all() and (buf[GUARD + shift + n:] == fill).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


class _with_batch:
    """A plan plus the canvas's shape, so that `gather` can take a flat, guarded view of the canvas."""

    def __init__(self, plan, canvas):
        self.__dict__.update(plan.__dict__)
        self.shape = canvas.shape


def gather(lib, canvas, plan, out):
    B, Cc = plan.shape[:2]
    return lib.sd_views_gather(P(canvas), P(out), B, Cc, plan.Hc, plan.Wc, plan.h, plan.w, ints(plan.ys), len(plan.ys),
                               ints(plan.xs), len(plan.xs), int(plan.wrap), stream())


def merge(lib, buf, out, wt, plan, G, B, vpc):
    return lib.sd_views_merge(P(buf), P(out), P(wt) if wt is not None else None, G, B, vo.KERNEL_CHANNELS, plan.Hc, plan.Wc,
                              plan.h, plan.w, ints(plan.ys), len(plan.ys), ints(plan.xs), len(plan.xs), int(plan.wrap), vpc,
                              stream())


# ------------------------------------------------------------------------------------------------ the gather
@pytest.mark.parametrize("shape", vo.KERNEL_SHAPES)
def test_gather_is_indexing(engine_lib, shape):
    """Bit-identical to indexing, nothing outside `windows` written; the vector shapes also run one element off the
    16-byte alignment (the scalar kernel on a shape the vector kernel takes)."""
    plan = vo.kernel_plan(shape)
    V = len(plan.views())
    for B in vo.KERNEL_BATCHES:
        g = torch.Generator().manual_seed(B)
        canvas = torch.randn(B, vo.KERNEL_CHANNELS, plan.Hc, plan.Wc, generator=g).half()
        want = torch.cat([plan.cut(canvas, y, x) for y, x in plan.views()])
        for shift in (0, 1):
            src_buf, src = guarded(canvas.numel(), torch.float16, 7.0, shift)
            src.copy_(canvas.reshape(-1))
            n = V * B * vo.KERNEL_CHANNELS * plan.h * plan.w
            buf, out = guarded(n, torch.float16, -3.0, shift)
            assert gather(engine_lib, src, _with_batch(plan, canvas), out) == 0, engine_lib.sd_last_error()
            torch.cuda.synchronize()
            assert same_bits(out.cpu(), want.reshape(-1)), (shape, B, shift)
            assert guards_intact(buf, n, -3.0, shift) and same_bits(src.cpu(), canvas.reshape(-1))


# ------------------------------------------------------------------------------------------------ the merge
@pytest.mark.parametrize("shape", vo.KERNEL_SHAPES)
def test_merge_is_the_weighted_mean(engine_lib, shape):
    """Every element within 2^-11 |O| + (2 n + 5) 2^-24 A + 2^-25 of the float64 merge O of the same fp16 values (n covering
    views, A the weighted mean of |e|; views_oracle.merge_bound).  Per-view magnitudes from {1e-3, 1, 30}; weights NULL,
    Gaussian, random in [0.05, 1]; G in {1, 2, 3}, B in {1, 2}, views_per_chunk in {1, 3, V}.  The buffer's rows behind
    the last chunk are NaN and the output stays finite; the guards around eps_out and the inputs are unchanged."""
    plan = vo.kernel_plan(shape)
    V, Cc = len(plan.views()), vo.KERNEL_CHANNELS
    worst = 0.0
    for G in vo.KERNEL_GROUPS:
        for B in vo.KERNEL_BATCHES:
            outs = vo.view_outputs(plan, G, B, seed=10 * G + B)
            for kind in ("none", "gaussian", "random"):
                wt = vo.kernel_weights(kind, plan.h, plan.w)
                wt_d = wt.cuda() if wt is not None else None
                O, A, n = vo.merge_reference(outs, plan, wt)
                bound = vo.merge_bound(O, A, n)
                for vpc in sorted({1, min(3, V), V}):
                    host = vo.chunked_buffer(outs, vpc)
                    tail = 2 * B * Cc * plan.h * plan.w                      # two more rows' worth of NaN behind the chunks
                    src = torch.full((host.numel() + tail,), float("nan"), dtype=torch.float16, device="cuda")
                    src[:host.numel()] = host.reshape(-1).cuda()
                    ne = G * B * Cc * plan.Hc * plan.Wc
                    buf, out = guarded(ne, torch.float16, -3.0)
                    assert merge(engine_lib, src, out, wt_d, plan, G, B, vpc) == 0, engine_lib.sd_last_error()
                    torch.cuda.synchronize()
                    got = out.cpu().reshape(O.shape)
                    assert torch.isfinite(got.float()).all(), (shape, G, B, kind, vpc)
                    err = (got.double() - O).abs()
                    worst = max(worst, (err / bound).max().item())
                    assert (err <= bound).all(), (shape, G, B, kind, vpc, (err / bound).max().item())
                    assert guards_intact(buf, ne, -3.0)
                    assert same_bits(src[:host.numel()].cpu(), host.reshape(-1)) and torch.isnan(src[host.numel():]).all()
    print(f"views merge {shape}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("shape", vo.KERNEL_SHAPES)
def test_uniform_merge_of_gathered_windows_is_the_canvas(engine_lib, shape):
    """merge(gather(x)) == x bit for bit with NULL weights, for every chunking (G = 1: the windows are the outputs); with
    one view both kernels are copies."""
    plan = vo.kernel_plan(shape)
    V, B, Cc = len(plan.views()), 2, vo.KERNEL_CHANNELS
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, Cc, plan.Hc, plan.Wc, generator=g).half()
    x[0, 0, 0, :8] = torch.tensor([6e-8, -6e-8, 65504.0, -65504.0, 0.0, 1e-5, 3.0, -0.333]).half()
    xd = x.cuda()
    windows = torch.empty(V * B, Cc, plan.h, plan.w, dtype=torch.float16, device="cuda")
    assert gather(engine_lib, xd, _with_batch(plan, x), windows) == 0, engine_lib.sd_last_error()
    if V == 1:
        assert same_bits(windows.cpu(), x)
    # G = 1: rows [chunk][view in chunk][b] are the windows' own order whatever the chunking
    for vpc in sorted({1, min(3, V), V}):
        buf, out = guarded(x.numel(), torch.float16, -3.0)
        assert merge(engine_lib, windows, out, None, plan, 1, B, vpc) == 0, engine_lib.sd_last_error()
        torch.cuda.synchronize()
        assert same_bits(out.cpu().reshape(x.shape), x), (shape, vpc)
        assert guards_intact(buf, x.numel(), -3.0)


# ------------------------------------------------------------------------------------------------ refusals
def test_invalid_calls_launch_nothing(engine_lib):
    canvas = torch.randn(2, 4, 24, 40).half().cuda()
    outs = torch.randn(2 * 8, 4, 16, 16).half().cuda()
    n = 2 * 8 * 4 * 16 * 16
    buf, out = guarded(n, torch.float16, -3.0)
    for label, entry, args in vo.invalid_view_calls():
        src = canvas if entry == "sd_views_gather" else outs
        rc = vo.call_view_entry(engine_lib, entry, args, (src.data_ptr(), out.data_ptr()), stream())
        assert rc == 1, label
        assert entry.encode() in engine_lib.sd_last_error(), label
    torch.cuda.synchronize()
    assert (buf == -3.0).all()
    # ... and the same buffers are fine with the valid call the table varies
    base = dict(canvas=1, out=1, G=2, B=1, C=4, Hc=24, Wc=40, h=16, w=16, ys=[0, 8], xs=[0, 8, 16, 24], wrap=0, vpc=3)
    for entry, src in (("sd_views_gather", canvas), ("sd_views_merge", outs)):
        assert vo.call_view_entry(engine_lib, entry, base, (src.data_ptr(), out.data_ptr()), stream()) == 0
        torch.cuda.synchronize()
        assert not (out == -3.0).all() and guards_intact(buf, n, -3.0)
        out.fill_(-3.0)


# ------------------------------------------------------------------------------------------------ loops
def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def model():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vsd = _f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12))
    return SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd),
                          vae=HipAutoencoderKL(vcfg).load_state_dict(vsd), scheduler=DDIMScheduler(), device="cuda")


def _inputs(B=2, seed=3, L=7):
    g = torch.Generator().manual_seed(seed)
    d = config.tiny_unet().cross_attention_dim
    return dict(pos=torch.randn(B, L, d, generator=g).half().cuda(), neg=torch.randn(B, L, d, generator=g).half().cuda(),
                lat=torch.randn(B, 4, 24, 40, generator=g).half().cuda())


VIEWS = dict(view_window=16, view_stride=8, view_batch_size=3)
FORWARDS = ("sd_unet_forward", "sd_unet_forward_ex", "sd_unet_forward_tc", "sd_unet_forward_cfg", "sd_unet_forward_cn",
            "sd_unet_forward_pag", "sd_unet_forward_concat")
STEPS = ("sd_cfg_linear_step", "sd_cfg_rescale_linear_step", "sd_lcm_step", "sd_sched_affine_step", "sd_pag_linear_step",
         "sd_ip2p_linear_step")


class CountingLib:
    """The engine library with every call counted by name (the UNet shim and the pipeline reach it through `unet._lib`)."""

    def __init__(self, lib):
        self._real, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted

    def count(self, names):
        names = (names,) if isinstance(names, str) else names
        return sum(1 for c in self.calls if c in names)

    def steps(self):
        return [c for c in self.calls if c in STEPS]


def _call(model, inp, do_cfg=True, host=False, steps=3, spy=None, **kw):
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    if host:
        pipe._device_step_kind = lambda *a: None
    emb = dict(prompt_embeds=inp["pos"], negative_prompt_embeds=inp["neg"]) if do_cfg else dict(prompt_embeds=inp["pos"])
    kw.setdefault("latents", inp["lat"])
    real = model.base._lib
    if spy is not None:
        model.base._lib = spy
    try:
        torch.manual_seed(3)
        return pipe(model, num_inference_steps=steps, guidance_scale=5.0, height=192, width=320, seed=7, **emb, **kw)
    finally:
        model.base._lib = real


@pytest.mark.parametrize("name", ["DDIM", "euler", "PNDM", "lcm"])
def test_windowed_device_loop_equals_the_host_loop(engine_lib, model, name):
    """B = 2, canvas 24 x 40, window 16, stride 8 (8 views), view_batch_size 3 (chunks 3, 3, 2), 3 steps: the device loop
    against the same call on scheduler.step; per iteration one gather, three forwards, one merge and the step entry the
    call without views takes; and the windows are live."""
    model.set_scheduler(name)
    inp = _inputs()
    iters = 4 if name == "PNDM" else 3
    spy = CountingLib(model.base._lib)
    dev = _call(model, inp, spy=spy, **VIEWS)
    plain_spy = CountingLib(model.base._lib)
    plain = _call(model, inp, spy=plain_spy)
    assert spy.count("sd_views_gather") == iters and spy.count("sd_views_merge") == iters, spy.calls
    assert spy.count(FORWARDS) == 3 * iters and spy.count("sd_unet_forward_cfg") == 3 * iters
    assert plain_spy.count(FORWARDS) == iters and plain_spy.count(("sd_views_gather", "sd_views_merge")) == 0
    assert spy.steps() == plain_spy.steps() and len(spy.steps()) == iters, (spy.steps(), plain_spy.steps())
    per_iter = [c for c in spy.calls if c in FORWARDS + STEPS + ("sd_views_gather", "sd_views_merge")]
    assert per_iter[:6] == ["sd_views_gather"] + ["sd_unet_forward_cfg"] * 3 + ["sd_views_merge", spy.steps()[0]]
    host = _call(model, inp, host=True, **VIEWS)
    e = rel_l2(dev, host)
    print(f"views loop {name}: device vs host rel-L2 {e:.2e}")
    assert tuple(dev.shape) == (2, 4, 24, 40) and torch.isfinite(dev.float()).all() and e < LOOP_TOL
    wide = _call(model, inp, **dict(VIEWS, view_stride=16))
    apart, apart16 = rel_l2(dev, plain), rel_l2(dev, wide)
    print(f"views loop {name}: {apart:.2e} from the plain call, {apart16:.2e} from stride 16")
    assert apart > 10 * LOOP_TOL and apart16 > 10 * LOOP_TOL


@pytest.mark.parametrize("name", ["DDIM", "PNDM"])
def test_a_window_of_the_canvas_is_the_plain_call(engine_lib, model, name):
    model.set_scheduler(name)
    inp = _inputs()
    plain = _call(model, inp)
    assert torch.equal(_call(model, inp, view_window=(24, 40), view_stride=8), plain)
    assert torch.equal(_call(model, inp, view_window=64), plain)               # clamped to the canvas


def test_windowed_loop_without_cfg(engine_lib, model):
    model.set_scheduler("euler_a")
    inp = _inputs()
    spy = CountingLib(model.base._lib)
    dev = _call(model, inp, do_cfg=False, spy=spy, **VIEWS)
    assert spy.count("sd_unet_forward") == 9 and spy.count(FORWARDS) == 9 and spy.steps() == ["sd_sched_affine_step"] * 3
    host = _call(model, inp, do_cfg=False, host=True, **VIEWS)
    e = rel_l2(dev, host)
    print(f"views loop euler_a without CFG: device vs host rel-L2 {e:.2e}")
    assert torch.isfinite(dev.float()).all() and e < LOOP_TOL


def test_windowed_loop_inpaint_4_channels(engine_lib, model):
    model.set_scheduler("DDIM")
    inp = _inputs(B=1, seed=4)
    g = torch.Generator().manual_seed(5)
    image = torch.randn(1, 4, 24, 40, generator=g).half().cuda()              # the image as latents: nothing is sampled
    mask = torch.zeros(1, 1, 192, 320)
    mask[:, :, :, 160:] = 1.0
    kw = dict(image=image, mask_image=mask.cuda(), **VIEWS)
    spy = CountingLib(model.base._lib)
    dev = _call(model, inp, spy=spy, **kw)
    assert spy.count("sd_inpaint_blend") == 3 and spy.count("sd_views_merge") == 3
    host = _call(model, inp, host=True, **kw)
    e = rel_l2(dev, host)
    print(f"views loop DDIM 4-channel inpainting: device vs host rel-L2 {e:.2e}")
    assert torch.isfinite(dev.float()).all() and e < LOOP_TOL
    assert torch.equal(dev[..., :20], image[..., :20])                         # outside the mask: the image's latents
    assert not torch.allclose(dev[..., 20:].float(), image[..., 20:].float(), atol=1e-2)
