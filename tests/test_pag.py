"""Perturbed-attention guidance without a GPU: layer names, the per-step scale, the host loop on test doubles, the
refused combinations, and the new C entries' presence and argument validation."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from stablediffusion_amd import _lib, config, pag, schedulers
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sd_unet_set_pag_layers", "sd_unet_forward_pag", "sd_pag_linear_step", "sd_pag_combine")


# ------------------------------------------------------------------------------------------------ layer names
def _down(i, js):
    return tuple(f"down_blocks.{i}.attentions.{j}" for j in js)


def _up(i, js):
    return tuple(f"up_blocks.{i}.attentions.{j}" for j in js)


MID = ("mid_block.attentions.0",)
SD15 = [
    ("mid", MID),
    (["mid"], MID),
    ("down.block_2", _down(2, (0, 1))),
    ("down.block_2.attentions_1", _down(2, (1,))),
    ("up.block_1", _up(1, (0, 1, 2))),
    ("up.block_1.attentions_0", _up(1, (0,))),
    (["up.block_1.attentions_0", "mid", "down.block_0"], _down(0, (0, 1)) + MID + _up(1, (0,))),   # execution order
    ("down", _down(0, (0, 1)) + _down(1, (0, 1)) + _down(2, (0, 1))),
    ("up", _up(1, (0, 1, 2)) + _up(2, (0, 1, 2)) + _up(3, (0, 1, 2))),
    (["mid", "mid.block_0"], MID),
]
SDXL = [
    ("mid", MID),
    ("down.block_1", _down(1, (0, 1))),
    ("down.block_2.attentions_0", _down(2, (0,))),
    ("up.block_0", _up(0, (0, 1, 2))),
    ("up.block_1.attentions_2", _up(1, (2,))),
]
UNKNOWN_SD15 = ["down.block_3", "up.block_0", "down.block_0.attentions_2", "up.block_1.attentions_3", "mid.block_1",
                "middle", "down.attentions_0", "mid_block.attentions.0", "", "down.block_4"]
UNKNOWN_SDXL = ["down.block_0", "up.block_2", "down.block_3", "up.block_0.attentions_3"]


@pytest.mark.parametrize("cfg_name,table", [("sd15", SD15), ("tiny", SD15), ("sdxl", SDXL)])
def test_layer_names_become_site_keys(cfg_name, table):
    cfg = {"sd15": config.sd15_unet, "tiny": config.tiny_unet, "sdxl": config.sdxl_unet}[cfg_name]()
    for names, want in table:
        assert pag.site_keys(cfg, names) == want, names
    assert pag.DEFAULT_LAYERS == ("mid",)


@pytest.mark.parametrize("cfg_name,names", [("sd15", UNKNOWN_SD15), ("tiny", UNKNOWN_SD15), ("sdxl", UNKNOWN_SDXL)])
def test_unknown_layer_names_raise(cfg_name, names):
    cfg = {"sd15": config.sd15_unet, "tiny": config.tiny_unet, "sdxl": config.sdxl_unet}[cfg_name]()
    for name in names:
        with pytest.raises(ValueError, match="pag_applied_layers"):
            pag.site_keys(cfg, name)
        with pytest.raises(ValueError, match="pag_applied_layers"):
            pag.site_keys(cfg, ["mid", name])
    with pytest.raises(ValueError):
        pag.site_keys(cfg, [])


def test_transformer_sites_are_the_engines_order():
    sites = pag.transformer_sites(config.sd15_unet())
    assert len(sites) == 6 + 1 + 9
    assert sites[0] == "down_blocks.0.attentions.0" and sites[6] == "mid_block.attentions.0"
    assert sites[-1] == "up_blocks.3.attentions.2"
    xl = pag.transformer_sites(config.sdxl_unet())
    assert xl[0] == "down_blocks.1.attentions.0" and len(xl) == 4 + 1 + 6


# ------------------------------------------------------------------------------------------------ the schedule
def test_adaptive_scale_schedule():
    assert pag.step_scale(3.0, 0.0, 981.0) == 3.0
    assert pag.step_scale(3.0, 0.0, 1.0) == 3.0
    assert pag.step_scale(3.0, 0.005, 1000.0) == 3.0
    assert pag.step_scale(3.0, 0.005, 750.0) == pytest.approx(1.75)
    assert pag.step_scale(3.0, 0.005, 400.0) == 0.0                   # exactly at the clamp: 3 - 0.005 * 600
    assert pag.step_scale(3.0, 0.005, 250.0) == 0.0                   # below it
    assert pag.step_scale(0.0, 0.0, 500.0) == 0.0
    for t in (999.0, 500.0, 0.0):
        assert pag.step_scale(2.0, 0.01, t) == max(0.0, 2.0 - 0.01 * (1000.0 - t))


# ------------------------------------------------------------------------------------------------ host loop
class GroupUNet:
    """A UNet-shaped double without forward_pag for B = 2 latents: group k of the batch comes back as
    (0.1 + 0.05 k) * sample, so the groups' outputs differ and their order shows in the result."""
    B = 2

    def __init__(self, cfg):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.deepcache = None
        self.calls = []     # per forward: (batch, t, embedding batch, extra kwargs, last two groups share an embedding)

    def to(self, *a, **k):
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False, **kw):
        n = sample.shape[0] // self.B
        shared = n >= 2 and torch.equal(ehs[-self.B:], ehs[-2 * self.B:-self.B])
        self.calls.append((sample.shape[0], float(t), ehs.shape[0], tuple(sorted(kw)), shared))
        scale = torch.cat([torch.full((self.B,), 0.1 + 0.05 * k) for k in range(n)])
        return (scale.view(-1, 1, 1, 1) * sample[:, :4],)


def _model(sched="DDIM", cfg=None):
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), to=lambda d: None)
    m = SDModelWrapper(base=GroupUNet(cfg or config.tiny_unet()), vae=vae, scheduler=schedulers.DDIMScheduler(), device="cpu")
    m.set_scheduler(sched)
    return m


def _inputs(B=2):
    g = torch.Generator().manual_seed(9)
    d = config.tiny_unet().cross_attention_dim
    return (torch.randn(B, 4, 8, 8, generator=g), torch.randn(B, 7, d, generator=g), torch.randn(B, 7, d, generator=g))


def _run(m, do_cfg, steps=3, **kw):
    lat, pe, ne = _inputs()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cpu", output_type="latents")
    emb = dict(prompt_embeds=pe, negative_prompt_embeds=ne) if do_cfg else dict(prompt_embeds=pe)
    return pipe(m, latents=lat, num_inference_steps=steps, height=64, width=64, guidance_scale=4.0, **emb, **kw)


@pytest.mark.parametrize("do_cfg", [True, False])
def test_host_loop_combine_is_the_formula(do_cfg):
    """The double scales group k by 0.1 + 0.05 k, so eps = c x with c known in closed form: the loop's result is the
    scheduler run on that eps."""
    g, s = 4.0, 3.0
    m = _model()
    got = _run(m, do_cfg, pag_scale=s)
    G = 2 if do_cfg else 1
    assert [c[0] for c in m.base.calls] == [2 * (G + 1)] * 3 and [c[2] for c in m.base.calls] == [2 * (G + 1)] * 3
    assert all(c[4] for c in m.base.calls)              # the perturbed group carries the text group's embeddings
    if do_cfg:
        u, t, p = 0.1, 0.15, 0.2
        c = u + g * (t - u) + s * (t - p)
    else:
        t, p = 0.1, 0.15
        c = t + s * (t - p)
    ref_sched = schedulers.REGISTRY["DDIM"](schedulers.DDIMScheduler().config)
    ref_sched.set_timesteps(3)
    x = _inputs()[0] * ref_sched.init_noise_sigma
    for ts in ref_sched.timesteps.tolist():
        x = ref_sched.step(c * ref_sched.scale_model_input(x, ts), ts, x, return_dict=False)[0]
    assert torch.allclose(got, x, rtol=1e-5, atol=1e-6)


def test_combine_function():
    u, t, p = torch.randn(3, 2, 4, generator=torch.Generator().manual_seed(1)).unbind(0)
    assert torch.equal(pag.combine(torch.cat([u, t, p]), 5.0, 2.0, True), u + 5.0 * (t - u) + 2.0 * (t - p))
    assert torch.equal(pag.combine(torch.cat([t, p]), 5.0, 2.0, False), t + 2.0 * (t - p))


@pytest.mark.parametrize("do_cfg", [True, False])
def test_adaptive_scale_switches_steps_back_to_the_plain_forward(do_cfg):
    m = _model()
    m.scheduler.set_timesteps(4)
    ts = [float(t) for t in m.scheduler.timesteps.tolist()]
    a = 0.005
    lat, pe, ne = _inputs()
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cpu", output_type="latents")
    emb = dict(prompt_embeds=pe, negative_prompt_embeds=ne) if do_cfg else dict(prompt_embeds=pe)
    G = 2 if do_cfg else 1
    want = [2 * (G + 1) if pag.step_scale(3.0, a, t) > 0 else 2 * G for t in ts]
    assert want[0] == 2 * (G + 1) and want[-1] == 2 * G
    pipe(m, latents=lat, num_inference_steps=4, height=64, width=64, guidance_scale=4.0, pag_scale=3.0,
         pag_adaptive_scale=a, **emb)
    assert [c[0] for c in m.base.calls] == want


@pytest.mark.parametrize("do_cfg", [True, False])
@pytest.mark.parametrize("sched", ["DDIM", "euler_a"])
def test_pag_scale_zero_is_the_call_without_the_kwargs(do_cfg, sched):
    a, b = _model(sched), _model(sched)
    torch.manual_seed(5)
    plain = _run(a, do_cfg)
    torch.manual_seed(5)
    zero = _run(b, do_cfg, pag_scale=0.0, pag_adaptive_scale=0.0)
    assert torch.equal(plain, zero)
    assert a.base.calls == b.base.calls and len(a.base.calls) == 3


def test_signature_keeps_the_existing_kwargs_in_place():
    names = list(inspect.signature(StableDiffusionUnifiedPipeline.__call__).parameters)
    assert names[-2:] == ["pag_scale", "pag_adaptive_scale"]
    assert names[-4:-2] == ["aesthetic_score", "negative_aesthetic_score"]
    p = inspect.signature(StableDiffusionUnifiedPipeline.__call__).parameters
    assert p["pag_scale"].default == 0.0 and p["pag_adaptive_scale"].default == 0.0


def test_applied_layers_are_checked_and_kept():
    m = _model()
    m.set_pag_applied_layers(["mid", "up.block_1"])
    assert m._pag == ("mid", "up.block_1")
    with pytest.raises(ValueError, match="pag_applied_layers"):
        m.set_pag_applied_layers("up.block_0")
    assert m._pag == ("mid", "up.block_1")
    seen = []
    fused = SimpleNamespace(set_pag_layers=lambda names: seen.append(tuple(names)))
    m._base_factory = lambda sd: fused
    assert m._rebuild_from({}, False, None, None, m._pag) is fused and seen == [("mid", "up.block_1")]


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_combinations_raise():
    from cn_oracle import synth_cn_state_dict
    from stablediffusion_amd import controlnet
    lat, pe, ne = _inputs()
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64, width=64,
              pag_scale=3.0)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    # an IP-Adapter image
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        pipe(_model(), ip_adapter_image_embeds=[torch.zeros(4, 1, 8)], **kw)
    # the refiner
    with pytest.raises(NotImplementedError, match="refiner"):
        pipe(_model(), use_refiner=True, **kw)
    with pytest.raises(NotImplementedError, match="refiner"):
        pipe(_model(), refiner_start=0.8, **kw)
    # DeepCache enabled
    m = _model()
    m.base.deepcache = (3, 1)
    with pytest.raises(NotImplementedError, match="DeepCache"):
        pipe(m, **kw)
    # a 9-channel inpaint UNet
    m9 = _model(cfg=config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=9)))
    with pytest.raises(NotImplementedError, match="9-channel"):
        pipe(m9, **kw)
    # a guidance-embedded UNet
    with pytest.raises(NotImplementedError, match="guidance-embedded"):
        pipe(_model(cfg=config.tiny_unet(time_cond=32)), **kw)
    # a ControlNet loaded
    mc = _model()
    mc.base.make_controlnet = lambda cn_cfg, sd: object()
    mc.base.attach_controlnet = lambda cn: mc.base
    mc.load_controlnet(synth_cn_state_dict(controlnet.encoder_config(config.tiny_unet()), seed=3, zero_scale=0.5))
    with pytest.raises(NotImplementedError, match="ControlNet"):
        pipe(mc, control_image=torch.rand(1, 3, 64, 64), **kw)
    # bad scales
    for bad in (dict(pag_scale=float("inf")), dict(pag_scale=3.0, pag_adaptive_scale=-1.0),
                dict(pag_scale=3.0, pag_adaptive_scale=float("nan"))):
        with pytest.raises(ValueError, match="pag_scale"):
            pipe(_model(), **{**kw, **bad})
    # and none of them with pag_scale = 0
    m.base.deepcache = None
    out = pipe(m, **{**kw, "pag_scale": 0.0})
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------ the C entries
def test_new_symbols_are_declared_bound_and_exported(engine_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sd_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(engine_lib, name) is not None
    so = os.path.join(ROOT, "stablediffusion_amd", "libsd_engine.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, exported), name
    assert len(_lib.SIGNATURES["sd_unet_forward_pag"][1]) == 15
    assert len(_lib.SIGNATURES["sd_pag_linear_step"][1]) == 13 and len(_lib.SIGNATURES["sd_pag_combine"][1]) == 7


def invalid_step_calls():
    """(label, entry, args with 1 standing for a valid pointer): every one is SD_ERR_INVALID before anything launches."""
    inf, nan = float("inf"), float("nan")
    lin = lambda mo=1, rows=3, lat=1, n=8, g=5.0, s=3.0: ("sd_pag_linear_step", (mo, rows, lat, 0, n, g, s, 1.0, 0.1, 0.0, 0.0, 0.0))
    com = lambda mo=1, rows=3, out=1, n=8, g=5.0, s=3.0: ("sd_pag_combine", (mo, rows, out, n, g, s))
    table = []
    for make, what in ((lin, "linear"), (com, "combine")):
        table += [(f"{what}: rows = {r}", *make(rows=r)) for r in (0, 1, 4, -1)]
        table += [(f"{what}: n = {n}", *make(n=n)) for n in (0, -8)]
        table += [(f"{what}: null model_out", *make(mo=0))]
        table += [(f"{what}: non-finite guidance_scale {v}", *make(g=v)) for v in (inf, -inf, nan)]
        table += [(f"{what}: non-finite pag_scale {v}", *make(s=v)) for v in (inf, nan)]
    table += [("linear: null latents", *lin(lat=0)), ("combine: null out", *com(out=0))]
    return table


def call_step(lib, entry, args, ptrs, stream=None):
    """args: invalid_step_calls' tuple; ptrs: what 1 becomes per pointer position (model_out, latents / out)."""
    a = list(args)
    a[0] = C.c_void_p(ptrs[0]) if a[0] else None
    a[2] = C.c_void_p(ptrs[1]) if a[2] else None
    if entry == "sd_pag_linear_step":
        a[3] = None
    return getattr(lib, entry)(*a, stream)


def test_invalid_step_arguments_are_refused(engine_lib):
    """Without a device: the refusal comes before any launch, so host memory stands in for the pointers."""
    mo = (C.c_uint16 * 24)()
    lat = (C.c_uint16 * 8)()
    for label, entry, args in invalid_step_calls():
        rc = call_step(engine_lib, entry, args, (C.addressof(mo), C.addressof(lat)))
        assert rc == 1, label
        assert entry.encode() in engine_lib.sd_last_error(), label
    assert not any(mo) and not any(lat)


def test_null_handles_are_refused(engine_lib):
    assert engine_lib.sd_unet_set_pag_layers(None, None, 0) == 1
    assert engine_lib.sd_unet_forward_pag(None, None, None, None, 7, None, None, 1.0, 1, 1, None, 1, 8, 8, None) == 1
