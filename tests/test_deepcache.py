"""DeepCache on the host: the oracle's two identities (tests/deepcache_oracle.py), the store / reuse sequence the
pipeline's loop sets on a recording double of the engine's UNet, and the argument checks of `enable_deepcache`."""
from types import SimpleNamespace

import pytest
import torch

import deepcache_oracle
from cn_oracle import synth_cn_state_dict
from oracle import unet_ref
from refiner_doubles import StubTextEncoder, StubTokenizer
from stablediffusion_amd import config, controlnet, schedulers, weights
from stablediffusion_amd.models import HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

PLAIN, STORE, REUSE = HipUNet2DConditionModel.DC_PLAIN, HipUNet2DConditionModel.DC_STORE, HipUNet2DConditionModel.DC_REUSE
CONFIGS = {"tiny": config.tiny_unet, "linear_sdxl": lambda: config.tiny_unet(linear=True, sdxl_cond=True),
           "refiner": config.tiny_refiner_unet}
SHAPES = [(2, 16, 16), (1, 8, 24), (3, 24, 24)]
_weights = {}


def _setup(name):
    if name not in _weights:
        cfg = CONFIGS[name]()
        sd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1)
        _weights[name] = cfg, {k: v.half().float() for k, v in sd.items()}
    return _weights[name]


def _inputs(cfg, B, H, W):
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, 4, H, W, generator=g).half().float()
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g).half().float()
    added = None
    if cfg.addition_embed_type == "text_time":
        n = cfg.num_time_ids
        tdim = cfg.projection_class_embeddings_input_dim - n * cfg.addition_time_embed_dim
        ids = [128.0, 128, 0, 0, 128, 128] if n == 6 else [128.0, 128, 0, 0, 6.0][:n]
        added = {"text_embeds": torch.randn(B, tdim, generator=g).half().float(), "time_ids": torch.tensor([ids] * B)}
    return x, ehs, added


# -------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_oracle_full_form_is_the_reference_and_reuse_on_the_same_inputs_is_the_full_form(name, B, H, W):
    cfg, sd = _setup(name)
    assert cfg.layers_per_block >= 2
    x, ehs, added = _inputs(cfg, B, H, W)
    t = torch.tensor(501.0)
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, sd, x, t, ehs, added)
        for d in (1, 2):
            full, feat = deepcache_oracle.forward(cfg, sd, x, t, ehs, added, d)
            assert torch.equal(full, ref), (name, d)
            c1 = cfg.block_out_channels[1] if d == cfg.layers_per_block else cfg.block_out_channels[0]
            assert feat.shape == (B, c1, H, W)
            again, feat2 = deepcache_oracle.forward(cfg, sd, x, t, ehs, added, d, cached=feat)
            assert torch.equal(again, full) and feat2 is feat, (name, d)


# ------------------------------------------------------------------------------------------------ pipeline
class ModeUNet:
    """The call surface of the engine's UNet the loop uses, without a network: returns 0.1 * sample and records the
    DeepCache mode each forward ran in."""

    def __init__(self, cfg, fail_at=None):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        if cfg.addition_embed_type == "text_time":
            self.add_embedding = SimpleNamespace(
                linear_1=SimpleNamespace(in_features=cfg.projection_class_embeddings_input_dim))
        self.deepcache = None
        self.mode = PLAIN
        self.mode_calls = []
        self.calls = []             # (mode, t) per forward
        self.fail_at = fail_at
        self.cn = None

    def to(self, *a, **k):
        return self

    def enable_deepcache(self, cache_interval=3, cache_depth=1):
        self.deepcache = (cache_interval, cache_depth)
        return self

    def disable_deepcache(self):
        self.deepcache = None
        return self

    def deep_cache_mode(self, mode):
        assert self.deepcache is not None or mode == PLAIN
        self.mode = mode
        self.mode_calls.append(mode)
        return self

    def make_controlnet(self, cn_cfg, state_dict):
        return object()

    def attach_controlnet(self, cn):
        self.cn = cn
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                 controlnet_cond=None, controlnet_conditioning_scale=None):
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("forward failed")
        self.calls.append((self.mode, float(t)))
        return (0.1 * sample[:, :4],)


def _model(sched="DDIM", fail_at=None):
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), to=lambda d: None)
    m = SDModelWrapper(base=ModeUNet(config.tiny_unet(), fail_at), vae=vae, scheduler=schedulers.DDIMScheduler(), device="cpu")
    m.set_scheduler(sched)
    return m


def _run(m, steps, **kw):
    g = torch.Generator().manual_seed(9)
    d = m.base.cfg.cross_attention_dim
    lat, pe, ne = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 77, d, generator=g), torch.randn(1, 77, d, generator=g)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    return pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, height=64, width=64,
                **kw)


def _modes(unet):
    return "".join("PSR"[mode] for mode, _ in unet.calls)


def test_loop_stores_every_interval_th_step_and_reuses_between():
    m = _model()
    m.enable_deepcache(3, 1)
    assert m.base.deepcache == (3, 1)
    out = _run(m, 7)
    assert torch.isfinite(out).all()
    assert _modes(m.base) == "SRRSRRS"
    assert m.base.mode == PLAIN and m.base.mode_calls[-1] == PLAIN          # put back after the loop
    # a second loop starts with a store step again, whatever the first ended on
    m.base.calls.clear()
    _run(m, 5)
    assert _modes(m.base) == "SRRSR"


def test_interval_one_stores_every_step_and_off_sets_no_mode():
    m = _model()
    m.enable_deepcache(1, 2)
    _run(m, 4)
    assert _modes(m.base) == "SSSS" and m.base.mode == PLAIN
    m.disable_deepcache()
    assert m.base.deepcache is None
    m.base.calls.clear()
    m.base.mode_calls.clear()
    _run(m, 4)
    assert _modes(m.base) == "PPPP" and m.base.mode_calls == []


def test_plain_is_restored_after_an_exception_inside_the_loop():
    m = _model(fail_at=2)
    m.enable_deepcache(3, 1)
    with pytest.raises(RuntimeError, match="forward failed"):
        _run(m, 6)
    assert _modes(m.base) == "SR"
    assert m.base.mode_calls == [STORE, REUSE, REUSE, PLAIN] and m.base.mode == PLAIN


def test_pndm_extra_model_call_is_an_iteration_like_any_other():
    m = _model("PNDM")
    m.enable_deepcache(2, 1)
    _run(m, 4)
    m.scheduler.set_timesteps(4)
    ts = [float(t) for t in m.scheduler.timesteps.tolist()]
    assert len(ts) == 5 and len(set(ts)) == 4                               # one timestep runs the model twice
    assert [t for _, t in m.base.calls] == ts
    assert _modes(m.base) == "SRSRS"


def test_refiner_loop_runs_plain():
    cfg_b = config.tiny_unet(linear=True, sdxl_cond=True)
    m = SDModelWrapper(base=ModeUNet(cfg_b), refiner=ModeUNet(config.tiny_refiner_unet()),
                       vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5),
                                           to=lambda d: None),
                       text_encoder=StubTextEncoder(64, 64, 1), tokenizer=StubTokenizer(),
                       text_encoder_2=StubTextEncoder(64, 64, 2), tokenizer_2=StubTokenizer(), model_type="sdxl",
                       device="cpu")
    m.set_scheduler("DDIM")
    m.enable_deepcache(2, 1)
    assert m.base.deepcache == (2, 1) and m.refiner.deepcache is None       # the wrapper addresses .base
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    pipe(m, prompt="a cat", negative_prompt="blurry", num_inference_steps=5, seed=7, guidance_scale=4.0, refiner_start=0.6)
    assert _modes(m.base) == "SRS"[: len(m.base.calls)] and len(m.base.calls) >= 2
    assert m.refiner.calls and _modes(m.refiner) == "P" * len(m.refiner.calls)
    assert m.refiner.mode_calls == [] and m.base.mode == PLAIN
    m.disable_deepcache()
    assert m.base.deepcache is None


def test_control_image_with_deepcache_raises():
    m = _model()
    m.load_controlnet(synth_cn_state_dict(controlnet.encoder_config(config.tiny_unet()), seed=3, zero_scale=0.5))
    ctrl = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    _run(m, 2, control_image=ctrl)                                          # fine while DeepCache is off
    m.enable_deepcache(3, 1)
    m.base.calls.clear()
    with pytest.raises(ValueError, match="DeepCache"):
        _run(m, 2, control_image=ctrl)
    assert m.base.calls == [] and m.base.mode == PLAIN


def test_lora_refuse_keeps_deepcache():
    class Rebuildable(ModeUNet):
        def rebuild(self, sd):
            return Rebuildable(self.cfg)

    cfg = config.tiny_unet()
    usd = weights.synth_state_dict(weights.unet_manifest(cfg), seed=4, perturb=0.1)
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), to=lambda d: None)
    m = SDModelWrapper(base=Rebuildable(cfg), vae=vae, scheduler=schedulers.DDIMScheduler(), device="cpu",
                       unet_state_dict=usd)
    m.base.enable_deepcache(5, 2)               # on .base directly: the engine's own record wins, as for FreeU
    old = m.base
    g = torch.Generator().manual_seed(1)
    key = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    w = usd[key + ".weight"]
    m.load_lora_weights({f"unet.{key}.lora.down.weight": torch.randn(4, w.shape[1], generator=g) * 0.05,
                         f"unet.{key}.lora.up.weight": torch.randn(w.shape[0], 4, generator=g) * 0.05}, "style")
    m.apply_adapters()
    assert m.base is not old and m.base.deepcache == (5, 2)
    m.disable_deepcache()
    m.set_adapters(["style"], [0.5])
    m.apply_adapters()
    assert m.base.deepcache is None


# ---------------------------------------------------------------------------------------------- arguments
def test_enable_deepcache_validates_its_arguments(engine_lib):
    net = HipUNet2DConditionModel(config.tiny_unet())               # (no weights, no device: the settings are host state)
    assert net.deepcache is None
    for bad in (dict(cache_interval=0), dict(cache_interval=-2), dict(cache_interval=2.0), dict(cache_interval=True),
                dict(cache_interval="3"), dict(cache_depth=0), dict(cache_depth=3), dict(cache_depth=1.0),
                dict(cache_depth=None)):
        with pytest.raises(ValueError, match="enable_deepcache"):
            net.enable_deepcache(**bad)
        assert net.deepcache is None
    assert net.enable_deepcache() is net and net.deepcache == (3, 1)
    assert net.enable_deepcache(cache_interval=1, cache_depth=2).deepcache == (1, 2)
    assert net.disable_deepcache() is net and net.deepcache is None
    with pytest.raises(RuntimeError, match="depth is 0"):
        net.deep_cache_mode(STORE)                                          # SD_ERR_STATE: nothing enabled
    net.deep_cache_mode(PLAIN)
    net.enable_deepcache(2, 1)
    with pytest.raises(RuntimeError, match="unknown mode"):
        net.deep_cache_mode(7)
    net.deep_cache_mode(REUSE).deep_cache_mode(PLAIN)
