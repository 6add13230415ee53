"""MultiControlNet without a GPU: keep_schedule against its formula, the wrapper's and the pipeline's argument checks
with an oracle double of the engine's UNet (nothing may run before they raise), the single-net behaviours that stay as
they are, sharding's refusal and the new C-ABI symbols."""
import json
import os

import pytest
import torch

from cn_oracle import synth_cn_state_dict
from mcn_oracle import unet_mcn_forward
from stablediffusion_amd import config, controlnet, distributed as sdd, schedulers, weights
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ keep_schedule
def _formula(n, scales, starts, ends):
    return [[s * (1.0 - float(i / n < a or (i + 1) / n > b)) for s, a, b in zip(scales, starts, ends)] for i in range(n)]


def test_keep_schedule_matches_the_formula():
    assert controlnet.keep_schedule(8, [0.9, 0.4], [0.0, 0.25], [0.5, 1.0]) == _formula(8, [0.9, 0.4], [0.0, 0.25], [0.5, 1.0])
    rows = controlnet.keep_schedule(4, [0.9, 0.4], [0.0, 0.25], [0.5, 1.0])
    assert rows == [[0.9, 0.0], [0.9, 0.4], [0.0, 0.4], [0.0, 0.4]]
    # floats broadcast to the net count
    assert controlnet.keep_schedule(5, [1.0, 0.5, 0.25], 0.2, 0.8) == _formula(5, [1.0, 0.5, 0.25], [0.2] * 3, [0.8] * 3)
    assert controlnet.keep_schedule(5, 0.7, [0.0, 0.4], 1.0) == _formula(5, [0.7, 0.7], [0.0, 0.4], [1.0, 1.0])
    # windows that never open: narrower than one step, or none of the steps lies inside
    assert controlnet.keep_schedule(4, [1.0, 1.0], [0.3, 0.55], [0.45, 0.7]) == [[0.0, 0.0]] * 4
    # a one-step loop keeps only the full window
    assert controlnet.keep_schedule(1, [0.8, 0.6], [0.0, 0.0], [1.0, 0.9]) == [[0.8, 0.0]]
    with pytest.raises(ValueError):
        controlnet.keep_schedule(4, [1.0, 1.0], [0.0, 0.0, 0.0], 1.0)


@pytest.mark.parametrize("n,scale,start,end", [(4, 0.7, 0.25, 0.75), (5, 1.0, 0.2, 0.6), (10, 0.9, 0.0, 0.8), (1, 0.5, 0.0, 1.0),
                                               (3, 1.3, 0.5, 1.0)])
def test_keep_schedule_single_net_values(n, scale, start, end):
    """The expression the single-net loop used before keep_schedule existed."""
    want = [float(scale) * (1.0 - float(i / n < start or (i + 1) / n > end)) for i in range(n)]
    assert [r[0] for r in controlnet.keep_schedule(n, scale, start, end)] == want
    assert all(len(r) == 1 for r in controlnet.keep_schedule(n, scale, start, end))


# ------------------------------------------------------------------------------------- wrapper and pipeline
def _mcn_oracle_unet(cfg, sd):
    from doubles import OracleUNet

    class MCNOracleUNet(OracleUNet):
        """attach_controlnet(s) / make_controlnet as the engine's; the forward through mcn_oracle; records its calls."""

        def __init__(self, cfg, sd):
            super().__init__(cfg, sd)
            self.cns, self.listed = [], False
            self.calls = []

        def rebuild(self, sd):
            return MCNOracleUNet(self.cfg, sd)

        def make_controlnet(self, cn_cfg, state_dict):
            return {"cfg": cn_cfg, "sd": state_dict}

        def attach_controlnet(self, cn):
            self.cns, self.listed = ([cn] if cn is not None else []), False
            return self

        def attach_controlnets(self, cns):
            self.cns, self.listed = list(cns), bool(cns)
            return self

        def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                     controlnet_cond=None, controlnet_conditioning_scale=None):
            self.calls.append({"cond": controlnet_cond, "scale": controlnet_conditioning_scale, "shape": tuple(sample.shape)})
            if not self.cns:
                assert controlnet_cond is None and controlnet_conditioning_scale is None
                return super().__call__(sample, t, ehs, cross_attention_kwargs, added_cond_kwargs, return_dict)
            conds, scales = controlnet_cond, controlnet_conditioning_scale
            if not self.listed:
                conds, scales = [conds], [scales]
            assert len(conds) == len(scales) == len(self.cns)
            return (unet_mcn_forward(self.cfg, self.sd, [(c["cfg"], c["sd"]) for c in self.cns], sample, t, ehs.float(),
                                     conds, scales, added_cond_kwargs),)

    return MCNOracleUNet(cfg, sd)


def _model():
    from doubles import OracleVAE
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    return SDModelWrapper(base=_mcn_oracle_unet(ucfg, uw), vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(),
                          device="cpu", unet_state_dict=uw)


def _cn_sd(seed=3):
    return synth_cn_state_dict(controlnet.encoder_config(config.tiny_unet()), seed=seed, zero_scale=0.5)


def _control(n=1, h=64, w=64, seed=2):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


def _run(m, total=1, **kw):
    g = torch.Generator().manual_seed(9)
    d = config.tiny_unet().cross_attention_dim
    lat, pe, ne = torch.randn(total, 4, 8, 8, generator=g), torch.randn(total, 77, d, generator=g), torch.randn(total, 77, d, generator=g)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")

    def no_text_encoder(*a, **k):
        raise AssertionError("the text encoder was reached")

    pipe.encode_prompt = no_text_encoder
    kw.setdefault("height", 64)
    kw.setdefault("width", 64)
    return pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, **kw)


def test_load_controlnets_and_unload():
    m = _model()
    assert not m.has_controlnet and m.controlnet_list_len == 0
    m.load_controlnets([_cn_sd(3), _cn_sd(5)])
    assert m.has_controlnet and m.controlnet_list_len == 2
    assert m.base.listed and len(m.base.cns) == 2
    m.unload_controlnet()
    assert not m.has_controlnet and m.controlnet_list_len == 0 and m.base.cns == []
    m.load_controlnets([_cn_sd(3)])
    assert m.has_controlnet and m.controlnet_list_len == 1
    m.load_controlnet(_cn_sd(3))                            # replaces the list by a single net
    assert m.has_controlnet and m.controlnet_list_len == 0 and not m.base.listed and len(m.base.cns) == 1
    for bad in ([], [_cn_sd()] * 5, _cn_sd()):
        with pytest.raises(ValueError):
            m.load_controlnets(bad)
    assert m.controlnet_list_len == 0 and len(m.base.cns) == 1          # a refused load changes nothing


def test_pipeline_windows_reach_the_unet_per_net():
    m = _model()
    m.load_controlnets([_cn_sd(3), _cn_sd(5)])
    a, b = _control(1, seed=2), _control(1, seed=6)
    with_both = _run(m, num_inference_steps=4, control_image=[a, b], controlnet_conditioning_scale=[0.9, 0.4],
                     control_guidance_start=[0.0, 0.25], control_guidance_end=[0.5, 1.0])
    assert [c["scale"] for c in m.base.calls] == [[0.9, 0.0], [0.9, 0.4], [0.0, 0.4], [0.0, 0.4]]
    assert all(len(c["cond"]) == 2 and c["cond"][0].shape == (1, 3, 64, 64) and c["shape"][0] == 2 for c in m.base.calls)
    assert torch.allclose(m.base.calls[0]["cond"][1], b, atol=1e-6)
    m.base.calls.clear()
    first_only = _run(m, num_inference_steps=4, control_image=[a, b], controlnet_conditioning_scale=[0.9, 0.0])
    assert [c["scale"] for c in m.base.calls] == [[0.9, 0.0]] * 4      # floats broadcast: the full window for both
    assert not torch.allclose(with_both, first_only)


def test_size_defaults_to_the_first_image():
    m = _model()
    m.load_controlnets([_cn_sd(3), _cn_sd(5)])
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    g = torch.Generator().manual_seed(9)
    d = config.tiny_unet().cross_attention_dim
    out = pipe(m, prompt_embeds=torch.randn(1, 77, d, generator=g), negative_prompt_embeds=torch.randn(1, 77, d, generator=g),
               num_inference_steps=1, seed=3, control_image=[_control(1, 128, 64), _control(1, 128, 64, seed=4)])
    assert out.shape == (1, 4, 16, 8)


def test_list_argument_checks_raise_before_anything_runs():
    m = _model()
    m.load_controlnets([_cn_sd(3), _cn_sd(5)])
    a, b = _control(1), _control(1, seed=6)
    bad = [dict(control_image=[a]),                                                     # not the net count
           dict(control_image=[a, b, a]),
           dict(control_image=[]),                                                      # empty
           dict(control_image=a),                                                       # not a list
           dict(control_image=[a, b], controlnet_conditioning_scale=[1.0]),
           dict(control_image=[a, b], controlnet_conditioning_scale=[1.0, 0.5, 0.2]),
           dict(control_image=[a, b], control_guidance_start=[0.0, 0.1, 0.2]),
           dict(control_image=[a, b], control_guidance_end=[1.0]),
           dict(control_image=[a, b], control_guidance_start=[0.0, 0.6], control_guidance_end=[1.0, 0.4]),
           dict(control_image=[a, _control(1, 64, 128)], height=None, width=None)]      # sizes differ after preprocessing
    for kw in bad:
        with pytest.raises(ValueError):
            _run(m, num_inference_steps=1, **kw)
        assert m.base.calls == [], kw
    with pytest.raises(NotImplementedError):
        _run(m, num_inference_steps=1, control_image=[a, b], guess_mode=True)
    with pytest.raises(ValueError):                                                     # loaded: control images required
        _run(m, num_inference_steps=1)
    assert m.base.calls == []


def test_single_net_behaviours_stay():
    m = _model()
    with pytest.raises(NotImplementedError):
        m.load_controlnet([_cn_sd(), _cn_sd()])
    m.load_controlnet(_cn_sd())
    want = json.load(open(os.path.join(HERE, "golden", "call_refusals.json")))
    recorded = json.dumps(want)
    for kw in (dict(controlnet_conditioning_scale=[1.0, 0.5]), dict(control_guidance_start=[0.0, 0.1]),
               dict(control_guidance_end=[1.0, 0.9])):
        with pytest.raises(NotImplementedError) as e:
            _run(m, num_inference_steps=1, control_image=_control(1), **kw)
        assert str(e.value) in recorded                     # the message the fixture records (cn_loaded+image/list_scale)
    assert m.base.calls == []
    _run(m, num_inference_steps=2, control_image=_control(1), controlnet_conditioning_scale=0.7, control_guidance_end=0.5)
    assert [c["scale"] for c in m.base.calls] == [0.7, 0.0]           # floats, as before


def test_sharded_txt2img_refuses_lists_of_control_batches():
    with pytest.raises(NotImplementedError):
        sdd.sharded_txt2img(None, None, torch.zeros(2, 4, 8, 8), torch.zeros(2, 77, 64), torch.zeros(2, 77, 64), 0, 1,
                            control_image=[_control(2), _control(2)])


# ------------------------------------------------------------------------------------------------------- C-ABI
NEW_SYMBOLS = ("sd_unet_set_controlnets", "sd_unet_forward_mcn", "sd_unet_cn_fold_count", "sd_cn_kcat_force",
               "sd_op_cn_fold_scales", "sd_op_controlnet_residuals_multi")


def test_new_symbols_exported_and_bound(engine_lib):
    from stablediffusion_amd import _lib
    header = open(os.path.join(HERE, "..", "include", "sd_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        fn = getattr(engine_lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    assert "#define SD_MAX_CONTROLNETS 4" in header and _lib.SD_MAX_CONTROLNETS == 4
    # host-only entries: no device needed
    assert engine_lib.sd_cn_kcat_force(0) == 0 and engine_lib.sd_cn_kcat_force(-1) == 0
    assert engine_lib.sd_unet_cn_fold_count(None) == 0
    assert engine_lib.sd_unet_set_controlnets(None, None, 0) == 1
