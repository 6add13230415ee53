"""ControlNet through SDModelWrapper and the pipeline, on CPU with an oracle double of the engine's UNet: loading,
the guidance window, control-image preprocessing and batch repeat, the run's size from the control image, the LoRA
re-fuse, sharding, and the rejections."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cn_oracle import synth_cn_state_dict, unet_cn_forward
from stablediffusion_amd import config, controlnet, distributed as sdd, schedulers, weights
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


def _cn_oracle_unet(cfg, sd):
    from doubles import OracleUNet

    class CNOracleUNet(OracleUNet):
        """attach_controlnet / make_controlnet as the engine's; the forward through cn_oracle; records its calls."""

        def __init__(self, cfg, sd):
            super().__init__(cfg, sd)
            self.cn = None
            self.calls = []

        def rebuild(self, sd):
            return CNOracleUNet(self.cfg, sd)

        def make_controlnet(self, cn_cfg, state_dict):
            return {"cfg": cn_cfg, "sd": state_dict}

        def attach_controlnet(self, cn):
            self.cn = cn
            return self

        def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False,
                     controlnet_cond=None, controlnet_conditioning_scale=None):
            self.calls.append({"cond": controlnet_cond, "scale": controlnet_conditioning_scale, "shape": tuple(sample.shape)})
            if self.cn is None:
                assert controlnet_cond is None and controlnet_conditioning_scale is None
                return super().__call__(sample, t, ehs, cross_attention_kwargs, added_cond_kwargs, return_dict)
            assert controlnet_cond is not None and sample.shape[0] % controlnet_cond.shape[0] == 0
            return (unet_cn_forward(self.cfg, self.sd, self.cn["cfg"], self.cn["sd"], sample, t, ehs.float(),
                                    controlnet_cond, controlnet_conditioning_scale, added_cond_kwargs),)

    return CNOracleUNet(cfg, sd)


def _model():
    from doubles import OracleVAE
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    return SDModelWrapper(base=_cn_oracle_unet(ucfg, uw), vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(),
                          device="cpu", unet_state_dict=uw)


def _cn_sd(seed=3):
    return synth_cn_state_dict(controlnet.encoder_config(config.tiny_unet()), seed=seed, zero_scale=0.5)


def _embeds(total, seed=9, hw=8):
    g = torch.Generator().manual_seed(seed)
    d = config.tiny_unet().cross_attention_dim
    return (torch.randn(total, 4, hw, hw, generator=g), torch.randn(total, 77, d, generator=g),
            torch.randn(total, 77, d, generator=g))


def _control(n, h=64, w=64, seed=2):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


def _run(m, total=2, **kw):
    lat, pe, ne = _embeds(total)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    kw.setdefault("height", 64)
    kw.setdefault("width", 64)
    return pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, **kw)


def test_guidance_window_txt2img():
    m = _model()
    m.load_controlnet(_cn_sd())
    _run(m, num_inference_steps=4, control_image=_control(1), controlnet_conditioning_scale=0.7,
         control_guidance_start=0.25, control_guidance_end=0.75)
    assert [c["scale"] for c in m.base.calls] == [0.0, 0.7, 0.7, 0.0]


def test_guidance_window_img2img_sliced_schedule():
    m = _model()
    m.load_controlnet(_cn_sd())
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(7)) * 2 - 1
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    _, pe, ne = _embeds(1)
    pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.5, num_inference_steps=10, seed=1,
         control_image=_control(1), controlnet_conditioning_scale=1.0, control_guidance_start=0.2,
         control_guidance_end=0.6)
    # strength 0.5 of 10 steps: a 5-step loop; keep when i/5 >= 0.2 and (i + 1)/5 <= 0.6
    assert [c["scale"] for c in m.base.calls] == [0.0, 1.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("n_img,batch,nipp,expect", [(1, 2, 1, 2), (1, 2, 2, 4), (2, 2, 1, 2), (2, 2, 2, 4), (1, 1, 3, 3)])
def test_control_image_preprocess_and_repeat(n_img, batch, nipp, expect):
    """diffusers prepare_image: a one-image batch repeats by batch x images per prompt, a larger one by images per
    prompt (repeat_interleave); [0, 1] values pass unnormalised, resized to the run's size."""
    m = _model()
    ctrl = _control(n_img, 32, 48)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    cond = pipe.prepare_control_image(m, ctrl, 64, 96, batch, nipp)
    assert cond.shape == (expect, 3, 64, 96)
    from stablediffusion_amd.image_processor import VaeImageProcessor
    ref = VaeImageProcessor(vae_scale_factor=8, do_convert_rgb=True, do_normalize=False).preprocess(ctrl, 64, 96)
    rep = expect if n_img == 1 else nipp
    assert torch.equal(cond, ref.repeat_interleave(rep, dim=0).float())
    assert cond.min() >= 0 and cond.max() <= 1                       # not normalised to [-1, 1]
    with pytest.raises(ValueError):
        pipe.prepare_control_image(m, _control(3), 64, 64, 2, 1)


def test_pipeline_passes_the_control_image_once_per_sample():
    m = _model()
    m.load_controlnet(_cn_sd())
    ctrl = _control(2)
    _run(m, num_inference_steps=1, control_image=ctrl)
    cond = m.base.calls[0]["cond"]
    assert cond.shape == (2, 3, 64, 64) and m.base.calls[0]["shape"][0] == 4       # CFG batch maps b -> b mod 2
    assert torch.allclose(cond, ctrl, atol=1e-6)


def test_size_from_control_image():
    m = _model()
    m.load_controlnet(_cn_sd())
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    _, pe, ne = _embeds(1)
    out = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=1, seed=3,
               control_image=_control(1, 128, 64))
    assert out.shape == (1, 4, 16, 8)
    assert m.base.calls[0]["cond"].shape == (1, 3, 128, 64)


def test_no_control_kwargs_without_controlnet_and_unload():
    m = _model()
    _run(m, num_inference_steps=2)
    assert all(c["cond"] is None and c["scale"] is None for c in m.base.calls)
    m.load_controlnet(_cn_sd())
    with_cn = _run(m, num_inference_steps=2, control_image=_control(1))
    m.unload_controlnet()
    m.base.calls.clear()
    plain = _run(m, num_inference_steps=2)
    assert all(c["cond"] is None for c in m.base.calls)
    assert not torch.allclose(with_cn, plain)


def test_rejections(tmp_path):
    m = _model()
    with pytest.raises(ValueError):                         # no ControlNet loaded
        _run(m, num_inference_steps=1, control_image=_control(1))
    m.load_controlnet(_cn_sd())
    with pytest.raises(ValueError):                         # loaded: control image required
        _run(m, num_inference_steps=1)
    with pytest.raises(NotImplementedError):
        _run(m, num_inference_steps=1, control_image=_control(1), guess_mode=True)
    with pytest.raises(NotImplementedError):
        _run(m, num_inference_steps=1, control_image=_control(1), controlnet_conditioning_scale=[1.0, 0.5])
    with pytest.raises(ValueError):
        _run(m, num_inference_steps=1, control_image=_control(1), control_guidance_start=0.6, control_guidance_end=0.4)
    with pytest.raises(NotImplementedError):
        m.load_controlnet([_cn_sd(), _cn_sd()])
    path = tmp_path / "control_v11e_sd15_shuffle.pth"
    torch.save(_cn_sd(), str(path))
    with pytest.raises(ValueError):
        m.load_controlnet(str(path))


def test_unet_shim_rejects_residual_tensors(engine_lib):
    from stablediffusion_amd.models import HipUNet2DConditionModel
    u = HipUNet2DConditionModel(config.tiny_unet())
    x, e = torch.zeros(1, 4, 8, 8), torch.zeros(1, 77, 64)
    for kw in ({"down_block_additional_residuals": [torch.zeros(1)]}, {"mid_block_additional_residual": torch.zeros(1)},
               {"guess_mode": True}):
        with pytest.raises(NotImplementedError):
            u(x, 1.0, e, **kw)


def test_lora_refuse_keeps_the_controlnet():
    m = _model()
    m.load_controlnet(_cn_sd())
    old = m.base
    g = torch.Generator().manual_seed(1)
    key = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    w = m._unet_sd[key + ".weight"]
    m.load_lora_weights({f"unet.{key}.lora.down.weight": torch.randn(4, w.shape[1], generator=g) * 0.05,
                         f"unet.{key}.lora.up.weight": torch.randn(w.shape[0], 4, generator=g) * 0.05}, "style")
    m.apply_adapters()
    assert m.base is not old
    assert m.base.cn is not None and m.base.cn["sd"] is m._cn[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, total, per_sample, out_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    sdd.init("gloo")
    lat, pe, ne = _embeds(total)
    if rank != 0:
        pe.zero_(); ne.zero_()                       # must arrive through the broadcast
    m = _model()
    m.load_controlnet(_cn_sd())
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    imgs = sdd.sharded_txt2img(pipe, m, lat, pe, ne, rank, world, num_inference_steps=2, height=64, width=64,
                               control_image=_control(total if per_sample else 1))
    if rank == 0:
        torch.save(imgs, out_path)
    sdd.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("per_sample", [True, False])
def test_sharded_txt2img_with_control_image_equals_unsharded(tmp_path, per_sample):
    total = 3
    out = str(tmp_path / "imgs.pt")
    mp.spawn(_worker, args=(2, _free_port(), total, per_sample, out), nprocs=2, join=True)
    sharded = torch.load(out, weights_only=True)
    torch.set_num_threads(2)
    lat, pe, ne = _embeds(total)
    m = _model()
    m.load_controlnet(_cn_sd())
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu")
    full = pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, height=64,
                width=64, control_image=_control(total if per_sample else 1))
    assert sharded.shape == full.shape == (total, 3, 64, 64)
    assert torch.allclose(sharded, full, atol=1e-5)
