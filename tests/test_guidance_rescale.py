"""guidance_rescale on the host: `rescale_noise_cfg` pinned to the reference's own function (tests/golden/
guidance_rescale.npz, written by tests/golden/make_guidance_rescale.py) and the pipeline's generic path on the CPU
doubles.  CPU only."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from doubles import OracleUNet, OracleVAE
from stablediffusion_amd import schedulers
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline, rescale_noise_cfg

HERE = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(min(8, os.cpu_count() or 1))


def test_rescale_noise_cfg_matches_the_references_function():
    d = np.load(os.path.join(HERE, "golden", "guidance_rescale.npz"))
    phis = d["phis"].tolist()
    assert phis == [0.3, 0.7, 1.0]
    seen = set()
    for name in d["cases"].tolist():
        cfg, text = torch.from_numpy(d[f"{name}_cfg"]), torch.from_numpy(d[f"{name}_text"])
        seen.add(cfg.dtype)
        for k, phi in enumerate(phis):
            want = torch.from_numpy(d[f"{name}_out{k}"])
            got = rescale_noise_cfg(cfg, text, guidance_rescale=phi)
            assert got.dtype == want.dtype and got.shape == want.shape
            if cfg.dtype == torch.float32:
                assert (got - want).abs().max().item() <= 1e-6, (name, phi)
            else:
                # one fp16 ulp: neighbouring representable values, compared on the bit patterns (same sign everywhere)
                gi, wi = got.view(torch.int16).int(), want.view(torch.int16).int()
                assert (gi - wi).abs().max().item() <= 1, (name, phi)
    assert seen == {torch.float32, torch.float16}


@pytest.fixture(scope="module")
def golden():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    ucfg, vcfg, uw, vw = mg.golden_weights()
    data = np.load(os.path.join(HERE, "golden", "tiny_sd.npz"))
    d = {k: torch.from_numpy(np.asarray(data[k])) for k in data.files}
    model = SDModelWrapper(base=OracleUNet(ucfg, uw), vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(),
                           device="cpu")
    neg, pos = d["pipe_embeds2b"][:1], d["pipe_embeds2b"][1:]
    kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, latents=d["pipe_latents0"], num_inference_steps=4,
              guidance_scale=5.0, height=64, width=64)
    return model, kw, d


def _run(model, kw, do_cfg=True, **extra):
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cpu", output_type="latents")
    return pipe(model, **dict(kw, **extra))


def test_pipeline_honours_guidance_rescale(golden):
    """The generic path against a loop written out by hand (std with ddof = 1 over each sample, computed from sums); the
    result really differs from the unrescaled one."""
    model, kw, d = golden
    phi, g = 0.7, kw["guidance_scale"]
    got = _run(model, kw, guidance_rescale=phi)
    sch = schedulers.DDIMScheduler()
    sch.set_timesteps(kw["num_inference_steps"])
    x = kw["latents"] * sch.init_noise_sigma
    ehs = torch.cat([kw["negative_prompt_embeds"], kw["prompt_embeds"]])
    for t in sch.timesteps.tolist():
        u, c = model.base(torch.cat([x, x]), float(t), ehs)[0].chunk(2)
        e = u + g * (c - u)
        n = e[0].numel()

        def std(z):
            z = z.double().reshape(z.shape[0], -1)
            return (((z - z.mean(1, keepdim=True)) ** 2).sum(1) / (n - 1)).sqrt().reshape(-1, 1, 1, 1)

        k = 1.0 + phi * (std(c) / std(e) - 1.0)
        x = sch.step((k * e.double()).float(), t, x)[0]
    assert rel_l2(got, x) < 1e-5
    plain = _run(model, kw, guidance_rescale=0.0)
    assert rel_l2(got, plain) > 1e-3                      # the kwarg is read


def test_guidance_rescale_zero_is_the_old_pipeline(golden):
    model, kw, d = golden
    plain = _run(model, kw)
    assert torch.equal(_run(model, kw, guidance_rescale=0.0), plain)
    assert rel_l2(plain, d["pipe_latents"]) < 1e-4        # the committed result of the loop without rescale


def test_guidance_rescale_range_and_cfg_off(golden):
    model, kw, d = golden
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="guidance_rescale"):
            _run(model, kw, guidance_rescale=bad)
    off = dict(kw, negative_prompt_embeds=None)
    assert torch.equal(_run(model, off, do_cfg=False, guidance_rescale=0.7), _run(model, off, do_cfg=False))


@pytest.mark.parametrize("name", ["euler", "PNDM"])
def test_guidance_rescale_with_v_prediction_and_other_schedulers(golden, name):
    """The generic path serves every scheduler and prediction type: finite, and different from the unrescaled run."""
    model, kw, d = golden
    m = SDModelWrapper(base=model.base, vae=model.vae, scheduler=schedulers.DDIMScheduler(), device="cpu",
                       prediction_type="v_prediction")
    m.set_scheduler(name)
    assert m.scheduler.v_prediction
    a, b = _run(m, kw, guidance_rescale=0.5), _run(m, kw)
    assert torch.isfinite(a).all() and rel_l2(a, b) > 1e-3
