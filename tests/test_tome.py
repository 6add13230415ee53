"""Token merging on the host: the float64 identity the design rests on (merging before or after the linear projections),
the step index the pipeline's loop hands a recording double of the engine's UNet, what the pipeline refuses, and the
argument checks of `enable_tome`."""
from types import SimpleNamespace

import pytest
import torch

import tome_oracle
from stablediffusion_amd import config, schedulers, weights
from stablediffusion_amd.models import HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


# -------------------------------------------------------------------------------------------------- oracle
def test_oracle_merge_order_identity_and_off_is_the_reference():
    from oracle import unet_ref
    cfg = config.tiny_unet()
    sd = {k: v.half().double() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1).items()}
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 16, 16, generator=g).double()
    ehs = torch.randn(1, 77, cfg.cross_attention_dim, generator=g).double()
    t = torch.tensor(501.0, dtype=torch.float64)
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, sd, x, t, ehs)
        off = tome_oracle.unet_forward(cfg, sd, x, t, ehs, None, tome_oracle.Tome(0.0))
        pre_t = tome_oracle.Tome(0.5, 2, seed=3, step=1, order="pre")
        pre = tome_oracle.unet_forward(cfg, sd, x, t, ehs, None, pre_t)
        post = tome_oracle.unet_forward(cfg, sd, x, t, ehs, None,
                                        tome_oracle.Tome(0.5, 2, seed=3, step=1, order="post",
                                                         maps={s: u["maps"] for s, u in pre_t.used.items()}))
    assert (off - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert sorted(pre_t.used) == [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]
    assert (pre - post).abs().max() <= 1e-10 * pre.abs().max()          # linear projections commute with the mean
    assert (pre - ref).abs().max() > 1e-3 * ref.abs().max()             # and merging is not a no-op


# ------------------------------------------------------------------------------------------------ pipeline
class TomeUNet:
    """The call surface of the engine's UNet the loop uses, without a network: returns 0.1 * sample and records the step
    index each forward ran under."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.tome = None
        self.step = None
        self.calls = []
        self._graph_on = False

    def to(self, *a, **k):
        return self

    def enable_tome(self, ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=True, seed=0):
        self.tome = (ratio, max_downsample, sx, sy, use_rand, seed)
        return self

    def disable_tome(self):
        self.tome = None
        return self

    def tome_step(self, i):
        assert self.tome is not None
        self.step = i
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
        self.calls.append(self.step)
        return (0.1 * sample[:, :4],)


def _model(cfg=None, sched="DDIM"):
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), to=lambda d: None)
    m = SDModelWrapper(base=TomeUNet(cfg or config.tiny_unet()), vae=vae, scheduler=schedulers.DDIMScheduler(), device="cpu")
    m.set_scheduler(sched)
    return m


def _run(m, steps, **kw):
    g = torch.Generator().manual_seed(9)
    d = m.base.cfg.cross_attention_dim
    lat, pe, ne = torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 77, d, generator=g), torch.randn(1, 77, d, generator=g)
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cpu", output_type="latents")
    return pipe(m, prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, height=64, width=64,
                **kw)


@pytest.mark.parametrize("sched", ["DDIM", "PNDM"])
def test_loop_hands_the_iteration_to_the_unet(sched):
    m = _model(sched=sched)
    m.enable_tome(0.5, seed=7)
    assert m.base.tome == (0.5, 1, 2, 2, True, 7)
    assert torch.isfinite(_run(m, 5)).all()
    n = len(m.base.calls)                                               # (PNDM runs the model twice at one timestep)
    assert n >= 5 and m.base.calls == list(range(n))
    m.base.calls.clear()
    _run(m, 3)                                                          # a second loop counts from 0 again
    assert m.base.calls == list(range(len(m.base.calls))) and len(m.base.calls) >= 3
    m.disable_tome()
    assert m.base.tome is None
    m.base.calls.clear()
    m.base.step = None
    _run(m, 3)
    assert set(m.base.calls) == {None}                                  # off: the loop sets nothing


def test_pipeline_refuses_before_anything_runs():
    m = _model()
    m.enable_tome(0.5)
    with pytest.raises(NotImplementedError, match="token merging"):
        _run(m, 3, pag_scale=2.0)
    m.base._graph_on = True
    with pytest.raises(NotImplementedError, match="use_graph"):
        _run(m, 3)
    m.base._graph_on = False
    with pytest.raises(NotImplementedError, match="view_window"):
        _run(m, 3, view_window=8)
    for attr, word in (("_freeu", "FreeU"), ("_cn", "ControlNet"), ("_ip", "IP-Adapter")):
        setattr(m.base, attr, object())
        with pytest.raises(NotImplementedError, match=word):
            _run(m, 3)
        setattr(m.base, attr, None)
    assert m.base.calls == []
    m8 = _model(config.tiny_unet())
    m8.base.config.in_channels = 8
    m8.enable_tome(0.5)
    with pytest.raises(NotImplementedError, match="8-channel"):
        _run(m8, 3, image=torch.zeros(1, 3, 64, 64))
    assert m8.base.calls == []


# ------------------------------------------------------------------------------------------ argument validation
class _Lib:
    def __init__(self):
        self.calls = []

    def sd_unet_set_tome(self, h, *a):
        self.calls.append(a)
        return 0

    def sd_unet_tome_step(self, h, i):
        self.calls.append(("step", i))
        return 0


def _shell():
    """A HipUNet2DConditionModel without an engine behind it: the methods under test only reach `_lib` and `_h`."""
    net = HipUNet2DConditionModel.__new__(HipUNet2DConditionModel)
    net._lib, net._h, net._tome = _Lib(), None, None
    return net


def test_enable_tome_validates_and_records():
    net = _shell()
    for bad in (dict(ratio=0.8), dict(ratio=-0.1), dict(ratio=float("nan")), dict(ratio="0.5"), dict(ratio=True),
                dict(sx=0), dict(sy=9), dict(sx=2.0), dict(max_downsample=3), dict(max_downsample=True), dict(seed=-1),
                dict(seed=2 ** 32), dict(seed=1.5)):
        with pytest.raises(ValueError, match="enable_tome"):
            net.enable_tome(**bad)
    assert net._lib.calls == [] and net.tome is None
    net.enable_tome(0.25, max_downsample=2, sx=2, sy=4, use_rand=False, seed=9)
    assert net.tome == (0.25, 2, 2, 4, False, 9)
    assert net._lib.calls[-1] == (0.25, 2, 2, 4, 0, 9)
    net.tome_step(2 ** 32 + 5)
    assert net._lib.calls[-1] == ("step", 5)
    net.enable_tome(0.0)                                                # ratio 0 is off
    assert net.tome is None and net._lib.calls[-1][0] == 0.0
    net.enable_tome()
    assert net.tome == (0.5, 1, 2, 2, True, 0)
    net.disable_tome()
    assert net.tome is None


def test_settings_survive_rebuild():
    made = []

    class Net(HipUNet2DConditionModel):
        def __init__(self, cfg=None, device=None):
            self.cfg, self.device = cfg, device
            self._lib, self._h = _Lib(), None
            self._freeu = self._deepcache = self._tome = None
            self._pag = ()
            made.append(self)

        def load_state_dict(self, sd):
            return self

    a = Net()
    a.enable_tome(0.5, seed=4)
    b = a.rebuild({})
    assert b is not a and b.tome == (0.5, 1, 2, 2, True, 4) and b._lib.calls == [(0.5, 1, 2, 2, 1, 4)]
    a.disable_tome()
    assert a.rebuild({}).tome is None
