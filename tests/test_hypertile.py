"""HyperTile on the host: the float64 oracle (off is the reference, one tile is the reference, tiling moves the output,
the rearrangement is a bijection), the step index the pipeline's loop hands a recording double of the engine's UNet, the
wrapper's forwarding to base and refiner, and the argument checks of `enable_hypertile`."""
from types import SimpleNamespace

import pytest
import torch

import hypertile_oracle
from stablediffusion_amd import config, schedulers, weights
from stablediffusion_amd.models import HipUNet2DConditionModel
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline


# -------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("B,Hs,Ws,nh,nw", [(2, 16, 16, 2, 2), (1, 12, 20, 2, 2), (3, 8, 24, 1, 3), (2, 24, 8, 3, 1), (1, 6, 4, 1, 1)])
def test_rearrangement_is_the_stated_row_map(B, Hs, Ws, nh, nw):
    th, tw = Hs // nh, Ws // nw
    rows = torch.arange(B * Hs * Ws, dtype=torch.float64).view(B, Hs * Ws, 1)
    tiles = hypertile_oracle.to_tiles(rows, Hs, Ws, nh, nw)
    assert tiles.shape == (B * nh * nw, th * tw, 1)
    flat = tiles.reshape(-1)
    for b, ty, tx, y, x in [(0, 0, 0, 0, 0), (B - 1, nh - 1, nw - 1, th - 1, tw - 1), (B - 1, 0, nw - 1, th // 2, 0),
                            (0, nh - 1, 0, 0, tw - 1)]:
        dst = ((b * nh + ty) * nw + tx) * th * tw + y * tw + x
        assert int(flat[dst]) == (b * Hs + ty * th + y) * Ws + tx * tw + x
    assert torch.equal(hypertile_oracle.from_tiles(tiles, Hs, Ws, nh, nw), rows)
    assert sorted(flat.long().tolist()) == list(range(B * Hs * Ws))


def test_tiled_attention_sees_only_its_tile():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(1, 8 * 12, 16, generator=g, dtype=torch.float64) for _ in range(3))
    base = hypertile_oracle.tiled_attention(q, k, v, 2, 8, 12, 2, 3)
    one = hypertile_oracle.tiled_attention(q, k, v, 2, 8, 12, 1, 1)
    full = torch.nn.functional.scaled_dot_product_attention(*(t.view(1, 96, 2, 8).transpose(1, 2) for t in (q, k, v)))
    assert torch.allclose(one, full.transpose(1, 2).reshape(1, 96, 16), atol=1e-13)
    # change k and v in tile (1, 2): only that tile's rows move
    k2, v2 = k.clone(), v.clone()
    inside = torch.zeros(8, 12, dtype=torch.bool)
    inside[4:, 8:] = True
    k2[0, inside.view(-1)] += 1.0
    v2[0, inside.view(-1)] -= 2.0
    moved = hypertile_oracle.tiled_attention(q, k2, v2, 2, 8, 12, 2, 3)
    changed = (moved != base).any(dim=-1).view(8, 12)
    assert torch.equal(changed, inside)


def test_oracle_off_is_the_reference_and_tiling_moves_the_output():
    from oracle import unet_ref
    cfg = config.tiny_unet()
    sd = {k: v.half().double() for k, v in weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1).items()}
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 4, 16, 16, generator=g).double()
    ehs = torch.randn(1, 77, cfg.cross_attention_dim, generator=g).double()
    t = torch.tensor(501.0, dtype=torch.float64)
    with torch.no_grad():
        ref = unet_ref.unet_forward(cfg, sd, x, t, ehs)
        off = hypertile_oracle.unet_forward(cfg, sd, x, t, ehs, None, hypertile_oracle.HyperTile(0))
        big = hypertile_oracle.HyperTile(16, 2, 0)
        whole = hypertile_oracle.unet_forward(cfg, sd, x, t, ehs, None, big)
        ht = hypertile_oracle.HyperTile(4, 2, 1, seed=0, step=0)
        on = hypertile_oracle.unet_forward(cfg, sd, x, t, ehs, None, ht)
        given = hypertile_oracle.HyperTile(4, 2, 1, divisions={s: u[2:4] for s, u in ht.used.items()})
        again = hypertile_oracle.unet_forward(cfg, sd, x, t, ehs, None, given)
    assert (off - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert (whole - ref).abs().max() <= 1e-12 * ref.abs().max()         # one tile per map: the plain attention
    assert sorted(big.used) == [0, 1, 13, 14, 15] and all(u[2:4] == (1, 1) for u in big.used.values())
    assert sorted(ht.used) == [0, 1, 2, 3, 10, 11, 12, 13, 14, 15]
    assert {u[4] for s, u in ht.used.items() if s in (2, 3, 10, 11, 12)} == {1}
    for s, (Hs, Ws, nh, nw, level) in ht.used.items():
        assert (nh, nw) == hypertile_oracle.plan(Hs, Ws, 4, 2, 0, 0, s)[:2]
    assert torch.equal(on, again)
    assert (on - ref).abs().max() > 1e-3 * ref.abs().max()              # tiling is not a no-op


# ------------------------------------------------------------------------------------------------ pipeline
class TileUNet:
    """The call surface of the engine's UNet the loop uses, without a network: returns 0.1 * sample and records the step
    index each forward ran under."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.config = SimpleNamespace(**cfg.to_dict())
        self.dtype = torch.float32
        self.hypertile = None
        self.step = None
        self.calls = []
        self._graph_on = False

    def to(self, *a, **k):
        return self

    def enable_hypertile(self, tile_size=32, swap_size=2, max_depth=0, seed=0):
        self.hypertile = (tile_size, swap_size, max_depth, seed)
        return self

    def disable_hypertile(self):
        self.hypertile = None
        return self

    def hypertile_step(self, i):
        assert self.hypertile is not None
        self.step = i
        return self

    def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
        self.calls.append(self.step)
        return (0.1 * sample[:, :4],)


def _model(sched="DDIM", refiner=None):
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5), to=lambda d: None)
    m = SDModelWrapper(base=TileUNet(config.tiny_unet()), vae=vae, scheduler=schedulers.DDIMScheduler(), device="cpu",
                       refiner=refiner)
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
    m.enable_hypertile(8, seed=7)
    assert m.base.hypertile == (8, 2, 0, 7)
    assert torch.isfinite(_run(m, 5)).all()
    n = len(m.base.calls)                                               # (PNDM runs the model twice at one timestep)
    assert n >= 5 and m.base.calls == list(range(n))
    m.base.calls.clear()
    _run(m, 3)                                                          # a second loop counts from 0 again
    assert m.base.calls == list(range(len(m.base.calls))) and len(m.base.calls) >= 3
    m.disable_hypertile()
    assert m.base.hypertile is None
    m.base.calls.clear()
    m.base.step = None
    _run(m, 3)
    assert set(m.base.calls) == {None}                                  # off: the loop sets nothing


def test_wrapper_forwards_to_base_and_refiner():
    ref = TileUNet(config.tiny_unet())
    m = _model(refiner=ref)
    m.enable_hypertile(16, 3, 1, 5)
    assert m.base.hypertile == (16, 3, 1, 5) == ref.hypertile
    m.disable_hypertile()
    assert m.base.hypertile is None and ref.hypertile is None
    alone = _model()
    alone.enable_hypertile()
    assert alone.base.hypertile == (32, 2, 0, 0)


# ------------------------------------------------------------------------------------------ argument validation
class _Lib:
    def __init__(self):
        self.calls = []

    def sd_unet_set_hypertile(self, h, *a):
        self.calls.append(a)
        return 0

    def sd_unet_hypertile_step(self, h, i):
        self.calls.append(("step", i))
        return 0


def _shell():
    """A HipUNet2DConditionModel without an engine behind it: the methods under test only reach `_lib` and `_h`."""
    net = HipUNet2DConditionModel.__new__(HipUNet2DConditionModel)
    net._lib, net._h, net._hypertile = _Lib(), None, None
    return net


def test_enable_hypertile_validates_and_records():
    net = _shell()
    for bad in (dict(tile_size=0), dict(tile_size=-1), dict(tile_size=8.0), dict(tile_size=True), dict(swap_size=0),
                dict(swap_size=9), dict(swap_size="2"), dict(max_depth=-1), dict(max_depth=4), dict(seed=-1),
                dict(seed=2 ** 32), dict(seed=1.5)):
        with pytest.raises(ValueError, match="enable_hypertile"):
            net.enable_hypertile(**bad)
    assert net._lib.calls == [] and net.hypertile is None
    net.enable_hypertile(16, swap_size=3, max_depth=1, seed=9)
    assert net.hypertile == (16, 3, 1, 9) and net._lib.calls[-1] == (16, 3, 1, 9)
    net.hypertile_step(2 ** 32 + 5)
    assert net._lib.calls[-1] == ("step", 5)
    net.enable_hypertile()
    assert net.hypertile == (32, 2, 0, 0)
    net.disable_hypertile()
    assert net.hypertile is None and net._lib.calls[-1][0] == 0


def test_settings_survive_rebuild():
    class Net(HipUNet2DConditionModel):
        def __init__(self, cfg=None, device=None):
            self.cfg, self.device = cfg, device
            self._lib, self._h = _Lib(), None
            self._freeu = self._deepcache = self._tome = self._hypertile = None
            self._pag = ()

        def load_state_dict(self, sd):
            return self

    a = Net()
    a.enable_hypertile(8, seed=4)
    b = a.rebuild({})
    assert b is not a and b.hypertile == (8, 2, 0, 4) and b._lib.calls == [(8, 2, 0, 4)]
    a.disable_hypertile()
    assert a.rebuild({}).hypertile is None
