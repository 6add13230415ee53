"""FreeU without a GPU: the test oracle (tests/freeu_oracle.py) against oracle.unet_ref and against the closed form the
engine's kernel computes, the wrapper's enable_freeu / disable_freeu, and the argument checks of the C-ABI."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freeu_oracle  # noqa: E402
from doubles import OracleUNet, OracleVAE  # noqa: E402
from oracle import unet_ref  # noqa: E402
from stablediffusion_amd import config, schedulers, weights  # noqa: E402
from stablediffusion_amd.models import HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper  # noqa: E402

SIZES = [(8, 8), (16, 16), (32, 32), (2, 2), (3, 5), (2, 7), (9, 16), (12, 20), (1, 3), (5, 1)]
FACTORS = (0.9, 0.2, 1.5, 1.6)


def _rel(a, b):
    return (torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b)).item()


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


@pytest.mark.parametrize("sdxl", [False, True])
def test_oracle_with_freeu_off_is_bitwise_unet_ref(sdxl):
    cfg = config.tiny_unet(linear=True, sdxl_cond=True) if sdxl else config.tiny_unet()
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 16, 16, generator=g)
    ehs = torch.randn(2, 77, cfg.cross_attention_dim, generator=g)
    added = {"text_embeds": torch.randn(2, 64, generator=g),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)} if sdxl else None
    with torch.no_grad():
        want = unet_ref.unet_forward(cfg, sd, x, torch.tensor(501.0), ehs, added)
        got = freeu_oracle.unet_forward(cfg, sd, x, torch.tensor(501.0), ehs, added)
        on = freeu_oracle.unet_forward(cfg, sd, x, torch.tensor(501.0), ehs, added, freeu=FACTORS)
        b_only = freeu_oracle.unet_forward(cfg, sd, x, torch.tensor(501.0), ehs, added, freeu=(1.0, 1.0, 1.5, 1.6))
        s_only = freeu_oracle.unet_forward(cfg, sd, x, torch.tensor(501.0), ehs, added, freeu=(0.9, 0.2, 1.0, 1.0))
    assert torch.equal(got, want)
    # either half of FreeU alone moves the output far beyond the 1e-2 bound of the GPU tests
    gaps = [_rel(on, want), _rel(b_only, want), _rel(s_only, want)]
    print("rel-L2 vs plain forward: both %.3f, b only %.3f, s only %.3f" % tuple(gaps))
    assert min(gaps) > 0.1


@pytest.mark.parametrize("H,W", SIZES)
def test_fft_filter_equals_closed_form(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64) + 0.5
    for s in (0.2, 0.0, 2.0, 1.0):
        want = freeu_oracle.fourier_filter(x, 1, s)
        got = freeu_oracle.closed_form_filter(x, s)
        assert want.dtype == torch.float64
        if max(H, W) <= 2 and s == 0.0:
            # every frequency of a map with axes <= 2 is inside the box: the filtered map is exactly zero and a relative
            # error has no denominator, so the closed form's cancellation is measured against the input instead
            assert torch.count_nonzero(want) == 0
            assert (torch.linalg.vector_norm(got) / torch.linalg.vector_norm(x)).item() < 1e-6, (H, W, s)
            continue
        assert _rel(got, want) < 1e-6, (H, W, s)
    assert torch.equal(freeu_oracle.closed_form_filter(x, 1.0), x)


def test_freeu_applies_to_the_first_two_up_blocks_only():
    g = torch.Generator().manual_seed(1)
    h, s = torch.randn(1, 8, 4, 4, generator=g), torch.randn(1, 6, 4, 4, generator=g)
    h0, s0 = freeu_oracle.apply_freeu(0, h, s, FACTORS)
    h1, s1 = freeu_oracle.apply_freeu(1, h, s, FACTORS)
    h2, s2 = freeu_oracle.apply_freeu(2, h, s, FACTORS)
    assert torch.equal(h0[:, :4], h[:, :4] * 1.5) and torch.equal(h0[:, 4:], h[:, 4:])
    assert torch.equal(h1[:, :4], h[:, :4] * 1.6) and torch.equal(h1[:, 4:], h[:, 4:])
    assert h2 is h and s2 is s
    assert _rel(s0, freeu_oracle.fourier_filter(s, 1, 0.9)) == 0 and _rel(s1, freeu_oracle.fourier_filter(s, 1, 0.2)) == 0
    # the DC term is inside the box: the plane mean is scaled by s
    assert torch.allclose(s1.mean(dim=(-2, -1)), 0.2 * s.mean(dim=(-2, -1)), atol=1e-6)


class _FreeuDouble(OracleUNet):
    """OracleUNet with the FreeU switch of the engine's shim: records what reaches it."""

    def __init__(self, cfg, sd, log=None):
        super().__init__(cfg, sd)
        self.log = [] if log is None else log
        self.freeu = None

    def enable_freeu(self, s1, s2, b1, b2):
        self.freeu = (s1, s2, b1, b2)
        self.log.append(("enable", s1, s2, b1, b2))

    def disable_freeu(self):
        self.freeu = None
        self.log.append(("disable",))

    def rebuild(self, sd):
        return _FreeuDouble(self.cfg, sd, self.log)


def test_wrapper_forwards_freeu_to_its_base_and_keeps_it_across_a_lora_rebuild():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    uw = weights.synth_state_dict(weights.unet_manifest(ucfg), seed=4, perturb=0.1)
    vw = weights.synth_state_dict(weights.vae_manifest(vcfg), seed=5, perturb=0.1)
    base = _FreeuDouble(ucfg, uw)
    m = SDModelWrapper(base=base, vae=OracleVAE(vcfg, vw), scheduler=schedulers.DDIMScheduler(), device="cpu",
                       unet_state_dict=uw)
    m.enable_freeu(s1=0.9, s2=0.2, b1=1.5, b2=1.6)             # diffusers' argument order
    assert base.freeu == FACTORS and base.log == [("enable",) + FACTORS]
    key = "mid_block.attentions.0.transformer_blocks.0.attn1.to_q"
    w = uw[key + ".weight"]
    m.load_lora_weights({f"unet.{key}.lora.down.weight": torch.zeros(4, w.shape[1]),
                         f"unet.{key}.lora.up.weight": torch.zeros(w.shape[0], 4)}, adapter_name="a")
    m.apply_adapters()
    assert m.base is not base and m.base.freeu == FACTORS       # the rebuilt base has it again
    m.disable_freeu()
    assert m.base.freeu is None and m.base.log[-1] == ("disable",)
    m.set_adapters(["a"], [0.5])
    m.apply_adapters()
    assert m.base.freeu is None


def test_non_finite_factors_raise(engine_lib):
    net = HipUNet2DConditionModel(config.tiny_unet())
    for bad in (float("nan"), float("inf"), -float("inf")):
        for pos in range(4):
            vals = [0.9, 0.2, 1.5, 1.6]
            vals[pos] = bad
            with pytest.raises(ValueError):
                net.enable_freeu(*vals)
            assert engine_lib.sd_unet_set_freeu(net._h, 1, *vals) == 1
            assert b"finite" in engine_lib.sd_last_error()
            assert engine_lib.sd_unet_set_freeu(net._h, 0, *vals) == 0     # enable = 0 ignores the factors
    assert net._freeu is None
    net.enable_freeu(*FACTORS)
    assert net._freeu == FACTORS
    net.disable_freeu()
    assert net._freeu is None
    assert engine_lib.sd_unet_set_freeu(None, 1, *FACTORS) == 1


def test_op_rejects_what_it_does_not_support(engine_lib):
    buf = torch.zeros(64, dtype=torch.float16)
    p = buf.data_ptr()
    assert engine_lib.sd_op_freeu(None, 1, 2, 2, 4, 4, 1.5, 0.2, None) == 1
    assert engine_lib.sd_op_freeu(p, 1, 2, 2, 3, 4, 1.5, 0.2, None) == 1          # odd C1
    assert engine_lib.sd_op_freeu(p, 1, 2, 2, 4, 0, 1.5, 0.2, None) == 1          # no skip channels
    assert engine_lib.sd_op_freeu(p, 0, 2, 2, 4, 4, 1.5, 0.2, None) == 1
    assert engine_lib.sd_op_freeu(p, 1, 2, 2, 4, 4, float("nan"), 0.2, None) == 1
    assert engine_lib.sd_op_freeu(p, 1, 2, 2, 4, 4, 1.5, float("inf"), None) == 1
    assert engine_lib.sd_op_freeu(p, 1, 4000, 200, 4, 4, 1.5, 0.2, None) == 4     # beyond the twiddle table
    assert b"freeu" in engine_lib.sd_last_error()
