#!/usr/bin/env python3
"""Generates tests/golden/call_refusals.json: which calls of StableDiffusionUnifiedPipeline are refused, with what
exception and message, and what a refused call had already touched.  tests/test_call_refusals.py replays every case
through the same harness and compares, so the rule for which feature combinations run is pinned as a whole and not
feature by feature.

    python tests/golden/make_call_refusals.py         # rewrites the fixture from the pipeline as it stands

The committed fixture was written by the pipeline as it stood BEFORE the refusals were gathered into
stablediffusion_amd/combos.py (every feature then raised its own, in seven places), so it pins the table to that
behaviour and not to itself.  Regenerate only when a combination is meant to change, and review the fixture's diff.

The harness runs on the CPU: one tiny model of test doubles (tests/doubles.py, tests/refiner_doubles.py, a
region-capable UNet like tests/region_oracle.py's), 64 x 64 px / 8 x 8 latents, embeddings and latents given.  Every
UNet double raises `Reached` on its first forward, so a call that is not refused ends there.  A SWITCH turns one fact on
the way the feature suites do.  The cases are every switch alone with CFG on and with CFG off, every unordered pair
with CFG on (but UNBUILDABLE), and HAND: what a raise of the pipeline needs beyond two switches to be reached.

Per case the fixture holds [id, outcome, untouched]: outcome is ["reached the forward"], [exception type, message] or, for a
loop left with no step, ["returned without a forward"];
untouched (refused cases only) says which of UNTOUCHED had not happened when the call raised.
"""
import itertools
import json
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "call_refusals.json")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from doubles import OracleUNet                                               # noqa: E402
from refiner_doubles import RecordingUNet, StubTextEncoder, StubTokenizer    # noqa: E402
from stablediffusion_amd import config                                       # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline      # noqa: E402

REACHED, RETURNED = "reached the forward", "returned without a forward"
# what a refused call must not have done, where the fixture says it had not: UNet.set_regions, SDModelWrapper.
# apply_adapters (where a LoRA re-fuse rebuilds .base), StableDiffusionUnifiedPipeline.encode_prompt, a UNet forward
UNTOUCHED = ("set_regions", "apply_adapters", "encode_prompt", "forward")


class Reached(Exception):
    """Raised by the UNet doubles' forward: the call was not refused."""


class _PlainUNet(OracleUNet):
    """`.base` without the engine's regional surface (what a torch module or the plain oracle double is)."""

    def __init__(self, cfg, log):
        super().__init__(cfg, None)
        self.log = log

    def deep_cache_mode(self, mode):
        return self

    def __call__(self, *a, **k):
        self.log.append("forward")
        raise Reached()


class _RegionUNet(_PlainUNet):
    def set_regions(self, weights):
        self.log.append("set_regions")
        return self

    def clear_regions(self):
        return self


class _Refiner(RecordingUNet):
    def __call__(self, *a, **k):
        self.log.append("forward")
        raise Reached()


def _tensors():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    masks = torch.zeros(2, 64, 64)
    masks[0, :, 8:24] = 1.0
    masks[1, :, 24:40] = 1.0
    return SimpleNamespace(latents=r(1, 4, 8, 8), pe=r(1, 77, 64), ne=r(1, 77, 64), pooled=r(1, 64), npooled=r(1, 64),
                           region=[r(1, 77, 64), r(1, 77, 64)], masks=masks, image=r(1, 4, 8, 8), ip=r(1, 1, 64),
                           control=torch.zeros(1, 3, 64, 64), mask=torch.ones(1, 1, 64, 64))


T = _tensors()              # read-only: shared by every case
_TINY = config.tiny_unet().to_dict()


def _diff(cfg):
    return {k: v for k, v in cfg.to_dict().items() if v != _TINY[k]}


def _set(attr, value, on="base"):
    """The switch sets m.<on>.<attr> (on the object, as tests/test_regions.py does), or m.<attr> for on=None."""
    def apply(m):
        setattr(m if on is None else getattr(m, on), attr, value)
    return apply


def _no_enc2(m):
    del m.text_encoder_2, m.tokenizer_2


# name -> (call arguments, UNet configuration fields, change to the model after it is built)
SWITCHES = {
    # ---- call arguments
    "regions": (dict(region_masks=T.masks, region_prompt_embeds=T.region), {}, None),
    "view_window": (dict(view_window=8), {}, None),
    "pag": (dict(pag_scale=2.0), {}, None),
    "use_refiner": (dict(use_refiner=True, image=T.image), {}, None),
    "refiner_start": (dict(refiner_start=0.6), {}, None),
    "ip_embeds": (dict(ip_adapter_image_embeds=[T.ip]), {}, None),
    "control_image": (dict(control_image=T.control), {}, None),                 # (no ControlNet loaded)
    "guess_mode": (dict(guess_mode=True), {}, None),
    "mask_image": (dict(mask_image=T.mask, image=T.image), {}, None),
    "guidance_rescale": (dict(guidance_rescale=0.5), {}, None),
    "image_guidance_scale": (dict(image_guidance_scale=1.5), {}, None),
    "strength": (dict(strength=0.5, image=T.image), {}, None),
    "denoising_end": (dict(denoising_end=0.8), {}, None),
    # ---- wrapper state
    "cn_loaded+image": (dict(control_image=T.control), {}, _set("_cn", (None, {}), on=None)),   # what load_controlnet leaves
    "cn_loaded": ({}, {}, _set("_cn", (None, {}), on=None)),
    "no_refiner": ({}, {}, _set("refiner", None, on=None)),
    "no_text_encoder_2": ({}, {}, _no_enc2),
    # ---- UNet attributes, on m.base
    "deepcache": ({}, {}, _set("deepcache", (3, 1))),
    "tome": ({}, {}, _set("tome", (0.5, 1, 2, 2, True, 0))),
    "graph": ({}, {}, _set("_graph_on", True)),
    "freeu": ({}, {}, _set("_freeu", (0.9, 0.2, 1.2, 1.4))),
    "unet_ip": ({}, {}, lambda m: (_set("_ip", object())(m), _set("_ip_scale", 1.0)(m))),
    "unet_ip_scale0": ({}, {}, lambda m: (_set("_ip", object())(m), _set("_ip_scale", 0.0)(m))),
    "unet_cn": ({}, {}, _set("_cn", object())),
    "plain_unet": ({}, {}, None),                                                # (handled in build: no set_regions)
    # ---- UNet configuration
    "in_channels_8": ({}, dict(in_channels=8), None),
    "in_channels_9": ({}, dict(in_channels=9), None),
    "text_time": ({}, _diff(config.tiny_unet(sdxl_cond=True)), None),
    "time_cond": ({}, _diff(config.tiny_unet(time_cond=32)), None),
    # ---- only in HAND cases: what some raises need besides two switches
    "prompt": (dict(prompt="a cat", negative_prompt="", prompt_embeds=None, negative_prompt_embeds=None), {}, None),
    "image": (dict(image=T.image), {}, None),
}
HAND_ONLY = ("prompt", "image")

# pairs that set one attribute to two values: they cannot be built.  No other pair is left out
UNBUILDABLE = {
    ("in_channels_8", "in_channels_9"): "config.in_channels is 8 or 9",
    ("unet_ip", "unet_ip_scale0"): "base._ip_scale is 1.0 or 0.0",
    ("cn_loaded+image", "cn_loaded"): "control_image is given or it is not",
    ("control_image", "cn_loaded+image"): "model._cn is None or loaded",
    ("control_image", "cn_loaded"): "model._cn is None or loaded (with control_image this is cn_loaded+image)",
}

# (id, switches, further call arguments, CFG, why): raises that one or two switches do not reach
HAND = [
    ("use_refiner+no_text_encoder_2+prompt", ("use_refiner", "no_text_encoder_2", "prompt"), {}, True,
     "the refiner's text encoder is only read when the call has to encode a prompt"),
    ("use_refiner/no_image", ("use_refiner",), dict(image=None), True, "use_refiner=True without image="),
    ("refiner_start+prompt", ("refiner_start", "prompt"), {}, True,
     "with prompt_embeds= every refiner_start call ends at 'refiner_start needs prompts'; this one hands off"),
    ("refiner_start+prompt+mask_image", ("refiner_start", "prompt", "mask_image"), {}, True, "the same, for inpainting"),
    ("refiner_start+prompt+no_text_encoder_2", ("refiner_start", "prompt", "no_text_encoder_2"), {}, True,
     "so that the hand-off's own text_encoder_2 check is not only seen behind 'needs prompts'"),
    ("refiner_start+prompt/out_of_range", ("refiner_start", "prompt"), dict(refiner_start=1.0), True, "refiner_start's bounds"),
    ("tome+in_channels_8+image", ("tome", "in_channels_8", "image"), {}, True,
     "an edit UNet without image= is refused before the token-merging block"),
    ("in_channels_8+image", ("in_channels_8", "image"), {}, True, "InstructPix2Pix as it runs"),
    ("in_channels_8+image+masked_image_latents", ("in_channels_8", "image"), dict(masked_image_latents=T.image), True,
     "the other half of 'takes no mask_image'"),
    ("in_channels_8+image/igs_nan", ("in_channels_8", "image"), dict(image_guidance_scale=float("nan")), True,
     "image_guidance_scale must be finite"),
    ("in_channels_8+image+strength", ("in_channels_8", "strength"), {}, True, "'there is no strength' needs image="),
    ("in_channels_8+image+guidance_rescale", ("in_channels_8", "image", "guidance_rescale"), {}, True,
     "'takes no guidance_rescale' needs image="),
] + [
    ("in_channels_8+image+" + s, ("in_channels_8", "image", s), {}, True, "InstructPix2Pix x %s needs image=" % s)
    for s in ("use_refiner", "refiner_start", "cn_loaded", "control_image", "ip_embeds", "pag", "deepcache", "text_time",
              "time_cond", "regions", "view_window")
] + [
    ("pag/nan_adaptive", ("pag",), dict(pag_adaptive_scale=float("nan")), True, "pag_adaptive_scale must be finite"),
    ("cn_loaded+image/list_scale", ("cn_loaded+image",), dict(controlnet_conditioning_scale=[1.0]), True, "MultiControlNet"),
    ("cn_loaded+image/window", ("cn_loaded+image",), dict(control_guidance_start=0.5, control_guidance_end=0.5), True,
     "the guidance window's bounds"),
    ("guidance_rescale/out_of_range", (), dict(guidance_rescale=1.5), True, "guidance_rescale in [0, 1]"),
    ("view_window/zero", (), dict(view_window=0), True, "view_window must be positive"),
    ("view_window/stride", ("view_window",), dict(view_stride=0), True, "view_stride >= 1"),
    ("view_window/batch", ("view_window",), dict(view_batch_size=0), True, "view_batch_size >= 1"),
    ("view_window/blend", ("view_window",), dict(view_blend="cubic"), True, "an unknown view_blend"),
    ("regions/no_masks", ("regions",), dict(region_masks=None), True, "regional arguments that contradict each other"),
    ("regions/str_prompts", ("regions",), dict(region_prompts="a cat", region_prompt_embeds=None), True, "the same"),
    ("regions/too_many", ("regions",), dict(region_prompt_embeds=T.region * 4, region_masks=torch.zeros(8, 64, 64)), True,
     "the same"),
    ("regions/empty", ("regions",), dict(region_prompt_embeds=[]), True, "the same"),
    ("regions/count", ("regions",), dict(region_masks=T.masks[:1]), True, "the same"),
    ("regions/mask_shape", ("regions",), dict(region_masks=torch.zeros(2, 2, 64, 64)), True, "the same"),
    ("regions/base_weight", ("regions",), dict(region_base_weight=-0.5), True, "the same"),
    ("regions/prompts_with_embeds", ("regions",), dict(region_prompts=["a cat", "a dog"], region_prompt_embeds=None), True,
     "prompt_embeds= with region_prompts="),
    ("regions+prompt", ("regions", "prompt"), {}, True, "prompt= with region_prompt_embeds="),
]


def build(names, cfg_on, extra=None):
    """The model, pipeline and call arguments of one case; `log` collects what of UNTOUCHED happens."""
    log = []
    fields = dict(_TINY)
    for n in names:
        fields.update(SWITCHES[n][1])
    ucfg = config.UNetConfig(**fields)
    base = (_PlainUNet if "plain_unet" in names else _RegionUNet)(ucfg, log)
    refiner = _Refiner(config.tiny_refiner_unet())
    refiner.log = log
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(1, 1, 1, 1), scaling_factor=0.5, latent_channels=4),
                          to=lambda d: None)
    m = SDModelWrapper(base=base, vae=vae, text_encoder=StubTextEncoder(64, 64, 1), tokenizer=StubTokenizer(),
                       text_encoder_2=StubTextEncoder(64, 64, 2), tokenizer_2=StubTokenizer(), model_type="sdxl",
                       refiner=refiner, device="cpu")
    kw = dict(prompt_embeds=T.pe, negative_prompt_embeds=T.ne, pooled_prompt_embeds=T.pooled,
              negative_pooled_prompt_embeds=T.npooled, latents=T.latents, num_inference_steps=2, height=64, width=64)
    for n in names:
        kw.update(SWITCHES[n][0])
        if SWITCHES[n][2] is not None:
            SWITCHES[n][2](m)
    kw.update(extra or {})
    pipe = StableDiffusionUnifiedPipeline(do_cfg=cfg_on, device="cpu", output_type="latents")
    apply_adapters, encode_prompt = m.apply_adapters, pipe.encode_prompt
    m.apply_adapters = lambda: (log.append("apply_adapters"), apply_adapters())[1]
    pipe.encode_prompt = lambda *a, **k: (log.append("encode_prompt"), encode_prompt(*a, **k))[1]
    return m, pipe, kw, log


def run(names, cfg_on, extra=None):
    """-> (outcome, untouched): [REACHED] or [type name, message]; for a refused call, what of UNTOUCHED is not in the log."""
    m, pipe, kw, log = build(names, cfg_on, extra)
    try:
        pipe(m, **kw)
    except Reached:
        return [REACHED], None
    except Exception as e:               # noqa: BLE001 (whatever the call raises is the record)
        return [type(e).__name__, str(e)], {k: k not in log for k in UNTOUCHED}
    return [RETURNED], None           # (a loop of no steps: strength x denoising_end leave none of the two)


def cases():
    """(id, switches, further arguments, CFG) of every case, in the fixture's order."""
    paired = [n for n in SWITCHES if n not in HAND_ONLY]
    out = [(n, (n,), {}, True) for n in paired]
    out += [(n + "/no_cfg", (n,), {}, False) for n in paired]
    for a, b in itertools.combinations(paired, 2):
        if (a, b) not in UNBUILDABLE and (b, a) not in UNBUILDABLE:
            out.append((a + "+" + b, (a, b), {}, True))
    out += [(cid, names, extra, cfg_on) for cid, names, extra, cfg_on, _ in HAND]
    out.append(("plain", (), {}, True))
    assert len({c[0] for c in out}) == len(out)
    return out


def main():
    rows = []
    for cid, names, extra, cfg_on in cases():
        outcome, untouched = run(names, cfg_on, extra)
        rows.append([cid, outcome] if untouched is None else [cid, outcome, untouched])
    doc = {"untouched": list(UNTOUCHED), "unbuildable": [[a, b, why] for (a, b), why in UNBUILDABLE.items()], "cases": rows}
    with open(OUT, "w") as f:
        f.write("{\n")
        f.write('"untouched": %s,\n' % json.dumps(doc["untouched"]))
        f.write('"unbuildable": %s,\n' % json.dumps(doc["unbuildable"]))
        f.write('"cases": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]\n}\n")
    refused = sum(1 for r in rows if len(r) == 3)
    print("%d cases, %d refused with %d distinct messages -> %s" % (len(rows), refused,
                                                                    len({tuple(r[1]) for r in rows if len(r) == 3}), OUT))


if __name__ == "__main__":
    main()
