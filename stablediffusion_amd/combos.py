"""Which pipeline calls are refused: the facts of one call, and one ordered table of the combinations that are not built.

`call_facts` reads the call's arguments, the wrapper and its UNets once; `refuse` raises the first row of REFUSALS whose
facts all hold.  Nothing else in the pipeline decides whether two features run together: a feature's own checker
validates its own arguments (counts, ranges, shapes) and no more.  A new feature adds its facts and its rows here.

Where two readings of "X is in play" can differ they are two facts: a ControlNet loaded on the wrapper, a control_image
given, a ControlNet attached to the UNet that runs; an IP-Adapter image given, an adapter attached, an adapter attached
at a non-zero scale; the state of `model.base` (`base_*`) and of the UNet this call runs (`run_*`: the refiner under
use_refiner=True).  The order of the rows is the order the checks had when every feature raised its own: it decides
which refusal a call that breaks two rules reports (tests/golden/call_refusals.json pins it).
"""
from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple

from . import pix2pix as _p2p


def guidance_embed_dim(unet) -> int:
    """`time_cond_proj_dim` of a guidance-embedded UNet, 0 for every other."""
    return int(getattr(getattr(unet, "config", None), "time_cond_proj_dim", None) or 0)


def _given(c, *names) -> bool:
    return any(c.kw[n] is not None for n in names)


def _on(unet, attr) -> bool:
    return getattr(unet, attr, None) is not None


def _cfg(unet, field, default=None):
    return getattr(getattr(unet, "config", None), field, default)


# name -> how the fact is read from c = (kw: the call's arguments, model, base: model.base, run: the UNet the call runs)
FACTS = {
    # ---- the call's arguments
    "regional": lambda c: _given(c, "region_prompts", "region_masks", "region_prompt_embeds"),
    "views": lambda c: _given(c, "view_window"),                                # MultiDiffusion
    "pag": lambda c: _given(c, "pag_scale") and float(c.kw["pag_scale"]) > 0.0,
    "use_refiner": lambda c: bool(c.kw["use_refiner"]),
    "refiner_start": lambda c: _given(c, "refiner_start"),
    "ip_image": lambda c: _given(c, "ip_adapter_image", "ip_adapter_image_embeds"),
    "control_image": lambda c: _given(c, "control_image"),
    "guess_mode": lambda c: bool(c.kw["guess_mode"]),
    "image": lambda c: _given(c, "image"),
    "mask_image": lambda c: _given(c, "mask_image"),
    "masked_image_latents": lambda c: _given(c, "masked_image_latents"),
    "strength": lambda c: c.kw["strength"] != 1.0,
    "guidance_rescale": lambda c: _given(c, "guidance_rescale") and float(c.kw["guidance_rescale"]) > 0.0,
    "image_guidance_scale": lambda c: _given(c, "image_guidance_scale"),
    "denoising_end": lambda c: _given(c, "denoising_end"),
    "prompt_embeds": lambda c: _given(c, "prompt_embeds"),
    # ---- the wrapper
    "cn_loaded": lambda c: bool(getattr(c.model, "has_controlnet", False)),     # SDModelWrapper.load_controlnet
    "has_refiner": lambda c: _on(c.model, "refiner"),
    "has_text_encoder_2": lambda c: _on(c.model, "text_encoder_2") and _on(c.model, "tokenizer_2"),
    # ---- model.base
    "edit": lambda c: _p2p.is_edit_unet(getattr(c.base, "config", None)),       # 8 channels: the call is InstructPix2Pix
    "base_inpaint": lambda c: int(_cfg(c.base, "in_channels", 4)) == 9,
    "base_4ch": lambda c: int(_cfg(c.base, "in_channels", 4)) == 4,
    "base_text_time": lambda c: _cfg(c.base, "addition_embed_type") == "text_time",     # SDXL
    "base_time_cond": lambda c: guidance_embed_dim(c.base) > 0,                 # guidance-embedded (LCM)
    "base_deepcache": lambda c: _on(c.base, "deepcache"),
    "base_tome": lambda c: _on(c.base, "tome"),
    "base_graph": lambda c: bool(getattr(c.base, "_graph_on", False)),
    "base_ip_scaled": lambda c: _on(c.base, "_ip") and float(getattr(c.base, "_ip_scale", 1.0)) != 0.0,
    "base_set_regions": lambda c: hasattr(c.base, "set_regions") and hasattr(c.base, "clear_regions"),
    # ---- the UNet this call runs
    "run_tome": lambda c: _on(c.run, "tome"),
    "run_edit": lambda c: _p2p.is_edit_unet(getattr(c.run, "config", None)),
    "run_graph": lambda c: bool(getattr(c.run, "_graph_on", False)),
    "run_freeu": lambda c: _on(c.run, "_freeu"),
    "run_cn": lambda c: _on(c.run, "_cn"),
    "run_ip": lambda c: _on(c.run, "_ip"),
}
# the facts of one call, all booleans; base_type is no fact: the class name one message quotes
CallFacts = namedtuple("CallFacts", list(FACTS) + ["base_type"])
_Call = namedtuple("_Call", "kw model base run")


def call_facts(pipe, model, **kw) -> CallFacts:
    """The facts of `pipe(model, **kw)`; `kw` holds every argument a fact reads (pipe._use_refiner is already this call's)."""
    c = _Call(kw, model, getattr(model, "base", None), pipe._unet(model))
    return CallFacts(*(bool(read(c)) for read in FACTS.values()), base_type=type(c.base).__name__)


class Row(NamedTuple):
    """Refused when every entry of `when` holds: "fact", "!fact" (absent), or a tuple of facts of which one holds."""
    when: tuple
    exc: type
    message: str                # ({base_type}: CallFacts.base_type)


_NI, _VE = NotImplementedError, ValueError
_REFINER = ("use_refiner", "refiner_start")         # "addresses the refiner"
_CN = ("cn_loaded", "control_image")                # "a ControlNet is in play", as most features read it
_EXTRA_CH = ("edit", "base_inpaint")                # an 8- or 9-channel UNet
_TOME = "token merging (enable_tome) with %s is not supported yet: the engine's forward refuses the combination (disable_tome)"

REFUSALS = (
    # ---- regional prompts (they read model.base)
    Row(("regional", _CN), _NI, "regional prompts with a ControlNet loaded are not supported (unload_controlnet)"),
    Row(("regional", "ip_image"), _NI, "regional prompts with an IP-Adapter image are not supported"),
    Row(("regional", "pag"), _NI, "regional prompts with perturbed-attention guidance (pag_scale > 0) are not supported"),
    Row(("regional", "views"), _NI, "regional prompts with view_window (MultiDiffusion) are not supported"),
    Row(("regional", _REFINER), _NI, "regional prompts do not address the refiner"),
    Row(("regional", "base_deepcache"), _NI, "regional prompts with DeepCache enabled are not supported (disable_deepcache)"),
    Row(("regional", "base_tome"), _NI, "regional prompts with token merging enabled are not supported (disable_tome)"),
    Row(("regional", "base_graph"), _NI, "regional prompts under use_graph are not supported"),
    Row(("regional", "base_ip_scaled"), _NI,
        "regional prompts with an IP-Adapter attached at a non-zero scale are not supported"),
    Row(("regional", _EXTRA_CH), _NI, "regional prompts with an 8- or 9-channel UNet are not supported"),
    Row(("regional", "base_time_cond"), _NI,
        "regional prompts with a guidance-embedded UNet (time_cond_proj_dim) are not supported"),
    Row(("regional", "!base_set_regions"), _NI, "{base_type} has no set_regions: regional prompts need the engine's UNet"),
    # ---- MultiDiffusion
    Row(("views", _REFINER), _NI, "view_window (MultiDiffusion) does not address the refiner"),
    Row(("views", _CN), _NI, "view_window (MultiDiffusion) with a ControlNet loaded is not supported "
                             "(unload_controlnet): the control image would need windows of its own"),
    Row(("views", "ip_image"), _NI, "view_window (MultiDiffusion) with an IP-Adapter image is not supported"),
    Row(("views", "pag"), _NI, "view_window (MultiDiffusion) with perturbed-attention guidance (pag_scale > 0) is not supported"),
    Row(("views", "base_deepcache"), _NI, "view_window (MultiDiffusion) with DeepCache enabled is not supported: one cached "
                                          "feature cannot serve several windows (disable_deepcache)"),
    Row(("views", _EXTRA_CH), _NI, "view_window (MultiDiffusion) with an 8- or 9-channel UNet is not supported: the extra "
                                   "channels would need windows of their own"),
    Row(("views", "base_text_time"), _NI, "view_window (MultiDiffusion) on a text_time (SDXL) UNet is not supported: every "
                                          "window would need its own crop conditioning"),
    Row(("views", "base_time_cond"), _NI,
        "view_window (MultiDiffusion) on a guidance-embedded UNet (time_cond_proj_dim) is not supported"),
    Row(("views", "guidance_rescale"), _VE, "view_window (MultiDiffusion) takes no guidance_rescale: its per-sample statistic "
                                            "differs between a window and the canvas"),
    # ---- InstructPix2Pix: an 8-channel model.base selects it
    Row(("image_guidance_scale", "!edit"), _VE, "image_guidance_scale is InstructPix2Pix's: it needs a UNet with in_channels == 8"),
    Row(("edit", ("mask_image", "masked_image_latents")), _VE, "InstructPix2Pix takes no mask_image (it edits the whole picture)"),
    Row(("edit", "strength"), _VE, "InstructPix2Pix starts from pure noise: there is no strength"),
    Row(("edit", "guidance_rescale"), _VE, "InstructPix2Pix takes no guidance_rescale"),
    Row(("edit", "!image"), _VE, "InstructPix2Pix (a UNet with in_channels == 8) needs image=, the picture to edit"),
    Row(("edit", _REFINER), _NI, "InstructPix2Pix does not address the refiner"),
    Row(("edit", _CN), _NI, "InstructPix2Pix with a ControlNet loaded is not supported (unload_controlnet)"),
    Row(("edit", "ip_image"), _NI, "InstructPix2Pix with an IP-Adapter image is not supported"),
    Row(("edit", "pag"), _NI, "InstructPix2Pix with perturbed-attention guidance (pag_scale > 0) is not supported"),
    Row(("edit", "base_deepcache"), _NI, "InstructPix2Pix with DeepCache enabled is not supported (disable_deepcache)"),
    Row(("edit", "base_text_time"), _NI, "InstructPix2Pix on a text_time (SDXL edit) UNet is not supported"),
    Row(("edit", "base_time_cond"), _NI, "InstructPix2Pix on a guidance-embedded UNet (time_cond_proj_dim) is not supported"),
    # ---- the refiner: refiner_start (base, then refiner, in one call) and use_refiner (the refiner's half alone)
    Row(("pag", _REFINER), _NI, "perturbed-attention guidance (pag_scale > 0) does not address the refiner"),
    Row(("refiner_start", "use_refiner"), _VE,
        "refiner_start runs base and refiner in one call: it cannot be combined with use_refiner=True"),
    Row(("refiner_start", "denoising_end"), _VE, "refiner_start sets the base's denoising_end itself: pass one or the other"),
    Row(("refiner_start", "!has_refiner"), _VE, "refiner_start given but the model has no refiner (SDModelWrapper.load_refiner)"),
    Row(("refiner_start", "!has_text_encoder_2"), _VE,
        "the refiner reads text_encoder_2 / tokenizer_2, which this model does not have"),
    Row(("refiner_start", "prompt_embeds"), _VE, "refiner_start needs prompts: base and refiner take different embeddings"),
    Row(("refiner_start", "mask_image"), _NI, "refiner_start with inpainting is not supported"),
    # ---- perturbed-attention guidance, ControlNet's guess mode
    Row(("pag", "ip_image"), _NI, "perturbed-attention guidance (pag_scale > 0) with an IP-Adapter image is not supported"),
    Row(("pag", "cn_loaded"), _NI,
        "perturbed-attention guidance (pag_scale > 0) with a ControlNet loaded is not supported (unload_controlnet)"),
    Row(("guess_mode",), _NI, "ControlNet guess_mode is not supported"),
    Row(("use_refiner", "!has_refiner"), _VE, "use_refiner=True but the model has no refiner (SDModelWrapper.load_refiner)"),
    Row(("use_refiner", "!prompt_embeds", "!has_text_encoder_2"), _VE,
        "the refiner reads text_encoder_2 / tokenizer_2, which this model does not have"),
    Row(("use_refiner", ("control_image", "ip_image")), _VE,
        "the refiner takes no ControlNet or IP-Adapter inputs (they belong to model.base)"),
    Row(("use_refiner", "!image"), _VE,
        "use_refiner=True is an image-to-image call: image= (pixels or 4-channel latents) is required"),
    # ---- ControlNet: loaded and given an image, or neither (the refiner's half runs without the base's)
    Row(("control_image", "!cn_loaded"), _VE, "control_image given but no ControlNet is loaded (SDModelWrapper.load_controlnet)"),
    Row(("cn_loaded", "!use_refiner", "!control_image"), _VE,
        "a ControlNet is loaded: control_image is required (or unload_controlnet)"),
    # ---- token merging on the UNet that runs: what the engine's forward refuses
    Row(("run_tome", "pag"), _NI,
        "token merging (enable_tome) with perturbed-attention guidance (pag_scale > 0) is not supported (disable_tome)"),
    Row(("run_tome", "run_edit"), _NI, "token merging (enable_tome) with an 8-channel edit UNet is not supported: its "
                                       "two-source forward runs without it (disable_tome)"),
    Row(("run_tome", "run_graph"), _NI, "token merging (enable_tome) under use_graph is not supported (disable_tome)"),
    Row(("run_tome", "views"), _NI, "token merging (enable_tome) with view_window (MultiDiffusion) is not supported (disable_tome)"),
    Row(("run_tome", "run_freeu"), _NI, _TOME % "FreeU enabled"),
    Row(("run_tome", "run_cn"), _NI, _TOME % "a ControlNet loaded"),
    Row(("run_tome", "run_ip"), _NI, _TOME % "an IP-Adapter loaded"),
    # ---- (from here on a call with pag or a ControlNet in use runs model.base: the rows above refused the refiner)
    Row(("pag", "base_deepcache"), _NI, "perturbed-attention guidance (pag_scale > 0) with DeepCache enabled is not "
                                        "supported: a reuse step skips the perturbed layers (disable_deepcache)"),
    Row(("pag", "base_inpaint"), _NI, "perturbed-attention guidance (pag_scale > 0) with a 9-channel inpaint UNet is not supported"),
    Row(("pag", "base_time_cond"), _NI,
        "perturbed-attention guidance (pag_scale > 0) with a guidance-embedded UNet (time_cond_proj_dim) is not supported"),
    Row(("cn_loaded", "!use_refiner", "base_time_cond"), _NI,
        "a guidance-embedded UNet (time_cond_proj_dim) with a ControlNet is not supported"),
    Row(("cn_loaded", "!use_refiner", "!base_4ch"), _VE,
        "ControlNet needs a 4-channel UNet (9-channel inpaint UNets are not supported)"),
    Row(("cn_loaded", "!use_refiner", "base_deepcache"), _VE,
        "DeepCache runs no ControlNet on its reuse steps: disable_deepcache() or drop control_image"),
)


def _holds(facts, cond) -> bool:
    if isinstance(cond, tuple):
        return any(getattr(facts, c) for c in cond)
    return not getattr(facts, cond[1:]) if cond[0] == "!" else getattr(facts, cond)


def matching(facts):
    """The first row of REFUSALS that applies, or None."""
    return next((row for row in REFUSALS if all(_holds(facts, c) for c in row.when)), None)


def refuse(facts) -> None:
    row = matching(facts)
    if row is not None:
        raise row.exc(row.message.format(base_type=facts.base_type))


# ---- the documented matrix: which features a row names, by the facts it asks for
FEATURES = (
    ("regional prompts", ("regional",)),
    ("MultiDiffusion", ("views",)),
    ("PAG", ("pag",)),
    ("refiner", _REFINER),
    ("IP-Adapter", ("ip_image", "base_ip_scaled", "run_ip")),
    ("ControlNet", ("cn_loaded", "control_image", "run_cn")),
    ("InstructPix2Pix", ("edit", "run_edit")),
    ("DeepCache", ("base_deepcache",)),
    ("ToMe", ("base_tome", "run_tome")),
    ("graph replay", ("base_graph", "run_graph")),
    ("FreeU", ("run_freeu",)),
    ("LCM UNet", ("base_time_cond",)),
    ("SDXL UNet", ("base_text_time",)),
    ("inpaint UNet", ("base_inpaint", "!base_4ch")),
    ("inpainting", ("mask_image", "masked_image_latents")),
    ("strength", ("strength",)),
    ("guidance_rescale", ("guidance_rescale",)),
    ("denoising_end", ("denoising_end",)),
)


def render_matrix() -> str:
    """The feature x feature table of INTEGRATION.md, in Markdown: `x` where a row of REFUSALS asks for a fact of both
    features (some form of the pair is refused; the row says which), `.` where the pair runs."""
    alts = lambda cond: set(cond if isinstance(cond, tuple) else (cond,))

    def hit(a, b):                       # two different conditions of one row: one names feature a, the other b
        return any(alts(c) & set(a) and alts(d) & set(b) for row in REFUSALS for c in row.when for d in row.when if c is not d)
    names = [n for n, _ in FEATURES]
    lines = ["| | " + " | ".join(str(i + 1) for i in range(len(names))) + " |", "|---|" + "---|" * len(names)]
    for i, (name, fa) in enumerate(FEATURES):
        cells = ["-" if i == j else "x" if hit(fa, fb) else "." for j, (_, fb) in enumerate(FEATURES)]
        lines.append("| %d %s | %s |" % (i + 1, name, " | ".join(cells)))
    return "\n".join(lines)


assert {c.lstrip("!") for row in REFUSALS for cond in row.when for c in (cond if isinstance(cond, tuple) else (cond,))} \
    <= set(FACTS), "a row of REFUSALS names a fact CallFacts does not have"
