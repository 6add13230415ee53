"""Host-side mirror of the reference's pipeline surface, driving the gfx950 engine.

`StableDiffusionUnifiedPipeline` keeps the constructor and the 26 `__call__` keyword arguments of
`/root/reference/pipelines/sd_unified_pipeline.py:116-166` and the same control flow for the
txt2img (`:216-231`) and img2img (`:236-264`) branches, the denoise loop (`:465-507`) and the VAE
decode (`:511-523`); `SDModelWrapper` keeps the attribute surface of
`/root/reference/models/stable_diffusion.py:40-103,187-227` (`.base .vae .text_encoder .tokenizer
.scheduler .vae_scale_factor .device .set_scheduler`).  What sits in `.base` / `.vae` is the HIP
engine (stablediffusion_amd.models) instead of diffusers modules.

Differences from the reference, on purpose:
  * `prompt_embeds= / negative_prompt_embeds= / pooled_*` are accepted (superset): the build box has
    no tokenizer vocabulary or CLIP weights, and the benchmark feeds synthetic embeddings.  The
    reference raises when `prompt is None` (`:565`).
  * reference defects listed in SURVEY.md §8b (relative import, tqdm.notebook, unbound `generator`,
    …) are not reproduced.  Quirk kept: the `output_type` kwarg is ignored, the constructor's wins.
  * inpainting (`:268-380`, `:492-506`): tensors only (image in [-1,1], mask in [0,1]; no PIL
    resize / `padding_mask_crop`).  4-channel UNets blend with the re-noised original latents as the
    reference does; 9-channel inpaint UNets get `[latents | mask | masked-image latents]`
    concatenated before the UNet, which the reference omits (`:465-482`, listed as a defect).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Union

import torch

from . import _lib, combos as _combos, pag as _pag, pix2pix as _p2p, regions as _regions, schedulers as _sched, views as _views
from .image_processor import VaeImageProcessor


class SDModelWrapper:
    """Holder of the five sub-models + scheduler (reference: models/stable_diffusion.py:40-103)."""

    def __init__(self, base=None, vae=None, text_encoder=None, tokenizer=None, scheduler=None,
                 text_encoder_2=None, tokenizer_2=None, model_type: str = "sd15", device: str = "cuda",
                 model_name: Optional[str] = None, unet_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 text_encoder_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 text_encoder_2_state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 image_encoder=None, feature_extractor=None, prediction_type: Optional[str] = None, refiner=None):
        self.base = base
        # the third UNet-shaped slot of models/stable_diffusion.py:40-103: the SDXL refiner (load_refiner).  LoRA, FreeU,
        # IP-Adapter and ControlNet address .base, as the reference's loaders do; a LoRA re-fuse leaves it alone
        self.refiner = refiner
        # IP-Adapter (sd_unified_pipeline.py:441-449): the image encoder and its preprocessing -- the engine's own
        # (load_image_encoder: HipCLIPVisionModelWithProjection + ClipImageProcessor) or a caller-built torch pair
        # (transformers' CLIPVisionModelWithProjection + CLIPImageProcessor); the adapter's converted weights stay
        # here so that a LoRA re-fuse (which rebuilds .base) can attach it again
        self.image_encoder = image_encoder
        self.feature_extractor = feature_extractor
        self._ip = None                  # (diffusers-named state dict, image_embed_dim, num_tokens)
        self._ip_scale = 1.0
        self._cn = None                  # ControlNet (configuration, diffusers-named state dict): load_controlnet
        self._cn_list = False            # ... or a list of those pairs: load_controlnets (MultiControlNet)
        self._freeu = None               # (s1, s2, b1, b2) while FreeU is on: enable_freeu
        self._motion = None              # motion adapter (configuration, engine-named state dict): load_motion_adapter
        self._pag = None                 # pag_applied_layers as given (set_pag_applied_layers); None: the default
        self._deepcache = None           # (cache_interval, cache_depth) while DeepCache is on: enable_deepcache
        # host copies of the weights the LoRA adapters are folded into (load_lora_weights); the engine
        # itself keeps only its packed device copy
        self._lora = None
        self._lora_applied = None        # signature of the adapter state the sub-models were last built from
        self._unet_sd = unet_state_dict
        self._te_sd = {"text_encoder": text_encoder_state_dict, "text_encoder_2": text_encoder_2_state_dict}
        self.vae = vae
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        if model_type == "sdxl":
            self.text_encoder_2 = text_encoder_2
            self.tokenizer_2 = tokenizer_2
        self.scheduler = scheduler if scheduler is not None else _sched.EulerDiscreteScheduler()
        # the reference leaves `scheduler_name` unset until the first set_scheduler (hasattr check,
        # models/stable_diffusion.py:200); it is only pre-set here when it is known to be true, so that
        # set_scheduler("euler") on a wrapper built around another scheduler really switches
        if type(self.scheduler) is _sched.EulerDiscreteScheduler:     # (not its euler_a subclass: ADVICE r2)
            self.scheduler_name = "euler"
        if prediction_type is not None:      # single-file checkpoints carry no scheduler configuration: the caller says
            self.configure_scheduler(prediction_type=prediction_type)
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        # models/stable_diffusion.py:96-101
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)
        self.mask_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_normalize=False,
                                                do_binarize=True, do_convert_grayscale=True)
        self.device = torch.device(device)
        self.type = model_type
        self.name = model_name
        self.path = None

    def to(self, device):
        self.vae.to(device)
        self.base.to(device)
        if self.refiner is not None:
            self.refiner.to(device)
        if self.text_encoder is not None:
            self.text_encoder.to(device)
        if getattr(self, "text_encoder_2", None) is not None:
            self.text_encoder_2.to(device)
        self.device = torch.device(device)

    # ---- SDXL refiner (models/stable_diffusion.py load_refiner; the pipeline takes use_refiner= / refiner_start=) ----
    def load_refiner(self, refiner, config=None):
        """The refiner UNet: an engine UNet (HipUNet2DConditionModel, or anything with its call surface), or a local
        path -- a UNet-only diffusers folder (`unet/config.json` + weights, or the folder itself:
        checkpoints.load_unet_folder) or a `.safetensors` file, single-file LDM naming or diffusers naming, read with
        `config` (default: config.sdxl_refiner_unet()).  The reference downloads its default from the hub; nothing here
        reaches the network, so None is an error.  Replaces a refiner loaded before."""
        if refiner is None:
            raise ValueError("load_refiner needs an engine UNet or a local folder / .safetensors file "
                             "(hub downloads are not supported)")
        if not isinstance(refiner, (str, os.PathLike)):
            if not (callable(refiner) and hasattr(refiner, "config")):
                raise ValueError("load_refiner needs an engine UNet or a local folder / .safetensors file, "
                                 f"got {type(refiner).__name__}")
            self.refiner = refiner
            return
        from . import checkpoints
        from .config import sdxl_refiner_unet
        from .models import HipUNet2DConditionModel
        path = os.fspath(refiner)
        if os.path.isdir(path):
            cfg, sd = checkpoints.load_unet_folder(path)
        elif path.endswith(".safetensors") and os.path.isfile(path):
            cfg = config if config is not None else sdxl_refiner_unet()
            sd = checkpoints.load_safetensors(path)
            if any(k.startswith(checkpoints.UNET_PREFIX) for k in sd):
                sd = checkpoints.ldm_to_diffusers_unet(sd, cfg)
        else:
            raise ValueError(f"load_refiner: {path!r} is neither a folder nor a .safetensors file")
        self.refiner = None                  # an old refiner's device memory goes before the new one is packed
        self.refiner = HipUNet2DConditionModel(cfg, str(self.device)).load_state_dict(sd)

    def unload_refiner(self):
        self.refiner = None

    @property
    def has_refiner(self) -> bool:
        return self.refiner is not None

    # ---- LoRA adapters (models/stable_diffusion.py:229-335), folded into the weights on the host ----
    def _adapters(self):
        if self._lora is None:
            if self._unet_sd is None:
                raise ValueError("LoRA needs the UNet's base weights on the host: build the wrapper with "
                                 "unet_state_dict=... (the engine keeps only its packed device copy)")
            if not hasattr(self.base, "rebuild"):
                raise ValueError(f"{type(self.base).__name__} cannot be rebuilt from a state dict")
            from .lora import LoraAdapters
            f = getattr(self.base, "rebuild_factory", None)
            self._base_factory = f() if f else self.base.rebuild
            self._lora = LoraAdapters(self._unet_sd, self._te_sd["text_encoder"], self._te_sd["text_encoder_2"])
        return self._lora

    def apply_adapters(self):
        """Rebuild the sub-models the adapters touch from the fused weights -- once per change of the adapter state,
        however many load / set / delete calls produced it (the reference's `load_loras` is delete + N loads + set:
        one re-pack here, not N + 2).  Called by the pipeline before it runs; callable by hand."""
        if self._lora is None:
            return
        sig = self._lora.signature()
        if sig == self._lora_applied:
            return
        if not hasattr(self.base, "rebuild"):
            raise ValueError(f"{type(self.base).__name__} cannot be rebuilt from a state dict")
        fused = self._lora.fused("unet")
        old = self.base
        graph = bool(getattr(old, "_graph_on", False))
        freeu = getattr(old, "_freeu", self._freeu)     # the engine's own record wins: enable_freeu may be called on .base
        deepcache = getattr(old, "deepcache", self._deepcache)
        tome = getattr(old, "tome", None)
        hypertile = getattr(old, "hypertile", None)
        self.base = None                     # the old engine's device memory goes before the new one is packed
        del old
        self.base = self._rebuild_from(fused, graph, freeu, deepcache, self._pag)
        if tome is not None:                 # token merging survives the re-fuse too
            self.base.enable_tome(*tome)
        if hypertile is not None:            # and HyperTile
            self.base.enable_hypertile(*hypertile)
        for part in ("text_encoder", "text_encoder_2"):
            if self._te_sd[part] is not None and (self._lora.touches(part) or self._lora_applied is not None):
                enc = getattr(self, part, None)
                sd = self._lora.fused(part)
                if hasattr(enc, "rebuild"):
                    setattr(self, part, enc.rebuild(sd))
                elif hasattr(enc, "load_state_dict"):
                    enc.load_state_dict(sd, strict=False)
                else:
                    raise ValueError(f"{type(enc).__name__} cannot take fused text-encoder LoRA weights")
        self._lora_applied = sig

    def _rebuild_from(self, fused, graph, freeu=None, deepcache=None, pag=None):
        base = self._base_factory(fused)
        if graph and hasattr(base, "use_graph"):
            base.use_graph(True)
        if self._ip is not None:             # the IP-Adapter survives the re-fuse
            self._attach_ip(base)
        if self._cn is not None:             # and so does the ControlNet
            self._attach_cn(base)
        if self._motion is not None:         # and the motion adapter
            self._attach_motion(base)
        self._freeu = freeu
        if freeu is not None:                # and FreeU
            base.enable_freeu(*freeu)
        self._deepcache = deepcache
        if deepcache is not None:            # and DeepCache
            base.enable_deepcache(*deepcache)
        self._pag = pag
        if pag is not None and hasattr(base, "set_pag_layers"):     # and the perturbed-attention layers
            base.set_pag_layers(pag)
        return base

    # ---- perturbed-attention guidance: which transformers `pag_scale > 0` perturbs (diffusers' pag_applied_layers) ----
    def set_pag_applied_layers(self, layers):
        """diffusers' `pag_applied_layers` ("mid", "down.block_2", "up.block_1.attentions_0", a list of them; the
        default without a call is ("mid",)).  Names are checked against the UNet's topology at once where it has one."""
        names = (layers,) if isinstance(layers, str) else tuple(layers)
        cfg = getattr(self.base, "cfg", None)
        if cfg is not None:
            _pag.site_keys(cfg, names)           # (raises for a name that selects nothing)
        if hasattr(self.base, "set_pag_layers"):
            self.base.set_pag_layers(names)
        self._pag = names

    # ---- FreeU (diffusers pipelines' enable_freeu / disable_freeu: forwarded to the UNet) ----
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        self.base.enable_freeu(s1, s2, b1, b2)
        self._freeu = (float(s1), float(s2), float(b1), float(b2))

    def disable_freeu(self):
        self.base.disable_freeu()
        self._freeu = None

    # ---- tiled / sliced VAE (diffusers pipelines' enable_vae_tiling / enable_vae_slicing: forwarded to the VAE; they
    #      live below every feature switch of the pipeline and take no call keyword) ----
    def enable_vae_tiling(self):
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        self.vae.disable_tiling()

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    # ---- DeepCache (forwarded to the base UNet; the refiner runs plain) ----
    def enable_deepcache(self, cache_interval: int = 3, cache_depth: int = 1):
        self.base.enable_deepcache(cache_interval, cache_depth)
        self._deepcache = (cache_interval, cache_depth)

    def disable_deepcache(self):
        self.base.disable_deepcache()
        self._deepcache = None

    # ---- token merging (tomesd.apply_patch's arguments; forwarded to the base UNet, the refiner runs plain) ----
    def enable_tome(self, ratio: float = 0.5, max_downsample: int = 1, sx: int = 2, sy: int = 2, use_rand: bool = True,
                    seed: int = 0):
        self.base.enable_tome(ratio, max_downsample, sx, sy, use_rand, seed)

    def disable_tome(self):
        self.base.disable_tome()

    # ---- HyperTile (forwarded to the base UNet, and to the refiner when one is loaded) ----
    def enable_hypertile(self, tile_size: int = 32, swap_size: int = 2, max_depth: int = 0, seed: int = 0):
        self.base.enable_hypertile(tile_size, swap_size, max_depth, seed)
        if self.refiner is not None and hasattr(self.refiner, "enable_hypertile"):
            self.refiner.enable_hypertile(tile_size, swap_size, max_depth, seed)

    def disable_hypertile(self):
        self.base.disable_hypertile()
        if self.refiner is not None and hasattr(self.refiner, "disable_hypertile"):
            self.refiner.disable_hypertile()

    # ---- AnimateDiff motion adapter (diffusers MotionAdapter; stablediffusion_amd.animatediff.animate runs it) ----
    def _attach_motion(self, base):
        cfg, sd = self._motion
        base.attach_motion_adapter(base.make_motion_adapter(cfg, sd))

    def load_motion_adapter(self, pretrained_model_name_or_path_or_dict, config=None):
        """A motion adapter for this model's UNet: a diffusers MotionAdapter folder, an original `mm_sd_v15*` file or a
        state dict in either naming (stablediffusion_amd.motion.load: converted, checked).  Replaces one loaded before;
        survives a LoRA re-fuse."""
        from . import motion
        cfg, sd = motion.load(pretrained_model_name_or_path_or_dict, self.base.cfg, config)
        self.unload_motion_adapter()
        self._motion = (cfg, sd)
        self._attach_motion(self.base)

    def unload_motion_adapter(self):
        if self._motion is not None:
            self.base.attach_motion_adapter(None)
        self._motion = None

    @property
    def has_motion_adapter(self) -> bool:
        return self._motion is not None

    # ---- ControlNet (diffusers ControlNetModel, or a list of them: MultiControlNetModel; the pipeline takes
    #      control_image=) ----
    def _attach_cn(self, base):
        if self._cn_list:
            base.attach_controlnets([base.make_controlnet(cfg, sd) for cfg, sd in self._cn])
            return
        cfg, sd = self._cn
        base.attach_controlnet(base.make_controlnet(cfg, sd))

    def load_controlnet(self, pretrained_model_name_or_path_or_dict):
        """A ControlNet for this model's UNet: a diffusers folder (config.json + weights), an original (lllyasviel 1.0 /
        1.1) `.pth` / `.safetensors` file, or a state dict (stablediffusion_amd.controlnet.load: converted, checked).
        Replaces whatever was loaded before.  A list (MultiControlNet) goes to load_controlnets."""
        from . import controlnet
        if isinstance(pretrained_model_name_or_path_or_dict, (list, tuple)):
            raise NotImplementedError("load_controlnet takes one ControlNet: a list (MultiControlNet) goes to load_controlnets")
        cfg, sd = controlnet.load(pretrained_model_name_or_path_or_dict, self.base.cfg)
        self.unload_controlnet()
        self._cn, self._cn_list = (cfg, sd), False
        self._attach_cn(self.base)

    def load_controlnets(self, sources):
        """MultiControlNet (diffusers MultiControlNetModel): a list of ControlNets, each given as load_controlnet takes
        one.  The pipeline then takes control_image= as a list with one entry per net, and scale / guidance window as
        floats or lists of that length.  Replaces whatever was loaded before."""
        from . import controlnet
        from ._lib import SD_MAX_CONTROLNETS
        if not isinstance(sources, (list, tuple)):
            raise ValueError("load_controlnets takes a list of ControlNets (load_controlnet takes one)")
        if not 1 <= len(sources) <= SD_MAX_CONTROLNETS:
            raise ValueError(f"load_controlnets takes 1 to {SD_MAX_CONTROLNETS} ControlNets, got {len(sources)}")
        loaded = [controlnet.load(src, self.base.cfg) for src in sources]
        self.unload_controlnet()
        self._cn, self._cn_list = loaded, True
        self._attach_cn(self.base)

    def unload_controlnet(self):
        if self._cn is not None:
            if self._cn_list:
                self.base.attach_controlnets([])
            else:
                self.base.attach_controlnet(None)
        self._cn, self._cn_list = None, False

    @property
    def controlnet_list_len(self) -> int:
        """The nets loaded through load_controlnets; 0 when none or a single one (load_controlnet) is loaded."""
        return len(self._cn) if self._cn_list else 0

    @property
    def has_controlnet(self) -> bool:
        return self._cn is not None

    # ---- IP-Adapter (diffusers load_ip_adapter / set_ip_adapter_scale / unload_ip_adapter) ----
    def _attach_ip(self, base):
        sd, d_img, n_tok = self._ip
        base.attach_ip_adapter(base.make_ip_adapter(sd, d_img, n_tok))
        base.set_ip_adapter_scale(self._ip_scale)
        self._sync_feature_tokens(base)

    @property
    def ip_adapter_is_plus(self) -> bool:
        """Whether the loaded IP-Adapter projects hidden_states[-2] through a Resampler (IP-Adapter Plus files)."""
        from . import ip_adapter
        return self._ip is not None and ip_adapter.is_resampler(self._ip[0])

    def _sync_feature_tokens(self, base=None):
        # a Resampler adapter reads (image_size / patch_size)^2 + 1 rows per image of the loaded tower
        base = self.base if base is None else base
        vcfg = getattr(self.image_encoder, "cfg", None) or getattr(self.image_encoder, "config", None)
        adapter = getattr(base, "ip_adapter", None)
        if self.ip_adapter_is_plus and hasattr(vcfg, "patch_size") and hasattr(adapter, "feature_tokens"):
            adapter.feature_tokens = (vcfg.image_size // vcfg.patch_size) ** 2 + 1

    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict):
        """An original IP-Adapter file (`.bin` / `.safetensors`, a local path) or its state dict: converted, checked
        against the UNet and attached (stablediffusion_amd.ip_adapter).  Replaces an adapter loaded before."""
        from . import ip_adapter
        sd, d_img, n_tok = ip_adapter.convert(pretrained_model_name_or_path_or_dict, self.base.cfg)
        self._ip = (sd, d_img, n_tok)
        self._ip_scale = 1.0
        self._attach_ip(self.base)

    def set_ip_adapter_scale(self, scale: float):
        self._ip_scale = float(scale)
        if self._ip is not None:
            self.base.set_ip_adapter_scale(self._ip_scale)

    def unload_ip_adapter(self):
        if self._ip is not None:
            self.base.attach_ip_adapter(None)
            self.base.set_ip_adapter_scale(1.0)
        self._ip = None
        self._ip_scale = 1.0

    def load_image_encoder(self, path_or_cfg, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        """The CLIP vision tower an IP-Adapter was trained against, on the engine: a local `image_encoder/` folder
        (checkpoints.load_image_encoder_folder) or a CLIPVisionConfig with its transformers-named state dict.  Sets
        `.image_encoder` (HipCLIPVisionModelWithProjection) and `.feature_extractor` (ClipImageProcessor at the tower's
        image size), so `ip_adapter_image=<PIL image>` runs with no torch module on the path.  A LoRA re-fuse rebuilds
        only the UNet and the text encoders and leaves both alone.  Nothing is downloaded."""
        from .config import CLIPVisionConfig
        from .image_processor import ClipImageProcessor
        from .models import HipCLIPVisionModelWithProjection
        if isinstance(path_or_cfg, CLIPVisionConfig):
            if state_dict is None:
                raise ValueError("load_image_encoder(config, state_dict): the state dict is missing")
            cfg = path_or_cfg
        else:
            if state_dict is not None:
                raise ValueError("load_image_encoder: a state dict goes with a CLIPVisionConfig, not with a path")
            from . import checkpoints
            cfg, state_dict = checkpoints.load_image_encoder_folder(os.fspath(path_or_cfg))
        self.image_encoder = None            # an old encoder's device memory goes before the new one is packed
        self.image_encoder = HipCLIPVisionModelWithProjection.from_state_dict(cfg, state_dict, device=str(self.device))
        self.feature_extractor = ClipImageProcessor(size=cfg.image_size)
        self._sync_feature_tokens()

    def unload_image_encoder(self):
        self.image_encoder = None
        self.feature_extractor = None

    def _refuse(self):
        # (kept for callers that want the rebuild now; load / set / delete only mark the state changed)
        self.apply_adapters()

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, **kwargs):
        """`pytorch_lora_weights.safetensors` or a kohya / A1111 file (a file, a folder holding one, or a dict) -> a named
        adapter, active at weight 1 as in diffusers; `set_adapters` changes names / weights.  UNet and text-encoder
        layers (`stable_diffusion.py:259-295`); the sub-models are rebuilt lazily (apply_adapters)."""
        self._adapters().load(pretrained_model_name_or_path_or_dict, adapter_name)

    def set_adapters(self, adapter_names, adapter_weights=None):
        self._adapters().set(adapter_names, adapter_weights)

    def delete_adapters(self, adapter_names):
        self._adapters().delete(adapter_names)

    def get_list_adapters(self):
        return {"base": self._lora.names()} if self._lora is not None and self._lora.names() else {}

    def set_lora_scale(self, scale: float):
        """`cross_attention_kwargs={"scale": s}` (sd_unified_pipeline.py:190): a run-time multiplier on every
        active adapter in diffusers, in effect for ONE call (the pipeline passes 1.0 when the kwarg is absent);
        here part of the adapter state, re-fused only when the value changes."""
        if self._lora is None:
            return
        self._lora.scale = float(scale)

    def configure_scheduler(self, **fields):
        """Rebuild the current scheduler (same class) with configuration fields changed: `prediction_type`
        ("epsilon" / "v_prediction"), `rescale_betas_zero_snr`, `timestep_spacing`, the beta range, ...  They live in
        `scheduler.config`, so a later set_scheduler(name) carries them to the next class."""
        self.scheduler = type(self.scheduler).from_config(self.scheduler.config, **fields)

    def load_scheduler_config(self, folder):
        """`scheduler/scheduler_config.json` of a diffusers checkpoint folder (checkpoints.read_scheduler_config) applied
        to this wrapper's scheduler: what makes an SD 2.x-768 / zero-terminal-SNR folder run as the v-prediction model it
        is.  The scheduler class stays the wrapper's own (set_scheduler chooses it)."""
        from . import checkpoints
        self.configure_scheduler(**checkpoints.read_scheduler_config(folder))

    def set_scheduler(self, scheduler_name):
        """Registry of models/stable_diffusion.py:199-227 (names the engine's host code implements)."""
        if getattr(self, "scheduler_name", None) == scheduler_name:
            return
        make = _sched.REGISTRY.get(scheduler_name) or _sched.EXTRA_SCHEDULERS.get(scheduler_name)
        if make is None:
            raise ValueError(f"Unknown scheduler name: {scheduler_name}")
        self.scheduler = make(self.scheduler.config)
        self.scheduler_name = scheduler_name


_DC_PLAIN, _DC_STORE, _DC_REUSE = 0, 1, 2       # DeepCache forward modes (sd_engine.h: SD_DC_*)


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    if rc:
        raise RuntimeError(lib.sd_last_error().decode())


def convert_pt_to_numpy(images: torch.Tensor):
    """`/root/reference/runpod-worker/handler_logic.py:21-29`: decoded images -> list of HWC uint8 arrays.
    fp16 CUDA tensors go through the engine's `sd_images_to_uint8` (one kernel, one [B,H,W,C] byte copy
    to the host instead of four torch ops and one copy per image; same roundings and truncation as
    the reference's op sequence); anything else runs that op sequence itself."""
    if images.is_cuda and images.dtype == torch.float16 and images.dim() == 4 and images.shape[1] <= 4:
        lib = _lib.load()
        images = images.contiguous()
        B, Cc, H, W = images.shape
        out = torch.empty(B, H, W, Cc, dtype=torch.uint8, device=images.device)
        _check(lib, lib.sd_images_to_uint8(_ptr(images), _ptr(out), B, Cc, H, W, _stream()))
        host = out.cpu().numpy()
        return [host[i] for i in range(B)]
    np_images = []
    for idx in range(len(images)):
        img = (images[idx] / 2 + 0.5).clamp(0, 1)
        np_images.append((img.permute(1, 2, 0) * 255).to(torch.uint8).cpu().numpy())
    return np_images


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """sd_unified_pipeline.py:46-57 (defined there, never called): guidance rescale of Lin et al., "Common Diffusion
    Noise Schedules and Sample Steps are Flawed", section 3.4.  The guided prediction is brought to the per-sample
    standard deviation of the text-conditioned one and mixed back with weight `guidance_rescale`.  torch's default
    (unbiased) std over everything but the batch axis, in the tensors' own dtype; std(noise_cfg) = 0 gives inf / nan
    as it does there.  The device form is sd_cfg_rescale_linear_step."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


def guidance_scale_embedding(w: torch.Tensor, embedding_dim: int = 512, dtype=torch.float32) -> torch.Tensor:
    """The `timestep_cond` of a guidance-embedded UNet (diffusers 0.27.2 LatentConsistencyModelPipeline.get_guidance_scale_embedding,
    recalled): w [B] (guidance_scale - 1) -> [B, embedding_dim] = [sin(1000 w f_i) | cos(1000 w f_i)],
    f_i = exp(-i ln(1e4) / (half - 1)), half = embedding_dim // 2, one zero column appended when embedding_dim is odd."""
    w = torch.as_tensor(w, dtype=dtype).reshape(-1) * 1000.0
    half = embedding_dim // 2
    freq = torch.exp(torch.arange(half, dtype=dtype) * -(torch.log(torch.tensor(10000.0, dtype=dtype)) / (half - 1)))
    ang = w[:, None] * freq[None, :]
    emb = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if embedding_dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1))
    return emb


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, **kwargs):
    """sd_unified_pipeline.py:61-95 (the custom timesteps / sigmas branches are never reached there)."""
    scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
    return scheduler.timesteps, num_inference_steps


def denoising_value_valid(dnv):
    return isinstance(dnv, float) and 0 < dnv < 1


class StableDiffusionUnifiedPipeline:
    def __init__(self, do_cfg: bool = True, device: Optional[str] = None, output_type: Optional[str] = None):
        self._do_cfg = bool(do_cfg)
        self._guidance_embedded = False      # set per call: the UNet takes the guidance scale as `timestep_cond`
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.output_type = output_type if output_type is not None else "pt"
        self.model: Optional[SDModelWrapper] = None
        # the fused CFG step lets the engine run the start of the UNet once per latent (HipUNet2DConditionModel.forward_cfg);
        # False keeps the engine's duplicate-then-forward form
        self.cfg_share = True
        # perturbed-attention guidance: the engine creates the perturbed group where it starts to differ
        # (HipUNet2DConditionModel.forward_pag); False duplicates up front
        self.pag_share = True
        self._use_refiner = False            # set per call: the UNet of this call is model.refiner
        self.is_inpaint = False              # set per call

    def _unet(self, model):
        """The UNet this call runs: `.base`, or `.refiner` under use_refiner=True."""
        return model.refiner if self._use_refiner else model.base

    @property
    def do_classifier_free_guidance(self) -> bool:
        # a guidance-embedded UNet (time_cond_proj_dim: Latent Consistency Models) runs without CFG whatever the
        # constructor said; the negative prompt is unused, as in diffusers' LCM pipeline
        return self._do_cfg and not self._guidance_embedded

    @do_classifier_free_guidance.setter
    def do_classifier_free_guidance(self, value):
        self._do_cfg = bool(value)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(
        self,
        model: SDModelWrapper,
        prompt: Union[str, List[str], None] = None,
        prompt_2=None,
        negative_prompt=None,
        negative_prompt_2=None,
        height: Optional[int] = None,
        width: Optional[int] = None,
        num_images_per_prompt: Optional[int] = 1,
        num_inference_steps: int = 50,
        denoising_end: Optional[float] = None,
        guidance_scale: float = 5.0,
        latents: Optional[torch.Tensor] = None,
        output_type: Optional[str] = "pt",
        cross_attention_kwargs: Optional[Dict[str, Any]] = None,
        guidance_rescale: float = 0.0,
        clip_skip: Optional[int] = None,
        seed: Optional[int] = None,
        image=None,
        strength: float = 1.0,
        denoising_start: Optional[float] = None,
        mask_image=None,
        masked_image_latents=None,
        padding_mask_crop: Optional[int] = None,
        # superset (see module docstring)
        prompt_embeds: Optional[torch.Tensor] = None,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        pooled_prompt_embeds: Optional[torch.Tensor] = None,
        negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
        # IP-Adapter image prompts (the reference's commented block at :441-449)
        ip_adapter_image=None,
        ip_adapter_image_embeds: Optional[List[torch.Tensor]] = None,
        # ControlNet (diffusers StableDiffusionControlNetPipeline and its SDXL / img2img / inpaint twins)
        control_image=None,
        controlnet_conditioning_scale: float = 1.0,
        control_guidance_start: float = 0.0,
        control_guidance_end: float = 1.0,
        guess_mode: bool = False,
        # InstructPix2Pix (diffusers StableDiffusionInstructPix2PixPipeline): an 8-channel UNet selects the mode, `image`
        # is the picture to edit; None: 1.5 there, and nothing anywhere else
        image_guidance_scale: Optional[float] = None,
        # MultiDiffusion (diffusers StableDiffusionPanoramaPipeline; stablediffusion_amd.views): the canvas is denoised as
        # overlapping windows of `view_window` latent pixels (an int or (h, w); None: off) every `view_stride` (default:
        # half the window), `view_batch_size` windows per UNet forward (default: 4 latents per forward), merged with
        # `view_blend` weights ("uniform" / "gaussian"); `circular_padding` wraps the x axis
        view_window=None,
        view_stride=None,
        view_batch_size: Optional[int] = None,
        view_blend: str = "uniform",
        circular_padding: bool = False,
        # regional prompts (stablediffusion_amd.regions; this project's own semantics): `prompt` holds wherever no mask
        # does, region_prompts[i] where region_masks[i] ([R-1, H, W] / [R-1, 1, H, W] in [0, 1], or PIL images) does;
        # region_base_weight >= 0 keeps that much of `prompt` everywhere.  With prompt_embeds=, region_prompt_embeds=
        # holds one [B, L, D] per region.  One UNet forward per step, whatever the number of regions
        region_prompts=None,
        region_masks=None,
        region_base_weight: float = 0.0,
        region_prompt_embeds=None,
        # SDXL refiner (diffusers StableDiffusionXLImg2ImgPipeline on model.refiner; the reference's handler TODO)
        use_refiner: bool = False,
        refiner_start: Optional[float] = None,
        aesthetic_score: float = 6.0,
        negative_aesthetic_score: float = 2.5,
        # perturbed-attention guidance (diffusers >= 0.30 StableDiffusionPAGPipeline; layers: set_pag_applied_layers)
        pag_scale: float = 0.0,
        pag_adaptive_scale: float = 0.0,
    ):
        self._use_refiner = bool(use_refiner)
        facts = _combos.call_facts(self, model, **{k: v for k, v in locals().items() if k not in ("self", "model")})
        _combos.refuse(facts)                # what does not run together is refused here, before anything runs
        regional, edit, pag_on = facts.regional, facts.edit, facts.pag
        if regional:
            _regions.check_call(region_prompts, region_masks, region_prompt_embeds, region_base_weight, prompt_embeds)
        views = None
        if view_window is not None:
            self._check_views(view_window, view_stride, view_batch_size, view_blend)
            views = dict(window=view_window, stride=view_stride, batch=view_batch_size, blend=view_blend,
                         circular=bool(circular_padding))
        if edit:
            if image_guidance_scale is not None and not math.isfinite(float(image_guidance_scale)):
                raise ValueError("image_guidance_scale must be finite")
            image_guidance_scale = float(_p2p.DEFAULT_IMAGE_GUIDANCE_SCALE if image_guidance_scale is None
                                         else image_guidance_scale)
        if refiner_start is not None:
            call = {k: v for k, v in locals().items() if k not in ("self", "facts", "edit", "views", "regional", "pag_on")}
            return self._ensemble_of_experts(call)
        if pag_on and (not math.isfinite(float(pag_scale)) or not math.isfinite(float(pag_adaptive_scale))
                       or pag_adaptive_scale < 0):
            raise ValueError("pag_scale and pag_adaptive_scale must be finite and non-negative")
        tc_dim = _combos.guidance_embed_dim(self._unet(model))
        self._guidance_embedded = tc_dim > 0
        if not 0.0 <= float(guidance_rescale) <= 1.0:
            raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale}")
        # as in diffusers: only with CFG on and a positive value
        guidance_rescale = float(guidance_rescale) if self.do_classifier_free_guidance else 0.0
        has_cn = facts.cn_loaded and not use_refiner     # (a ControlNet belongs to .base)
        n_cn_list = getattr(model, "controlnet_list_len", 0) if has_cn else 0
        if n_cn_list:
            # MultiControlNet: argument checks of the lists, before anything runs
            from . import controlnet as _controlnet
            controlnet_conditioning_scale, control_guidance_start, control_guidance_end = _controlnet.list_arguments(
                n_cn_list, control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end)
            proc = self.control_image_processor(model)
            sizes = [tuple(proc.preprocess(ci, height=height, width=width).shape[-2:]) for ci in control_image]
            if len(set(sizes)) != 1:
                raise ValueError(f"control images of different sizes after preprocessing: {sizes}")
        elif has_cn:
            if any(isinstance(v, (list, tuple)) for v in (controlnet_conditioning_scale, control_guidance_start,
                                                          control_guidance_end)):
                raise NotImplementedError("MultiControlNet (lists of scales / guidance windows) is not supported")
            if not 0.0 <= control_guidance_start < control_guidance_end <= 1.0:
                raise ValueError("need 0 <= control_guidance_start < control_guidance_end <= 1")
        if model.device != self.device:
            model.to(self.device)
        self.model = model
        if hasattr(model, "set_lora_scale"):
            # `:190`: the LoRA scale of THIS call -- 1.0 when the kwarg is absent (diffusers / peft un-scale after the
            # forward; a scale left over from an earlier call would be a different model: ADVICE r2)
            lora_scale = cross_attention_kwargs.get("scale", None) if cross_attention_kwargs is not None else None
            model.set_lora_scale(1.0 if lora_scale is None else lora_scale)
        if hasattr(model, "apply_adapters"):
            model.apply_adapters()
        unet = self._unet(model)             # (after the re-fuse, which replaces model.base)
        if image is not None and mask_image is None:
            # img2img keeps the image's own size (`:238` preprocesses without height / width); PIL, numpy and
            # tensor inputs alike go through the image processor (rounded down to a multiple of the VAE factor)
            image = model.image_processor.preprocess(image)
            if image.shape[1] != 4:
                height, width = image.shape[-2], image.shape[-1]
            elif use_refiner or edit:
                # the hand-off passes latents: the size the time ids state is theirs (diffusers' img2img reads it back
                # from the prepared latents), not the refiner's sample_size.  (InstructPix2Pix: image latents as given.)
                height = height or image.shape[-2] * model.vae_scale_factor
                width = width or image.shape[-1] * model.vae_scale_factor
        if has_cn and image is None and (height is None or width is None):
            # txt2img: the run's size comes from the control image (diffusers' check_image / prepare_image)
            first = control_image[0] if n_cn_list else control_image       # (a list: the first net's image)
            ci = self.control_image_processor(model).preprocess(first, height=height, width=width)
            height, width = ci.shape[-2], ci.shape[-1]
        height = height or unet.config.sample_size * model.vae_scale_factor
        width = width or unet.config.sample_size * model.vae_scale_factor
        if views is not None:                # a plan that cannot be made is refused here, before anything runs
            _views.plan_views(height // model.vae_scale_factor, width // model.vae_scale_factor, views["window"],
                              views["stride"], views["circular"])

        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        elif prompt_embeds is not None:
            batch_size = prompt_embeds.shape[0]
        else:
            raise ValueError("either `prompt` or `prompt_embeds` is required")

        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = \
                self.encode_prompt(prompt, prompt_2, negative_prompt, negative_prompt_2,
                                   num_images_per_prompt, None, clip_skip)
        else:
            prompt_embeds = prompt_embeds.to(self.device)
            if self.do_classifier_free_guidance:
                if negative_prompt_embeds is None:
                    raise ValueError("negative_prompt_embeds is required with prompt_embeds when CFG is on")
                negative_prompt_embeds = negative_prompt_embeds.to(self.device)

        if regional:
            # one encoder_hidden_states of R L tokens: [prompt | region 1 | ...]; the negative repeats per segment
            if region_prompt_embeds is None:
                region_prompt_embeds = []
                for rp in region_prompts:
                    rp = batch_size * [rp] if isinstance(rp, str) else list(rp)
                    if len(rp) != batch_size:
                        raise ValueError(f"a region prompt list holds {len(rp)} prompts for a batch of {batch_size}")
                    region_prompt_embeds.append(self.encode_prompt(rp, None, negative_prompt, negative_prompt_2,
                                                                   num_images_per_prompt, None, clip_skip)[0])
            prompt_embeds, negative_prompt_embeds = _regions.join_embeds(
                prompt_embeds, list(region_prompt_embeds),
                negative_prompt_embeds if self.do_classifier_free_guidance else None)

        timesteps, num_inference_steps = retrieve_timesteps(model.scheduler, num_inference_steps, self.device)

        self.is_inpaint = False
        mask = masked_image_latents_2b = image_latents = noise = None
        num_channels_unet = unet.config.in_channels
        edit_latents = None
        if edit:
            # ---- InstructPix2Pix: pure noise, as txt2img; the image enters through the UNet's last four channels ----
            n = batch_size * num_images_per_prompt
            shape = (n, model.vae.config.latent_channels, height // model.vae_scale_factor, width // model.vae_scale_factor)
            latents = self.prepare_latents_txt2img(shape, prompt_embeds.dtype, seed, latents)
            edit_latents = self.prepare_image_latents_pix2pix(image, n, latents.dtype, tuple(latents.shape[-2:]))
        elif image is None:
            shape = (batch_size * num_images_per_prompt, unet.config.in_channels,
                     height // model.vae_scale_factor, width // model.vae_scale_factor)
            latents = self.prepare_latents_txt2img(shape, prompt_embeds.dtype, seed, latents)
        elif mask_image is not None:
            # ---- inpaint (:268-380) ----
            if padding_mask_crop is not None:           # `:270-275`: work on the masked region only
                crops_coords = model.mask_processor.get_crop_region(mask_image, width, height, pad=padding_mask_crop)
                resize_mode = "fill"
            else:
                crops_coords, resize_mode = None, "default"
            latent_input = isinstance(image, torch.Tensor) and image.ndim == 4 and image.shape[1] == 4
            init_image = model.image_processor.preprocess(
                image, height=None if latent_input else height, width=None if latent_input else width,
                crops_coords=crops_coords, resize_mode=resize_mode).to(torch.float32)
            mask = model.mask_processor.preprocess(mask_image, height=height, width=width, resize_mode=resize_mode,
                                                   crops_coords=crops_coords)
            if masked_image_latents is not None:
                masked_image = masked_image_latents
            elif init_image.shape[1] == 4:
                masked_image = None
            else:
                masked_image = init_image * (mask < 0.5)
            timesteps, num_inference_steps = self.get_timesteps(
                num_inference_steps, strength, denoising_start if denoising_value_valid(denoising_start) else None)
            if num_inference_steps < 1:
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the "
                                 f"number of pipeline steps is {num_inference_steps} which is < 1.")
            latent_timestep = timesteps[:1].repeat(batch_size * num_images_per_prompt)
            is_strength_max = strength == 1.0
            num_channels_latents = model.vae.config.latent_channels
            return_image_latents = num_channels_unet == 4
            shape = (batch_size * num_images_per_prompt, num_channels_latents,
                     height // model.vae_scale_factor, width // model.vae_scale_factor)
            latents, noise, image_latents = self.prepare_latents_inpaint(
                shape, prompt_embeds.dtype, seed, latents, init_image, latent_timestep, is_strength_max,
                add_noise=denoising_start is None, return_image_latents=return_image_latents)
            mask, masked_image_latents_2b = self.prepare_mask_latents(
                mask, masked_image, batch_size * num_images_per_prompt, height // model.vae_scale_factor,
                width // model.vae_scale_factor, prompt_embeds.dtype, seed)
            if num_channels_unet == 9:
                if masked_image_latents_2b is None:
                    raise ValueError("a 9-channel inpaint UNet needs a pixel-space image (or masked_image_latents)")
                if num_channels_latents + mask.shape[1] + masked_image_latents_2b.shape[1] != num_channels_unet:
                    raise ValueError("Incorrect configuration settings! latents + mask + masked image channels "
                                     f"!= unet in_channels ({num_channels_unet})")
            elif num_channels_unet != 4:
                raise ValueError(f"The unet {unet.__class__} should have either 4 or 9 input channels, "
                                 f"not {num_channels_unet}.")
            height, width = (d * model.vae_scale_factor for d in latents.shape[-2:])
            self.is_inpaint = True
        else:
            timesteps, num_inference_steps = self.get_timesteps(num_inference_steps, strength, denoising_start)
            latent_timestep = timesteps[:1].repeat(batch_size * num_images_per_prompt)
            add_noise = denoising_start is None
            latents = self.prepare_latents_img2img(image, latent_timestep, batch_size, num_images_per_prompt,
                                                   prompt_embeds.dtype, seed, add_noise)

        if (denoising_end is not None and denoising_start is not None and denoising_value_valid(denoising_end)
                and denoising_value_valid(denoising_start) and denoising_start >= denoising_end):
            raise ValueError(f"`denoising_start`: {denoising_start} cannot be larger than or equal to "
                             f"`denoising_end`:  {denoising_end} when using type float.")
        elif denoising_end is not None and denoising_value_valid(denoising_end):
            cutoff = int(round(model.scheduler.config.num_train_timesteps
                               - denoising_end * model.scheduler.config.num_train_timesteps))
            num_inference_steps = len([ts for ts in timesteps if ts >= cutoff])
            timesteps = timesteps[:num_inference_steps]

        # SDXL added conditions (:407-435)
        if getattr(unet.config, "addition_embed_type", None) == "text_time":
            add_text_embeds = pooled_prompt_embeds
            if use_refiner:
                # StableDiffusionXLImg2ImgPipeline with requires_aesthetics_score: the score takes target_size's place,
                # and the negative half carries its own
                add_time_ids, add_neg_time_ids = self._get_add_time_ids(
                    (height, width), (0, 0), None, prompt_embeds.dtype, aesthetic_score=aesthetic_score,
                    negative_aesthetic_score=negative_aesthetic_score)
            else:
                add_time_ids = self._get_add_time_ids((height, width), (0, 0), (height, width), prompt_embeds.dtype)
                add_neg_time_ids = add_time_ids
            add_time_ids = add_time_ids.repeat(batch_size * num_images_per_prompt, 1)
            if self.do_classifier_free_guidance:
                add_neg_time_ids = add_neg_time_ids.repeat(batch_size * num_images_per_prompt, 1)
                add_text_embeds = torch.cat([negative_pooled_prompt_embeds, add_text_embeds], dim=0)
                add_time_ids = torch.cat([add_neg_time_ids, add_time_ids], dim=0)
            added_cond_kwargs = {"text_embeds": add_text_embeds.to(self.device),
                                 "time_ids": add_time_ids.to(self.device)}
        else:
            added_cond_kwargs = None

        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            image_embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, ip_adapter_image_embeds, self.device,
                                                                batch_size * num_images_per_prompt,
                                                                self.do_classifier_free_guidance)
            if self.device.type == "cuda":       # one fp16 buffer for the whole loop: the engine caches its image K/V
                image_embeds = [e.to(torch.float16).contiguous() for e in image_embeds]
            added_cond_kwargs = dict(added_cond_kwargs or {}, image_embeds=image_embeds)

        # guidance-embedded UNet: the guidance scale goes in as an embedding, once per call, to every forward
        tc_kwargs = {}
        if tc_dim:
            w = torch.full((batch_size * num_images_per_prompt,), float(guidance_scale) - 1.0)
            tc_kwargs = {"timestep_cond": guidance_scale_embedding(w, tc_dim).to(self.device)}

        control = None
        if has_cn:
            if n_cn_list:
                control = [self.prepare_control_image(model, ci, height, width, batch_size, num_images_per_prompt)
                           for ci in control_image]
            else:
                control = self.prepare_control_image(model, control_image, height, width, batch_size, num_images_per_prompt)

        if self.do_classifier_free_guidance and edit:
            prompt_embeds = _p2p.embed_rows(prompt_embeds, negative_prompt_embeds)       # [text ; image ; uncond]
        elif self.do_classifier_free_guidance:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds], dim=0)
        prompt_embeds = prompt_embeds.to(self.device)

        if regional:
            # the [2B, R, h, w] weights (uncond rows one-hot on the base prompt) are engine state for this loop only
            rw = _regions.region_weights(_regions.masks_tensor(model, region_masks, height, width), latents.shape[-2],
                                         latents.shape[-1], region_base_weight)
            unet.set_regions(_regions.batch_weights(rw, latents.shape[0], self.do_classifier_free_guidance))
        try:
            latents = self._denoise(model, latents, timesteps, prompt_embeds, cross_attention_kwargs, added_cond_kwargs,
                                    tc_kwargs, guidance_scale, guidance_rescale, seed, control=control,
                                    controlnet_conditioning_scale=controlnet_conditioning_scale,
                                    control_guidance_start=control_guidance_start, control_guidance_end=control_guidance_end,
                                    mask=mask, masked_image_latents=masked_image_latents_2b, image_latents=image_latents,
                                    image_noise=noise,
                                    pag=(float(pag_scale), float(pag_adaptive_scale)) if pag_on else None,
                                    edit=(edit_latents, image_guidance_scale) if edit else None, views=views)
        finally:
            if regional:
                unet.clear_regions()

        # ---- decode (:511-529) ----
        if self.output_type == "pt":
            cfg = model.vae.config
            mean = getattr(cfg, "latents_mean", None)
            std = getattr(cfg, "latents_std", None)
            if mean is not None and std is not None:
                m = torch.tensor(mean).view(1, -1, 1, 1).to(latents.device, latents.dtype)
                s = torch.tensor(std).view(1, -1, 1, 1).to(latents.device, latents.dtype)
                latents = latents * s / cfg.scaling_factor + m
            else:
                latents = latents / cfg.scaling_factor
            images = model.vae.decode(latents, return_dict=False)[0]
        elif self.output_type == "latents":
            images = latents
        else:
            raise ValueError(f"Unknown output_type = '{self.output_type}'")
        return images

    # ------------------------------------------------------------------------------------------
    def _denoise(self, model, latents, timesteps, prompt_embeds, cross_attention_kwargs, added_cond_kwargs, tc_kwargs,
                 guidance_scale, guidance_rescale, seed, control=None, controlnet_conditioning_scale=1.0,
                 control_guidance_start=0.0, control_guidance_end=1.0, mask=None, masked_image_latents=None,
                 image_latents=None, image_noise=None, pag=None, edit=None, views=None):
        """The denoising loop (:465-507): `timesteps` over `latents`, the scheduler's update on the device where
        `_device_step_kind` finds one (`_device_iteration`) and in `scheduler.step` otherwise.  `tc_kwargs` is the
        guidance-embedded UNet's `timestep_cond`, `control` the prepared ControlNet image; `mask`, `masked_image_latents`
        (doubled under CFG), `image_latents` and `image_noise` are the inpainting tensors; `edit` is InstructPix2Pix's
        (image latents, image_guidance_scale): `latents` then hold 4 of the UNet's 8 channels; `views` is MultiDiffusion's
        window plan (__call__'s view_* arguments): every model output of the loop then comes from ViewRunner.forward."""
        unet = self._unet(model)
        num_channels_unet = unet.config.in_channels
        # The reference iterates over the device tensor `timesteps`; reading each element on the host
        # (scheduler.step does int(t)) is a stream-ordered device->host copy, i.e. a full sync behind
        # the UNet forward of every step.  One copy of the schedule to the host before the loop
        # removes those 50 bubbles; the values are the same.
        timesteps_host = [float(v) for v in timesteps.tolist()]
        # ControlNet guidance window (diffusers' controlnet_keep) over this loop's steps; the UNet gets the image once
        # per prompt image (its batch under CFG maps sample b onto image b mod N: diffusers' cat([image] * 2))
        cn_scales = None
        if control is not None:
            from .controlnet import keep_schedule
            rows = keep_schedule(len(timesteps_host), controlnet_conditioning_scale, control_guidance_start,
                                 control_guidance_end)
            cn_scales = rows if isinstance(control, list) else [r[0] for r in rows]
        # prompt_embeds is the same tensor on every step: the engine keeps its cross-attention K/V
        # projections for the duration of this loop (switched off again right after it)
        # DeepCache on this loop's UNet: iteration i runs the full forward and keeps the deep feature when
        # i % interval == 0 (so the first step of every loop stores: a stale cache is never read), the shallow one on
        # that feature otherwise.  The mode is engine state, set in front of every forward whichever path the step takes
        deepcache = getattr(unet, "deepcache", None)
        tome_on = getattr(unet, "tome", None) is not None and hasattr(unet, "tome_step")
        hypertile_on = getattr(unet, "hypertile", None) is not None and hasattr(unet, "hypertile_step")
        kv_cache = getattr(unet, "text_kv_cache", None)
        if kv_cache is not None:
            # the cache is keyed by the buffer's address: hand the engine ONE fp16 contiguous tensor for the whole loop
            # (a per-step conversion inside the shim would make a fresh temporary each step: ADVICE r2)
            if prompt_embeds.device.type == "cuda" and (prompt_embeds.dtype != torch.float16 or not prompt_embeds.is_contiguous()):
                prompt_embeds = prompt_embeds.to(torch.float16).contiguous()
            kv_cache(True)
        # Perturbed-attention guidance: (pag_scale, pag_adaptive_scale); the step's scale s comes from the scheduler's
        # timestep on the host, and a step with s = 0 is the plain step.  guidance_rescale > 0 with it takes scheduler.step.
        pag_rows = None
        if pag is not None:
            names = getattr(model, "_pag", None) or _pag.DEFAULT_LAYERS
            if hasattr(unet, "set_pag_layers"):
                unet.set_pag_layers(names)
            else:
                # a UNet without the engine's forward_pag gets the (G + 1)-group batch: the perturbed group's embeddings
                # and added conditions are the text group's
                text = (lambda x: x.chunk(2)[1]) if self.do_classifier_free_guidance else (lambda x: x)
                pag_rows = (torch.cat([prompt_embeds, text(prompt_embeds)]),
                            None if added_cond_kwargs is None else
                            {k: torch.cat([v, text(v)]) for k, v in added_cond_kwargs.items()})
        # MultiDiffusion: the windows of this loop, their buffers and the embeddings repeated per chunk size, made once (after
        # the conversion above: the repeats are what the engine's K/V cache then sees)
        runner = None
        if views is not None:
            groups = 2 if self.do_classifier_free_guidance else 1
            B = latents.shape[0]
            plan = _views.plan_views(latents.shape[-2], latents.shape[-1], views["window"], views["stride"], views["circular"])
            batch = max(1, 4 // B) if views["batch"] is None else int(views["batch"])
            runner = _views.ViewRunner(plan, B, groups, batch, views["blend"], prompt_embeds, lib=getattr(unet, "_lib", None))
        kind = self._device_step_kind(model, latents, num_channels_unet, guidance_rescale)
        if pag is not None and guidance_rescale > 0.0:
            kind = None
        # what the device steps keep from one iteration to the next: "linear"'s fp32 history (made by the first plan that
        # reads one), "affine"'s fp32 bank of `affine_slots` latents-sized slots, LCM's noise generator
        state = SimpleNamespace(hist=None, bank=None, gen=None)
        # LCMScheduler: one noise draw per non-final step from a generator of this call's own (seeded with `seed`), made the
        # same way at the same point whether the step then runs on the device (sd_lcm_step) or in scheduler.step
        lcm = isinstance(model.scheduler, _sched.LCMScheduler)
        if lcm:
            # the scheduler's own last step adds no noise (a loop cut short by denoising_end does not reach it)
            lcm_final_t = float(model.scheduler.timesteps[-1])
            state.gen = torch.Generator(device=latents.device)
            if seed is not None:
                state.gen.manual_seed(int(seed))
            else:
                state.gen.seed()
        if kind == "affine" and model.scheduler.affine_slots:
            state.bank = torch.empty((model.scheduler.affine_slots,) + tuple(latents.shape), device=latents.device,
                                     dtype=torch.float32)
        blend = None
        if kind and self.is_inpaint:         # 4-channel inpainting: device-side blend after every step
            f16 = lambda x: x.to(device=latents.device, dtype=torch.float16).contiguous()
            m1 = mask.chunk(2)[0] if self.do_classifier_free_guidance else mask
            blend = (f16(image_latents), f16(image_noise), f16(m1.expand(latents.shape[0], 1, *latents.shape[2:])))
        try:
            for i, t in enumerate(timesteps_host):
                cn_kwargs = {} if control is None else dict(controlnet_cond=control,
                                                            controlnet_conditioning_scale=cn_scales[i])
                if deepcache is not None:
                    unet.deep_cache_mode(_DC_STORE if i % deepcache[0] == 0 else _DC_REUSE)
                if tome_on:
                    unet.tome_step(i)        # the iteration token merging's destination draw hashes
                if hypertile_on:
                    unet.hypertile_step(i)   # and the one HyperTile's division draw hashes
                # the step's noise, drawn before the forward.  The affine schedulers that add noise draw it as their `step`
                # does: from the global generator, once per step (the last included, whose noise coefficient is 0), so the
                # device and the host loop consume the same stream
                step_noise = None
                if lcm and t != lcm_final_t:
                    step_noise = torch.randn(latents.shape, dtype=latents.dtype, device=latents.device, generator=state.gen)
                if kind == "affine" and getattr(model.scheduler, "affine_noise", False):
                    step_noise = torch.randn(latents.shape, device=latents.device, dtype=latents.dtype)
                pag_s = _pag.step_scale(pag[0], pag[1], t) if pag is not None else 0.0
                if edit is not None and not kind:
                    # InstructPix2Pix on scheduler.step: the same forward, [text ; image ; uncond] -> eps
                    x = model.scheduler.scale_model_input(latents, t)
                    noise_pred = self._edit_forward(unet, x, 1.0, t, prompt_embeds, edit[0], cross_attention_kwargs)
                    if self.do_classifier_free_guidance:
                        # (in fp32, as the device entries combine: three terms at g_t = 7.5 cost fp16 a digit)
                        noise_pred = _p2p.combine(noise_pred.float(), guidance_scale, edit[1]).to(noise_pred.dtype)
                    latents = self._host_step(model, noise_pred, t, latents, step_noise if lcm else None, lcm)
                    continue
                if kind:
                    # "linear" leaves `timestep_cond` out, which the host path and the other two kinds pass.  Kept as found;
                    # it cannot show today (a guidance-embedded UNet turns CFG off, and "linear" needs CFG)
                    unet_kwargs = cn_kwargs if kind == "linear" else {**cn_kwargs, **tc_kwargs}
                    latents = self._device_iteration(kind, state, model, latents, step_noise, t, prompt_embeds,
                                                     cross_attention_kwargs, added_cond_kwargs, guidance_scale,
                                                     guidance_rescale, pag_s=pag_s, edit=edit, views=runner, **unet_kwargs)
                    if blend is not None:
                        last = i == len(timesteps_host) - 1
                        a, b = (1.0, 0.0) if last else model.scheduler.add_noise_coefficients(timesteps_host[i + 1])
                        self._device_inpaint_blend(model, latents, blend, a, b, with_noise=not last)
                    continue
                if pag_s > 0.0:
                    # [uncond ; text ; perturbed] or [text ; perturbed] -> eps = u + g (t - u) + s (t - p) / t + s (t - p)
                    if pag_rows is None:
                        x = model.scheduler.scale_model_input(latents, t)
                        noise_pred = unet.forward_pag(x, t, prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                                                      cfg=self.do_classifier_free_guidance, share=self.pag_share)[0]
                    else:
                        groups = 3 if self.do_classifier_free_guidance else 2
                        x = model.scheduler.scale_model_input(torch.cat([latents] * groups), t)
                        noise_pred = unet(x, t, pag_rows[0], cross_attention_kwargs=cross_attention_kwargs,
                                          added_cond_kwargs=pag_rows[1], return_dict=False)[0]
                    noise_pred_text = noise_pred.chunk(3)[1] if self.do_classifier_free_guidance else None
                    noise_pred = _pag.combine(noise_pred, guidance_scale, pag_s, self.do_classifier_free_guidance)
                    if guidance_rescale > 0.0:
                        noise_pred = rescale_noise_cfg(noise_pred, noise_pred_text, guidance_rescale)
                    latents = self._host_step(model, noise_pred, t, latents, step_noise if lcm else None, lcm)
                    latents = self._host_inpaint_blend(model, latents, i, timesteps_host, mask, image_latents, image_noise,
                                                       num_channels_unet)
                    continue
                if runner is not None:
                    # MultiDiffusion: the same forward per chunk of windows, merged into a canvas-shaped [G B, ...] output
                    def run(windows, embeds, out, groups=runner.G):
                        x = torch.cat([windows] * groups) if groups > 1 else windows
                        return unet(x, t, embeds, cross_attention_kwargs=cross_attention_kwargs, added_cond_kwargs=None,
                                    return_dict=False)[0]
                    noise_pred = runner.forward(model.scheduler.scale_model_input(latents, t), run)
                else:
                    latent_model_input = torch.cat([latents] * 2) if self.do_classifier_free_guidance else latents
                    latent_model_input = model.scheduler.scale_model_input(latent_model_input, t)
                    if self.is_inpaint and num_channels_unet == 9:
                        latent_model_input = torch.cat([latent_model_input, mask.to(latent_model_input.dtype),
                                                        masked_image_latents.to(latent_model_input.dtype)], dim=1)
                    noise_pred = unet(latent_model_input, t, prompt_embeds,
                                      cross_attention_kwargs=cross_attention_kwargs,
                                      added_cond_kwargs=added_cond_kwargs, return_dict=False, **cn_kwargs, **tc_kwargs)[0]
                if self.do_classifier_free_guidance:
                    noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
                    noise_pred = guidance_scale * (noise_pred_text - noise_pred_uncond) + noise_pred_uncond
                    if guidance_rescale > 0.0:
                        noise_pred = rescale_noise_cfg(noise_pred, noise_pred_text, guidance_rescale)
                if lcm:
                    latents = model.scheduler.step(noise_pred, t, latents, noise=step_noise, return_dict=False)[0]
                else:
                    latents = model.scheduler.step(noise_pred, t, latents, return_dict=False)[0]
                if self.is_inpaint and num_channels_unet == 4:          # :492-506
                    init_latents_proper = image_latents
                    init_mask = mask.chunk(2)[0] if self.do_classifier_free_guidance else mask
                    if i < len(timesteps_host) - 1:
                        init_latents_proper = model.scheduler.add_noise(init_latents_proper, image_noise,
                                                                        torch.as_tensor([timesteps_host[i + 1]]))
                    latents = ((1 - init_mask) * init_latents_proper.float() + init_mask * latents.float()).to(latents.dtype)
        finally:
            if deepcache is not None:
                unet.deep_cache_mode(_DC_PLAIN)
            if kv_cache is not None:
                kv_cache(False)
        return latents

    @staticmethod
    def _check_views(view_window, view_stride, view_batch_size, view_blend):
        """MultiDiffusion's own arguments (what it does not run with: combos.REFUSALS)."""
        if min(_views.as_pair(view_window)) < 1:
            raise ValueError("view_window must be positive")
        if view_stride is not None and min(_views.as_pair(view_stride)) < 1:
            raise ValueError("view_stride must be at least 1")
        if view_batch_size is not None and int(view_batch_size) < 1:
            raise ValueError("view_batch_size must be at least 1")
        _views.window_weights(view_blend, 1, 1)          # (an unknown name raises)

    @staticmethod
    def _host_step(model, noise_pred, t, latents, noise, lcm):
        if lcm:
            return model.scheduler.step(noise_pred, t, latents, noise=noise, return_dict=False)[0]
        return model.scheduler.step(noise_pred, t, latents, return_dict=False)[0]

    def _host_inpaint_blend(self, model, latents, i, timesteps_host, mask, image_latents, image_noise, num_channels_unet):
        """The 4-channel inpaint blend of the host loop (:492-506), for the perturbed-attention steps."""
        if not (self.is_inpaint and num_channels_unet == 4):
            return latents
        init_latents_proper = image_latents
        init_mask = mask.chunk(2)[0] if self.do_classifier_free_guidance else mask
        if i < len(timesteps_host) - 1:
            init_latents_proper = model.scheduler.add_noise(init_latents_proper, image_noise,
                                                            torch.as_tensor([timesteps_host[i + 1]]))
        return ((1 - init_mask) * init_latents_proper.float() + init_mask * latents.float()).to(latents.dtype)

    def _device_inpaint_blend(self, model, latents, blend, a, b, with_noise):
        lib = self._unet(model)._lib
        img, noise, m = blend
        B, Cc, H, W = latents.shape
        _check(lib, lib.sd_inpaint_blend(_ptr(latents), _ptr(img), _ptr(noise) if with_noise else None, _ptr(m),
                                         float(a), float(b), B, Cc, H, W, _stream()))

    def _engine_step_possible(self, model, latents, num_channels_unet) -> bool:
        """What every device step needs: the HIP engine, fp16 CUDA latents and no 9-channel inpainting UNet."""
        return ((not self.is_inpaint or num_channels_unet == 4) and hasattr(self._unet(model), "_lib")
                and latents.is_cuda and latents.dtype == torch.float16)

    def _fused_step_available(self, model, latents, num_channels_unet=4) -> bool:
        """CFG combine + scheduler update as ONE device kernel each side of the UNet:
        the scheduler still computes its coefficients on the host (`fused_plan`: DDIM, Euler, DPM++ 2M are
        all affine in x, eps and the previous x0 prediction), the engine applies them
        (`sd_cfg_duplicate`, `sd_cfg_linear_step`, or `sd_cfg_rescale_linear_step` when guidance_rescale > 0),
        and for inpainting with a 4-channel UNet the mask blend of `:492-506` follows as a third kernel (`sd_inpaint_blend`).  Only with CFG on the HIP engine;
        9-channel inpainting UNets and non-CFG calls take the generic path."""
        return (self.do_classifier_free_guidance and hasattr(model.scheduler, "fused_plan")
                and getattr(model.scheduler, "supports_fused", True) and hasattr(model.scheduler, "add_noise_coefficients")
                and self._engine_step_possible(model, latents, num_channels_unet))

    def _lcm_step_available(self, model, latents, num_channels_unet=4, guidance_rescale=0.0) -> bool:
        """LCMScheduler's step as one device kernel (`sd_lcm_step`: guidance combine, boundary condition, re-noising) on
        the HIP engine with fp16 CUDA latents -- with or without CFG, unlike `_fused_step_available`.  9-channel
        inpainting UNets and guidance_rescale (a per-sample statistic) take scheduler.step."""
        return not guidance_rescale > 0.0 and self._engine_step_possible(model, latents, num_channels_unet)

    def _affine_step_available(self, model, latents, num_channels_unet=4, guidance_rescale=0.0) -> bool:
        """The step of a scheduler with an `affine_plan` (euler_a, DPM++ 2M SDE, PNDM, UniPC) as one device kernel
        (`sd_sched_affine_step`: guidance combine, update, history writes) on the HIP engine with fp16 CUDA latents, with
        or without CFG.  9-channel inpainting UNets and guidance_rescale (a per-sample statistic) take scheduler.step."""
        return (hasattr(model.scheduler, "affine_plan") and not guidance_rescale > 0.0
                and self._engine_step_possible(model, latents, num_channels_unet))

    def _device_step_kind(self, model, latents, num_channels_unet, guidance_rescale):
        """The device step of this call's loop (the table in DESIGN.md): "linear" (sd_cfg_linear_step, or
        sd_cfg_rescale_linear_step under guidance_rescale), "lcm" (sd_lcm_step), "affine" (sd_sched_affine_step), or None
        for the host path (scheduler.step).  The three predicates are the switches that turn a path off."""
        if self._fused_step_available(model, latents, num_channels_unet):
            return "linear"
        if (isinstance(model.scheduler, _sched.LCMScheduler)
                and self._lcm_step_available(model, latents, num_channels_unet, guidance_rescale)):
            return "lcm"
        if self._affine_step_available(model, latents, num_channels_unet, guidance_rescale):
            return "affine"
        return None

    def _device_iteration(self, kind, state, model, latents, noise, t, prompt_embeds, cross_attention_kwargs,
                          added_cond_kwargs, guidance_scale, guidance_rescale=0.0, pag_s=0.0, edit=None, views=None,
                          **unet_kwargs):
        """One iteration with the scheduler's update on the device: the plan from the scheduler, the UNet forward, one
        step entry of the engine over a copy of the latents, the plan committed.  -> the new latents.  `views`
        (MultiDiffusion's ViewRunner) makes the model output from the canvas's windows; it has the canvas's shape, so
        everything after it is the same."""
        sched, unet = model.scheduler, self._unet(model)
        lib = unet._lib
        plan = sched.affine_plan(t) if kind == "affine" else sched.fused_plan(t)
        latents = latents.contiguous()
        rows = 2 if self.do_classifier_free_guidance else 1          # ("linear" runs under CFG only)
        if edit is not None:
            # InstructPix2Pix: rows = [text ; image ; uncond] or the one conditioned group, from the un-duplicated,
            # un-concatenated latents and image latents
            rows = _p2p.GROUPS if self.do_classifier_free_guidance else 1
            model_out = self._edit_forward(unet, latents, plan.in_scale, t, prompt_embeds, edit[0], cross_attention_kwargs)
        elif pag_s > 0.0:
            # perturbed-attention guidance: rows = [uncond ; text ; perturbed] or [text ; perturbed], one engine forward
            rows += 1
            model_out = unet.forward_pag(latents, t, prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                                         in_scale=plan.in_scale, cfg=self.do_classifier_free_guidance,
                                         share=self.pag_share)[0]
        elif views is not None and rows == 2:
            # one forward_cfg per chunk of windows, written straight into the runner's buffer
            def run(windows, embeds, dst):
                unet.forward_cfg(windows, t, embeds, in_scale=plan.in_scale, share=self.cfg_share, out=dst)
            model_out = views.forward(latents, run)
        elif views is not None:
            def run(windows, embeds, dst):
                unet(windows, t, embeds, cross_attention_kwargs=cross_attention_kwargs, return_dict=False, out=dst)
            model_out = views.forward(sched.scale_model_input(latents, t) if kind == "affine" else latents, run)
        elif rows == 2:                              # rows = [uncond ; text], from the un-duplicated latents
            model_out = self._cfg_forward(model, latents, plan.in_scale, t, prompt_embeds, cross_attention_kwargs,
                                          added_cond_kwargs, **unet_kwargs)
        else:
            # "lcm" (guidance-embedded: timestep_cond in unet_kwargs, or no guidance) feeds the latents as they are; its
            # scale_model_input is the identity
            x = sched.scale_model_input(latents, t) if kind == "affine" else latents
            model_out = unet(x, t, prompt_embeds, cross_attention_kwargs=cross_attention_kwargs,
                             added_cond_kwargs=added_cond_kwargs, return_dict=False, **unet_kwargs)[0]
        if kind == "linear" and plan.use_hist and state.hist is None:
            state.hist = torch.zeros(latents.shape, device=latents.device, dtype=torch.float32)
        out = latents.clone()
        n, g = out.numel(), float(guidance_scale)
        if pag_s > 0.0 and kind != "linear":
            # the combine as a launch of its own, then the scheduler's entry on its one-row result
            m = torch.empty_like(out)
            _check(lib, lib.sd_pag_combine(_ptr(model_out), rows, _ptr(m), n, g, float(pag_s), _stream()))
            model_out, rows = m, 1
        if edit is not None and rows == _p2p.GROUPS and kind != "linear":
            m = torch.empty_like(out)
            _check(lib, lib.sd_ip2p_combine(_ptr(model_out), _ptr(m), n, g, float(edit[1]), _stream()))
            model_out, rows = m, 1
        if kind == "linear":
            hist_p = _ptr(state.hist) if plan.use_hist else None
            if edit is not None:
                rc = lib.sd_ip2p_linear_step(_ptr(model_out), _ptr(out), hist_p, n, g, float(edit[1]), plan.c_x, plan.c_eps,
                                             plan.c_hist, plan.h_x, plan.h_eps, _stream())
            elif pag_s > 0.0:
                rc = lib.sd_pag_linear_step(_ptr(model_out), rows, _ptr(out), hist_p, n, g, float(pag_s), plan.c_x, plan.c_eps,
                                            plan.c_hist, plan.h_x, plan.h_eps, _stream())
            elif guidance_rescale > 0.0:
                # the rescale needs a standard deviation per sample, so it is not affine: its own statistics + update kernels
                rc = lib.sd_cfg_rescale_linear_step(_ptr(model_out), _ptr(out), hist_p, out.shape[0], out[0].numel(), g,
                                                    float(guidance_rescale), plan.c_x, plan.c_eps, plan.c_hist, plan.h_x,
                                                    plan.h_eps, None, _stream())
            else:
                rc = lib.sd_cfg_linear_step(_ptr(model_out), _ptr(out), hist_p, n, g, plan.c_x, plan.c_eps, plan.c_hist,
                                            plan.h_x, plan.h_eps, _stream())
        else:
            noise_p = _ptr(noise.contiguous()) if plan.needs_noise else None
            if kind == "lcm":
                rc = lib.sd_lcm_step(_ptr(model_out), rows, _ptr(out), noise_p, None, n, g, plan.d_x, plan.d_out,
                                     plan.p_den, plan.p_noise, _stream())
            else:
                bank_p = _ptr(state.bank) if state.bank is not None else None
                rc = lib.sd_sched_affine_step(_ptr(model_out), rows, _ptr(out), noise_p, bank_p, n, n, g,
                                              C.byref(_lib.step_plan(plan)), _stream())
        _check(lib, rc)
        (sched.affine_commit if kind == "affine" else sched.fused_commit)()
        return out

    def _edit_forward(self, unet, latents, in_scale, t, prompt_embeds, image_latents, cross_attention_kwargs):
        """The UNet forward of one InstructPix2Pix step from the un-duplicated 4-channel latents and the image latents:
        [3B, ...] in [text ; image ; uncond] order under CFG (the third group reads zero image latents), [B, ...] without.
        The engine takes both tensors as they are (forward_concat); any other UNet gets the 8-channel sample."""
        cfg = self.do_classifier_free_guidance
        B = latents.shape[0]
        if hasattr(unet, "forward_concat"):
            return unet.forward_concat(latents, t, prompt_embeds, image_latents, zero_from=2 * B if cfg else B,
                                       in_scale=in_scale)[0]
        x = latents if in_scale == 1.0 else latents * in_scale
        if cfg:
            x, image_latents = torch.cat([x] * _p2p.GROUPS), _p2p.image_rows(image_latents)
        return unet(torch.cat([x, image_latents.to(x.dtype)], dim=1), t, prompt_embeds,
                    cross_attention_kwargs=cross_attention_kwargs, added_cond_kwargs=None, return_dict=False)[0]

    def _cfg_forward(self, model, latents, in_scale, t, prompt_embeds, cross_attention_kwargs, added_cond_kwargs,
                     **unet_kwargs):
        """The UNet forward of one CFG step from the un-duplicated fp16 latents: [2B, ...], negative half first."""
        unet = self._unet(model)
        B = latents.shape[0]
        if not unet_kwargs and hasattr(unet, "forward_cfg") and getattr(unet, "controlnet", None) is None:
            # the engine takes the un-duplicated latents: no 2B-row copy, and the layers in front of the first
            # cross-attention run once per latent
            return unet.forward_cfg(latents, t, prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                                          in_scale=in_scale, share=self.cfg_share)[0]
        # ControlNet calls: duplicate, then the forward that takes the control image
        lib = unet._lib
        lat2 = torch.empty((2 * B,) + tuple(latents.shape[1:]), device=latents.device, dtype=latents.dtype)
        _check(lib, lib.sd_cfg_duplicate(_ptr(latents), _ptr(lat2), latents[0].numel(), B, in_scale, _stream()))
        return unet(lat2, t, prompt_embeds, cross_attention_kwargs=cross_attention_kwargs,
                          added_cond_kwargs=added_cond_kwargs, return_dict=False, **unet_kwargs)[0]

    @staticmethod
    def control_image_processor(model):
        # diffusers: VaeImageProcessor(vae_scale_factor, do_convert_rgb=True, do_normalize=False)
        return VaeImageProcessor(vae_scale_factor=model.vae_scale_factor, do_convert_rgb=True, do_normalize=False)

    def prepare_control_image(self, model, image, height, width, batch_size, num_images_per_prompt):
        """diffusers prepare_image without the CFG doubling: [N, 3, height, width] in [0, 1], N = batch_size x
        num_images_per_prompt (a one-image batch repeats by N, a larger one by num_images_per_prompt).  On the HIP
        device one fp16 buffer for the whole loop (the engine caches the conditioning embedding by its address)."""
        if isinstance(image, (list, tuple)) and image and isinstance(image[0], (list, tuple)):
            raise NotImplementedError("MultiControlNet (a list of control-image lists) is not supported")
        img = self.control_image_processor(model).preprocess(image, height=height, width=width).to(torch.float32)
        if img.shape[1] != 3:
            raise ValueError(f"control_image must have 3 channels, got {img.shape[1]}")
        repeat_by = batch_size * num_images_per_prompt if img.shape[0] == 1 else num_images_per_prompt
        img = img.repeat_interleave(repeat_by, dim=0)
        if img.shape[0] != batch_size * num_images_per_prompt:
            raise ValueError(f"control_image batch {img.shape[0] // repeat_by} does not match the prompt batch {batch_size}")
        img = img.to(self.device)
        if img.is_cuda:
            img = img.to(torch.float16).contiguous()
        return img

    def encode_image(self, image, device, num_images_per_prompt):
        """diffusers 0.27.2 `encode_image` for the base adapters' ImageProjection: image_encoder(feature_extractor(image)
        .pixel_values).image_embeds, repeated per prompt image; the negative is zeros_like (it still goes through the
        adapter's projection in the UNet, so its tokens are not zero).  Once per call: on the engine with
        load_image_encoder's tower (which answers parameters() with its device and dtype), in PyTorch with a torch one.
        With an IP-Adapter Plus (Resampler) adapter loaded: hidden_states[-2] of the image, [n_img, T_feat, D_emb], and
        the same of a zero image as the negative."""
        m = self.model
        if m.image_encoder is None:
            raise ValueError("ip_adapter_image needs model.image_encoder (or pass ip_adapter_image_embeds)")
        p = next(iter(m.image_encoder.parameters()), None)
        enc_device = p.device if p is not None else torch.device("cpu")
        dtype = p.dtype if p is not None else torch.float32
        if not isinstance(image, torch.Tensor):
            if m.feature_extractor is None:
                raise ValueError("ip_adapter_image needs model.feature_extractor for non-tensor images")
            image = m.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=enc_device, dtype=dtype)
        if getattr(m, "ip_adapter_is_plus", False):
            # diffusers' branch for projection layers other than ImageProjection: the penultimate hidden states of the
            # image, and of a zero image as the negative: [n_img, T_feat, D_emb] each
            pos = m.image_encoder(image, output_hidden_states=True).hidden_states[-2]
            neg = m.image_encoder(torch.zeros_like(image), output_hidden_states=True).hidden_states[-2]
            return (pos.repeat_interleave(num_images_per_prompt, dim=0).to(device),
                    neg.repeat_interleave(num_images_per_prompt, dim=0).to(device))
        image_embeds = m.image_encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        return image_embeds.to(device), torch.zeros_like(image_embeds).to(device)

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt,
                                        do_classifier_free_guidance):
        """diffusers 0.27.2 `prepare_ip_adapter_image_embeds` for one adapter -> a list of one [N(.2), n_img, D_img]
        tensor, N = batch x images per prompt, negative half first under CFG (the order of the prompt embeddings).
        Precomputed embeds ([R(.2), n_img, D_img], negative half first under CFG) pass unchanged when R = N and are
        repeated N / R times otherwise (diffusers repeats them N times: the same for the usual R = 1).  With an
        IP-Adapter Plus adapter loaded every tensor has one more axis: [.., n_img, T_feat, D_emb]."""
        if ip_adapter_image_embeds is None:
            if isinstance(ip_adapter_image, list) and len(ip_adapter_image) == 1:
                ip_adapter_image = ip_adapter_image[0]
            pos, neg = self.encode_image(ip_adapter_image, device, 1)
            pos = torch.stack([pos] * num_images_per_prompt, dim=0)
            neg = torch.stack([neg] * num_images_per_prompt, dim=0)
            return [torch.cat([neg, pos]).to(device) if do_classifier_free_guidance else pos.to(device)]
        if isinstance(ip_adapter_image_embeds, torch.Tensor):
            ip_adapter_image_embeds = [ip_adapter_image_embeds]
        if len(ip_adapter_image_embeds) != 1:
            raise ValueError(f"one IP-Adapter is supported, got image embeds for {len(ip_adapter_image_embeds)}")
        e = ip_adapter_image_embeds[0]
        if getattr(getattr(self, "model", None), "ip_adapter_is_plus", False):
            if e.ndim != 4:
                raise ValueError("ip_adapter_image_embeds: an IP-Adapter Plus adapter takes the image encoder's "
                                 f"hidden_states[-2] as [batch, n_img, T_feat, D_emb], got {tuple(e.shape)}")
        elif e.ndim != 3:
            raise ValueError(f"ip_adapter_image_embeds: expected [batch, n_img, D_img], got {tuple(e.shape)}")
        halves = e.chunk(2) if do_classifier_free_guidance else (e,)
        rows = halves[0].shape[0]
        if rows == num_images_per_prompt:
            return [e.to(device)]
        if num_images_per_prompt % rows != 0 or any(h.shape[0] != rows for h in halves):
            raise ValueError(f"ip_adapter_image_embeds: {rows} rows per half do not divide the batch {num_images_per_prompt}")
        rep = num_images_per_prompt // rows
        return [torch.cat([h.repeat(rep, *([1] * (h.ndim - 1))) for h in halves]).to(device)]

    def encode_prompt(self, prompt, prompt_2=None, negative_prompt=None, negative_prompt_2=None,
                      num_images_per_prompt=1, lora_scale=None, clip_skip=None):
        """sd_unified_pipeline.py:532-719: CLIP stays host PyTorch-ROCm (north_star)."""
        m = self.model
        refiner = self._use_refiner
        if refiner:
            if getattr(m, "tokenizer_2", None) is None or getattr(m, "text_encoder_2", None) is None:
                raise ValueError("the refiner reads text_encoder_2 / tokenizer_2, which this model does not have")
        elif m.tokenizer is None or m.text_encoder is None:
            raise ValueError("model has no tokenizer / text_encoder: pass prompt_embeds instead")
        sdxl = hasattr(m, "text_encoder_2") and hasattr(m, "tokenizer_2")
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        toks, encs, prompts = [m.tokenizer], [m.text_encoder], [prompt]
        if refiner:
            # diffusers' StableDiffusionXLImg2ImgPipeline without tokenizer / text_encoder: the second pair alone
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            toks, encs, prompts = [m.tokenizer_2], [m.text_encoder_2], [prompt_2]
        elif sdxl:
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            toks, encs, prompts = [m.tokenizer, m.tokenizer_2], [m.text_encoder, m.text_encoder_2], [prompt, prompt_2]

        def run(texts_list):
            embeds, pooled = [], None
            for texts, tok, enc in zip(texts_list, toks, encs):
                ids = tok(texts, padding="max_length", max_length=tok.model_max_length, truncation=True,
                          return_tensors="pt").input_ids.to(self.device)
                out = enc(ids, output_hidden_states=True)
                pooled = out[0]
                if clip_skip is None:
                    e = out.hidden_states[-2] if sdxl else out[0]
                else:
                    # transformers 4.39 (the reference's pin) nests the layers under `.text_model`;
                    # newer releases expose `final_layer_norm` on the model itself
                    final_ln = getattr(enc, "text_model", enc).final_layer_norm
                    e = (out.hidden_states[-(clip_skip + 2)] if sdxl
                         else final_ln(out.hidden_states[-(clip_skip + 1)]))
                embeds.append(e)
            return torch.concat(embeds, dim=-1), pooled

        prompt_embeds, pooled = run(prompts)
        neg_embeds = neg_pooled = None
        if self.do_classifier_free_guidance:
            negative_prompt = negative_prompt or ""
            negative_prompt_2 = negative_prompt_2 or negative_prompt
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            negative_prompt_2 = (batch_size * [negative_prompt_2] if isinstance(negative_prompt_2, str)
                                 else negative_prompt_2)
            if batch_size != len(negative_prompt):
                raise ValueError("`negative_prompt` batch size does not match `prompt`")
            neg_embeds, neg_pooled = run([negative_prompt_2] if refiner else [negative_prompt, negative_prompt_2])
        dt = self._unet(m).dtype
        bs, seq, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.to(dtype=dt, device=self.device).repeat(1, num_images_per_prompt, 1)
        prompt_embeds = prompt_embeds.view(bs * num_images_per_prompt, seq, -1)
        if neg_embeds is not None:
            neg_embeds = neg_embeds.to(dtype=dt, device=self.device).repeat(1, num_images_per_prompt, 1)
            neg_embeds = neg_embeds.view(batch_size * num_images_per_prompt, seq, -1)
        if sdxl:
            pooled = pooled.repeat(1, num_images_per_prompt).view(bs * num_images_per_prompt, -1)
            if neg_pooled is not None:
                neg_pooled = neg_pooled.repeat(1, num_images_per_prompt).view(bs * num_images_per_prompt, -1)
        return prompt_embeds, neg_embeds, pooled, neg_pooled

    def get_timesteps(self, num_inference_steps, strength, denoising_start=None):
        """sd_unified_pipeline.py:722-761."""
        sch = self.model.scheduler
        if denoising_start is None:
            init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
            t_start = max(num_inference_steps - init_timestep, 0)
        else:
            t_start = 0
        timesteps = sch.timesteps[t_start * sch.order:]
        if denoising_start is not None:
            cutoff = int(round(sch.config.num_train_timesteps - denoising_start * sch.config.num_train_timesteps))
            n = int((timesteps < cutoff).sum().item())
            if sch.order == 2 and n % 2 == 0:
                n += 1
            return timesteps[-n:], n
        return timesteps, num_inference_steps - t_start

    def prepare_latents_txt2img(self, shape, dtype, seed=None, latents=None):
        """sd_unified_pipeline.py:764-787 (generator lives on self.device, like the reference)."""
        generator = None
        if seed is not None:
            generator = torch.Generator(device=self.device).manual_seed(int(seed))
        if latents is None:
            latents = torch.randn(shape, generator=generator, device=self.device, dtype=dtype)
        else:
            latents = latents.to(self.device)
        return latents * self.model.scheduler.init_noise_sigma

    def prepare_image_latents_pix2pix(self, image, batch_size, dtype, hw):
        """InstructPix2Pix's image latents [batch_size, 4, h, w]: the MODE of vae.encode(image), not multiplied by the
        scaling factor (diffusers' prepare_image_latents); a 4-channel `image` is taken as those latents.  Encoded once."""
        if not isinstance(image, torch.Tensor):
            raise ValueError(f"`image` has to be a torch.Tensor in [-1, 1] (got {type(image)})")
        image = image.to(device=self.device, dtype=dtype)
        z = image if image.shape[1] == 4 else self.model.vae.encode(image).latent_dist.mode().to(dtype)
        if tuple(z.shape[-2:]) != tuple(hw):
            raise ValueError(f"image latents are {tuple(z.shape[-2:])}, the run's latents {tuple(hw)}")
        if batch_size > z.shape[0] and batch_size % z.shape[0] == 0:
            z = torch.cat([z] * (batch_size // z.shape[0]), dim=0)
        elif batch_size != z.shape[0]:
            raise ValueError(f"Cannot duplicate `image` of batch size {z.shape[0]} to {batch_size} text prompts.")
        return z.contiguous()

    def prepare_latents_img2img(self, image, timestep, batch_size, num_images_per_prompt, dtype, seed=None,
                                add_noise=True):
        """sd_unified_pipeline.py:790-845."""
        if not isinstance(image, torch.Tensor):
            raise ValueError(f"`image` has to be a torch.Tensor in [-1, 1] (got {type(image)})")
        image = image.to(device=self.device, dtype=dtype)
        batch_size = batch_size * num_images_per_prompt
        generator = None
        if seed is not None:
            generator = torch.Generator(device=self.device).manual_seed(int(seed))
        if image.shape[1] == 4:
            init_latents = image
        else:
            init_latents = self._encode_vae_image(image, generator)
        if batch_size > init_latents.shape[0] and batch_size % init_latents.shape[0] == 0:
            init_latents = torch.cat([init_latents] * (batch_size // init_latents.shape[0]), dim=0)
        elif batch_size > init_latents.shape[0]:
            raise ValueError(f"Cannot duplicate `image` of batch size {init_latents.shape[0]} to {batch_size} text prompts.")
        if add_noise:
            noise = torch.randn(init_latents.shape, generator=generator, device=self.device, dtype=dtype)
            init_latents = self.model.scheduler.add_noise(init_latents, noise, timestep)
        return init_latents

    def prepare_latents_inpaint(self, shape, dtype, seed=None, latents=None, image=None, timestep=None,
                                is_strength_max=True, add_noise=True, return_image_latents=False):
        """sd_unified_pipeline.py:848-913; always returns (latents, noise, image_latents-or-None)."""
        batch_size = shape[0]
        generator = None
        if seed is not None:
            generator = torch.Generator(device=self.device).manual_seed(int(seed))
        if (image is None or timestep is None) and not is_strength_max:
            raise ValueError("Since strength < 1. initial latents are to be initialised as a combination of Image + "
                             "Noise. However, either the image or the noise timestep has not been provided.")
        image_latents = None
        if image.shape[1] == 4:
            image_latents = image.to(device=self.device, dtype=dtype)
            image_latents = image_latents.repeat(batch_size // image_latents.shape[0], 1, 1, 1)
        elif return_image_latents or (latents is None and not is_strength_max):
            image_latents = self._encode_vae_image(image.to(device=self.device, dtype=dtype), generator)
            image_latents = image_latents.repeat(batch_size // image_latents.shape[0], 1, 1, 1)
        if latents is None and add_noise:
            noise = torch.randn(shape, generator=generator, device=self.device, dtype=dtype)
            latents = noise if is_strength_max else self.model.scheduler.add_noise(image_latents, noise, timestep)
            latents = latents * self.model.scheduler.init_noise_sigma if is_strength_max else latents
        elif add_noise:
            noise = latents.to(self.device)
            latents = noise * self.model.scheduler.init_noise_sigma
        else:
            noise = torch.randn(shape, generator=generator, device=self.device, dtype=dtype)
            latents = image_latents.to(self.device)
        return latents, noise, (image_latents if return_image_latents else None)

    def prepare_mask_latents(self, mask, masked_image, batch_size, height, width, dtype, seed=None):
        """sd_unified_pipeline.py:916-976."""
        mask = torch.nn.functional.interpolate(mask, size=(height, width)).to(device=self.device, dtype=dtype)
        if mask.shape[0] < batch_size:
            if batch_size % mask.shape[0] != 0:
                raise ValueError("The passed mask and the required batch size don't match.")
            mask = mask.repeat(batch_size // mask.shape[0], 1, 1, 1)
        mask = torch.cat([mask] * 2) if self.do_classifier_free_guidance else mask
        generator = None
        if seed is not None:
            generator = torch.Generator(device=self.device).manual_seed(int(seed))
        masked_image_latents = masked_image if (masked_image is not None and masked_image.shape[1] == 4) else None
        if masked_image is not None:
            if masked_image_latents is None:
                masked_image_latents = self._encode_vae_image(masked_image.to(device=self.device, dtype=dtype), generator)
            if masked_image_latents.shape[0] < batch_size:
                if batch_size % masked_image_latents.shape[0] != 0:
                    raise ValueError("The passed images and the required batch size don't match.")
                masked_image_latents = masked_image_latents.repeat(batch_size // masked_image_latents.shape[0], 1, 1, 1)
            if self.do_classifier_free_guidance:
                masked_image_latents = torch.cat([masked_image_latents] * 2)
            masked_image_latents = masked_image_latents.to(device=self.device, dtype=dtype)
        return mask, masked_image_latents

    def _encode_vae_image(self, image, generator):
        """sd_unified_pipeline.py:1017-1041."""
        vae = self.model.vae
        dist = vae.encode(image).latent_dist
        z = dist.sample(generator)
        return (z * vae.config.scaling_factor).to(image.dtype)

    def _get_add_time_ids(self, original_size, crops_coords_top_left, target_size, dtype, aesthetic_score=None,
                          negative_aesthetic_score=None):
        """sd_unified_pipeline.py:979-1014.  With `aesthetic_score` (the refiner: diffusers' img2img form with
        requires_aesthetics_score) the score takes target_size's place and the result is (ids, negative ids)."""
        cfg = self._unet(self.model).config
        ad = cfg.addition_time_embed_dim
        pooled = getattr(cfg, "pooled_projection_dim", None) or cfg.projection_class_embeddings_input_dim - 6 * ad
        if aesthetic_score is None:
            ids = list(original_size + crops_coords_top_left + target_size)
            neg = None
        else:
            ids = list(original_size + crops_coords_top_left + (aesthetic_score,))
            neg = list(original_size + crops_coords_top_left + (negative_aesthetic_score,))
        passed = ad * len(ids) + pooled
        expected = self._unet(self.model).add_embedding.linear_1.in_features
        if expected < passed and passed - expected == ad:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of "
                             f"{passed} was created. Please make sure to disable `requires_aesthetics_score` with "
                             "`pipe.register_to_config(requires_aesthetics_score=False)` to make sure `target_size` "
                             f"{target_size} is correctly used by the model.")
        elif passed != expected:
            raise ValueError(f"Model expects an added time embedding vector of length {expected}, but a vector of "
                             f"{passed} was created. The model has an incorrect config. Please check "
                             "`unet.config.time_embedding_type` and `text_encoder_2.config.projection_dim`.")
        if neg is None:
            return torch.tensor([ids], dtype=dtype)
        return torch.tensor([ids], dtype=dtype), torch.tensor([neg], dtype=dtype)

    def _ensemble_of_experts(self, call):
        """`refiner_start=r`: the base denoises the timesteps at or above the cut-off and the refiner the rest, as two
        calls of this pipeline with the same prompts, seed and steps -- A: base, denoising_end=r, latents out;
        B: use_refiner=True, image = A's latents, denoising_start=r (the scheduler is set again at the hand-off, as two
        diffusers calls do).  The latents stay where A left them (on the device)."""
        r = call.pop("refiner_start")
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 < float(r) < 1.0:
            raise ValueError(f"refiner_start must lie in (0, 1), got {r!r}")
        saved = self.output_type
        self.output_type = "latents"
        try:
            latents = self(**dict(call, denoising_end=float(r)))
        finally:
            self.output_type = saved
        # the refiner's half: no start latents, ControlNet or IP-Adapter inputs of the base's
        return self(**dict(call, use_refiner=True, image=latents, denoising_start=float(r), latents=None, strength=1.0,
                           control_image=None, ip_adapter_image=None, ip_adapter_image_embeds=None))
