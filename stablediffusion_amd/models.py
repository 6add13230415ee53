"""Duck-typed stand-ins for the two model objects the reference keeps in `SDModelWrapper.base`
and `SDModelWrapper.vae` (`/root/reference/models/stable_diffusion.py:110-123`), backed by the
gfx950 engine through the C-ABI (`include/sd_engine.h`).

Surface kept:
  base(sample, t, ehs, cross_attention_kwargs=, added_cond_kwargs=, return_dict=False) -> (tensor,)
        sd_unified_pipeline.py:475-482
  base.config.{sample_size,in_channels,addition_time_embed_dim}   :176, :220, :418
  base.add_embedding.linear_1.in_features                          :419
  base.dtype, base.to(device)                                      :680, stable_diffusion.py:189
  vae.decode(z, return_dict=False) -> (tensor,)                    :523
  vae.encode(x).latent_dist.{sample(generator), mode()}            :98-106, :1027-1032
  vae.config.{scaling_factor,latents_mean,latents_std,force_upcast,latent_channels,block_out_channels}
  vae.to(device | dtype=)                                          stable_diffusion.py:188, :1022,1036
PyTorch is plumbing here (device buffers + the current HIP stream); all arithmetic is in the .so.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib
from .config import UNetConfig, VAEConfig


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _read_taps(lib, handle, model: str) -> Dict[str, dict]:
    """The debug-tap records of a handle's last forward (sd_engine.h: sd_unet_tap / sd_vae_tap), by block name:
    {"in", "out": the views as NCHW tensors (fp32 [rows, cols] for the time embedding), "in_rows", "out_rows",
    "pre_rows": the whole NHWC rows [N, H, W, ld] the view was copied with (only where it is narrower than its row),
    "out_c0": the view's first column in them, "scale": the factor the stored activations carry}."""
    count = getattr(lib, f"sd_{model}_tap_count")
    info_fn, read = getattr(lib, f"sd_{model}_tap_info"), getattr(lib, f"sd_{model}_tap_read")
    kinds = {_lib.SD_TAP_IN: "in", _lib.SD_TAP_OUT: "out", _lib.SD_TAP_PRE: "pre"}
    taps: Dict[str, dict] = {}
    for i in range(count(handle)):
        info = _lib.SdTapInfo()
        _lib.check(info_fn(handle, i, C.byref(info)), f"sd_{model}_tap_info")
        f32 = info.dtype == _lib.SD_DTYPE_F32
        rows = torch.empty((info.N, info.H, info.W, info.ld), dtype=torch.float32 if f32 else torch.float16)
        _lib.check(read(handle, i, C.c_void_p(rows.data_ptr()), rows.numel() * rows.element_size()), f"sd_{model}_tap_read")
        rec = taps.setdefault(info.name.decode(), {"scale": float(info.scale)})
        kind = kinds[info.kind]
        if f32:
            rec[kind] = rows.reshape(info.N, info.ld)
            continue
        if kind != "pre":
            rec[kind] = rows[..., info.c0:info.c0 + info.C].permute(0, 3, 1, 2).contiguous()
        if info.ld != info.C:
            rec[kind + "_rows"] = rows
            rec[kind + "_c0"] = info.c0
    return taps


def _poison(obj, model: str, pattern: int) -> int:
    """sd_<model>_poison_workspace on `obj`'s handle (a test facility, sd_engine.h): the scratch memory of the handle is
    filled with NaN (pattern 0: bytes 0xFF) or fp16 +Inf (pattern 1: words 0x7C00).  Returns the bytes filled."""
    n = C.c_int64()
    name = f"sd_{model}_poison_workspace"
    with torch.cuda.device(obj.device):
        _lib.check(getattr(obj._lib, name)(obj._h, int(pattern), C.byref(n)), name)
    return n.value


def _as_f16(x: torch.Tensor, device) -> torch.Tensor:
    return x.to(device=device, dtype=torch.float16).contiguous()


class _Config(SimpleNamespace):
    def get(self, k, d=None):
        return getattr(self, k, d)


def _load_weights(lib, handle, prefix: str, state_dict: Dict[str, torch.Tensor], strict: bool = True):
    num = getattr(lib, f"sd_{prefix}_num_weights")(handle)
    info = getattr(lib, f"sd_{prefix}_weight_info")
    setw = getattr(lib, f"sd_{prefix}_set_weight")
    expected = []
    for i in range(num):
        key = C.c_char_p()
        shape = (C.c_int64 * 4)()
        ndim = C.c_int()
        _lib.check(info(handle, i, C.byref(key), shape, C.byref(ndim)), "weight_info")
        expected.append((key.value.decode(), tuple(shape[j] for j in range(ndim.value))))
    missing = [k for k, _ in expected if k not in state_dict]
    if missing:
        raise KeyError(f"state_dict is missing {len(missing)} keys, e.g. {missing[:3]}")
    if strict:
        names = {k for k, _ in expected}
        extra = [k for k in state_dict if k not in names]
        if extra:
            raise KeyError(f"state_dict has {len(extra)} unexpected keys, e.g. {extra[:3]}")
    for key, shape in expected:
        t = state_dict[key]
        if tuple(t.shape) != shape:
            raise ValueError(f"{key}: expected shape {shape}, got {tuple(t.shape)}")
        if t.dtype == torch.float16:
            code = _lib.SD_DTYPE_F16
        else:
            t = t.float()
            code = _lib.SD_DTYPE_F32
        t = t.contiguous()
        shp = (C.c_int64 * len(shape))(*shape)
        _lib.check(setw(handle, key.encode(), C.c_void_p(t.data_ptr()), shp, len(shape), code),
                   f"set_weight({key})")
    return expected


def _unet_config_struct(config: UNetConfig):
    nb = len(config.block_out_channels)
    c = _lib.SdUNetConfig()
    c.in_channels = config.in_channels
    c.out_channels = config.out_channels
    c.num_blocks = nb
    for i in range(nb):
        c.block_out_channels[i] = config.block_out_channels[i]
        c.down_block_has_attn[i] = int(config.down_block_types[i] == "CrossAttnDownBlock2D")
        c.up_block_has_attn[i] = int(config.up_block_types[i] == "CrossAttnUpBlock2D")
        c.num_heads[i] = config.attention_head_dim[i]
        c.transformer_layers[i] = config.transformer_layers_per_block[i]
    c.layers_per_block = config.layers_per_block
    c.cross_attention_dim = config.cross_attention_dim
    c.use_linear_projection = int(config.use_linear_projection)
    c.norm_num_groups = config.norm_num_groups
    c.norm_eps = config.norm_eps
    c.flip_sin_to_cos = int(config.flip_sin_to_cos)
    c.freq_shift = float(config.freq_shift)
    c.addition_time_embed_dim = config.addition_time_embed_dim or 0
    c.projection_class_embeddings_input_dim = config.projection_class_embeddings_input_dim or 0
    c.num_time_ids = config.num_time_ids
    c.time_cond_proj_dim = getattr(config, "time_cond_proj_dim", None) or 0
    return c


def _check_time_ids(add_ids, cfg: UNetConfig):
    if add_ids.ndim != 2 or add_ids.shape[1] != cfg.num_time_ids:
        raise ValueError(f"time_ids: expected [B, {cfg.num_time_ids}] for this UNet, got {tuple(add_ids.shape)}")


class HipUNet2DConditionModel:
    """gfx950 engine behind the `UNet2DConditionModel` call surface the reference uses."""

    def __init__(self, config: UNetConfig, device: str = "cuda"):
        self._lib = _lib.load()
        self.cfg = config
        self.device = torch.device(device)
        self.dtype = torch.float16
        c = _unet_config_struct(config)
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_unet_create(C.byref(c), C.byref(self._h)), "sd_unet_create")
        self.config = _Config(**config.to_dict())
        if config.addition_embed_type == "text_time":
            self.add_embedding = SimpleNamespace(
                linear_1=SimpleNamespace(in_features=config.projection_class_embeddings_input_dim))
        self._finalized = False
        self._ip = None                # attached HipIPAdapter (attach_ip_adapter)
        self._ip_scale = 1.0
        self._cn = None                # attached HipControlNetModel (attach_controlnet); the first of an attached list
        self._cns = None               # the attached list (attach_controlnets), None while a single net or none is attached
        self._freeu = None             # (s1, s2, b1, b2) while FreeU is on (enable_freeu)
        self._deepcache = None         # (cache_interval, cache_depth) while DeepCache is on (enable_deepcache)
        self._pag = ()                 # site keys of the perturbed transformers (set_pag_layers)
        self._tome = None              # (ratio, max_downsample, sx, sy, use_rand, seed) while token merging is on
        self._hypertile = None         # (tile_size, swap_size, max_depth, seed) while HyperTile is on
        self._regions = None           # (Bw, R, H, W) while regional prompts are set (set_regions)
        self._motion = None            # attached HipMotionAdapter (attach_motion_adapter)

    # -- weights -------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_gpu()
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "unet", state_dict, strict)
            _lib.check(self._lib.sd_unet_finalize(self._h), "sd_unet_finalize")
        self._finalized = True
        return self

    def rebuild(self, state_dict: Dict[str, torch.Tensor]):
        """A fresh engine of the same configuration on the same device with other weights (LoRA re-fuse:
        the packed weights are immutable once finalized)."""
        new = type(self)(self.cfg, self.device).load_state_dict(state_dict)
        if self._freeu is not None:          # FreeU survives the rebuild
            new.enable_freeu(*self._freeu)
        if self._deepcache is not None:      # and so does DeepCache
            new.enable_deepcache(*self._deepcache)
        if self._pag:                        # and the perturbed-attention layers
            new.set_pag_layers(self._pag)
        if self._tome is not None:           # and token merging
            new.enable_tome(*self._tome)
        if getattr(self, "_hypertile", None) is not None:    # and HyperTile
            new.enable_hypertile(*self._hypertile)
        return new

    def rebuild_factory(self):
        """`rebuild` without a reference to this engine: the LoRA re-fuse drops the old engine (and its device memory)
        BEFORE it packs the new one (peak memory was twice the UNet weights)."""
        cls, cfg, dev = type(self), self.cfg, self.device
        return lambda state_dict: cls(cfg, dev).load_state_dict(state_dict)

    def memory(self):
        w, s = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_unet_memory(self._h, C.byref(w), C.byref(s)), "sd_unet_memory")
        return w.value, s.value

    def _poison_workspace(self, pattern: int = 0) -> int:
        """Test facility: overwrite the engine's scratch memory (see `_poison`); returns the bytes filled."""
        return _poison(self, "unet", pattern)

    def use_graph(self, enable: bool = True):
        """Replay the forward from a captured hipGraph (one host call per step instead of ~480)."""
        _lib.check(self._lib.sd_unet_use_graph(self._h, int(bool(enable))), "sd_unet_use_graph")
        self._graph_on = bool(enable)          # (carried over to the engine a LoRA re-fuse builds)
        return self

    def graph_stats(self):
        """(captures, replays) of `use_graph` on this engine since it was created (sd_unet_graph_stats)."""
        c, r = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_unet_graph_stats(self._h, C.byref(c), C.byref(r)), "sd_unet_graph_stats")
        return c.value, r.value

    def text_kv_cache(self, enable: bool = True):
        """Reuse the cross-attention K/V projections of `encoder_hidden_states` across the forwards of one
        denoise loop (same tensor every step).  Each call invalidates the cache; the pipeline calls it with
        True before its loop and with False after it."""
        _lib.check(self._lib.sd_unet_text_kv_cache(self._h, int(bool(enable))), "sd_unet_text_kv_cache")
        return self

    def attach_ip_adapter(self, adapter: Optional["HipIPAdapter"]):
        """Attach an IP-Adapter built for this configuration (None detaches).  While attached, every call needs
        added_cond_kwargs["image_embeds"] and each cross-attention adds scale * SDPA(q, K_ip, V_ip)."""
        if adapter is not None and adapter.cfg.to_dict() != self.cfg.to_dict():
            raise ValueError("IP-Adapter was built for another UNet configuration")
        _lib.check(self._lib.sd_unet_set_ip_adapter(self._h, adapter._h if adapter is not None else None),
                   "sd_unet_set_ip_adapter")
        if self._ip is not None and self._ip is not adapter:
            self._ip._unet = None
        if adapter is not None:
            old = adapter._unet() if adapter._unet is not None else None
            if old is not None and old is not self:
                old._ip = None
            adapter._unet = weakref.ref(self)      # (no cycle: a dropped engine frees its device memory at once)
        self._ip = adapter
        return self

    def make_ip_adapter(self, state_dict: Dict[str, torch.Tensor], image_embed_dim: int, num_tokens: int):
        """A HipIPAdapter for this engine's configuration, loaded from diffusers-named weights.  The projection kind
        comes from the state dict: with an IP-Adapter Plus Resampler under it, its sizes are read from the shapes."""
        from . import ip_adapter
        rc = ip_adapter.resampler_config(state_dict, self.cfg) if ip_adapter.is_resampler(state_dict) else None
        return HipIPAdapter(self, image_embed_dim, num_tokens, resampler=rc).load_state_dict(state_dict)

    @property
    def ip_adapter(self):
        return self._ip

    def set_ip_adapter_scale(self, scale: float):
        """diffusers' set_ip_adapter_scale: lambda of the image branch (default 1.0; 0 = text attention only)."""
        _lib.check(self._lib.sd_unet_set_ip_adapter_scale(self._h, float(scale)), "sd_unet_set_ip_adapter_scale")
        self._ip_scale = float(scale)
        return self

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' UNet2DConditionModel.enable_freeu (same argument order): in up blocks 0 and 1 the first half of
        the backbone channels is scaled by b1 / b2 and the skip's lowest frequencies by s1 / s2, one in-place engine
        launch per resnet.  The settings survive `rebuild`.  Not available under `use_graph`."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        if not all(math.isfinite(v) for v in vals):
            raise ValueError(f"enable_freeu: s1, s2, b1, b2 must be finite, got {vals}")
        _lib.check(self._lib.sd_unet_set_freeu(self._h, 1, *vals), "sd_unet_set_freeu")
        self._freeu = vals
        return self

    def disable_freeu(self):
        """diffusers' disable_freeu: the forward is again exactly the plain one."""
        _lib.check(self._lib.sd_unet_set_freeu(self._h, 0, 1.0, 1.0, 1.0, 1.0), "sd_unet_set_freeu")
        self._freeu = None
        return self

    def enable_tome(self, ratio: float = 0.5, max_downsample: int = 1, sx: int = 2, sy: int = 2, use_rand: bool = True,
                    seed: int = 0):
        """Token merging (tomesd.apply_patch with its defaults, same argument names): the self-attention of every
        transformer block at most `max_downsample` times smaller than the sample runs on the tokens left after
        `int(T * ratio)` of them were merged into their most similar destination token (one per `sy` x `sx` cell, drawn
        per step when `use_rand`).  Lossy and opt-in.  The settings survive `rebuild`.  Not available under `use_graph`,
        in `forward_pag` or on an 8-channel edit UNet's two-source forward."""
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= float(ratio) <= 0.75:
            raise ValueError(f"enable_tome: ratio must be in [0, 0.75], got {ratio!r}")
        for name, v in (("sx", sx), ("sy", sy)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 8:
                raise ValueError(f"enable_tome: {name} must be an int in 1..8, got {v!r}")
        if isinstance(max_downsample, bool) or max_downsample not in (1, 2, 4, 8):
            raise ValueError(f"enable_tome: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"enable_tome: seed must be an int in [0, 2^32), got {seed!r}")
        if float(ratio) == 0.0:
            return self.disable_tome()
        vals = (float(ratio), int(max_downsample), int(sx), int(sy), bool(use_rand), int(seed))
        _lib.check(self._lib.sd_unet_set_tome(self._h, vals[0], vals[1], vals[2], vals[3], int(vals[4]), vals[5]),
                   "sd_unet_set_tome")
        self._tome = vals
        return self

    def disable_tome(self):
        """The forward is again exactly the plain one and the engine releases the merge plans' buffer."""
        _lib.check(self._lib.sd_unet_set_tome(self._h, 0.0, 1, 2, 2, 0, 0), "sd_unet_set_tome")
        self._tome = None
        return self

    def enable_hypertile(self, tile_size: int = 32, swap_size: int = 2, max_depth: int = 0, seed: int = 0):
        """HyperTile: the self-attention of every transformer block of a level <= `max_depth` attends within the tiles
        of a division of its map that is drawn anew per step (stablediffusion_amd.hypertile.plan; `tile_size` in tokens
        of the block's own level, `swap_size` candidates per axis).  Lossy and opt-in.  The settings survive `rebuild`.
        Not together with token merging, not under `use_graph`, not in `forward_pag` (EngineError, SD_ERR_UNSUPPORTED)."""
        for name, v, lo, hi in (("tile_size", tile_size, 1, 2 ** 31 - 1), ("swap_size", swap_size, 1, 8),
                                ("max_depth", max_depth, 0, 3), ("seed", seed, 0, 2 ** 32 - 1)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"enable_hypertile: {name} must be an int in [{lo}, {hi}], got {v!r}")
        vals = (int(tile_size), int(swap_size), int(max_depth), int(seed))
        _lib.check(self._lib.sd_unet_set_hypertile(self._h, *vals), "sd_unet_set_hypertile")
        self._hypertile = vals
        return self

    def disable_hypertile(self):
        """The forward is again exactly the plain one."""
        _lib.check(self._lib.sd_unet_set_hypertile(self._h, 0, 1, 0, 0), "sd_unet_set_hypertile")
        self._hypertile = None
        return self

    @property
    def hypertile(self):
        """(tile_size, swap_size, max_depth, seed) while HyperTile is on, else None."""
        return self._hypertile

    def hypertile_step(self, i: int):
        """The denoising iteration the division draw of the following forwards hashes (the pipeline's loop calls it)."""
        _lib.check(self._lib.sd_unet_hypertile_step(self._h, int(i) & 0xFFFFFFFF), "sd_unet_hypertile_step")
        return self

    def hypertile_sites(self):
        """The self-attention sites HyperTile covered in the last forward, in execution order: dicts with site, H, W,
        nh, nw, images, copied (the gather / scatter launches ran) and level."""
        out = []
        for k in range(self._lib.sd_unet_hypertile_sites(self._h)):
            info = (C.c_int32 * 8)()
            _lib.check(self._lib.sd_unet_hypertile_read(self._h, k, info), "sd_unet_hypertile_read")
            out.append(dict(site=info[0], H=info[1], W=info[2], nh=info[3], nw=info[4], images=info[5],
                            copied=bool(info[6]), level=info[7]))
        return out

    def set_regions(self, weights):
        """Regional prompts (stablediffusion_amd.regions): weights [Bw, R, H, W] at the sample's latent size, one row per
        batch row of the following forwards (row n reads n % Bw; under CFG the [2B, ...] of regions.batch_weights), summing
        to 1 over R.  Until clear_regions() every `attn2` of __call__ / forward_cfg weighs the R segments of an
        encoder_hidden_states of R L tokens per query, in one engine launch; everything else is the plain forward.
        Not with a ControlNet, an IP-Adapter at a non-zero scale, forward_pag / forward_concat, timestep_cond, graph
        replay, token merging or a DeepCache store / reuse step (EngineError, SD_ERR_UNSUPPORTED)."""
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        if not isinstance(weights, torch.Tensor) or weights.ndim != 4:
            raise ValueError("set_regions: expected weights [Bw, R, H, W]")
        Bw, R, H, W = weights.shape
        if not 1 <= R <= 8:
            raise ValueError(f"set_regions: 1 to 8 regions, got {R}")
        w = weights.to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            rc = self._lib.sd_unet_set_regions(self._h, C.c_void_p(w.data_ptr()), Bw, R, H, W, C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_unet_set_regions")
        self._regions = (Bw, R, H, W)
        return self

    def clear_regions(self):
        """The forward is again exactly the plain one and the engine releases the regional weights."""
        _lib.check(self._lib.sd_unet_set_regions(self._h, None, 0, 0, 0, 0, None), "sd_unet_set_regions")
        self._regions = None
        return self

    @property
    def regions(self):
        """(Bw, R, H, W) while regional prompts are set, else None."""
        return self._regions

    @property
    def tome(self):
        """(ratio, max_downsample, sx, sy, use_rand, seed) while token merging is on, else None."""
        return self._tome

    def tome_step(self, i: int):
        """The denoising iteration the destination draw of the following forwards hashes (the pipeline's loop calls it)."""
        _lib.check(self._lib.sd_unet_tome_step(self._h, int(i) & 0xFFFFFFFF), "sd_unet_tome_step")
        return self

    def tome_sites(self):
        """The blocks that merged in the last forward, in execution order: dicts with site, H, W, r, T_merged and the
        unmerge maps [images, H * W] (int32 tensor on the CPU)."""
        out = []
        for k in range(self._lib.sd_unet_tome_sites(self._h)):
            info = (C.c_int32 * 5)()
            n = self._lib.sd_unet_tome_read(self._h, k, info, None, 0)
            if n < 0:
                _lib.check(-n, "sd_unet_tome_read")
            maps = torch.empty(n, info[1] * info[2], dtype=torch.int32)
            n = self._lib.sd_unet_tome_read(self._h, k, info, C.cast(maps.data_ptr(), C.POINTER(C.c_int32)), maps.numel())
            if n < 0:
                _lib.check(-n, "sd_unet_tome_read")
            out.append(dict(site=info[0], H=info[1], W=info[2], r=info[3], T_merged=info[4], maps=maps))
        return out

    def set_pag_layers(self, layers):
        """Which transformers `forward_pag` perturbs: diffusers' `pag_applied_layers` spellings ("mid", "down.block_2",
        "up.block_1.attentions_0", a list of them) or the engine's site keys ("mid_block.attentions.0", ...); None or an
        empty list clears them.  A name that selects no transformer of this UNet is a ValueError.  The settings survive
        `rebuild`; every other forward ignores them."""
        from . import pag
        if layers is None or (not isinstance(layers, str) and len(tuple(layers)) == 0):
            keys = ()
        else:
            names = (layers,) if isinstance(layers, str) else tuple(layers)
            sites = pag.transformer_sites(self.cfg)
            keys = tuple(names) if all(n in sites for n in names) else pag.site_keys(self.cfg, names)
            keys = tuple(k for k in sites if k in keys)
        if keys == self._pag:                # (every call resets the engine's plans and its text K/V cache)
            return self
        arr = (C.c_char_p * max(len(keys), 1))(*[k.encode() for k in keys])
        _lib.check(self._lib.sd_unet_set_pag_layers(self._h, arr, len(keys)), "sd_unet_set_pag_layers")
        self._pag = keys
        return self

    @property
    def pag_layers(self):
        """The engine's site keys of the perturbed transformers, in execution order."""
        return self._pag

    # the forward modes of DeepCache (sd_engine.h: SD_DC_*)
    DC_PLAIN, DC_STORE, DC_REUSE = 0, 1, 2

    def enable_deepcache(self, cache_interval: int = 3, cache_depth: int = 1):
        """DeepCache (Ma, Fang, Wang, CVPR 2024): the pipeline's loop runs the full UNet on every `cache_interval`-th
        step and, on the steps between, only `cache_depth` layers of down block 0 and the `cache_depth + 1` last layers
        of the last up block, on the deep feature the full step left in the engine.  Lossy and opt-in; interval 1 is
        the plain loop.  The settings survive `rebuild`.  Not available under `use_graph` or with a ControlNet that
        runs.  By hand: `deep_cache_mode`."""
        for name, v in (("cache_interval", cache_interval), ("cache_depth", cache_depth)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"enable_deepcache: {name} must be an int, got {v!r}")
        if cache_interval < 1:
            raise ValueError(f"enable_deepcache: cache_interval must be >= 1, got {cache_interval}")
        if not 1 <= cache_depth <= self.cfg.layers_per_block:
            raise ValueError(f"enable_deepcache: cache_depth must be in 1..{self.cfg.layers_per_block} "
                             f"(layers_per_block), got {cache_depth}")
        _lib.check(self._lib.sd_unet_set_deep_cache(self._h, cache_depth), "sd_unet_set_deep_cache")
        self._deepcache = (cache_interval, cache_depth)
        return self

    def disable_deepcache(self):
        """The forward is again exactly the plain one and the engine releases the cached feature's buffer."""
        _lib.check(self._lib.sd_unet_set_deep_cache(self._h, 0), "sd_unet_set_deep_cache")
        self._deepcache = None
        return self

    @property
    def deepcache(self):
        """(cache_interval, cache_depth) while DeepCache is on, else None."""
        return self._deepcache

    def deep_cache_mode(self, mode: int):
        """Mode of the following forwards, until changed: DC_PLAIN (0), DC_STORE (1: the full forward, which keeps the
        deep feature) or DC_REUSE (2: the shallow forward on the kept feature)."""
        _lib.check(self._lib.sd_unet_deep_cache_mode(self._h, int(mode)), "sd_unet_deep_cache_mode")
        return self

    def attach_motion_adapter(self, adapter: Optional["HipMotionAdapter"]):
        """Attach an AnimateDiff motion adapter built for this UNet's topology (None detaches: every forward is again
        exactly the plain one).  Attached, a call with num_frames= treats its batch as videos of that many consecutive
        frames and runs a motion module behind every (resnet, transformer) pair; without num_frames nothing changes."""
        _lib.check(self._lib.sd_unet_set_motion(self._h, adapter._h if adapter is not None else None), "sd_unet_set_motion")
        if self._motion is not None and self._motion is not adapter:
            self._motion._unet = None
        if adapter is not None:
            old = adapter._unet() if adapter._unet is not None else None
            if old is not None and old is not self:
                old._motion = None
            adapter._unet = weakref.ref(self)
        self._motion = adapter
        return self

    def make_motion_adapter(self, config, state_dict: Dict[str, torch.Tensor]):
        """A HipMotionAdapter for this engine from an engine-named state dict (stablediffusion_amd.motion.load)."""
        return HipMotionAdapter(self, config).load_state_dict(state_dict)

    @property
    def motion_adapter(self):
        return self._motion

    def attach_controlnet(self, controlnet: Optional["HipControlNetModel"]):
        """Attach a ControlNet built for this UNet (None detaches).  While attached, every call needs controlnet_cond=
        and controlnet_conditioning_scale=; the residuals are added inside the engine's forward."""
        _lib.check(self._lib.sd_unet_set_controlnet(self._h, controlnet._h if controlnet is not None else None),
                   "sd_unet_set_controlnet")
        if self._cn is not None and self._cn is not controlnet:
            self._cn._unet = None
        if controlnet is not None:
            old = controlnet._unet() if controlnet._unet is not None else None
            if old is not None and old is not self:
                old._forget_controlnet(controlnet)
            controlnet._unet = weakref.ref(self)
        for other in self._cns or ():
            if other is not controlnet:
                other._unet = None
        self._cn = controlnet
        self._cns = None
        return self

    def attach_controlnets(self, controlnets):
        """Attach a list of ControlNets built for this UNet (MultiControlNet; an empty list detaches all).  While a list
        is attached, controlnet_cond= and controlnet_conditioning_scale= are lists with one entry per net (a float scale
        broadcasts); a net at scale 0 does not run."""
        nets = list(controlnets)
        if len(nets) > _lib.SD_MAX_CONTROLNETS:
            raise ValueError(f"at most {_lib.SD_MAX_CONTROLNETS} ControlNets, got {len(nets)}")
        arr = (C.c_void_p * max(len(nets), 1))(*[n._h for n in nets])
        _lib.check(self._lib.sd_unet_set_controlnets(self._h, arr, len(nets)), "sd_unet_set_controlnets")
        for old in ([self._cn] if self._cn is not None else []) + list(self._cns or ()):
            if not any(old is n for n in nets):
                old._unet = None
        for n in nets:
            prev = n._unet() if n._unet is not None else None
            if prev is not None and prev is not self:
                prev._forget_controlnet(n)
            n._unet = weakref.ref(self)
        self._cn = nets[0] if nets else None
        self._cns = nets if nets else None
        return self

    @property
    def controlnets(self):
        """The attached list (attach_controlnets), or the single attached net as a list of one; [] without."""
        return list(self._cns) if self._cns is not None else ([self._cn] if self._cn is not None else [])

    def cn_fold_count(self) -> int:
        """Launches of the MultiControlNet scale fold since this engine was created (sd_unet_cn_fold_count)."""
        return int(self._lib.sd_unet_cn_fold_count(self._h))

    def _forget_controlnet(self, net):
        """`net` was attached elsewhere or destroyed: the engine has dropped it from this UNet's list already."""
        if self._cns is not None:
            self._cns = [n for n in self._cns if n is not net] or None
            self._cn = self._cns[0] if self._cns else None
        elif self._cn is net:
            self._cn = None

    def make_controlnet(self, cn_config: UNetConfig, state_dict: Dict[str, torch.Tensor]):
        """A HipControlNetModel for this engine, loaded from diffusers-named weights."""
        return HipControlNetModel(self, cn_config).load_state_dict(state_dict)

    @property
    def controlnet(self):
        return self._cn

    def _control(self, controlnet_cond, scale, B, H, W, dev):
        if self._cn is None:
            if controlnet_cond is not None or scale is not None:
                raise ValueError("controlnet_cond / controlnet_conditioning_scale given but no ControlNet is attached")
            return None, 0.0
        if controlnet_cond is None or scale is None:
            raise ValueError("a ControlNet is attached: controlnet_cond and controlnet_conditioning_scale are required")
        if self._cns is not None:
            return self._control_list(controlnet_cond, scale, B, H, W, dev)
        if isinstance(controlnet_cond, (list, tuple)) or isinstance(scale, (list, tuple)):
            raise NotImplementedError("MultiControlNet (lists of control images / scales) needs a list of nets: "
                                      "attach_controlnets")
        return self._control_image(controlnet_cond, B, H, W, dev), float(scale)

    @staticmethod
    def _control_image(controlnet_cond, B, H, W, dev):
        cond = _as_f16(controlnet_cond, dev)
        n = cond.shape[0]
        if cond.ndim != 4 or cond.shape[1] != 3 or cond.shape[2] != 8 * H or cond.shape[3] != 8 * W:
            raise ValueError(f"controlnet_cond: expected [n, 3, {8 * H}, {8 * W}], got {tuple(cond.shape)}")
        if n < 1 or B % n:
            raise ValueError(f"controlnet_cond: {n} images do not divide the batch {B}")
        return cond

    def _control_list(self, controlnet_cond, scale, B, H, W, dev):
        """With a list attached: one image and one scale per net (a float scale broadcasts); a net at scale 0 does not
        run and its image may be None.  Returns ([images or None], [scales])."""
        N = len(self._cns)
        if not isinstance(controlnet_cond, (list, tuple)) or len(controlnet_cond) != N:
            raise ValueError(f"a list of {N} ControlNets is attached: controlnet_cond must be a list of {N} images")
        if isinstance(scale, (list, tuple)):
            if len(scale) != N:
                raise ValueError(f"controlnet_conditioning_scale: {len(scale)} scales for {N} ControlNets")
            scales = [float(v) for v in scale]
        else:
            scales = [float(scale)] * N
        conds = []
        for img, sc in zip(controlnet_cond, scales):
            if img is None:
                if sc != 0.0:
                    raise ValueError("controlnet_cond: None for a ControlNet at a non-zero scale")
                conds.append(None)
            else:
                conds.append(self._control_image(img, B, H, W, dev))
        return conds, scales

    def _image_embeds(self, added_cond_kwargs, B, dev):
        embeds = (added_cond_kwargs or {}).get("image_embeds")
        if self._ip is None:
            if embeds is not None:
                raise ValueError("added_cond_kwargs['image_embeds'] given but no IP-Adapter is attached")
            return None
        if embeds is None:
            raise ValueError("an IP-Adapter is attached: added_cond_kwargs['image_embeds'] is required")
        if isinstance(embeds, (list, tuple)):
            if len(embeds) != 1:
                raise ValueError(f"one IP-Adapter is attached, got image_embeds for {len(embeds)}")
            embeds = embeds[0]
        if self._ip.kind == "resampler":
            want = (B, self._ip.feature_tokens, self._ip.image_embed_dim)
            if embeds.ndim != 4 or (embeds.shape[0], embeds.shape[2], embeds.shape[3]) != want:
                raise ValueError(f"image_embeds: an IP-Adapter Plus (Resampler) adapter is attached: expected the image "
                                 f"encoder's hidden_states[-2] as [{B}, n_img, {want[1]}, {want[2]}], got {tuple(embeds.shape)}")
            return _as_f16(embeds, dev)
        if embeds.ndim == 2:               # deprecated diffusers form [B, D_img]: one image per prompt
            embeds = embeds[:, None]
        if embeds.ndim != 3 or embeds.shape[0] != B or embeds.shape[2] != self._ip.image_embed_dim:
            raise ValueError(f"image_embeds: expected [{B}, n_img, {self._ip.image_embed_dim}], got {tuple(embeds.shape)}")
        return _as_f16(embeds, dev)

    def _prepare(self, sample, timestep, encoder_hidden_states, added_cond_kwargs, groups=None):
        """What the three forward entries share: the fp16 sample (or un-duplicated latents) [B, C, H, W], the text rows,
        the timesteps [B] fp32 and the text_time pair as pointers.  `groups` (forward_cfg / forward_pag): the text and
        text_time tensors hold groups x B rows and the timestep holds one value or B; None: the plain forward."""
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        dev = self.device
        sample = _as_f16(sample, dev)
        B = sample.shape[0]
        ehs = _as_f16(encoder_hidden_states, dev)
        if ehs.shape[0] != (groups or 1) * B:
            raise ValueError(f"encoder_hidden_states batch {ehs.shape[0]} != " +
                             (f"sample batch {B}" if groups is None else f"{groups} x latents batch {B}"))
        if ehs.shape[2] != self.cfg.cross_attention_dim:
            raise ValueError("encoder_hidden_states width != cross_attention_dim")
        if isinstance(timestep, (int, float)):
            # a fill kernel, not a pageable host-to-device copy (which synchronises) on every step
            t = torch.full((B,), float(timestep), device=dev, dtype=torch.float32)
        else:
            t = torch.as_tensor(timestep, device=dev).to(torch.float32).reshape(-1)
            if groups is not None and t.numel() not in (1, B):
                raise ValueError(f"timestep: expected a scalar or {B} values (one per latent), got {t.numel()}")
            t = t.expand(B).contiguous() if t.numel() == 1 else t.contiguous()
        pt = pi = None
        keep = ()
        if self.cfg.addition_embed_type == "text_time":
            if not added_cond_kwargs or "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
                raise ValueError("added_cond_kwargs needs text_embeds and time_ids for text_time conditioning")
            add_text = _as_f16(added_cond_kwargs["text_embeds"], dev)
            add_ids = added_cond_kwargs["time_ids"].to(device=dev, dtype=torch.float32).contiguous()
            _check_time_ids(add_ids, self.cfg)
            if groups is not None and (add_text.shape[0] != groups * B or add_ids.shape[0] != groups * B):
                raise ValueError(f"text_embeds / time_ids must hold {groups} x latents batch rows")
            pt, pi = C.c_void_p(add_text.data_ptr()), C.c_void_p(add_ids.data_ptr())
            keep = (add_text, add_ids)          # (the caller holds them until its engine call has been issued)
        return dev, sample, ehs, t, pt, pi, keep

    # -- reference surface ---------------------------------------------------------------------
    def to(self, device=None, dtype=None):
        if device is not None and torch.device(device).type != "cuda":
            raise _lib.EngineError("HipUNet2DConditionModel lives on the HIP device only")
        return self

    def eval(self):
        return self

    def __call__(self, sample, timestep, encoder_hidden_states, cross_attention_kwargs=None,
                 added_cond_kwargs=None, return_dict=False, controlnet_cond=None, controlnet_conditioning_scale=None,
                 timestep_cond=None, out=None, num_frames=None, **unused):
        # diffusers' residual-tensor interface (a ControlNet run outside the engine): not taken -- silently dropping
        # it would return the plain UNet's output.  Attach the ControlNet instead (attach_controlnet).
        for k in ("down_block_additional_residuals", "mid_block_additional_residual", "down_intrablock_additional_residuals",
                  "guess_mode"):
            v = unused.get(k)
            if v is not None and v is not False:
                raise NotImplementedError(f"HipUNet2DConditionModel: {k} is not supported; attach the ControlNet to the "
                                          "engine (attach_controlnet) and pass controlnet_cond=")
        dev, sample, ehs, t, pt, pi, _keep = self._prepare(sample, timestep, encoder_hidden_states, added_cond_kwargs)
        B, _, H, W = sample.shape
        if num_frames and self._ip is not None and self._ip_scale == 0.0 and not (added_cond_kwargs or {}).get("image_embeds"):
            img = None          # frames with an IP-Adapter at scale 0: the text attention alone, no image_embeds needed
        else:
            img = self._image_embeds(added_cond_kwargs, B, dev)
        ctrl, cscale = self._control(controlnet_cond, controlnet_conditioning_scale, B, H, W, dev)
        tc = None
        if timestep_cond is not None:
            # guidance-embedded UNet (LCM): [B, time_cond_proj_dim], fp32 for the engine.  A tensor that is fp32 and
            # contiguous on the device already -- what the pipeline makes once per call -- passes through untouched.
            if self._cn is not None:
                raise NotImplementedError("timestep_cond with a ControlNet attached is not supported")
            tc = timestep_cond.to(device=dev, dtype=torch.float32).contiguous()
            if tc.ndim != 2 or tc.shape[0] != B:
                raise ValueError(f"timestep_cond: expected [{B}, time_cond_proj_dim], got {tuple(tc.shape)}")
        out = self._out_buffer(out, (B, self.cfg.out_channels, H, W), dev)
        # one argument list; the entry is the narrowest that takes what is present (sd_engine.h)
        head = (self._h, C.c_void_p(sample.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(ehs.data_ptr()), ehs.shape[1],
                pt, pi)
        images = (C.c_void_p(img.data_ptr()) if img is not None else None, img.shape[1] if img is not None else 0)
        tail = (C.c_void_p(out.data_ptr()), B, H, W, C.c_void_p(_stream_ptr()))
        if num_frames:
            # videos of num_frames consecutive frames through the attached motion adapter: the entry takes neither images
            # nor a ControlNet nor timestep_cond, and the engine refuses every state it does not compose with frames
            if tc is not None or ctrl is not None or img is not None or pt is not None:
                raise NotImplementedError("num_frames= takes no timestep_cond, ControlNet, image_embeds or text_time conditions")
            fn, extra = self._lib.sd_unet_forward_motion, None
        elif tc is not None:
            fn, extra = self._lib.sd_unet_forward_tc, images + (C.c_void_p(tc.data_ptr()), tc.shape[1])
        elif isinstance(ctrl, list):
            N = len(ctrl)
            ptrs = (C.c_void_p * N)(*[c.data_ptr() if c is not None else None for c in ctrl])
            counts = (C.c_int * N)(*[c.shape[0] if c is not None else 0 for c in ctrl])
            fn, extra = self._lib.sd_unet_forward_mcn, images + (ptrs, counts, (C.c_float * N)(*cscale), N)
        elif ctrl is not None:
            fn, extra = self._lib.sd_unet_forward_cn, images + (C.c_void_p(ctrl.data_ptr()), ctrl.shape[0], cscale)
        elif img is not None:
            fn, extra = self._lib.sd_unet_forward_ex, images
        else:
            fn, extra = self._lib.sd_unet_forward, ()
        with torch.cuda.device(dev):
            if extra is None:
                rc = fn(*head[:5], int(num_frames), *tail)
            else:
                rc = fn(*head, *extra, *tail)
        _lib.check(rc, "sd_unet_forward")
        if return_dict:
            return SimpleNamespace(sample=out)
        return (out,)

    forward = __call__

    def forward_tapped(self, *args, **kwargs):
        """One plain forward (the arguments of __call__) with the engine's debug taps on: (out, taps), `taps` as
        _read_taps returns them with the sample as conv_in's input and the output as the tail's."""
        _lib.check(self._lib.sd_unet_tap(self._h, 1), "sd_unet_tap")
        try:
            out = self(*args, **kwargs)[0]
            taps = _read_taps(self._lib, self._h, "unet")
        finally:
            _lib.check(self._lib.sd_unet_tap(self._h, 0), "sd_unet_tap")
        sample = args[0] if args else kwargs["sample"]
        taps["conv_in"]["in"] = sample.detach().to("cpu", torch.float16)
        taps["tail"]["out"] = out.cpu()
        return out, taps

    @property
    def cfg_share_eligible(self) -> bool:
        """Whether this topology lets forward_cfg run the CFG-shared start of the UNet once per latent."""
        c = _unet_config_struct(self.cfg)
        return bool(self._lib.sd_unet_cfg_share(C.byref(c)))

    @staticmethod
    def _out_buffer(out, shape, dev):
        """The forward's output tensor: a fresh one, or the caller's `out=` (fp16, contiguous, on the device, of exactly
        the output's shape -- e.g. a slice of a larger buffer), which the engine then writes in place."""
        if out is None:
            return torch.empty(shape, device=dev, dtype=torch.float16)
        same_dev = out.device.type == dev.type and (dev.index is None or out.device.index == dev.index)
        if tuple(out.shape) != tuple(shape) or out.dtype != torch.float16 or not same_dev or not out.is_contiguous():
            raise ValueError(f"out= must be a contiguous fp16 tensor of shape {tuple(shape)} on {dev}")
        return out

    def forward_cfg(self, latents, timestep, encoder_hidden_states, added_cond_kwargs=None, in_scale: float = 1.0,
                    share: bool = True, out=None, num_frames=None):
        """One classifier-free-guidance forward from the UN-duplicated latents [B, C, H, W]: what
        self(torch.cat([fp16(latents * in_scale)] * 2), timestep, encoder_hidden_states) returns ([2B, ...], negative
        half first; encoder_hidden_states and added_cond_kwargs hold 2B rows).  With `share` the engine runs everything
        in front of the first cross-attention once per latent where the topology allows (sd_unet_forward_cfg);
        otherwise it duplicates itself and the result is bitwise the two-step one.  Not for an attached ControlNet."""
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        if self._cn is not None:
            raise ValueError("forward_cfg takes no ControlNet: duplicate the latents and call the model")
        dev, latents, ehs, t, pt, pi, _keep = self._prepare(latents, timestep, encoder_hidden_states, added_cond_kwargs, 2)
        B, _, H, W = latents.shape
        img = self._image_embeds(added_cond_kwargs, 2 * B, dev)
        out = self._out_buffer(out, (2 * B, self.cfg.out_channels, H, W), dev)
        head = (self._h, C.c_void_p(latents.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(ehs.data_ptr()), ehs.shape[1],
                pt, pi, C.c_void_p(img.data_ptr()) if img is not None else None, img.shape[1] if img is not None else 0,
                float(in_scale), int(bool(share)))
        tail = (C.c_void_p(out.data_ptr()), B, H, W, C.c_void_p(_stream_ptr()))
        with torch.cuda.device(dev):
            if num_frames:      # the B latents are B / num_frames videos (attach_motion_adapter)
                rc = self._lib.sd_unet_forward_cfg_ex(*head, int(num_frames), *tail)
            else:
                rc = self._lib.sd_unet_forward_cfg(*head, *tail)
        _lib.check(rc, "sd_unet_forward_cfg")
        return (out,)

    def forward_pag(self, latents, timestep, encoder_hidden_states, added_cond_kwargs=None, in_scale: float = 1.0,
                    cfg: bool = True, share: bool = True):
        """One perturbed-attention-guidance forward from the UN-duplicated latents [B, C, H, W]: the model output of
        [uncond ; text ; perturbed] (`cfg`) or [text ; perturbed], [(G + 1) B, ...] with G = 2 or 1.
        encoder_hidden_states and added_cond_kwargs hold the G B rows of the un-perturbed groups; the perturbed group
        takes the text group's, and in the transformers of `set_pag_layers` its self-attention map is the identity.
        With `share` the engine creates the perturbed group only where it starts to differ (sd_unet_forward_pag).
        Not with a ControlNet, an IP-Adapter at a non-zero scale, DeepCache store / reuse, graph replay or a
        guidance-embedded UNet (EngineError, SD_ERR_UNSUPPORTED)."""
        G = 2 if cfg else 1
        dev, latents, ehs, t, pt, pi, _keep = self._prepare(latents, timestep, encoder_hidden_states, added_cond_kwargs, G)
        B, _, H, W = latents.shape
        out = torch.empty(((G + 1) * B, self.cfg.out_channels, H, W), device=dev, dtype=torch.float16)
        with torch.cuda.device(dev):
            rc = self._lib.sd_unet_forward_pag(self._h, C.c_void_p(latents.data_ptr()), C.c_void_p(t.data_ptr()),
                                               C.c_void_p(ehs.data_ptr()), ehs.shape[1], pt, pi, float(in_scale),
                                               int(bool(cfg)), int(bool(share)), C.c_void_p(out.data_ptr()), B, H, W,
                                               C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_unet_forward_pag")
        return (out,)

    def forward_concat(self, latents, timestep, encoder_hidden_states, image_latents, zero_from: Optional[int] = None,
                       added_cond_kwargs=None, in_scale: float = 1.0):
        """One forward of a UNet whose sample is [latents | image latents] (InstructPix2Pix) from the un-concatenated,
        UN-duplicated inputs: latents [B_lat, 4, H, W], image_latents [rows, in_channels - 4, H, W] and
        encoder_hidden_states [B, ...] with B a multiple of B_lat.  Image n of the B reads fp16(latents[n % B_lat] *
        in_scale) and image_latents[n % rows], or zeros from image `zero_from` on (default B: none); the timesteps (a
        scalar or B_lat values) repeat per group.  What self(torch.cat([...], dim=1), ...) returns on that sample, without
        the sample ever being built where the engine's two-source conv_in takes the shape (sd_unet_forward_concat).
        Not with a ControlNet, an IP-Adapter at a non-zero scale, DeepCache store / reuse, graph replay, a
        guidance-embedded UNet or a text_time UNet, whose added conditions differ per group (EngineError,
        SD_ERR_UNSUPPORTED)."""
        ehs_rows = encoder_hidden_states.shape[0]
        B_lat = latents.shape[0]
        if B_lat < 1 or ehs_rows % B_lat != 0:
            raise ValueError(f"encoder_hidden_states batch {ehs_rows} is no multiple of the latents batch {B_lat}")
        dev, latents, ehs, t, pt, pi, _keep = self._prepare(latents, timestep, encoder_hidden_states, added_cond_kwargs,
                                                            ehs_rows // B_lat)
        B, (_, Cl, H, W) = ehs_rows, latents.shape
        extra = _as_f16(image_latents, dev)
        if extra.ndim != 4 or tuple(extra.shape[2:]) != (H, W) or extra.shape[0] < 1:
            raise ValueError(f"image_latents: expected [rows, C, {H}, {W}], got {tuple(extra.shape)}")
        if Cl + extra.shape[1] != self.cfg.in_channels:
            raise ValueError(f"latents ({Cl}) + image_latents ({extra.shape[1]}) channels != in_channels {self.cfg.in_channels}")
        zero_from = B if zero_from is None else int(zero_from)
        out = torch.empty((B, self.cfg.out_channels, H, W), device=dev, dtype=torch.float16)
        with torch.cuda.device(dev):
            rc = self._lib.sd_unet_forward_concat(self._h, C.c_void_p(latents.data_ptr()), B_lat, float(in_scale),
                                                  C.c_void_p(extra.data_ptr()), extra.shape[1], extra.shape[0], zero_from,
                                                  C.c_void_p(t.data_ptr()), C.c_void_p(ehs.data_ptr()), ehs.shape[1], pt, pi,
                                                  C.c_void_p(out.data_ptr()), B, H, W, C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_unet_forward_concat")
        return (out,)

    # LoRA adapters arrive fused into the weights (stablediffusion_amd.weights.fuse_lora); the
    # reference's runtime adapter switches (stable_diffusion.py:252-335) are not part of the engine.
    def set_adapters(self, *a, **k):
        raise NotImplementedError("fuse LoRA weights on load (stablediffusion_amd.weights.fuse_lora)")

    delete_adapters = add_adapter = set_adapters

    def parameters(self):
        return iter(())

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.sd_unet_destroy(self._h)
                self._h = None
        except Exception:
            pass


class HipIPAdapter:
    """IP-Adapter image projection + per-site to_k_ip / to_v_ip on the engine, bound to a UNet configuration
    (sd_ip_adapter_*).  Weights in diffusers' post-load naming (stablediffusion_amd.ip_adapter.convert).
    resampler: an ip_adapter.resampler_config() for an IP-Adapter Plus projection (kind "resampler": image_embeds are
    then [B, n_img, feature_tokens, image_embed_dim]); None for the base adapters' linear + LayerNorm (kind "linear")."""

    def __init__(self, unet: HipUNet2DConditionModel, image_embed_dim: int, num_tokens: int = 4, resampler=None):
        self._lib = _lib.load()
        self.cfg = unet.cfg
        self.device = unet.device
        self.image_embed_dim = int(image_embed_dim)
        self.num_tokens = int(num_tokens)
        self.kind = "linear" if resampler is None else "resampler"
        self.resampler = dict(resampler) if resampler is not None else None
        self._feature_tokens = 257 if resampler is not None else 1
        self._unet = None
        self._h = C.c_void_p()
        pc = _lib.SdIPProjectionConfig(kind=_lib.SD_IP_PROJ_LINEAR, image_embed_dim=self.image_embed_dim,
                                       num_tokens=self.num_tokens)
        if resampler is not None:
            pc.kind = _lib.SD_IP_PROJ_RESAMPLER
            pc.dim, pc.heads, pc.depth, pc.ff_mult = (int(resampler[k]) for k in ("dim", "heads", "depth", "ff_mult"))
        _lib.check(self._lib.sd_ip_adapter_create_ex(unet._h, C.byref(pc), C.byref(self._h)), "sd_ip_adapter_create_ex")
        self._finalized = False

    @property
    def feature_tokens(self) -> int:
        """Rows of one image's features the Resampler reads (hidden_states[-2] of the tower: patches + class token)."""
        return self._feature_tokens

    @feature_tokens.setter
    def feature_tokens(self, n: int):
        _lib.check(self._lib.sd_ip_adapter_set_feature_tokens(self._h, int(n)), "sd_ip_adapter_set_feature_tokens")
        self._feature_tokens = int(n)

    def project(self, image_embeds: torch.Tensor) -> torch.Tensor:
        """The image projection alone: embeds as the UNet takes them, [rows, (T_feat,) D] -> tokens [rows, n_tok, ctx]."""
        _lib.require_gpu()
        x = _as_f16(image_embeds, self.device)
        rows = x.shape[0]
        out = torch.empty(rows, self.num_tokens, self.cfg.cross_attention_dim, dtype=torch.float16, device=x.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.sd_ip_adapter_project(self._h, C.c_void_p(x.data_ptr()), rows, C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(_stream_ptr())), "sd_ip_adapter_project")
        return out

    def memory(self):
        w, s = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_ip_adapter_memory(self._h, C.byref(w), C.byref(s)), "sd_ip_adapter_memory")
        return w.value, s.value

    def _poison_workspace(self, pattern: int = 0) -> int:
        """Test facility: overwrite the scratch memory of `project` (see `_poison`); returns the bytes filled."""
        return _poison(self, "ip_adapter", pattern)

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_gpu()
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "ip_adapter", state_dict, strict)
            _lib.check(self._lib.sd_ip_adapter_finalize(self._h), "sd_ip_adapter_finalize")
        self._finalized = True
        return self

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                u = self._unet() if self._unet is not None else None
                if u is not None:
                    u._ip = None
                self._lib.sd_ip_adapter_destroy(self._h)     # (detaches it first)
                self._h = None
        except Exception:
            pass


class HipMotionAdapter:
    """diffusers MotionAdapter (AnimateDiff) on the engine, built for a UNet's topology (sd_motion_*): attach it with
    HipUNet2DConditionModel.attach_motion_adapter and pass num_frames= to the UNet's calls.  Weights in diffusers naming
    without the stored position tables (stablediffusion_amd.motion.load converts and checks both file layouts)."""

    def __init__(self, unet: HipUNet2DConditionModel, config):
        self._lib = _lib.load()
        self.cfg = config
        self.device = unet.device
        self._unet = None
        config.check(unet.cfg)
        nb = len(config.block_out_channels)
        c = _lib.SdMotionConfig(num_blocks=nb, layers_per_block=config.motion_layers_per_block,
                                max_seq_length=config.motion_max_seq_length, use_mid_block=int(config.use_motion_mid_block))
        for i in range(nb):
            c.block_out_channels[i] = config.block_out_channels[i]
            c.num_heads[i] = config.motion_num_attention_heads[i]
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_motion_create(unet._h, C.byref(c), C.byref(self._h)), "sd_motion_create")
        self._finalized = False

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_gpu()
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "motion", state_dict, strict)
            _lib.check(self._lib.sd_motion_finalize(self._h), "sd_motion_finalize")
        self._finalized = True
        return self

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                u = self._unet() if self._unet is not None else None
                if u is not None:
                    u._motion = None
                self._lib.sd_motion_destroy(self._h)     # (detaches it first)
                self._h = None
        except Exception:
            pass


class HipControlNetModel:
    """diffusers ControlNetModel on the engine, bound to a UNet (sd_controlnet_*): attach it with
    HipUNet2DConditionModel.attach_controlnet; the UNet's forward then runs it.  Weights in diffusers naming
    (stablediffusion_amd.controlnet converts original files)."""

    def __init__(self, unet: HipUNet2DConditionModel, cn_config: UNetConfig, conditioning_channels: int = 3):
        self._lib = _lib.load()
        self.cfg = cn_config
        self.device = unet.device
        self._unet = None
        c = _unet_config_struct(cn_config)
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_controlnet_create(unet._h, C.byref(c), int(conditioning_channels), C.byref(self._h)),
                   "sd_controlnet_create")
        self._finalized = False

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_gpu()
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "controlnet", state_dict, strict)
            _lib.check(self._lib.sd_controlnet_finalize(self._h), "sd_controlnet_finalize")
        self._finalized = True
        return self

    def cond_embedding(self, image: torch.Tensor) -> torch.Tensor:
        """controlnet_cond_embedding(image): [n, 3, 8h, 8w] -> [n, C0, h, w] (fp16)."""
        x = _as_f16(image, self.device)
        n, _, H8, W8 = x.shape
        if H8 % 8 or W8 % 8:
            raise ValueError("control image height and width must be multiples of 8")
        c0 = self.cfg.block_out_channels[0]
        out = torch.empty((n, H8 // 8, W8 // 8, c0), device=self.device, dtype=torch.float16)
        with torch.cuda.device(self.device):
            rc = self._lib.sd_op_controlnet_cond_embed(self._h, C.c_void_p(x.data_ptr()), n, H8 // 8, W8 // 8,
                                                       C.c_void_p(out.data_ptr()), 0, None, C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_op_controlnet_cond_embed")
        return out.permute(0, 3, 1, 2)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                u = self._unet() if self._unet is not None else None
                if u is not None:
                    u._forget_controlnet(self)
                self._lib.sd_controlnet_destroy(self._h)     # (detaches it first)
                self._h = None
        except Exception:
            pass


class _LatentDist:
    """DiagonalGaussianDistribution surface used at sd_unified_pipeline.py:98-106 (host-side sampling)."""

    def __init__(self, moments: torch.Tensor):
        self.mean, logvar = moments.float().chunk(2, dim=1)
        self.logvar = logvar.clamp(-30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return (self.mean + self.std * noise).to(torch.float16)

    def mode(self):
        return self.mean.to(torch.float16)


class HipAutoencoderKL:
    """gfx950 engine behind the `AutoencoderKL` call surface the reference uses."""

    def __init__(self, config: VAEConfig, device: str = "cuda"):
        self._lib = _lib.load()
        self.cfg = config
        self.device = torch.device(device)
        self.dtype = torch.float16
        c = _lib.SdVAEConfig()
        c.in_channels = config.in_channels
        c.out_channels = config.out_channels
        c.latent_channels = config.latent_channels
        c.num_blocks = len(config.block_out_channels)
        for i, ch in enumerate(config.block_out_channels):
            c.block_out_channels[i] = ch
        c.layers_per_block = config.layers_per_block
        c.norm_num_groups = config.norm_num_groups
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_vae_create(C.byref(c), C.byref(self._h)), "sd_vae_create")
        self.config = _Config(**config.to_dict())
        self._finalized = False
        self._enc_shift = 0           # sd_vae_encode_range_shift in effect (force_upcast VAEs: raised on overflow)
        # diffusers' AutoencoderKL tiling state (autoencoder_kl.py __init__; semantics recalled: DESIGN.md section 8)
        self.use_tiling = False
        self.use_slicing = False
        self.tile_sample_min_size = config.sample_size
        self.tile_latent_min_size = int(config.sample_size / (2 ** (len(config.block_out_channels) - 1)))
        self.tile_overlap_factor = 0.25
        self.tile_batch = 4           # images per stacked tile chunk: the batch the benchmark's decode is measured at

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        _lib.require_gpu()
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "vae", state_dict, strict)
            _lib.check(self._lib.sd_vae_finalize(self._h), "sd_vae_finalize")
        self._finalized = True
        return self

    def memory(self):
        w, s = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_vae_memory(self._h, C.byref(w), C.byref(s)), "sd_vae_memory")
        return w.value, s.value

    def _poison_workspace(self, pattern: int = 0) -> int:
        """Test facility: overwrite the engine's scratch memory (see `_poison`); returns the bytes filled."""
        return _poison(self, "vae", pattern)

    def to(self, device=None, dtype=None):
        # the reference flips the VAE to fp32 around encode when force_upcast is set
        # (sd_unified_pipeline.py:1020-1036); the engine keeps fp32 accumulators and statistics and fp16
        # activations, so dtype requests are accepted and ignored; a force_upcast VAE whose activations leave
        # fp16's range is re-run range-shifted by encode_moments (see there).
        if device is not None and not isinstance(device, torch.dtype) and torch.device(device).type != "cuda":
            raise _lib.EngineError("HipAutoencoderKL lives on the HIP device only")
        return self

    def eval(self):
        return self

    # -- diffusers' AutoencoderKL switches (enable_tiling / enable_slicing and the three tile attributes, all writable)
    def enable_tiling(self, use_tiling: bool = True):
        """Decode / encode canvases larger than one tile as overlapping tiles (diffusers' tiled_decode / tiled_encode;
        sd_vae_decode_tiled / sd_vae_encode_tiled): the workspace stops growing with the canvas."""
        self.use_tiling = bool(use_tiling)

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        """Decode / encode one image of the batch at a time and concatenate."""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def memory_tiled(self):
        """(weight bytes, arena bytes, bytes of the tiled calls' chunk-input and tile-stack buffers)."""
        w, s, t = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_vae_memory_tiled(self._h, C.byref(w), C.byref(s), C.byref(t)), "sd_vae_memory_tiled")
        return w.value, s.value, t.value

    def _call(self, name: str, src: torch.Tensor, dst: torch.Tensor, *args):
        """One engine entry `name(handle, src, dst, *args, stream)` on this model's device."""
        with torch.cuda.device(self.device):
            rc = getattr(self._lib, name)(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), *args,
                                          C.c_void_p(_stream_ptr()))
        _lib.check(rc, name)

    def _tile_args(self):
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        tl, ts = int(self.tile_latent_min_size), int(self.tile_sample_min_size)
        if ts != tl * f:
            raise _lib.EngineError(f"tile_sample_min_size ({ts}) must be tile_latent_min_size ({tl}) times the VAE's scale ({f})")
        return tl, float(self.tile_overlap_factor), int(self.tile_batch)

    def _run(self, kind: str, src: torch.Tensor, dst: torch.Tensor):
        """decode / encode `src` into `dst`, routed as diffusers routes: sliced per image when slicing is on and the batch
        holds more than one, tiled when tiling is on and the canvas exceeds one tile in either direction."""
        if self.use_slicing and src.shape[0] > 1:
            for i in range(src.shape[0]):
                self._run_one(kind, src[i:i + 1], dst[i:i + 1])
        else:
            self._run_one(kind, src, dst)

    def _run_one(self, kind: str, src: torch.Tensor, dst: torch.Tensor):
        B, _, h, w = src.shape
        tile = self.tile_latent_min_size if kind == "decode" else self.tile_sample_min_size
        if self.use_tiling and (h > tile or w > tile):
            self._call(f"sd_vae_{kind}_tiled", src, dst, B, h, w, *self._tile_args())
        else:
            self._call(f"sd_vae_{kind}", src, dst, B, h, w)

    def decode(self, z, return_dict=False, **unused):
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        z = _as_f16(z, self.device)
        B, _, h, w = z.shape
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        img = torch.empty((B, self.cfg.out_channels, h * f, w * f), device=self.device, dtype=torch.float16)
        self._run("decode", z, img)
        if return_dict:
            return SimpleNamespace(sample=img)
        return (img,)

    def encode_moments(self, x):
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        x = _as_f16(x, self.device)
        B, _, H, W = x.shape
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        mom = torch.empty((B, 2 * self.cfg.latent_channels, H // f, W // f), device=self.device,
                          dtype=torch.float16)
        self._run("encode", x, mom)
        if getattr(self.cfg, "force_upcast", False) and not bool(torch.isfinite(mom).all()):
            # The reference runs the VAE in fp32 around encode when force_upcast is set (sd_unified_pipeline.py:1020-1036:
            # the SDXL VAE's activations leave fp16's range on some images).  The engine's equivalent: the same encoder
            # with every inter-layer activation stored 2^-k times smaller (GroupNorm is scale-invariant, eps scaled
            # along: sd_vae_encode_range_shift), k raised until the moments are finite and kept for the handle's next
            # calls.  fp32 accumulators and statistics as always; nothing overflows silently.  A sliced or tiled encode
            # is re-run whole -- every image, every tile -- at the raised shift.
            for shift in (4, 8, 12):
                if shift <= self._enc_shift:
                    continue
                _lib.check(self._lib.sd_vae_encode_range_shift(self._h, shift), "sd_vae_encode_range_shift")
                self._enc_shift = shift
                self._run("encode", x, mom)
                if bool(torch.isfinite(mom).all()):
                    break
            else:
                raise _lib.EngineError("VAE encode left fp16's range even with its activations stored 2^-12 times smaller "
                                       "(config.force_upcast is set); no latents were produced")
        return mom

    def encode(self, x, return_dict=True):
        return SimpleNamespace(latent_dist=_LatentDist(self.encode_moments(x)))

    def _tapped(self, fn, x, first: str, last: str):
        _lib.check(self._lib.sd_vae_tap(self._h, 1), "sd_vae_tap")
        try:
            out = fn(x)
            taps = _read_taps(self._lib, self._h, "vae")
        finally:
            _lib.check(self._lib.sd_vae_tap(self._h, 0), "sd_vae_tap")
        taps[first]["in"] = x.detach().to("cpu", torch.float16)
        taps[last]["out"] = out.cpu()
        return out, taps

    def decode_tapped(self, z):
        """decode(z) with the engine's debug taps on: (img, taps), `taps` as _read_taps returns them."""
        return self._tapped(lambda t: self.decode(t)[0], z, "decoder.conv_in", "decoder.tail")

    def encode_tapped(self, x):
        """One sd_vae_encode at the range shift in effect, with the debug taps on: (moments, taps)."""
        return self._tapped(self.encode_moments, x, "encoder.conv_in", "encoder.tail")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.sd_vae_destroy(self._h)
                self._h = None
        except Exception:
            pass


class _ClipOutput(tuple):
    """Indexable like transformers' ModelOutput (positional order of the non-None fields) with the
    same attribute names: encode_prompt uses `out[0]`, `out[-1][-(k+1)]` and `out.hidden_states[-2]`
    (/root/reference/pipelines/sd_unified_pipeline.py:596-608)."""

    def __new__(cls, names, values):
        o = super().__new__(cls, values)
        o._names = tuple(names)
        return o

    def __getattr__(self, name):
        names = object.__getattribute__(self, "_names")
        if name in names:
            return self[names.index(name)]
        if name in ("last_hidden_state", "pooler_output", "text_embeds", "hidden_states", "attentions"):
            return None
        raise AttributeError(name)

    def keys(self):
        return list(self._names)


class HipCLIPTextModel:
    """gfx950 engine behind the call surface the reference uses on `SDModelWrapper.text_encoder` /
    `.text_encoder_2` (transformers CLIPTextModel / CLIPTextModelWithProjection): `__call__(input_ids,
    output_hidden_states=True)`, `.text_model.final_layer_norm`, `.config`, `.dtype`, `.to`.
    `projection_dim > 0` in the config selects the WithProjection flavour (`out[0]` = text_embeds)."""

    def __init__(self, config, device: str = "cuda"):
        from .config import CLIPTextConfig
        if not isinstance(config, CLIPTextConfig):
            raise TypeError("config must be a stablediffusion_amd.config.CLIPTextConfig (see CLIPTextConfig.from_hf)")
        acts = {"quick_gelu": 0, "gelu": 1}
        if config.hidden_act not in acts:
            raise _lib.EngineError(f"unsupported CLIP activation {config.hidden_act!r}")
        self._lib = _lib.load()
        self.cfg = config
        self.device = torch.device(device)
        self.dtype = torch.float16
        c = _lib.SdClipConfig()
        c.vocab_size = config.vocab_size
        c.hidden_size = config.hidden_size
        c.intermediate_size = config.intermediate_size
        c.num_layers = config.num_hidden_layers
        c.num_heads = config.num_attention_heads
        c.max_positions = config.max_position_embeddings
        c.hidden_act = acts[config.hidden_act]
        c.projection_dim = config.projection_dim
        c.layer_norm_eps = config.layer_norm_eps
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_clip_create(C.byref(c), C.byref(self._h)), "sd_clip_create")
        self.config = _Config(**config.to_dict())
        self._finalized = False
        self.text_model = SimpleNamespace(final_layer_norm=self._final_layer_norm)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.sd_clip_destroy(self._h)
        except Exception:
            pass

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """transformers state-dict keys; the `text_model.` prefix is optional (transformers >= 5 drops it
        for CLIPTextModel), buffers such as `position_ids` are ignored."""
        _lib.require_gpu()
        sd = {}
        for k, v in state_dict.items():
            if k.endswith("position_ids"):
                continue
            if not k.startswith("text_model.") and not k.startswith("text_projection."):
                k = "text_model." + k
            if k.startswith("text_projection.") and self.cfg.projection_dim == 0:
                continue
            sd[k] = v
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "clip", sd, strict)
            _lib.check(self._lib.sd_clip_finalize(self._h), "sd_clip_finalize")
        self._finalized = True
        return self

    def memory(self):
        w, s = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_clip_memory(self._h, C.byref(w), C.byref(s)), "sd_clip_memory")
        return w.value, s.value

    def _poison_workspace(self, pattern: int = 0) -> int:
        """Test facility: overwrite the engine's scratch memory (see `_poison`); returns the bytes filled."""
        return _poison(self, "clip", pattern)

    def to(self, device=None, dtype=None):
        if device is not None and not isinstance(device, torch.dtype) and torch.device(device).type != "cuda":
            raise _lib.EngineError("HipCLIPTextModel lives on the HIP device only")
        return self

    def eval(self):
        return self

    def _final_layer_norm(self, x: torch.Tensor) -> torch.Tensor:
        x = _as_f16(x, self.device)
        y = torch.empty_like(x)
        rows = x.numel() // self.cfg.hidden_size
        with torch.cuda.device(self.device):
            rc = self._lib.sd_clip_final_layer_norm(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), rows,
                                                    C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_clip_final_layer_norm")
        return y

    def _eos_index(self, ids: torch.Tensor) -> torch.Tensor:
        # transformers modeling_clip: legacy configs (eos_token_id == 2) pool at ids.argmax, newer ones
        # at the first eos_token_id
        if self.cfg.eos_token_id == 2:
            return ids.argmax(dim=-1).to(torch.int32)
        return (ids == self.cfg.eos_token_id).int().argmax(dim=-1).to(torch.int32)

    def __call__(self, input_ids, attention_mask=None, position_ids=None, output_attentions=None,
                 output_hidden_states=None, return_dict=True, **unused):
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        if attention_mask is not None or position_ids is not None or output_attentions:
            raise NotImplementedError("HipCLIPTextModel: attention_mask / position_ids / output_attentions are not "
                                      "used by the reference's encode_prompt and not supported")
        ids = input_ids.to(self.device)
        B, T = ids.shape
        H, L, P = self.cfg.hidden_size, self.cfg.num_hidden_layers, self.cfg.projection_dim
        ids32 = ids.to(torch.int32).contiguous()
        eos = self._eos_index(ids).contiguous()
        f16 = dict(device=self.device, dtype=torch.float16)
        hs = torch.empty((L + 1, B, T, H), **f16) if output_hidden_states else None
        last = torch.empty((B, T, H), **f16)
        pooled = torch.empty((B, H), **f16)
        emb = torch.empty((B, P), **f16) if P > 0 else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            rc = self._lib.sd_clip_forward(self._h, ptr(ids32), ptr(eos), ptr(hs), ptr(last), ptr(pooled), ptr(emb), B, T,
                                           C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_clip_forward")
        names, vals = [], []
        if P > 0:       # CLIPTextModelOutput: text_embeds, last_hidden_state, hidden_states
            names += ["text_embeds", "last_hidden_state"]; vals += [emb, last]
        else:           # BaseModelOutputWithPooling: last_hidden_state, pooler_output, hidden_states
            names += ["last_hidden_state", "pooler_output"]; vals += [last, pooled]
        if hs is not None:
            names.append("hidden_states"); vals.append(tuple(hs[i] for i in range(L + 1)))
        return _ClipOutput(names, vals)


class HipCLIPVisionModelWithProjection:
    """gfx950 engine behind the call surface `encode_image` uses on `SDModelWrapper.image_encoder` (transformers
    CLIPVisionModelWithProjection): `__call__(pixel_values, output_hidden_states=False)` -> `.image_embeds`,
    `.last_hidden_state` (no final norm), `.pooler_output`, `.hidden_states`; `.config`, `.dtype`, `.device`,
    `.parameters()`.  `interpolate_pos_encoding` and attention masks are not supported."""

    def __init__(self, config, device: str = "cuda"):
        from .config import CLIPVisionConfig
        if not isinstance(config, CLIPVisionConfig):
            raise TypeError("config must be a stablediffusion_amd.config.CLIPVisionConfig (see CLIPVisionConfig.from_dict)")
        acts = {"quick_gelu": 0, "gelu": 1}
        if config.hidden_act not in acts:
            raise _lib.EngineError(f"unsupported CLIP activation {config.hidden_act!r}")
        if config.num_channels != 3:
            raise _lib.EngineError("the CLIP vision tower reads 3-channel images")
        self._lib = _lib.load()
        self.cfg = config
        self.device = torch.device(device)
        self.dtype = torch.float16
        c = _lib.SdClipVisionConfig()
        c.hidden_size = config.hidden_size
        c.intermediate_size = config.intermediate_size
        c.num_layers = config.num_hidden_layers
        c.num_heads = config.num_attention_heads
        c.image_size = config.image_size
        c.patch_size = config.patch_size
        c.hidden_act = acts[config.hidden_act]
        c.projection_dim = config.projection_dim
        c.layer_norm_eps = config.layer_norm_eps
        self._h = C.c_void_p()
        _lib.check(self._lib.sd_clip_vision_create(C.byref(c), C.byref(self._h)), "sd_clip_vision_create")
        self.config = _Config(**config.to_dict())
        self._finalized = False

    @classmethod
    def from_state_dict(cls, config, state_dict: Dict[str, torch.Tensor], device: str = "cuda"):
        return cls(config, device=device).load_state_dict(state_dict)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.sd_clip_vision_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """transformers state-dict keys (`vision_model.*`, `visual_projection.weight`); `position_ids` buffers are
        ignored, and so is the text half of a full CLIPModel checkpoint."""
        _lib.require_gpu()
        sd = {k: v for k, v in state_dict.items()
              if not k.endswith("position_ids") and (k.startswith("vision_model.") or k.startswith("visual_projection."))}
        with torch.cuda.device(self.device):
            _load_weights(self._lib, self._h, "clip_vision", sd, strict)
            _lib.check(self._lib.sd_clip_vision_finalize(self._h), "sd_clip_vision_finalize")
        self._finalized = True
        return self

    def memory(self):
        w, s = C.c_int64(), C.c_int64()
        _lib.check(self._lib.sd_clip_vision_memory(self._h, C.byref(w), C.byref(s)), "sd_clip_vision_memory")
        return w.value, s.value

    def _poison_workspace(self, pattern: int = 0) -> int:
        """Test facility: overwrite the engine's scratch memory (see `_poison`); returns the bytes filled."""
        return _poison(self, "clip_vision", pattern)

    def to(self, device=None, dtype=None):
        if device is not None and not isinstance(device, torch.dtype) and torch.device(device).type != "cuda":
            raise _lib.EngineError("HipCLIPVisionModelWithProjection lives on the HIP device only")
        return self

    def eval(self):
        return self

    def parameters(self):
        # encode_image reads the first parameter for where and in which dtype the encoder wants its pixels
        return iter((torch.empty(0, device=self.device, dtype=self.dtype),))

    def __call__(self, pixel_values, output_attentions=None, output_hidden_states=None, return_dict=True,
                 interpolate_pos_encoding: bool = False, **unused):
        if not self._finalized:
            raise _lib.EngineError("weights not loaded")
        if output_attentions or interpolate_pos_encoding:
            raise NotImplementedError("HipCLIPVisionModelWithProjection: output_attentions / interpolate_pos_encoding "
                                      "are not supported")
        S, H, L, P = self.cfg.image_size, self.cfg.hidden_size, self.cfg.num_hidden_layers, self.cfg.projection_dim
        if pixel_values.ndim != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B, 3, {S}, {S}], got {tuple(pixel_values.shape)}")
        px = _as_f16(pixel_values, self.device)
        B = px.shape[0]
        T = 1 + (S // self.cfg.patch_size) ** 2
        f16 = dict(device=self.device, dtype=torch.float16)
        hs = torch.empty((L + 1, B, T, H), **f16) if output_hidden_states else None
        last = torch.empty((B, T, H), **f16)
        pooled = torch.empty((B, H), **f16)
        emb = torch.empty((B, P), **f16)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            rc = self._lib.sd_clip_vision_forward(self._h, ptr(px), ptr(hs), ptr(last), ptr(pooled), ptr(emb), B,
                                                  C.c_void_p(_stream_ptr()))
        _lib.check(rc, "sd_clip_vision_forward")
        # CLIPVisionModelOutput: image_embeds, last_hidden_state, hidden_states (+ pooler_output by name)
        names, vals = ["image_embeds", "last_hidden_state"], [emb, last]
        if hs is not None:
            names.append("hidden_states"); vals.append(tuple(hs[i] for i in range(L + 1)))
        out = _ClipOutput(names, vals)
        out.pooler_output = pooled
        return out
