"""AnimateDiff text-to-video on the engine: `animate(pipe, model, prompt, ...)`.

To the pipeline a video is V F samples: the prompt encoder, the wrapper's scheduler, the un-duplicated `forward_cfg` and
the device step of every scheduler are the ones `StableDiffusionUnifiedPipeline.__call__` uses; the only difference is
that the UNet's calls name `num_frames`, so the motion adapter's modules run (HipUNet2DConditionModel
.attach_motion_adapter).  Noise is drawn as [V, 4, F, h, w] -- diffusers' AnimateDiffPipeline.prepare_latents -- and moved
to frame-major order, so a seed means what it means there.  Frames are decoded in chunks and returned as [V, F, ...].

Kept out of `__call__` on purpose: it composes with none of the pipeline's other features yet, and says so itself."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from .pipeline import retrieve_timesteps


class _FramesUNet:
    """The wrapper's UNet with `num_frames` on every forward; everything else is the UNet's own."""

    def __init__(self, unet, num_frames: int):
        self._u, self._frames = unet, int(num_frames)

    def __getattr__(self, name):
        return getattr(self._u, name)

    def __call__(self, *args, **kwargs):
        return self._u(*args, num_frames=self._frames, **kwargs)

    def forward_cfg(self, *args, **kwargs):
        return self._u.forward_cfg(*args, num_frames=self._frames, **kwargs)


def check_state(model, num_frames: int):
    """What `animate` cannot run with, refused before anything is encoded or launched.  Leaves the wrapper untouched."""
    unet = model.base
    adapter = getattr(unet, "motion_adapter", None)
    if adapter is None:
        raise ValueError("animate needs a motion adapter: SDModelWrapper.load_motion_adapter")
    if getattr(model, "type", "sd15") == "sdxl" or getattr(unet.config, "addition_embed_type", None) == "text_time":
        raise NotImplementedError("animate: SDXL bases (AnimateDiff-SDXL) are not supported")
    if unet.config.in_channels != 4:
        raise NotImplementedError("animate: the base UNet must take 4 latent channels (no inpainting / InstructPix2Pix bases)")
    if not 1 <= int(num_frames) <= adapter.cfg.motion_max_seq_length:
        raise ValueError(f"animate: num_frames must be in 1..{adapter.cfg.motion_max_seq_length} "
                         "(longer clips need sliding context windows)")
    busy = []
    if getattr(model, "has_controlnet", False):
        busy.append("a ControlNet is loaded")
    if getattr(model, "_ip", None) is not None:
        busy.append("an IP-Adapter is loaded")
    if getattr(unet, "deepcache", None) is not None:
        busy.append("DeepCache is enabled")
    if getattr(unet, "tome", None) is not None:
        busy.append("token merging is enabled")
    if getattr(unet, "hypertile", None) is not None:
        busy.append("HyperTile is enabled")
    if getattr(unet, "_graph_on", False):
        busy.append("graph replay is enabled")
    if busy:
        raise NotImplementedError("animate does not compose with: " + ", ".join(busy))


def video_noise(videos: int, channels: int, num_frames: int, h: int, w: int, seed, device, dtype) -> torch.Tensor:
    """randn [V, C, F, h, w] from `seed` on `device` (diffusers' layout), as frame-major samples [V F, C, h, w]."""
    g = None
    if seed is not None:
        g = torch.Generator(device=device).manual_seed(int(seed))
    z = torch.randn((videos, channels, num_frames, h, w), generator=g, device=device, dtype=dtype)
    return z.permute(0, 2, 1, 3, 4).reshape(videos * num_frames, channels, h, w).contiguous()


def decode_frames(model, latents: torch.Tensor, decode_chunk_size: int) -> torch.Tensor:
    """vae.decode over chunks of frames; [N, 4, h, w] scaled latents -> [N, 3, 8h, 8w]."""
    z = latents / model.vae.config.scaling_factor
    n = max(1, int(decode_chunk_size))
    return torch.cat([model.vae.decode(z[i:i + n], return_dict=False)[0] for i in range(0, z.shape[0], n)])


@torch.no_grad()
def animate(pipe, model, prompt, negative_prompt=None, num_frames: int = 16, height: Optional[int] = None,
            width: Optional[int] = None, num_inference_steps: int = 25, guidance_scale: float = 7.5, seed: Optional[int] = None,
            latents: Optional[torch.Tensor] = None, decode_chunk_size: int = 8, output_type: str = "pt",
            prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None):
    """Text-to-video.  `prompt`: a string or a list (one video each); `latents`: [V, 4, F, h, w] noise instead of the
    seed's.  Returns [V, F, 3, H, W] frames ("pt") or the [V, F, 4, h, w] latents ("latents")."""
    if output_type not in ("pt", "latents"):
        raise ValueError(f"Unknown output_type = '{output_type}'")
    check_state(model, num_frames)
    F = int(num_frames)
    saved = (pipe.model, pipe._use_refiner, pipe.is_inpaint, pipe._guidance_embedded)
    pipe.model, pipe._use_refiner, pipe.is_inpaint, pipe._guidance_embedded = model, False, False, False
    try:
        if hasattr(model, "apply_adapters"):
            model.apply_adapters()
        unet = model.base
        height = height or unet.config.sample_size * model.vae_scale_factor
        width = width or unet.config.sample_size * model.vae_scale_factor
        if prompt_embeds is None:
            prompt_embeds, negative_prompt_embeds, _, _ = pipe.encode_prompt(prompt, None, negative_prompt, None, 1, None, None)
        else:
            prompt_embeds = prompt_embeds.to(pipe.device)
            if pipe.do_classifier_free_guidance:
                if negative_prompt_embeds is None:
                    raise ValueError("negative_prompt_embeds is required with prompt_embeds when CFG is on")
                negative_prompt_embeds = negative_prompt_embeds.to(pipe.device)
        V = prompt_embeds.shape[0]
        # a video's text embedding, repeated per frame; under CFG the negative half first
        per_frame = lambda e: e.repeat_interleave(F, dim=0)
        embeds = per_frame(prompt_embeds)
        if pipe.do_classifier_free_guidance:
            embeds = torch.cat([per_frame(negative_prompt_embeds), embeds])
        timesteps, num_inference_steps = retrieve_timesteps(model.scheduler, num_inference_steps, pipe.device)
        h, w = height // model.vae_scale_factor, width // model.vae_scale_factor
        if latents is None:
            x = video_noise(V, 4, F, h, w, seed, pipe.device, prompt_embeds.dtype)
        else:
            if tuple(latents.shape) != (V, 4, F, h, w):
                raise ValueError(f"latents: expected {(V, 4, F, h, w)}, got {tuple(latents.shape)}")
            x = latents.to(pipe.device, prompt_embeds.dtype).permute(0, 2, 1, 3, 4).reshape(V * F, 4, h, w).contiguous()
        x = x * model.scheduler.init_noise_sigma
        frames_model = SimpleNamespace(base=_FramesUNet(unet, F), refiner=None, scheduler=model.scheduler, vae=model.vae,
                                       _pag=None)
        x = pipe._denoise(frames_model, x, timesteps, embeds, None, None, {}, guidance_scale, 0.0, seed)
        if output_type == "latents":
            return x.reshape(V, F, 4, h, w)
        frames = decode_frames(model, x, decode_chunk_size)
        return frames.reshape(V, F, *frames.shape[1:])
    finally:
        pipe.model, pipe._use_refiner, pipe.is_inpaint, pipe._guidance_embedded = saved
