"""InstructPix2Pix (Brooks et al., "InstructPix2Pix: Learning to Follow Image Editing Instructions", 2023) -- the host
side: which UNets select the mode, the batch's row order and the combine.

Semantics as in diffusers 0.27.2 (`StableDiffusionInstructPix2PixPipeline`) and the paper's eq. 3, recalled: diffusers
is not installed here, so nothing below is pinned against it.

  * the UNet reads 8 channels: [latents | image latents], `scale_model_input` on the latent channels only;
  * the image latents are `vae.encode(image).latent_dist.mode()`, NOT multiplied by the VAE's scaling factor;
  * batch order [text ; image ; uncond]: the prompt with the image, the negative prompt with the image, the negative
    prompt with zero image latents -- prompt embeddings [prompt ; negative ; negative];
  * eps = u + g_t (t - i) + g_i (i - u), g_t = guidance_scale (default 7.5), g_i = image_guidance_scale (default 1.5);
  * the latents start as pure noise x init_noise_sigma: there is no `strength`.
"""
from __future__ import annotations

import torch

IN_CHANNELS = 8
DEFAULT_IMAGE_GUIDANCE_SCALE = 1.5
GROUPS = 3


def is_edit_unet(unet_config) -> bool:
    """An InstructPix2Pix UNet: 4 latent + 4 image-latent input channels."""
    return int(getattr(unet_config, "in_channels", 4)) == IN_CHANNELS


def embed_rows(prompt_embeds, negative_prompt_embeds):
    """[prompt ; negative ; negative]: the text rows of [text ; image ; uncond]."""
    return torch.cat([prompt_embeds, negative_prompt_embeds, negative_prompt_embeds], dim=0)


def image_rows(image_latents):
    """[image ; image ; 0]: the image-latent rows of [text ; image ; uncond]."""
    return torch.cat([image_latents, image_latents, torch.zeros_like(image_latents)], dim=0)


def combine(noise_pred, guidance_scale: float, image_guidance_scale: float):
    """The guided prediction from a model output in [text ; image ; uncond] order (any tensor library's chunk /
    arithmetic)."""
    t, i, u = noise_pred.chunk(GROUPS)
    return u + guidance_scale * (t - i) + image_guidance_scale * (i - u)
