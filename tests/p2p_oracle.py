"""float64 restatement of InstructPix2Pix's denoising loop (Brooks et al. 2023, eq. 3; diffusers 0.27.2
StableDiffusionInstructPix2PixPipeline) for the tests (not a test module).  Recalled, not pinned: diffusers is not
installed where this was written.

What is restated: the batch [text ; image ; uncond] from one set of latents, `scale_model_input` on the latent channels
only, the un-scaled image latents behind them with zeros for the uncond group, eps = u + g_t (t - i) + g_i (i - u), and
-- for the schedulers that work in sigma space (Euler) -- diffusers' round trip: every row to x0 = x - sigma eps before
the combine, and the combined x0 back to (x0 - x) / (-sigma) after it.  The three weights g_t, g_i - g_t and 1 - g_i sum
to 1, so in exact arithmetic the round trip is the identity; `combine` and `combine_sigma_space` show it numerically.
The schedulers are oracle/schedulers_ref.py's (numpy float64)."""
import torch


def combine(noise_pred, g_t, g_i):
    """eps of rows [text ; image ; uncond], float64."""
    t, i, u = noise_pred.double().chunk(3)
    return u + g_t * (t - i) + g_i * (i - u)


def combine_sigma_space(noise_pred, latents, sigma, g_t, g_i):
    """The same through diffusers' sigma-space round trip; `latents` are the UN-scaled latents of one group."""
    x = latents.double()
    x0 = torch.cat([x] * 3) - sigma * noise_pred.double()
    return (combine(x0, g_t, g_i) - x) / (-sigma)


def edit_sample(scaled_latents, image_latents, do_cfg):
    """The UNet's 8-channel sample from the already scaled latents of one group."""
    x, im = scaled_latents.double(), image_latents.double()
    if do_cfg:
        x, im = torch.cat([x] * 3), torch.cat([im, im, torch.zeros_like(im)])
    return torch.cat([x, im], dim=1)


def loop(unet, sched, noise, image_latents, prompt_embeds, negative_prompt_embeds, steps, g_t, g_i, do_cfg=True):
    """`unet(sample, t, ehs)` over `steps` steps of a schedulers_ref scheduler -> the final latents, float64.
    `noise` is the start noise (multiplied by init_noise_sigma here), `image_latents` the un-scaled mode."""
    sched.set_timesteps(steps)
    sigma_space = hasattr(sched, "sigmas")
    x = noise.double() * sched.init_noise_sigma
    ehs = prompt_embeds.double()
    if do_cfg:
        ehs = torch.cat([ehs, negative_prompt_embeds.double(), negative_prompt_embeds.double()])
    for k, t in enumerate(sched.timesteps):
        scaled = torch.from_numpy(sched.scale_model_input(x.numpy(), t))
        out = unet(edit_sample(scaled, image_latents, do_cfg), float(t), ehs).double()
        if not do_cfg:
            eps = out
        elif sigma_space:
            eps = combine_sigma_space(out, x, float(sched.sigmas[k]), g_t, g_i)
        else:
            eps = combine(out, g_t, g_i)
        x = torch.from_numpy(sched.step(eps.numpy(), t, x.numpy()))
    return x

