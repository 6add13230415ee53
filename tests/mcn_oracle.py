"""fp32 restatement of diffusers 0.27.2's MultiControlNetModel feeding UNet2DConditionModel, for the tests (not a test
module): every net's ControlNetModel.forward residuals (tests/cn_oracle.py), summed in net order, into the UNet."""
from cn_oracle import controlnet_forward, unet_forward_res


def multi_controlnet_residuals(nets, sample, timestep, ehs, images, scales, added_cond_kwargs=None):
    """nets: [(cfg, weights)], images / scales: one per net.  MultiControlNetModel.forward: the first net's residuals,
    every further net's added to them.  A net at scale 0 is skipped (its residuals are exact zeros)."""
    down, mid = None, None
    for (ccfg, csd), img, s in zip(nets, images, scales):
        if s == 0.0:
            continue
        d, m = controlnet_forward(ccfg, csd, sample.float(), timestep, ehs.float(), img, s, added_cond_kwargs)
        if down is None:
            down, mid = d, m
        else:
            down = [a + b for a, b in zip(down, d)]
            mid = mid + m
    return down, mid


def unet_mcn_forward(ucfg, usd, nets, sample, timestep, ehs, images, scales, added_cond_kwargs=None):
    """The pipeline's composition with a list of ControlNets."""
    down, mid = multi_controlnet_residuals(nets, sample, timestep, ehs, images, scales, added_cond_kwargs)
    return unet_forward_res(ucfg, usd, sample.float(), timestep, ehs.float(), added_cond_kwargs, down, mid)
