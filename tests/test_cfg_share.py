"""Which UNet topologies let sd_unet_forward_cfg run the CFG-shared start of the forward once per latent
(sd_unet_cfg_share: a host function, no device needed)."""
import ctypes as C

import pytest

from stablediffusion_amd import config
from stablediffusion_amd.models import _unet_config_struct


def _eligible(engine_lib, cfg):
    c = _unet_config_struct(cfg)
    return engine_lib.sd_unet_cfg_share(C.byref(c))


@pytest.mark.parametrize("make", [config.sd15_unet, config.tiny_unet])
def test_sd1x_topologies_are_eligible(engine_lib, make):
    assert _eligible(engine_lib, make()) == 1


@pytest.mark.parametrize("make", [config.sdxl_unet, lambda: config.tiny_unet(sdxl_cond=True)])
def test_text_time_topologies_are_not(engine_lib, make):
    # the pooled text embedding makes the time embedding differ between the halves (and SDXL's first block has no attention)
    assert _eligible(engine_lib, make()) == 0


def test_null_config_is_not_eligible(engine_lib):
    assert engine_lib.sd_unet_cfg_share(None) == 0
