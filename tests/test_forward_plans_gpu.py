"""Every kind of UNet forward through ONE handle, interleaved so that the arena plans, the persistent buffers and the
caches take turns: each output must be bitwise what a fresh handle, configured the same way, returns for that call alone.

The kinds (all on config.tiny_unet(), synthetic weights): the plain forward at two shapes, forward_cfg shared and
duplicated, forward_pag with and without CFG, widened late and duplicated up front (the mid transformer flagged), a
DeepCache store / reuse pair at depth 1, a forward with an IP-Adapter attached, one with a ControlNet attached at scale
0.9 and at scale 0; the text K/V cache off in the first round, armed and re-armed in the second.  SEQUENCE holds every
kind at least twice, never next to itself except where a repeat is there to hit a cache.  A second handle
(config.tiny_refiner_unet(), five time ids) alternates a plain and a forward_pag call so that add_text / add_time_ids
travel the same way.

There is no tolerance: a call's result may not depend on what the handle ran before it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import config, controlnet, weights  # noqa: E402
from stablediffusion_amd.models import HipControlNetModel, HipIPAdapter, HipUNet2DConditionModel  # noqa: E402

pytestmark = pytest.mark.gpu

MID = "mid_block.attentions.0"
D_IMG, N_TOK, IP_SCALE = 128, 4, 0.7
T, T2, IN_SCALE = 501.0, 481.0, 0.5


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


class Handle:
    """A UNet handle with its own adapter and ControlNet (both are bound to the UNet they were created for)."""

    def __init__(self, w):
        self.net = HipUNet2DConditionModel(w["cfg"]).load_state_dict(w["unet"])
        self.net.set_pag_layers((MID,))
        self.w, self._ad, self._cn = w, None, None

    @property
    def ad(self):
        if self._ad is None:
            self._ad = HipIPAdapter(self.net, D_IMG, N_TOK).load_state_dict(self.w["ip"])
        return self._ad

    @property
    def cn(self):
        if self._cn is None:
            self._cn = HipControlNetModel(self.net, self.w["cn_cfg"]).load_state_dict(self.w["cn"])
        return self._cn


def tiny_weights():
    cfg = config.tiny_unet()
    cn_cfg = controlnet.encoder_config(cfg)
    return {"cfg": cfg, "unet": _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=21, perturb=0.1)),
            "ip": synth_ip_state_dict(cfg, D_IMG, N_TOK, seed=3), "cn_cfg": cn_cfg, "cn": synth_cn_state_dict(cn_cfg, seed=4)}


def refiner_weights():
    cfg = config.tiny_refiner_unet()
    return {"cfg": cfg, "unet": _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=22, perturb=0.1))}


def make_inputs(cfg):
    """The device tensors of every kind of call, made once: both handles read the same ones, and a pointer the text K/V
    cache has seen keeps its contents."""
    g = torch.Generator().manual_seed(7)
    dim = cfg.cross_attention_dim

    def lat(B, H, W):
        return torch.randn(B, 4, H, W, generator=g).half().cuda()

    def ehs(rows):
        return torch.randn(rows, 77, dim, generator=g).half().cuda()

    def added(rows):
        if cfg.addition_embed_type != "text_time":
            return None
        ids = torch.tensor([[128.0, 128, 0, 0, 6.0], [128.0, 128, 0, 0, 2.5]])[:rows]
        return {"text_embeds": torch.randn(rows, 64, generator=g).half().cuda(), "time_ids": ids.cuda()}

    return {
        "plain_b2": (lat(2, 16, 16), ehs(2), added(2)),
        "plain_b1_8x8": (lat(1, 8, 8), ehs(1), added(1)),
        "cfg": (lat(1, 16, 16), ehs(2), added(2)),
        "pag_cfg": (lat(1, 16, 16), ehs(2), added(2)),
        "pag_nocfg": (lat(1, 16, 16), ehs(1), added(1)),
        "dc": (lat(2, 16, 16), ehs(2), added(2), lat(2, 16, 16)),
        "ip": (lat(2, 16, 16), ehs(2), torch.randn(2, 1, D_IMG, generator=g).half().cuda()),
        "cn": (lat(2, 16, 16), ehs(2), torch.rand(1, 3, 128, 128, generator=g).half().cuda()),
    }


def run_case(h, name, inp):
    """One kind of call on the handle `h`, configured for it and put back afterwards.  Returns its output(s)."""
    net = h.net
    if name in ("plain_b2", "plain_b1_8x8"):
        x, e, add = inp[name]
        return net(x, T, e, added_cond_kwargs=add)[0]
    if name in ("cfg_share", "cfg_dup"):
        x, e, add = inp["cfg"]
        return net.forward_cfg(x, T, e, added_cond_kwargs=add, in_scale=IN_SCALE, share=name == "cfg_share")[0]
    if name.startswith("pag_"):
        _, mode, where = name.split("_")
        x, e, add = inp["pag_" + mode]
        return net.forward_pag(x, T, e, added_cond_kwargs=add, in_scale=IN_SCALE, cfg=mode == "cfg", share=where == "late")[0]
    if name == "dc_pair":                       # (leaves the depth set and the buffer in place: DC_OFF releases it)
        x, e, add, x2 = inp["dc"]
        net.enable_deepcache(cache_interval=2, cache_depth=1)
        try:
            net.deep_cache_mode(net.DC_STORE)
            a = net(x, T, e, added_cond_kwargs=add)[0]
            net.deep_cache_mode(net.DC_REUSE)
            b = net(x2, T2, e, added_cond_kwargs=add)[0]
        finally:
            net.deep_cache_mode(net.DC_PLAIN)
        return torch.cat([a, b])
    if name == "ip":
        x, e, emb = inp["ip"]
        net.attach_ip_adapter(h.ad).set_ip_adapter_scale(IP_SCALE)
        try:
            return net(x, T, e, added_cond_kwargs={"image_embeds": [emb]})[0]
        finally:
            net.attach_ip_adapter(None).set_ip_adapter_scale(1.0)
    if name in ("cn_0.9", "cn_0"):
        x, e, img = inp["cn"]
        net.attach_controlnet(h.cn)
        try:
            return net(x, T, e, controlnet_cond=img, controlnet_conditioning_scale=float(name[3:]))[0]
        finally:
            net.attach_controlnet(None)
    raise KeyError(name)


KV_ON, KV_OFF, DC_OFF = "kv_on", "kv_off", "dc_off"
SETTINGS = (KV_ON, KV_OFF, DC_OFF)
# first round: text K/V cache off; second round: armed, re-armed half way, with three repeats that hit it
SEQUENCE = [
    "plain_b2", "cfg_share", "pag_cfg_late", "plain_b1_8x8", "cn_0.9", "cfg_dup", "pag_nocfg_late", "ip", "dc_pair",
    "pag_cfg_front", "cn_0", DC_OFF, "pag_nocfg_front",
    KV_ON,
    "pag_nocfg_front", "plain_b2", "ip", "pag_cfg_late", "pag_cfg_late", "cfg_share", "cfg_share", "plain_b1_8x8", "cn_0",
    KV_ON,
    "dc_pair", "cfg_dup", "cn_0.9", "cn_0.9", "pag_nocfg_late", "pag_cfg_front", "plain_b2", "dc_pair", "ip", DC_OFF,
    KV_OFF,
    "plain_b1_8x8", "cfg_share", "pag_cfg_late", "plain_b2",
]
REFINER_SEQUENCE = ["plain_b2", "pag_cfg_late", KV_ON, "plain_b2", "pag_nocfg_front", "pag_cfg_late", KV_OFF, "pag_nocfg_front",
                    "plain_b2"]


def run_sequence(h, seq, inp):
    """[(step index, name, output)] of the calls of `seq` on the one handle `h`."""
    outs = []
    try:
        for i, name in enumerate(seq):
            if name == DC_OFF:
                h.net.disable_deepcache()
            elif name in (KV_ON, KV_OFF):
                h.net.text_kv_cache(name == KV_ON)
            else:
                outs.append((i, name, run_case(h, name, inp).clone()))
    finally:
        h.net.text_kv_cache(False)
    return outs


def _check(w, seq):
    inp = make_inputs(w["cfg"])
    kinds = [n for n in dict.fromkeys(seq) if n not in SETTINGS]
    for n in kinds:                              # every kind at least twice, not only next to itself
        at = [i for i, s in enumerate(seq) if s == n]
        assert len(at) >= 2 and at[-1] - at[0] > 1, n
    ref = {}
    for n in kinds:                              # a fresh handle per kind, one call on it
        ref[n] = run_case(Handle(w), n, inp).clone()
    assert all(torch.isfinite(r.float()).all() for r in ref.values())
    assert not torch.equal(ref["pag_cfg_late"][1:2], ref["pag_cfg_late"][2:3])      # the perturbed group is perturbed
    bad = [(i, n) for i, n, out in run_sequence(Handle(w), seq, inp) if not torch.equal(out, ref[n])]
    assert not bad, f"calls that depend on the handle's history (step, kind): {bad}"


def test_interleaved_forwards_are_bitwise_the_fresh_handle(engine_lib):
    w = tiny_weights()
    _check(w, SEQUENCE)
    inp = make_inputs(w["cfg"])
    a, b = run_case(Handle(w), "cn_0.9", inp), run_case(Handle(w), "cn_0", inp)
    assert not torch.equal(a, b)                                                    # the ControlNet runs at 0.9


def test_interleaved_text_time_forwards_are_bitwise_the_fresh_handle(engine_lib):
    _check(refiner_weights(), REFINER_SEQUENCE)
