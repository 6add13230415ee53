"""fp32 restatement of diffusers 0.27.2's IP-Adapter for the tests (not a test module): ImageProjection in fp32, and
an `attention` for oracle.unet_ref that, given ctx = (text_states, ip_tokens) at an `.attn2`, adds
scale * SDPA(q, K_ip, V_ip) before to_out, as IPAdapterAttnProcessor2_0 does.  unet_forward (and
pipeline_ref.denoise_ref through it) carry the tuple through unchanged; the tests monkeypatch
oracle.unet_ref.attention with `ip_attention(...)`, nothing under oracle/ is edited."""
import torch
import torch.nn.functional as F

from oracle import unet_ref
from stablediffusion_amd import ip_adapter

PROJ = ip_adapter.PROJ


def synth_ip_state_dict(cfg, d_img, n_tok, seed=0):
    """Random adapter weights in diffusers naming, fp16-rounded (projection scaled like a trained linear)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in ip_adapter.ip_adapter_manifest(cfg, d_img, n_tok).items():
        if k.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) / shp[-1] ** 0.5
        sd[k] = t.half().float()
    return sd


def project(ip_sd, image_embeds, n_tok):
    """[B, n_img, D_img] -> ip tokens [B, n_img * n_tok, ctx] (fp32)."""
    B, n_img, _ = image_embeds.shape
    x = F.linear(image_embeds.float().reshape(B * n_img, -1), ip_sd[f"{PROJ}.image_embeds.weight"].float(),
                 ip_sd[f"{PROJ}.image_embeds.bias"].float())
    x = x.reshape(B * n_img, n_tok, -1)
    x = F.layer_norm(x, (x.shape[-1],), ip_sd[f"{PROJ}.norm.weight"].float(), ip_sd[f"{PROJ}.norm.bias"].float(), 1e-5)
    return x.reshape(B, n_img * n_tok, -1)


def ip_attention(ip_sd, scale, orig=unet_ref.attention):
    def attention(x, ctx, w, p, heads, qkv_bias=False):
        if not isinstance(ctx, tuple):
            return orig(x, ctx, w, p, heads, qkv_bias)
        text, tok = ctx
        B, T, C = x.shape
        d = C // heads
        split = lambda t: t.reshape(B, -1, heads, d).transpose(1, 2)  # noqa: E731
        q = split(F.linear(x, w[p + ".to_q.weight"]))
        o = F.scaled_dot_product_attention(q, split(F.linear(text, w[p + ".to_k.weight"])),
                                           split(F.linear(text, w[p + ".to_v.weight"])))
        site = p + ".processor"
        kip = split(F.linear(tok, ip_sd[site + ".to_k_ip.0.weight"].float()))
        vip = split(F.linear(tok, ip_sd[site + ".to_v_ip.0.weight"].float()))
        o = o + scale * F.scaled_dot_product_attention(q, kip, vip)
        o = o.transpose(1, 2).reshape(B, T, C)
        return F.linear(o, w[p + ".to_out.0.weight"], w[p + ".to_out.0.bias"])
    return attention


class IPOracleUNet:
    """IP-aware oracle double of HipUNet2DConditionModel for the CPU pipeline tests: make_ip_adapter /
    attach_ip_adapter / set_ip_adapter_scale as the engine's, the forward through unet_ref with ip_attention."""

    def __new__(cls, cfg, sd):
        from doubles import OracleUNet

        class _IP(OracleUNet):
            calls = []

            def __init__(self, cfg, sd):
                super().__init__(cfg, sd)
                self.ip_adapter = None
                self.ip_scale = 1.0

            def rebuild(self, sd):
                return _IP(self.cfg, sd)

            def make_ip_adapter(self, state_dict, image_embed_dim, num_tokens):
                return {"sd": state_dict, "d_img": image_embed_dim, "n_tok": num_tokens}

            def attach_ip_adapter(self, adapter):
                self.ip_adapter = adapter
                return self

            def set_ip_adapter_scale(self, scale):
                self.ip_scale = float(scale)
                return self

            def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
                self.calls.append({"added_cond_kwargs": added_cond_kwargs, "cross_attention_kwargs": cross_attention_kwargs})
                embeds = (added_cond_kwargs or {}).get("image_embeds")
                if self.ip_adapter is None:
                    assert embeds is None
                    return super().__call__(sample, t, ehs, cross_attention_kwargs, added_cond_kwargs, return_dict)
                a = self.ip_adapter
                tok = project(a["sd"], embeds[0].float(), a["n_tok"])
                orig = unet_ref.attention
                unet_ref.attention = ip_attention(a["sd"], self.ip_scale, orig)
                try:
                    return (unet_ref.unet_forward(self.cfg, self.sd, sample.float(), t, (ehs.float(), tok),
                                                  added_cond_kwargs),)
                finally:
                    unet_ref.attention = orig

        return _IP(cfg, sd)
