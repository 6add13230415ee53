"""Float64 restatement of the IP-Adapter Plus Resampler for the tests (not a test module), from plain torch ops, as the
IP-Adapter repository's `Resampler` / `PerceiverAttention` / `FeedForward` are recalled (no copy of that package or of
diffusers' IPAdapterPlusImageProjection is installed to pin against):

    lat = latents per image;  x = proj_in(x)
    per layer:  xn = norm1(x); ln = norm2(lat); q = to_q(ln); k, v = to_kv(cat([xn, ln], 1)).chunk(2, -1)
                lat = to_out(softmax((q 64^-1/4)(k 64^-1/4)^T) v) + lat;  lat = W2 gelu_erf(W1 LN(lat)) + lat
    tokens = norm_out(proj_out(lat))

`resampler_modules` is a second, module-style restatement (nn.LayerNorm, nn.Linear, F.scaled_dot_product_attention in
fp32) the first is checked against, so that a slip in the hand-written one does not become the yardstick.  Also here:
synthetic weights, and the IP-aware oracle double of the UNet with the Resampler in front (CPU pipeline tests)."""
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

import ip_oracle
from oracle import unet_ref
from stablediffusion_amd import ip_adapter

PROJ = ip_adapter.PROJ
DIM_HEAD = 64


def synth_resampler_state_dict(cfg, d_emb, dim, heads, depth, n_q, ff_mult=4, seed=0):
    """Random IP-Adapter Plus weights in the engine's naming, fp16-rounded: N(0, 1 / sqrt(K)) linears, LayerNorm affines
    near 1 / 0, latents N(0, 1 / sqrt(dim)) as the module initialises them."""
    g = torch.Generator().manual_seed(seed)
    rc = dict(dim=dim, heads=heads, depth=depth, num_tokens=n_q, image_embed_dim=d_emb, ff_mult=ff_mult)
    sd = {}
    for k, shp in ip_adapter.ip_adapter_manifest(cfg, d_emb, n_q, rc).items():
        name = k[len(PROJ) + 1:] if k.startswith(PROJ) else k
        is_norm = re.fullmatch(r"norm_out\..*|layers\.\d+\.0\.norm[12]\..*|layers\.\d+\.1\.0\..*", name) is not None
        if name == "latents":
            t = torch.randn(shp, generator=g) / dim ** 0.5
        elif is_norm and name.endswith("weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif name.endswith("bias"):
            t = 0.1 * torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) / shp[-1] ** 0.5
        sd[k] = t.half().float()
    return sd


def _p(sd, name, dtype):
    return sd[f"{PROJ}.{name}"].to(dtype)


def _ln(x, sd, name, dtype):
    w, b = _p(sd, name + ".weight", dtype), _p(sd, name + ".bias", dtype)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def resampler_forward(sd, x, dtype=torch.float64):
    """x [R, T_feat, D_emb] (hidden_states[-2] of R images) -> tokens [R, n_q, ctx]."""
    rc = ip_adapter.resampler_config(sd)
    heads = rc["heads"]
    x = x.to(dtype)
    R = x.shape[0]
    lat = _p(sd, "latents", dtype).expand(R, -1, -1)
    x = x @ _p(sd, "proj_in.weight", dtype).T + _p(sd, "proj_in.bias", dtype)
    split = lambda t: t.reshape(R, t.shape[1], heads, DIM_HEAD).transpose(1, 2)  # noqa: E731
    s = DIM_HEAD ** -0.25
    for i in range(rc["depth"]):
        a = f"layers.{i}.0"
        xn, ln = _ln(x, sd, a + ".norm1", dtype), _ln(lat, sd, a + ".norm2", dtype)
        q = split(ln @ _p(sd, a + ".to_q.weight", dtype).T)
        kv = torch.cat([xn, ln], dim=1) @ _p(sd, a + ".to_kv.weight", dtype).T
        k, v = (split(t) for t in kv.chunk(2, dim=-1))
        w = torch.softmax((q * s) @ (k * s).transpose(-1, -2), dim=-1)
        o = (w @ v).transpose(1, 2).reshape(R, -1, heads * DIM_HEAD)
        lat = o @ _p(sd, a + ".to_out.weight", dtype).T + lat
        f = _ln(lat, sd, f"layers.{i}.1.0", dtype) @ _p(sd, f"layers.{i}.1.1.weight", dtype).T
        f = 0.5 * f * (1.0 + torch.erf(f / 2.0 ** 0.5))
        lat = f @ _p(sd, f"layers.{i}.1.3.weight", dtype).T + lat
    out = lat @ _p(sd, "proj_out.weight", dtype).T + _p(sd, "proj_out.bias", dtype)
    return _ln(out, sd, "norm_out", dtype)


def resampler_modules(sd, x):
    """The same function from torch modules in fp32 (the cross-check of resampler_forward)."""
    rc = ip_adapter.resampler_config(sd)
    dim, heads, ctx = rc["dim"], rc["heads"], sd[f"{PROJ}.proj_out.weight"].shape[0]

    def linear(name, bias=False):
        w = _p(sd, name + ".weight", torch.float32)
        m = nn.Linear(w.shape[1], w.shape[0], bias=bias)
        m.weight.data.copy_(w)
        if bias:
            m.bias.data.copy_(_p(sd, name + ".bias", torch.float32))
        return m

    def norm(name, width):
        m = nn.LayerNorm(width, eps=1e-5)
        m.weight.data.copy_(_p(sd, name + ".weight", torch.float32))
        m.bias.data.copy_(_p(sd, name + ".bias", torch.float32))
        return m

    with torch.no_grad():
        x = linear("proj_in", True)(x.float())
        R = x.shape[0]
        lat = _p(sd, "latents", torch.float32).repeat(R, 1, 1)
        heads_of = lambda t: t.view(R, t.shape[1], heads, DIM_HEAD).permute(0, 2, 1, 3)  # noqa: E731
        for i in range(rc["depth"]):
            a = f"layers.{i}.0"
            xn, ln = norm(a + ".norm1", dim)(x), norm(a + ".norm2", dim)(lat)
            q = linear(a + ".to_q")(ln)
            k, v = linear(a + ".to_kv")(torch.cat((xn, ln), dim=-2)).chunk(2, dim=-1)
            o = F.scaled_dot_product_attention(heads_of(q), heads_of(k), heads_of(v))
            lat = linear(a + ".to_out")(o.permute(0, 2, 1, 3).reshape(R, -1, heads * DIM_HEAD)) + lat
            ff = nn.Sequential(norm(f"layers.{i}.1.0", dim), linear(f"layers.{i}.1.1"), nn.GELU(), linear(f"layers.{i}.1.3"))
            lat = ff(lat) + lat
        return norm("norm_out", ctx)(linear("proj_out", True)(lat))


def project_plus(sd, image_embeds, dtype=torch.float64):
    """[B, n_img, T_feat, D_emb] -> ip tokens [B, n_img * n_q, ctx] (fp32), the layout ip_oracle.project returns."""
    B, n_img, T, D = image_embeds.shape
    tok = resampler_forward(sd, image_embeds.reshape(B * n_img, T, D), dtype)
    return tok.reshape(B, n_img * tok.shape[1], -1).float()


def PlusOracleUNet(cfg, sd):
    """ip_oracle.IPOracleUNet whose forward runs the Resampler when the attached adapter's state dict holds one."""
    base = type(ip_oracle.IPOracleUNet(cfg, sd))

    class _Plus(base):
        calls = []

        def rebuild(self, sd):
            return _Plus(self.cfg, sd)

        def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
            a = self.ip_adapter
            if a is None or not ip_adapter.is_resampler(a["sd"]):
                return super().__call__(sample, t, ehs, cross_attention_kwargs, added_cond_kwargs, return_dict)
            self.calls.append({"added_cond_kwargs": added_cond_kwargs, "cross_attention_kwargs": cross_attention_kwargs})
            embeds = added_cond_kwargs["image_embeds"][0]
            if embeds.ndim != 4:
                raise ValueError(f"image_embeds: expected [B, n_img, T_feat, D_emb], got {tuple(embeds.shape)}")
            tok = project_plus(a["sd"], embeds.float())
            orig = unet_ref.attention
            unet_ref.attention = ip_oracle.ip_attention(a["sd"], self.ip_scale, orig)
            try:
                return (unet_ref.unet_forward(self.cfg, self.sd, sample.float(), t, (ehs.float(), tok), added_cond_kwargs),)
            finally:
                unet_ref.attention = orig

    return _Plus(cfg, sd)


# ---------------------------------------------------------------------------------- sd_op_resampler_attention
LOG2E = 1.4426950408889634
OP_T_FEAT = (1, 15, 16, 17, 31, 32, 33, 257, 304)
OP_N_Q = (1, 4, 15, 16)
OP_HEADS_B = ((1, 1), (3, 1), (1, 3), (3, 3))


def op_inputs(B, n_q, T, heads, seed, kx_scale=1.0, kl_scale=1.0):
    """q [B, n_q, A], kx / vx [B, T, A], kl / vl [B, n_q, A] in fp16 (A = heads * 64)."""
    g = torch.Generator().manual_seed(seed)
    A = heads * DIM_HEAD
    r = lambda n, s=1.0: (torch.randn(B, n, A, generator=g) * s).half()  # noqa: E731
    return r(n_q), r(T, kx_scale), r(T), r(n_q, kl_scale), r(n_q)


def op_reference(q, kx, vx, kl, vl, heads):
    """float64 SDPA over the concatenated fp16 operands: O = softmax(q k^T / 8) v and A = softmax(..) |v|."""
    B, n_q, _ = q.shape
    sp = lambda t: t.double().reshape(B, t.shape[1], heads, DIM_HEAD).transpose(1, 2)  # noqa: E731
    k, v = sp(torch.cat([kx, kl], 1)), sp(torch.cat([vx, vl], 1))
    P = torch.softmax(sp(q) @ k.transpose(-1, -2) / 8.0, dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B, n_q, heads * DIM_HEAD)  # noqa: E731
    return back(P @ v), back(P @ v.abs())


def op_bound(O, A, Tk, vmax):
    """tests/attn_cases.elementwise_bound: fp16 probabilities, fp32 sums, fp16 store.  Here the probabilities are
    normalised in fp32 and rounded to nearest (2^-11 each, 2^-25 absolute in fp16's subnormal range), which is inside
    the truncation terms that bound was derived for."""
    return 2.0 ** -9 * A + 2.0 ** -10 * O.abs() + Tk * 2.0 ** -23 * vmax + 2.0 ** -24


def op_emulate(q, kx, vx, kl, vl, heads):
    """The kernel's arithmetic in torch on the CPU: fp32 scores in the log2 domain, one exact softmax over both
    segments, probabilities normalised in fp32 then rounded to fp16, fp32 PV sums, fp16 output."""
    B, n_q, _ = q.shape
    sp = lambda t: t.float().reshape(B, t.shape[1], heads, DIM_HEAD).transpose(1, 2)  # noqa: E731
    k, v = sp(torch.cat([kx, kl], 1)), sp(torch.cat([vx, vl], 1))
    c = torch.tensor(LOG2E / 8.0, dtype=torch.float32)
    S = sp(q) @ k.transpose(-1, -2)
    p = torch.exp2(S * c - S.amax(dim=-1, keepdim=True) * c)
    P = (p * (1.0 / p.sum(dim=-1, keepdim=True))).half().float()
    return (P @ v).half().transpose(1, 2).reshape(B, n_q, heads * DIM_HEAD)
