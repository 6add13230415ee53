"""Restatement of the regional prompts' semantics for the tests (not a test module): an `attention` for
oracle.unet_ref that, given ctx = (text [N, R L, D], weights [Bw, R, h, w]) at an `.attn2`, returns

    to_out( sum_r W_l[n % Bw, :, r] * SDPA(q, K[:, rL:(r+1)L], V[:, rL:(r+1)L]) )

with W_l the 2x2 mean of the sample-resolution weights, taken once per halving down to the transformer's map.
unet_forward (and pipeline_ref.denoise_ref through it) carry the tuple through unchanged; the tests monkeypatch
oracle.unet_ref.attention with `region_attention()`, nothing under oracle/ is edited.  Also the inputs the GPU tests
run (so that the CPU suite can check, without a device, that they tell the regional forward from the plain one) and an
oracle double of the engine's UNet for the CPU pipeline tests."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import unet_ref


def level_of(weights, T):
    h, w = weights.shape[-2:]
    lvl = 0
    while (h >> lvl) * (w >> lvl) > T:
        lvl += 1
    assert (h >> lvl) * (w >> lvl) == T and (h >> lvl) << lvl == h and (w >> lvl) << lvl == w, (h, w, T)
    return lvl


def weights_at(weights, T):
    """[Bw, R, h, w] -> [Bw, R, T] for a transformer of T tokens."""
    for _ in range(level_of(weights, T)):
        weights = F.avg_pool2d(weights, 2)
    return weights.flatten(2)


def region_attention(orig=unet_ref.attention):
    def attention(x, ctx, w, p, heads, qkv_bias=False):
        if not isinstance(ctx, tuple):
            return orig(x, ctx, w, p, heads, qkv_bias)
        text, weights = ctx
        B, T, C = x.shape
        R = weights.shape[1]
        assert text.shape[1] % R == 0
        L = text.shape[1] // R
        d = C // heads
        wl = weights_at(weights.to(x.dtype), T)                                   # [Bw, R, T]
        rows = torch.arange(B) % weights.shape[0]
        split = lambda t: t.reshape(B, -1, heads, d).transpose(1, 2)  # noqa: E731
        q = split(F.linear(x, w[p + ".to_q.weight"]))
        o = torch.zeros_like(q)
        for r in range(R):
            seg = text[:, r * L:(r + 1) * L]
            k = split(F.linear(seg, w[p + ".to_k.weight"]))
            v = split(F.linear(seg, w[p + ".to_v.weight"]))
            o = o + wl[rows, r][:, None, :, None] * F.scaled_dot_product_attention(q, k, v)
        o = o.transpose(1, 2).reshape(B, T, C)
        return F.linear(o, w[p + ".to_out.0.weight"], w[p + ".to_out.0.bias"])
    return attention


@contextlib.contextmanager
def patched():
    orig = unet_ref.attention
    unet_ref.attention = region_attention(orig)
    try:
        yield
    finally:
        unet_ref.attention = orig


def forward(cfg, sd, x, t, ehs, weights, added_cond_kwargs=None):
    """The oracle's UNet forward with regions: ehs [N, R L, D], weights [Bw, R, h, w]."""
    with patched(), torch.no_grad():
        return unet_ref.unet_forward(cfg, sd, x.float(), t, (ehs.float(), weights.float()), added_cond_kwargs)


# ---------------------------------------------------------------------------- the inputs the GPU tests run
def stripe_weights(Bw, R, h, w, soft=False, seed=0):
    """[Bw, R, h, w]: vertical stripes of unequal width whose edges fall off the 2x2 grid (so the coarser levels mix
    regions), another assignment per row; `soft`: positive everywhere instead."""
    if soft:
        g = torch.Generator().manual_seed(seed)
        m = torch.rand(Bw, R, h, w, generator=g) + 0.05
        return m / m.sum(1, keepdim=True)
    cuts = [0] + [max(1, (w * r) // R - 1 + (r % 2) * 3) for r in range(1, R)] + [w]
    out = torch.zeros(Bw, R, h, w)
    for b in range(Bw):
        for r in range(R):
            out[b, (r + b) % R, :, cuts[r]:cuts[r + 1]] = 1.0
    return out


def unet_inputs(cfg, B, h, w, R, seed, L=77, scale=3.0):
    """x [B, 4, h, w], ehs [B, R L, D] fp16-rounded: R prompts of unit-variance rows times `scale` -- far enough apart
    that the regional forward is more than 5e-2 (rel-L2) away from the plain forward on the base prompt, which the CPU
    suite checks on the oracle."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg.in_channels, h, w, generator=g).half()
    ehs = (torch.randn(B, R * L, cfg.cross_attention_dim, generator=g) * scale).half()
    return x, ehs


def sdxl_cond(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    n_ids = cfg.num_time_ids
    text = torch.randn(B, cfg.projection_class_embeddings_input_dim - n_ids * cfg.addition_time_embed_dim, generator=g).half()
    ids = torch.tensor([[64.0, 64.0, 0.0, 0.0, 64.0, 64.0][:n_ids]]).repeat(B, 1)
    return {"text_embeds": text, "time_ids": ids}


# ---------------------------------------------------------------------------- a double of the engine's UNet
def RegionOracleUNet(cfg, sd):
    from doubles import OracleUNet

    class _Regions(OracleUNet):
        calls = []

        def __init__(self, cfg, sd):
            super().__init__(cfg, sd)
            self.weights = None
            self.history = []              # every set_regions / clear_regions, in order

        def rebuild(self, sd):
            return _Regions(self.cfg, sd)

        def set_regions(self, weights):
            self.weights = weights.float().clone()
            self.history.append(("set", tuple(weights.shape)))
            return self

        def clear_regions(self):
            self.weights = None
            self.history.append(("clear",))
            return self

        def __call__(self, sample, t, ehs, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
            self.calls.append({"ehs": ehs, "weights": self.weights, "added_cond_kwargs": added_cond_kwargs})
            if self.weights is None:
                return super().__call__(sample, t, ehs, cross_attention_kwargs, added_cond_kwargs, return_dict)
            return (forward(self.cfg, self.sd, sample, t, ehs, self.weights, added_cond_kwargs),)

    return _Regions(cfg, sd)
