"""No forward may depend on what an earlier call left in the handle's scratch memory, non-finite values included.

Every handle (UNet, VAE, CLIP text, CLIP vision, IP-Adapter projection) runs on a bump-allocated workspace that is never
cleared and is reused at whatever offsets the current call's plan gives.  A column that is read but never written, times
a zero-padded weight, is 0 * stale = 0 while everything the handle ran before was finite -- and NaN for the life of the
process after one call that overflowed fp16.

(a) sd_*_poison_workspace (a test facility, include/sd_engine.h) fills the workspace with NaN (bytes 0xFF) or fp16 +Inf
(words 0x7C00) over its whole capacity.  Each handle first makes a "grow" call larger than anything that follows, so the
slab is bigger than the next plan and the neighbours of every buffer are live; then, per call and per pattern: poison,
bytes filled == memory()'s workspace, run, compare.  (b) the same without the hook: a call with NaN / Inf inputs returns
0 and a non-finite output, and the clean call after it is the fresh handle's.

There is no tolerance.  The reference of a call is that one call on a fresh handle built from the same weights
(test_forward_plans_gpu.py's rule); every comparison is torch.equal, and every reference is finite, so a NaN anywhere in an
output fails it.

Scratch that holds indices or counts, where stale contents could turn a read-before-write into an out-of-range access
instead of a wrong number -- from the alloc / alloc_h / alloc_f call sites of unet.cpp, vae.cpp, clip.cpp, clip_vision.cpp,
controlnet.cpp and runtime.cpp: there is none.  Every arena allocation is an fp16 activation, an fp32 embedding row, an
fp32 statistics buffer (row (mean, M2) parts, GroupNorm summaries and their scratch) or an fp32 split-K partial; no kernel
uses a global atomic, counter or ticket.  The indices a forward reads on the device live elsewhere:
  - CLIP token ids and eos indices: the caller's tensors (launch_clip_embed clamps the ids to the table);
  - the token-merging plan (rank -> token table, unmerge map, member lists and offsets): tome_buf, a tagged buffer the
    hook leaves alone; prep / match / select rewrite all of it before merge / unmerge read it, and merge checks its header;
  - the row-duplication segments and the ControlNet residual problems: kernel arguments passed by value;
  - the staged inputs of graph replay (io_slab, poisoned): floats and halves, copied in again before every replay.
Token merging with NaN latents (b): tome_prep_kernel gives a row whose squared norm is not > 0 the reciprocal norm 0, so a
NaN / Inf row scores NaN; tome_match_kernel only takes a score that compares greater, so NaN never reaches node_max, and a
row that never won reports destination 0 at score 0; tome_select_kernel's radix select runs a fixed four rounds on the
bit patterns of node_max (any pattern is a valid key; Ns >= r keys always leave a digit to pick) and clamps node_idx to
[0, Nd): it terminates and emits in-range indices whatever the activations hold."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
import resampler_oracle as ro  # noqa: E402
from test_forward_plans_gpu import (D_IMG, IN_SCALE, N_TOK, T, Handle, make_inputs, refiner_weights, run_case,  # noqa: E402
                                    tiny_weights)
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import (HipAutoencoderKL, HipCLIPTextModel, HipCLIPVisionModelWithProjection,  # noqa: E402
                                        HipIPAdapter, HipUNet2DConditionModel)

pytestmark = pytest.mark.gpu

PATTERNS = (0, 1)                           # SD_POISON_NAN, SD_POISON_INF
RUN_CASE_KINDS = ("plain_b2", "plain_b1_8x8", "cfg_share", "cfg_dup", "pag_cfg_late", "pag_cfg_front", "pag_nocfg_late",
                  "pag_nocfg_front", "dc_pair", "ip", "cn_0.9", "cn_0")
FREEU = (0.9, 0.2, 1.2, 1.4)


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


def _finite(t):
    return bool(torch.isfinite(t.float()).all())


def _settle(net):
    """Release the two state buffers memory() counts next to the scratch ones (the DeepCache feature, the merge plans)."""
    net.disable_deepcache()
    net.disable_tome()


def _poison(model, pattern):
    """Poison, and check the hook's count against the handle's own report."""
    n = model._poison_workspace(pattern)
    assert n == model.memory()[1] and n > 0, (n, model.memory())


# ------------------------------------------------------------------------------------------------------ UNet
def run_kind(h, name, inp):
    """run_case plus the kinds merged after it was written."""
    net = h.net
    if name == "tome":
        net.enable_tome(0.5, max_downsample=1)
        try:
            out = run_case(h, "plain_b2", inp)
            assert net.tome_sites(), "no block merged: the case runs the plain forward"
            return out
        finally:
            net.disable_tome()
    if name == "freeu":
        net.enable_freeu(*FREEU)
        try:
            return run_case(h, "plain_b2", inp)
        finally:
            net.disable_freeu()
    return run_case(h, name, inp)


def _added(cfg, rows, g):
    """text_time conditioning of `rows` samples with as many time ids as the configuration reads."""
    if cfg.addition_embed_type != "text_time":
        return None
    nid = (cfg.projection_class_embeddings_input_dim - 64) // cfg.addition_time_embed_dim
    base = torch.tensor([128.0, 96.0, 0.0, 8.0, 6.0, 2.5, 112.0, 64.0])
    ids = torch.stack([base[:nid] + 3.0 * r for r in range(rows)])
    return {"text_embeds": torch.randn(rows, 64, generator=g).half().cuda(), "time_ids": ids.cuda()}


def _inputs(cfg):
    """make_inputs, with the time ids as wide as the configuration reads (make_inputs has the refiner's five)."""
    inp = make_inputs(cfg)
    if cfg.addition_embed_type == "text_time":
        g = torch.Generator().manual_seed(8)
        for k, v in inp.items():
            if len(v) > 2 and isinstance(v[2], dict):
                inp[k] = v[:2] + (_added(cfg, v[1].shape[0], g),) + v[3:]
    return inp


def _grow(net, cfg, channels=4):
    """A plain B = 3 24x24 forward: more rows than any call of this file, so the arena outgrows every later plan."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, channels, 24, 24, generator=g).half().cuda()
    e = torch.randn(3, 77, cfg.cross_attention_dim, generator=g).half().cuda()
    out = net(x, T, e, added_cond_kwargs=_added(cfg, 3, g))[0]
    assert _finite(out)
    return net.memory()[1]


class UNetCase:
    """Weights, inputs and the fresh-handle references of one configuration, made once per module."""

    def __init__(self, w):
        self.w, self.cfg = w, w["cfg"]
        self.inp = _inputs(self.cfg)
        self._ref = {}

    def ref(self, kind):
        if kind not in self._ref:
            out = run_kind(Handle(self.w), kind, self.inp).clone()
            assert _finite(out), kind
            self._ref[kind] = out
        return self._ref[kind]

    def grown(self):
        h = Handle(self.w)
        _grow(h.net, self.cfg)
        return h

    def check_poisoned(self, h, kinds):
        bad = []
        for kind in kinds:
            want = self.ref(kind)
            for pattern in PATTERNS:
                _settle(h.net)
                _poison(h.net, pattern)
                got = run_kind(h, kind, self.inp)
                if not torch.equal(got, want):
                    bad.append((kind, pattern, "finite" if _finite(got) else "non-finite"))
        _settle(h.net)
        assert not bad, f"calls that read poisoned scratch memory (kind, pattern, output): {bad}"


@pytest.fixture(scope="module")
def tiny():
    return UNetCase(tiny_weights())


def test_hook_on_a_handle_that_allocated_nothing(engine_lib):
    """0 bytes and SD_OK before the first forward; the documented refusals."""
    net = HipUNet2DConditionModel(config.tiny_unet())
    n = C.c_int64(-1)
    for pattern in PATTERNS:
        assert engine_lib.sd_unet_poison_workspace(net._h, pattern, C.byref(n)) == 0 and n.value == 0
    assert engine_lib.sd_unet_poison_workspace(net._h, 2, C.byref(n)) == 1
    assert engine_lib.sd_unet_poison_workspace(None, 0, C.byref(n)) == 1
    assert engine_lib.sd_unet_poison_workspace(net._h, 0, None) == 1
    vae = HipAutoencoderKL(config.tiny_vae())
    assert engine_lib.sd_vae_poison_workspace(vae._h, 1, C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("kinds", [RUN_CASE_KINDS[:4], RUN_CASE_KINDS[4:8], RUN_CASE_KINDS[8:], ("tome", "freeu")],
                         ids=["plain_cfg", "pag", "dc_ip_cn", "tome_freeu"])
def test_unet_on_poisoned_scratch(engine_lib, tiny, kinds):
    tiny.check_poisoned(tiny.grown(), kinds)


def test_unet_deepcache_reuse_on_poisoned_scratch(engine_lib, tiny):
    """Poison between the store and the reuse step: the reuse forward reads the kept feature (dc_buf, left alone) and
    nothing else of the store forward's."""
    h, (x, e, add, x2) = tiny.grown(), tiny.inp["dc"]
    want = tiny.ref("dc_pair")
    net = h.net
    for pattern in PATTERNS:
        net.enable_deepcache(cache_interval=2, cache_depth=1)
        try:
            net.deep_cache_mode(net.DC_STORE)
            a = net(x, T, e, added_cond_kwargs=add)[0]
            assert net._poison_workspace(pattern) > 0
            net.deep_cache_mode(net.DC_REUSE)
            b = net(x2, 481.0, e, added_cond_kwargs=add)[0]
        finally:
            net.deep_cache_mode(net.DC_PLAIN)
        assert torch.equal(torch.cat([a, b]), want), pattern
    net.disable_deepcache()


def test_unet_graph_replay_on_poisoned_scratch(engine_lib, tiny):
    """Capture, poison (the arena and the staging slab the graph's addresses point into), replay."""
    h, (x, e, _) = tiny.grown(), tiny.inp["plain_b2"]
    want = tiny.ref("plain_b2")
    net = h.net
    net.use_graph(True)
    try:
        assert torch.equal(net(x, T, e)[0], want)
        assert net.graph_stats() == (1, 0)
        for i, pattern in enumerate(PATTERNS):
            _poison(net, pattern)
            got = net(x, T, e)[0]
            assert net.graph_stats() == (1, i + 1), "the call after the poison must be a replay"
            assert torch.equal(got, want), pattern
    finally:
        net.use_graph(False)


def test_unet_forward_concat_on_poisoned_scratch(engine_lib):
    cfg = config.UNetConfig(**dict(config.tiny_unet().to_dict(), in_channels=8))
    sd = _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=23, perturb=0.1))
    g = torch.Generator().manual_seed(10)
    lat = (torch.randn(2, 4, 16, 16, generator=g) * 3).half().cuda()
    img = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    ehs = torch.randn(6, 77, cfg.cross_attention_dim, generator=g).half().cuda()
    t = torch.tensor([981.0, 301.0]).cuda()

    def call(net):
        return net.forward_concat(lat, t, ehs, img, zero_from=4, in_scale=IN_SCALE)[0]

    want = call(HipUNet2DConditionModel(cfg).load_state_dict(sd)).clone()
    assert _finite(want)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    _grow(net, cfg, channels=8)
    for pattern in PATTERNS:
        _poison(net, pattern)
        assert torch.equal(call(net), want), pattern


@pytest.mark.parametrize("name", ["sdxl_linear_six_ids", "refiner_five_ids"])
def test_text_time_unets_on_poisoned_scratch(engine_lib, name):
    """Six and five time ids through run_temb (the five-id row is zero-padded to the packed K), linear projections."""
    if name == "refiner_five_ids":
        w = refiner_weights()
    else:
        cfg = config.tiny_unet(linear=True, sdxl_cond=True)
        w = {"cfg": cfg, "unet": _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=24, perturb=0.1))}
    case = UNetCase(w)
    case.check_poisoned(case.grown(), ("plain_b2", "pag_cfg_late"))


# ------------------------------------------------------------------------------- the other handles: one frame
def check_model(make, grow, calls):
    """make() -> a fresh handle; grow(model) the large call; calls = [(tag, setup or None, run)]: setup(model) changes a
    setting on the working handle and on the reference handle alike, run(model) -> the call's output tensors."""
    refs = []
    for i, (tag, _, run) in enumerate(calls):
        m = make()
        for _, earlier, _ in calls[:i + 1]:
            if earlier:
                earlier(m)
        out = [o.clone() for o in run(m)]
        assert all(_finite(o) for o in out), tag
        refs.append(out)
    m = make()
    for o in grow(m):
        assert _finite(o)
    bad = []
    for (tag, setup, run), want in zip(calls, refs):
        if setup:
            setup(m)
        for pattern in PATTERNS:
            _poison(m, pattern)
            got = run(m)
            for i, (a, b) in enumerate(zip(got, want)):
                if not torch.equal(a, b):
                    bad.append((tag, pattern, i, "finite" if _finite(a) else "non-finite"))
    assert not bad, f"calls that read poisoned scratch memory (call, pattern, output index, output): {bad}"


def _flat(out):
    """Every tensor of a CLIP output, hidden states included."""
    ts = []
    for v in list(out) + [getattr(out, "pooler_output", None)]:
        if isinstance(v, tuple):
            ts += list(v)
        elif v is not None and not any(v is t for t in ts):
            ts.append(v)
    return ts


def synth_from_manifest(model, prefix, seed):
    """Random fp16-rounded weights for every tensor the handle declares: linears N(0, 1 / fan_in), norm weights near 1,
    biases and embeddings small."""
    lib, g, sd = model._lib, torch.Generator().manual_seed(seed), {}
    for i in range(getattr(lib, f"sd_{prefix}_num_weights")(model._h)):
        key, shape, ndim = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert getattr(lib, f"sd_{prefix}_weight_info")(model._h, i, C.byref(key), shape, C.byref(ndim)) == 0
        k, shp = key.value.decode(), tuple(shape[j] for j in range(ndim.value))
        r = torch.randn(shp, generator=g)
        if k.endswith(".bias"):
            v = 0.05 * r
        elif "norm" in k:
            v = 1.0 + 0.1 * r
        elif "embedding" in k and "patch" not in k:
            v = 0.3 * r
        else:
            v = r / (r[0].numel() ** 0.5)
        sd[k] = v.half().float()
    return sd


# ------------------------------------------------------------------------------------------------------- VAE
def test_vae_on_poisoned_scratch(engine_lib):
    cfg = config.tiny_vae()
    sd = _f16_round(weights.synth_state_dict(weights.vae_manifest(cfg), seed=25, perturb=0.1))
    g = torch.Generator().manual_seed(11)
    z_grow = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    z1, z2 = torch.randn(2, 4, 8, 12, generator=g).half().cuda(), torch.randn(1, 4, 9, 7, generator=g).half().cuda()
    img = (torch.rand(2, 3, 64, 48, generator=g) * 2 - 1).half().cuda()

    def shift8(v):
        _lib.check(v._lib.sd_vae_encode_range_shift(v._h, 8), "sd_vae_encode_range_shift")

    check_model(lambda: HipAutoencoderKL(cfg).load_state_dict(sd), lambda v: v.decode(z_grow),
                [("decode 2x4x8x12", None, lambda v: v.decode(z1)), ("decode 1x4x9x7", None, lambda v: v.decode(z2)),
                 ("encode 2x3x64x48", None, lambda v: (v.encode_moments(img),)),
                 ("encode 2x3x64x48 shift 8", shift8, lambda v: (v.encode_moments(img),))])


# ------------------------------------------------------------------------------------------------- CLIP text
CLIP_TEXT = {
    "h128_quick_gelu": config.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=3,
                                             num_attention_heads=2, eos_token_id=2),
    "h192_gelu_projection": config.CLIPTextConfig(vocab_size=500, hidden_size=192, intermediate_size=320,
                                                  num_hidden_layers=2, num_attention_heads=3, hidden_act="gelu",
                                                  projection_dim=96, eos_token_id=499, bos_token_id=498, pad_token_id=1),
}


def _ids(cfg, B, Tn, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, cfg.vocab_size - 10, (B, Tn), generator=g)
    ids[:, 0] = cfg.bos_token_id
    eos = cfg.vocab_size - 1 if cfg.eos_token_id == 2 else cfg.eos_token_id      # (legacy configs pool at the argmax)
    for b in range(B):
        ids[b, min(5 + 7 * b, Tn - 1)] = eos
    return ids.cuda()


@pytest.mark.parametrize("name", list(CLIP_TEXT))
def test_clip_text_on_poisoned_scratch(engine_lib, name):
    cfg = CLIP_TEXT[name]
    sd = synth_from_manifest(HipCLIPTextModel(cfg), "clip", seed=26)
    grow_ids, a, b = _ids(cfg, 3, 77, 1), _ids(cfg, 1, 77, 2), _ids(cfg, 2, 20, 3)
    check_model(lambda: HipCLIPTextModel(cfg).load_state_dict(sd), lambda m: _flat(m(grow_ids, output_hidden_states=True)),
                [("B1 T77 hidden states", None, lambda m: _flat(m(a, output_hidden_states=True))),
                 ("B2 T20", None, lambda m: _flat(m(b)))])


# ----------------------------------------------------------------------------------------------- CLIP vision
CLIP_VISION = {
    "a_h128": config.CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                                      image_size=56, patch_size=14, hidden_act="quick_gelu", projection_dim=128),
    "b_h160": config.CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2,
                                      image_size=112, patch_size=14, hidden_act="gelu", projection_dim=96),
    "c_h208": config.CLIPVisionConfig(hidden_size=208, intermediate_size=416, num_hidden_layers=2, num_attention_heads=2,
                                      image_size=42, patch_size=14, hidden_act="gelu", projection_dim=64),
}


@pytest.mark.parametrize("name", list(CLIP_VISION))
def test_clip_vision_on_poisoned_scratch(engine_lib, name):
    """(b) and (c): the hidden width is no multiple of 64, so the LayerNorm, attention and fc1 outputs feed GEMMs whose
    packed K is wider than what their producers write: run_clip_layers has to zero those columns in every call."""
    cfg = CLIP_VISION[name]
    sd = synth_from_manifest(HipCLIPVisionModelWithProjection(cfg), "clip_vision", seed=27)
    g = torch.Generator().manual_seed(12)
    px3 = (torch.rand(3, 3, cfg.image_size, cfg.image_size, generator=g) * 4.0 - 1.8).half().cuda()
    px1 = (torch.rand(1, 3, cfg.image_size, cfg.image_size, generator=g) * 4.0 - 1.8).half().cuda()
    check_model(lambda: HipCLIPVisionModelWithProjection(cfg).load_state_dict(sd),
                lambda m: _flat(m(px3, output_hidden_states=True)),
                [("B1 hidden states", None, lambda m: _flat(m(px1, output_hidden_states=True))),
                 ("B1", None, lambda m: _flat(m(px1)))])


# ----------------------------------------------------------------------------------------- IP-Adapter projection
def test_ip_adapter_linear_projection_on_poisoned_scratch(engine_lib, tiny):
    net = Handle(tiny.w).net
    g = torch.Generator().manual_seed(13)
    big, small = torch.randn(8, D_IMG, generator=g).half().cuda(), torch.randn(2, D_IMG, generator=g).half().cuda()
    check_model(lambda: HipIPAdapter(net, D_IMG, N_TOK).load_state_dict(tiny.w["ip"]), lambda ad: (ad.project(big),),
                [("rows 2", None, lambda ad: (ad.project(small),))])


def test_ip_adapter_resampler_projection_on_poisoned_scratch(engine_lib, tiny):
    """T_feat 17 and 50 with four queries: 21 and 54 keys, neither a multiple of the attention's key tile."""
    d_emb, dim, heads, depth, n_q = 128, 128, 2, 2, 4
    net = Handle(tiny.w).net
    ip_sd = ro.synth_resampler_state_dict(tiny.cfg, d_emb, dim, heads, depth, n_q, seed=7)
    g = torch.Generator().manual_seed(14)
    big = torch.randn(4, 50, d_emb, generator=g).half().cuda()
    x17, x50 = torch.randn(2, 17, d_emb, generator=g).half().cuda(), torch.randn(1, 50, d_emb, generator=g).half().cuda()

    def tokens(n):
        def setup(ad):
            ad.feature_tokens = n
        return setup

    def grow(ad):
        ad.feature_tokens = 50
        return (ad.project(big),)

    check_model(lambda: net.make_ip_adapter(ip_sd, d_emb, n_q), grow,
                [("T_feat 17 rows 2", tokens(17), lambda ad: (ad.project(x17),)),
                 ("T_feat 50 rows 1", tokens(50), lambda ad: (ad.project(x50),))])


# ------------------------------------------------------------------- (b) a non-finite call does not outlive itself
NAN_KINDS = {"plain_b2": "plain_b2", "cfg_share": "cfg", "pag_cfg_late": "pag_cfg", "ip": "ip", "cn_0.9": "cn", "tome": "plain_b2"}


def _with_nan_latents(inp, key):
    bad = dict(inp)
    bad[key] = (torch.full_like(inp[key][0], float("nan")),) + tuple(inp[key][1:])
    return bad


@pytest.mark.parametrize("kind", list(NAN_KINDS))
def test_unet_call_after_nan_latents(engine_lib, tiny, kind):
    """(The text K/V cache is off, as on every new handle: the kept buffers are state and not this test's.)"""
    h = Handle(tiny.w)
    assert _finite(run_kind(h, "plain_b2", tiny.inp))                        # a working handle
    out = run_kind(h, kind, _with_nan_latents(tiny.inp, NAN_KINDS[kind]))    # (returns: the entry's code was 0)
    assert not _finite(out), "the NaN latents did not reach the output: nothing was poisoned"
    assert torch.equal(run_kind(h, kind, tiny.inp), tiny.ref(kind))


def test_unet_call_after_inf_text(engine_lib, tiny):
    h = Handle(tiny.w)
    x, e, add = tiny.inp["plain_b2"]
    bad = dict(tiny.inp)
    e_inf = e.clone()
    e_inf[0, 5, :] = float("inf")
    bad["plain_b2"] = (x, e_inf, add)
    assert _finite(run_kind(h, "plain_b2", tiny.inp))
    assert not _finite(run_kind(h, "plain_b2", bad))
    assert torch.equal(run_kind(h, "plain_b2", tiny.inp), tiny.ref("plain_b2"))


def test_deepcache_pair_after_a_nan_store(engine_lib, tiny):
    h, (x, e, add, _) = Handle(tiny.w), tiny.inp["dc"]
    net = h.net
    net.enable_deepcache(cache_interval=2, cache_depth=1)
    try:
        net.deep_cache_mode(net.DC_STORE)
        out = net(torch.full_like(x, float("nan")), T, e, added_cond_kwargs=add)[0]
    finally:
        net.deep_cache_mode(net.DC_PLAIN)
    assert not _finite(out)
    assert torch.equal(run_kind(h, "dc_pair", tiny.inp), tiny.ref("dc_pair"))
    net.disable_deepcache()


def test_vae_calls_after_non_finite_inputs(engine_lib):
    cfg = config.tiny_vae()
    sd = _f16_round(weights.synth_state_dict(weights.vae_manifest(cfg), seed=25, perturb=0.1))
    g = torch.Generator().manual_seed(15)
    z = torch.randn(2, 4, 8, 12, generator=g).half().cuda()
    img = (torch.rand(2, 3, 64, 48, generator=g) * 2 - 1).half().cuda()
    want_img = HipAutoencoderKL(cfg).load_state_dict(sd).decode(z)[0].clone()
    want_mom = HipAutoencoderKL(cfg).load_state_dict(sd).encode_moments(img).clone()
    assert _finite(want_img) and _finite(want_mom)
    vae = HipAutoencoderKL(cfg).load_state_dict(sd)
    assert not _finite(vae.decode(torch.full_like(z, float("nan")))[0])
    assert torch.equal(vae.decode(z)[0], want_img)
    img_inf = img.clone()
    img_inf[1, 2, 17, 5:9] = float("inf")
    assert not _finite(vae.encode_moments(img_inf))
    assert torch.equal(vae.encode_moments(img), want_mom)
    assert torch.equal(vae.decode(z)[0], want_img)
