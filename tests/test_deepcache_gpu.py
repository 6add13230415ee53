"""DeepCache on the GPU (sd_unet_set_deep_cache / sd_unet_deep_cache_mode): a store forward is the plain forward bit for
bit with the same launches; a reuse forward on unchanged inputs is the full forward bit for bit; on new inputs it
matches the restated forward of tests/deepcache_oracle.py fed its own cached feature, and is far from both the full
forward at the new inputs and the stored step's output; it runs only the layers it names; every row of the error table
returns its code with nothing launched; "off means off"; and the pipeline's loop sets the modes a hand-set loop sets.

Bounds: 1e-2 is the project's UNet-vs-oracle rel-L2 bound (the full forward measures 1-3e-3).  The 0.1 gaps are
conditions, not measurements: on CPU the two oracles are 0.90-1.10 apart and the reuse output 0.71-0.96 from the stored
step's for every configuration, shape and depth here."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_l2  # noqa: E402  (first: it puts the repository root on sys.path for the child process too)
import deepcache_oracle  # noqa: E402
from cn_oracle import synth_cn_state_dict  # noqa: E402
from ip_oracle import synth_ip_state_dict  # noqa: E402
from stablediffusion_amd import _lib, config, controlnet, schedulers, weights  # noqa: E402
from stablediffusion_amd.config import UNetConfig  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipControlNetModel, HipIPAdapter, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-2
GAP = 0.1
PLAIN, STORE, REUSE = HipUNet2DConditionModel.DC_PLAIN, HipUNet2DConditionModel.DC_STORE, HipUNet2DConditionModel.DC_REUSE
FREEU = (0.9, 0.2, 1.5, 1.6)
CONFIGS = {"tiny": config.tiny_unet, "linear_sdxl": lambda: config.tiny_unet(linear=True, sdxl_cond=True),
           "refiner": config.tiny_refiner_unet}
SHAPES = [(2, 16, 16), (1, 8, 24), (3, 24, 24)]
DEPTHS = [1, 2]
CASES = [(n, B, H, W, d) for n in CONFIGS for (B, H, W) in SHAPES for d in DEPTHS]


def _f16_round(sd):
    return {k: v.half().float() for k, v in sd.items()}


def _weights(cfg):
    return _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=11, perturb=0.1))


_nets = {}


def _setup(name):
    """(cfg, weights, the engine under test, an engine DeepCache was never enabled on), built once per configuration."""
    if name not in _nets:
        cfg = CONFIGS[name]()
        sd = _weights(cfg)
        _nets[name] = (cfg, sd, HipUNet2DConditionModel(cfg).load_state_dict(sd),
                       HipUNet2DConditionModel(cfg).load_state_dict(sd))
    return _nets[name]


def _added(cfg, rows):
    if cfg.addition_embed_type != "text_time":
        return None
    n = cfg.num_time_ids
    tdim = cfg.projection_class_embeddings_input_dim - n * cfg.addition_time_embed_dim
    g = torch.Generator().manual_seed(8)
    ids = [128.0, 128, 0, 0, 128, 128] if n == 6 else [128.0, 128, 0, 0, 6.0]
    return {"text_embeds": torch.randn(rows, tdim, generator=g).half(), "time_ids": torch.tensor([ids] * rows)}


def _inputs(cfg, B, H, W, rows=None):
    """x0, ehs, then an independent x1 from the same generator; the text_time conditions for `rows`."""
    g = torch.Generator().manual_seed(B * 100 + H)
    x0 = torch.randn(B, 4, H, W, generator=g).half()
    ehs = torch.randn(rows or B, 77, cfg.cross_attention_dim, generator=g).half()
    x1 = torch.randn(B, 4, H, W, generator=g).half()
    return x0, ehs, x1, _added(cfg, rows or B)


def _kw(added):
    return {} if added is None else {"added_cond_kwargs": {k: v.cuda() for k, v in added.items()}}


def _launches(lib, run):
    run()
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    try:
        run()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    return {e.kernel.decode(): e.launches for e in ents[: n.value]}


def _cache_elems(cfg, B, H, W, d):
    boc = cfg.block_out_channels
    return B * H * W * ((boc[1] if d == cfg.layers_per_block else boc[0]) + boc[0])


def _is_attention(kernel):
    return kernel.startswith("attn_kernel<") or kernel.startswith("ip_xattn_kernel<")


# ----------------------------------------------------------------------------------------- 1. store is plain
@pytest.mark.parametrize("name,B,H,W,d", CASES)
def test_store_is_the_plain_forward(engine_lib, name, B, H, W, d):
    cfg, sd, net, never = _setup(name)
    x, ehs, _, added = _inputs(cfg, B, H, W)
    xd, ed, kw = x.cuda(), ehs.cuda(), _kw(added)
    want = never(xd, 501.0, ed, **kw)[0]
    before = net.memory()[1]
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        run = lambda: net(xd, 501.0, ed, **kw)[0]   # noqa: E731
        assert torch.equal(run(), want)
        assert _launches(engine_lib, run) == _launches(engine_lib, lambda: never(xd, 501.0, ed, **kw)[0])
        # the buffer is the handle's and is counted
        assert net.memory()[1] - before >= 2 * _cache_elems(cfg, B, H, W, d)
    finally:
        net.disable_deepcache()


@pytest.mark.parametrize("share", [True, False], ids=["share", "noshare"])
@pytest.mark.parametrize("name,B,H,W,d", CASES)
def test_store_is_the_plain_forward_cfg(engine_lib, name, B, H, W, d, share):
    cfg, sd, net, never = _setup(name)
    x, ehs, _, added = _inputs(cfg, B, H, W, rows=2 * B)
    xd, ed, kw = x.cuda(), ehs.cuda(), _kw(added)
    want = never.forward_cfg(xd, 501.0, ed, in_scale=0.7, share=share, **kw)[0]
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        assert torch.equal(net.forward_cfg(xd, 501.0, ed, in_scale=0.7, share=share, **kw)[0], want)
    finally:
        net.disable_deepcache()


# -------------------------------------------------------- 2. reuse on unchanged inputs is the full forward
@pytest.mark.parametrize("name,B,H,W,d", CASES)
def test_reuse_on_unchanged_inputs_is_the_full_forward(engine_lib, name, B, H, W, d):
    cfg, sd, net, never = _setup(name)
    x, ehs, _, added = _inputs(cfg, B, H, W)
    xd, ed, kw = x.cuda(), ehs.cuda(), _kw(added)
    want = never(xd, 501.0, ed, **kw)[0]
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        assert torch.equal(net(xd, 501.0, ed, **kw)[0], want)
        net.deep_cache_mode(REUSE)
        assert torch.equal(net(xd, 501.0, ed, **kw)[0], want)
        assert torch.equal(net(xd, 501.0, ed, **kw)[0], want)          # and again: a reuse step leaves the cache as it was
    finally:
        net.disable_deepcache()


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("d", DEPTHS)
def test_reuse_through_forward_cfg_shared(engine_lib, B, H, W, d):
    cfg, sd, net, never = _setup("tiny")
    assert net.cfg_share_eligible
    x, ehs, _, _ = _inputs(cfg, B, H, W, rows=2 * B)
    xd, ed = x.cuda(), ehs.cuda()
    want = never.forward_cfg(xd, 501.0, ed, in_scale=0.7, share=True)[0]
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        assert torch.equal(net.forward_cfg(xd, 501.0, ed, in_scale=0.7, share=True)[0], want)
        net.deep_cache_mode(REUSE)
        assert torch.equal(net.forward_cfg(xd, 501.0, ed, in_scale=0.7, share=True)[0], want)
    finally:
        net.disable_deepcache()


@pytest.mark.parametrize("d", DEPTHS)
def test_reuse_with_freeu_on(engine_lib, d):
    cfg, sd, net, never = _setup("tiny")
    assert len(cfg.block_out_channels) == 4
    x, ehs, _, _ = _inputs(cfg, 2, 16, 16)
    xd, ed = x.cuda(), ehs.cuda()
    never.enable_freeu(*FREEU)
    net.enable_freeu(*FREEU)
    net.enable_deepcache(3, d)
    try:
        want = never(xd, 501.0, ed)[0]
        net.deep_cache_mode(STORE)
        assert torch.equal(net(xd, 501.0, ed)[0], want)
        net.deep_cache_mode(REUSE)
        assert torch.equal(net(xd, 501.0, ed)[0], want)
    finally:
        net.disable_deepcache()
        net.disable_freeu()
        never.disable_freeu()
    assert not torch.equal(never(xd, 501.0, ed)[0], want)


@pytest.mark.parametrize("d", DEPTHS)
def test_reuse_with_an_ip_adapter_attached(engine_lib, d):
    cfg, sd, net, never = _setup("tiny")
    ipsd = synth_ip_state_dict(cfg, 128, 4, seed=3)
    ad, ad_never = HipIPAdapter(net, 128, 4).load_state_dict(ipsd), HipIPAdapter(never, 128, 4).load_state_dict(ipsd)
    x, ehs, _, _ = _inputs(cfg, 2, 16, 16)
    xd, ed = x.cuda(), ehs.cuda()
    g = torch.Generator().manual_seed(6)
    kw = {"added_cond_kwargs": {"image_embeds": [torch.randn(2, 1, 128, generator=g).half().cuda()]}}
    never.attach_ip_adapter(ad_never)
    net.attach_ip_adapter(ad)
    net.enable_deepcache(3, d)
    try:
        want = never(xd, 501.0, ed, **kw)[0]
        net.deep_cache_mode(STORE)
        assert torch.equal(net(xd, 501.0, ed, **kw)[0], want)
        net.deep_cache_mode(REUSE)
        assert torch.equal(net(xd, 501.0, ed, **kw)[0], want)
        launches = _launches(engine_lib, lambda: net(xd, 501.0, ed, **kw)[0])
        assert sum(n for k, n in launches.items() if k.startswith("ip_xattn_kernel<")) == 2 * d + 1
    finally:
        net.disable_deepcache()
        net.attach_ip_adapter(None)
        never.attach_ip_adapter(None)


@pytest.mark.parametrize("d", DEPTHS)
def test_store_reuse_sequence_across_shapes(engine_lib, d):
    """S R R S at one shape, then another shape, then the first again: every forward on its step's own inputs equals
    the plain forward there (the reuse steps repeat the store step's inputs, so they are the full forward)."""
    cfg, sd, net, never = _setup("tiny")
    net.enable_deepcache(3, d)
    try:
        for B, H, W in [(2, 16, 16), (1, 8, 24), (2, 16, 16)]:
            x0, ehs, x1, _ = _inputs(cfg, B, H, W)
            ed = ehs.cuda()
            for mode, x, t in [(STORE, x0, 501.0), (REUSE, x0, 501.0), (REUSE, x0, 501.0), (STORE, x1, 441.0),
                               (REUSE, x1, 441.0)]:
                net.deep_cache_mode(mode)
                assert torch.equal(net(x.cuda(), t, ed)[0], never(x.cuda(), t, ed)[0]), (B, H, W, mode, t)
    finally:
        net.disable_deepcache()


# ----------------------------------------------------------- 3. reuse on new inputs matches the oracle
def _check_new_inputs(cfg, sd, net, B, H, W, d, what, gaps=True):
    x0, ehs, x1, added = _inputs(cfg, B, H, W)
    ref_added = None if added is None else {k: v.float() for k, v in added.items()}
    t0, t1 = torch.tensor(501.0), torch.tensor(441.0)
    with torch.no_grad():
        full0, feat = deepcache_oracle.forward(cfg, sd, x0.float(), t0, ehs.float(), ref_added, d)
        want, _ = deepcache_oracle.forward(cfg, sd, x1.float(), t1, ehs.float(), ref_added, d, cached=feat)
        full1, _ = deepcache_oracle.forward(cfg, sd, x1.float(), t1, ehs.float(), ref_added, d)
    ed, kw = ehs.cuda(), _kw(added)
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        stored = net(x0.cuda(), t0, ed, **kw)[0]
        net.deep_cache_mode(REUSE)
        got = net(x1.cuda(), t1, ed, **kw)[0]
    finally:
        net.disable_deepcache()
    e_store, e, e_full, e_prev = rel_l2(stored, full0), rel_l2(got, want), rel_l2(got, full1), rel_l2(got, stored)
    print(f"{what} B={B} {H}x{W} d={d}: store vs oracle {e_store:.2e}, reuse vs oracle's reuse form {e:.2e}, vs the full "
          f"forward at the new inputs {e_full:.2f} (oracles apart {rel_l2(want, full1):.2f}), vs the stored step {e_prev:.2f}")
    assert e_store < TOL
    assert e < TOL
    if gaps:
        assert e_full > GAP
        assert e_prev > GAP


@pytest.mark.parametrize("name,B,H,W,d", CASES)
def test_reuse_on_new_inputs_matches_the_oracle(engine_lib, name, B, H, W, d):
    cfg, sd, net, _ = _setup(name)
    _check_new_inputs(cfg, sd, net, B, H, W, d, name)


def _gn_cat_child():
    """Runs under SD_GN_CAT=1 (read once per process, the first time the up path runs).  Only the oracle bound: the plain
    forward then merges GroupNorm summaries a reuse step does not have, so the bit identities are not claimed here."""
    assert os.environ.get("SD_GN_CAT") == "1"
    for name in CONFIGS:
        cfg = CONFIGS[name]()
        sd = _weights(cfg)
        net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
        for B, H, W in SHAPES:
            for d in DEPTHS:
                _check_new_inputs(cfg, sd, net, B, H, W, d, f"SD_GN_CAT=1 {name}", gaps=False)
    print("gn-cat-child-ok")


def test_reuse_on_new_inputs_under_gn_cat(engine_lib):
    env = dict(os.environ, SD_GN_CAT="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "gn_cat_child"], env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gn-cat-child-ok" in r.stdout


# --------------------------------------------------------------------------- 4. reuse skips the rest
@pytest.mark.parametrize("name,B,H,W,d", CASES)
def test_reuse_runs_only_its_layers(engine_lib, name, B, H, W, d):
    cfg, sd, net, never = _setup(name)
    x, ehs, _, added = _inputs(cfg, B, H, W)
    xd, ed, kw = x.cuda(), ehs.cuda(), _kw(added)
    plain = _launches(engine_lib, lambda: never(xd, 501.0, ed, **kw)[0])
    net.enable_deepcache(3, d)
    try:
        net.deep_cache_mode(STORE)
        net(xd, 501.0, ed, **kw)
        net.deep_cache_mode(REUSE)
        reuse = _launches(engine_lib, lambda: net(xd, 501.0, ed, **kw)[0])
    finally:
        net.disable_deepcache()
    assert sum(reuse.values()) < sum(plain.values()), (reuse, plain)
    blocks = 0
    if cfg.down_block_types[0] == "CrossAttnDownBlock2D":
        blocks += d * cfg.transformer_layers_per_block[0]
    if cfg.up_block_types[-1] == "CrossAttnUpBlock2D":
        blocks += (d + 1) * cfg.transformer_layers_per_block[0]
    assert sum(n for k, n in reuse.items() if _is_attention(k)) == 2 * blocks, reuse
    assert sum(n for k, n in plain.items() if _is_attention(k)) > 2 * blocks
    # the tail: one launch of the kernel the plain forward's tail takes
    tails = ("conv_tail_kernel", "conv3x3_small_cout_kernel")
    for k in tails:
        assert reuse.get(k, 0) == plain.get(k, 0), (k, reuse, plain)
    assert sum(reuse.get(k, 0) for k in tails) <= 1
    assert reuse.get("conv_head_kernel", 0) == plain.get("conv_head_kernel", 0)
    assert not any("freeu" in k or k.startswith("cn_") for k in reuse)


# ----------------------------------------------------------------------- 5. errors and off means off
def _fails(lib, run, code, match):
    """`run` raises the engine's error `code` with a message, having launched nothing."""
    torch.cuda.synchronize()
    lib.sd_prof_enable(1)
    try:
        with pytest.raises(_lib.EngineError, match=f"error {code}: .*{match}"):
            run()
        ents = (_lib.SdProfEntry * 512)()
        n = C.c_int()
        _lib.check(lib.sd_prof_collect(ents, 512, C.byref(n)), "sd_prof_collect")
    finally:
        lib.sd_prof_enable(0)
    assert n.value == 0, [(e.kernel.decode(), e.launches) for e in ents[: n.value]]
    assert lib.sd_last_error()


def _two_block_config():
    return UNetConfig(sample_size=16, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"),
                      up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"), block_out_channels=(64, 128),
                      cross_attention_dim=64, attention_head_dim=(2, 4), transformer_layers_per_block=(1, 1))


def test_error_table(engine_lib):
    lib = engine_lib
    cfg, sd, net, never = _setup("tiny")
    L = cfg.layers_per_block
    x, ehs, _, _ = _inputs(cfg, 2, 16, 16)
    xd, ed = x.cuda(), ehs.cuda()
    run = lambda: net(xd, 501.0, ed)[0]   # noqa: E731
    try:
        # depth outside 0..L, an unknown mode: SD_ERR_INVALID
        for depth in (-1, L + 1):
            assert lib.sd_unet_set_deep_cache(net._h, depth) == 1 and lib.sd_last_error()
        net.enable_deepcache(3, 1)
        for mode in (-1, 3):
            assert lib.sd_unet_deep_cache_mode(net._h, mode) == 1 and lib.sd_last_error()
        # a non-plain mode while the depth is 0: SD_ERR_STATE
        net.disable_deepcache()
        for mode in (STORE, REUSE):
            assert lib.sd_unet_deep_cache_mode(net._h, mode) == 2 and lib.sd_last_error()
        assert torch.equal(run(), never(xd, 501.0, ed)[0])
        # a reuse forward without a valid cache of the call's shape: SD_ERR_STATE
        net.enable_deepcache(3, 1)
        net.deep_cache_mode(REUSE)
        _fails(lib, run, 2, "reuse")                                      # nothing stored yet
        net.deep_cache_mode(STORE)
        run()
        net.deep_cache_mode(REUSE)
        run()
        x2, ehs2, _, _ = _inputs(cfg, 1, 8, 24)
        _fails(lib, lambda: net(x2.cuda(), 501.0, ehs2.cuda()), 2, "reuse")        # another shape
        _fails(lib, lambda: net.forward_cfg(xd[:1], 501.0, ed, share=True), 2, "reuse")   # same B H W, the shared prefix
        run()                                                                 # the stored step is still good
        net.enable_deepcache(3, 1)                                            # every set call invalidates (and resets the mode)
        assert torch.equal(run(), never(xd, 501.0, ed)[0])
        net.deep_cache_mode(REUSE)
        _fails(lib, run, 2, "reuse")
        for invalidate in (lambda: net.enable_freeu(*FREEU).disable_freeu(),
                           lambda: net.attach_ip_adapter(None),
                           lambda: net.attach_controlnet(None)):
            net.deep_cache_mode(STORE)
            run()
            invalidate()
            net.deep_cache_mode(REUSE)
            _fails(lib, run, 2, "reuse")
        # graph replay on: SD_ERR_UNSUPPORTED
        net.use_graph(True)
        for mode in (STORE, REUSE):
            net.deep_cache_mode(mode)
            _fails(lib, run, 4, "graph")
        net.use_graph(False)
        # a ControlNet that would run: SD_ERR_UNSUPPORTED
        ccfg = controlnet.encoder_config(cfg)
        cn = HipControlNetModel(net, ccfg).load_state_dict(synth_cn_state_dict(ccfg, seed=4))
        img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(5)).half().cuda()
        net.attach_controlnet(cn)
        net.deep_cache_mode(STORE)
        _fails(lib, lambda: net(xd, 501.0, ed, controlnet_cond=img, controlnet_conditioning_scale=0.8), 4, "ControlNet")
        net.attach_controlnet(None)
    finally:
        net.use_graph(False)
        net.attach_controlnet(None)
        net.disable_deepcache()
    assert torch.equal(run(), never(xd, 501.0, ed)[0])


def test_freeu_on_fewer_than_three_blocks_is_rejected(engine_lib):
    cfg = _two_block_config()
    sd = _weights(cfg)
    net = HipUNet2DConditionModel(cfg).load_state_dict(sd)
    g = torch.Generator().manual_seed(4)
    xd = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
    ed = torch.randn(2, 77, 64, generator=g).half().cuda()
    run = lambda: net(xd, 501.0, ed)[0]   # noqa: E731
    plain = run()
    with torch.no_grad():
        ref, _ = deepcache_oracle.forward(cfg, sd, xd.cpu().float(), torch.tensor(501.0), ed.cpu().float(), None, 1)
    assert rel_l2(plain, ref) < TOL
    net.enable_deepcache(2, 1)
    net.deep_cache_mode(STORE)
    assert torch.equal(run(), plain)                                     # two blocks without FreeU: fine
    net.deep_cache_mode(REUSE)
    assert torch.equal(run(), plain)
    net.enable_freeu(*FREEU)
    for mode in (STORE, REUSE):
        net.deep_cache_mode(mode)
        _fails(engine_lib, run, 4, "FreeU")
    net.deep_cache_mode(PLAIN)
    net.disable_freeu()
    net.disable_deepcache()
    assert torch.equal(run(), plain)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_off_means_off(engine_lib, name):
    cfg, sd, net, never = _setup(name)
    x, ehs, x1, added = _inputs(cfg, 2, 16, 16)
    xd, ed, kw = x.cuda(), ehs.cuda(), _kw(added)
    run = lambda: net(xd, 501.0, ed, **kw)[0]   # noqa: E731
    want = never(xd, 501.0, ed, **kw)[0]
    off = _launches(engine_lib, lambda: never(xd, 501.0, ed, **kw)[0])
    net.enable_deepcache(2, 2)
    net.deep_cache_mode(STORE)
    run()
    net.deep_cache_mode(REUSE)
    shallow = net(x1.cuda(), 441.0, ed, **kw)[0]
    held = net.memory()[1]
    net.disable_deepcache()                                              # sd_unet_set_deep_cache(u, 0)
    assert held - net.memory()[1] >= 2 * _cache_elems(cfg, 2, 16, 16, 2)  # the buffer is released
    assert torch.equal(run(), want) and not torch.equal(shallow, never(x1.cuda(), 441.0, ed, **kw)[0])
    assert _launches(engine_lib, run) == off


# ------------------------------------------------------------------------------------------- 6. pipeline
class HandModes:
    """The engine's UNet with DeepCache hidden from the pipeline (`deepcache` is None, so the loop sets no mode) and the
    modes set by hand instead: forward i runs in modes[i]."""

    def __init__(self, net, modes):
        self._net, self._modes, self.i = net, modes, 0

    deepcache = None

    def __getattr__(self, name):
        return getattr(self._net, name)

    def _next(self):
        self._net.deep_cache_mode(self._modes[self.i])
        self.i += 1

    def __call__(self, *a, **k):
        self._next()
        return self._net(*a, **k)

    def forward_cfg(self, *a, **k):
        self._next()
        return self._net.forward_cfg(*a, **k)


@pytest.fixture(scope="module")
def pipe_parts():
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    net = HipUNet2DConditionModel(ucfg).load_state_dict(_weights(ucfg))
    vae = HipAutoencoderKL(vcfg).load_state_dict(_f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12)))
    return net, vae


def _loop(model, sched, do_cfg, steps=6):
    model.set_scheduler(sched)
    B, g = 2, torch.Generator().manual_seed(3)
    dim = config.tiny_unet().cross_attention_dim
    kw = dict(prompt_embeds=torch.randn(B, 7, dim, generator=g).half().cuda(),
              latents=torch.randn(B, 4, 16, 16, generator=g).half().cuda(), num_inference_steps=steps, guidance_scale=5.0,
              height=128, width=128)
    neg = torch.randn(B, 7, dim, generator=g).half().cuda()
    if do_cfg:
        kw["negative_prompt_embeds"] = neg
    pipe = StableDiffusionUnifiedPipeline(do_cfg=do_cfg, device="cuda", output_type="latents")
    torch.manual_seed(3)
    out = pipe(model, **kw)
    assert torch.isfinite(out.float()).all()
    return out


# "DDIM" under CFG takes the "linear" device step, "PNDM" the "affine" one (7 iterations for 6 steps), "DDIM" without CFG
# the host path (scheduler.step)
@pytest.mark.parametrize("sched,do_cfg,iters", [("DDIM", True, 6), ("PNDM", True, 7), ("PNDM", False, 7), ("DDIM", False, 6)],
                         ids=["linear", "affine", "affine-nocfg", "host"])
def test_pipeline_loop(engine_lib, pipe_parts, sched, do_cfg, iters):
    net, vae = pipe_parts
    model = SDModelWrapper(base=net, vae=vae, scheduler=schedulers.DDIMScheduler(), device="cuda")
    off = _loop(model, sched, do_cfg)
    try:
        model.enable_deepcache(1, 1)
        assert torch.equal(_loop(model, sched, do_cfg), off)                 # interval 1: every step is a store step
        model.enable_deepcache(3, 1)
        on = _loop(model, sched, do_cfg)
        assert not torch.equal(on, off)
        # the same loop with the modes set by hand
        hand = HandModes(net, [STORE if i % 3 == 0 else REUSE for i in range(iters)])
        by_hand = _loop(SDModelWrapper(base=hand, vae=vae, scheduler=schedulers.DDIMScheduler(), device="cuda"), sched, do_cfg)
        assert hand.i == iters
        net.deep_cache_mode(PLAIN)
        assert torch.equal(on, by_hand)
        print(f"{sched} cfg={do_cfg}: interval 3 is {rel_l2(on, off):.3f} from the plain loop (synthetic weights: not a "
              "quality figure)")
    finally:
        net.deep_cache_mode(PLAIN)
        model.disable_deepcache()
    assert torch.equal(_loop(model, sched, do_cfg), off)


if __name__ == "__main__" and sys.argv[1:] == ["gn_cat_child"]:
    _gn_cat_child()
