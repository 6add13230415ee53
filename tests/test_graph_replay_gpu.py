"""Graph replay (sd_unet_use_graph) against the eager forward through every change of the handle's state.

A graph handle keeps more from call to call than any other: a captured executable with workspace addresses baked in, a
staging slab, a private stream and two events.  tests/test_forward_plans_gpu.py's rule -- a call's result may not depend
on what the handle ran before it -- is applied to it here, together with sd_unet_graph_stats, which tells a replay
from a capture: a handle that captured on every call would be bitwise eager without ever launching a graph.

Every model is a tiny configuration with synthetic fp16-rounded weights; latents are 16x16, 8x8 and one 24x16.  The
reference of every call is a second handle, eager and without caches, built from the same weights and given the same
tensors.  Every call gets fresh tensors with fresh contents, so a stale staging copy or cache cannot agree by accident.
Every comparison is torch.equal.

Which call captures is the rule of model.h's graph_may_replay (walked through on the host by tests/host_pieces.cpp): no
graph yet, another (B, H, W, L, timestep_cond present), or a workspace / staging slab reallocated since the capture."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (puts the repository root on sys.path)
from test_forward_plans_gpu import D_IMG, Handle, _f16_round, refiner_weights, tiny_weights  # noqa: E402
from stablediffusion_amd import _lib, config, weights  # noqa: E402
from stablediffusion_amd.models import HipAutoencoderKL, HipUNet2DConditionModel  # noqa: E402
from stablediffusion_amd.pipeline import SDModelWrapper, StableDiffusionUnifiedPipeline  # noqa: E402
from stablediffusion_amd.schedulers import DDIMScheduler  # noqa: E402

pytestmark = pytest.mark.gpu

TC_DIM, IN_SCALE, UNSUPPORTED = 32, 0.5, 4
KV_L = 7                    # text length of the cache tests (the pipeline tests' prompt length)
SENTINEL = 12344.0          # (an fp16 value no output of these models comes near)


def P(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def synth(cfg, seed):
    return {"cfg": cfg, "unet": _f16_round(weights.synth_state_dict(weights.unet_manifest(cfg), seed=seed, perturb=0.1))}


class Pair:
    """A graph handle and its eager reference on the same weights, the generator every call's tensors come from, and
    the captures / replays the graph handle must have counted so far."""

    def __init__(self, w, graph=None, eager=None, seed=9):
        self.cfg = w["cfg"]
        self.eager = eager if eager is not None else HipUNet2DConditionModel(self.cfg).load_state_dict(w["unet"])
        self.graph = graph if graph is not None else HipUNet2DConditionModel(self.cfg).load_state_dict(w["unet"])
        self.graph.use_graph(True)
        self.g = torch.Generator().manual_seed(seed)
        self.key, self.captures, self.replays = None, 0, 0
        self.regrown = False        # the test grew the workspace since the last capture: the next call captures

    def tensors(self, B, H, W, L=77, tc=False, cfg=False, ehs=None):
        """Fresh inputs of one call: B latents; the text rows and added conditions hold 2B rows for a forward_cfg call."""
        rows, g, c = (2 * B if cfg else B), self.g, self.cfg
        d = {"x": torch.randn(B, c.in_channels, H, W, generator=g).half().cuda(),
             "t": (torch.rand(B, generator=g) * 999).cuda(),
             "ehs": ehs if ehs is not None else torch.randn(rows, L, c.cross_attention_dim, generator=g).half().cuda(),
             "add": None, "tc": None}
        if c.addition_embed_type == "text_time":
            d["add"] = {"text_embeds": torch.randn(rows, 64, generator=g).half().cuda(),
                        "time_ids": torch.randint(0, 1024, (rows, c.num_time_ids), generator=g).float().cuda()}
        if tc:
            d["tc"] = torch.randn(B, TC_DIM, generator=g).cuda()
        return d

    @staticmethod
    def run(net, d, cfg, share):
        if cfg:
            return net.forward_cfg(d["x"], d["t"], d["ehs"], added_cond_kwargs=d["add"], in_scale=IN_SCALE, share=share)[0]
        return net(d["x"], d["t"], d["ehs"], added_cond_kwargs=d["add"], timestep_cond=d["tc"])[0]

    def expect(self, key):
        """Count the call with `key` as the rule says and compare with the handle's own counters."""
        if key != self.key or self.regrown:
            self.captures += 1
        else:
            self.replays += 1
        self.key, self.regrown = key, False
        got = self.graph.graph_stats()
        assert got == (self.captures, self.replays), f"captures / replays {got}, expected {(self.captures, self.replays)} at {key}"

    def call(self, B, H, W, L=77, tc=False, cfg=False, ehs=None):
        """One call with fresh tensors on both handles -> whether the graph handle's output is bitwise the eager one.
        The graph handle gets copies (all but a given `ehs`, whose address is the point), which must come back unchanged;
        under graph a sharing forward_cfg must be the duplicate form, so the eager handle runs share=False."""
        d = self.tensors(B, H, W, L, tc, cfg, ehs)
        want = self.run(self.eager, d, cfg, share=False)
        mine = {k: (v if k == "ehs" and ehs is not None else
                    {n: a.clone() for n, a in v.items()} if isinstance(v, dict) else v.clone() if v is not None else None)
                for k, v in d.items()}
        got = self.run(self.graph, mine, cfg, share=True)
        self.expect((2 * B if cfg else B, H, W, d["ehs"].shape[1], tc))
        for k in ("x", "t", "ehs", "tc"):
            assert d[k] is None or torch.equal(mine[k], d[k]), f"the call changed its input {k}"
        assert torch.isfinite(want.float()).all()
        return torch.equal(got, want)


def workspace(net):
    return net.memory()[1]


# ------------------------------------------------------------------------------------------------ 1, 2, 3
def test_same_key_calls_replay(engine_lib):
    p = Pair(synth(config.tiny_unet(), 61))
    assert p.graph.graph_stats() == (0, 0)
    assert [p.call(2, 16, 16) for _ in range(3)] == [True] * 3
    assert p.graph.graph_stats() == (1, 2) and p.eager.graph_stats() == (0, 0)


def test_each_key_field_captures_once(engine_lib):
    """B, H, W, L and the presence of timestep_cond, one at a time: the change captures, the call after it replays.  The
    way back to the first key captures again: a handle holds one graph."""
    p = Pair(synth(config.tiny_unet(time_cond=TC_DIM), 62))
    # (a change of W alone needs a latent outside the file's three sizes: 16x8)
    keys = [dict(B=2, H=16, W=16), dict(B=1, H=16, W=16), dict(B=1, H=24, W=16), dict(B=1, H=16, W=16),
            dict(B=1, H=16, W=8), dict(B=1, H=16, W=8, L=33), dict(B=1, H=16, W=8, L=33, tc=True), dict(B=2, H=16, W=16)]
    bad = []
    for i, k in enumerate(keys):
        before = p.graph.graph_stats()
        ok = [p.call(**k), p.call(**k)]
        assert p.graph.graph_stats() == (before[0] + 1, before[1] + 1), k
        bad += [(i, j) for j in range(2) if not ok[j]]
    assert not bad, f"(key, call) not bitwise eager: {bad}"
    assert p.graph.graph_stats() == (len(keys), len(keys))


KINDS = {
    # per configuration: the kinds of call a graph handle takes, each twice and not next to itself
    "plain": (lambda: synth(config.tiny_unet(), 63),
              [dict(B=2, H=16, W=16), dict(B=1, H=16, W=16, cfg=True), dict(B=1, H=8, W=8), dict(B=2, H=16, W=16),
               dict(B=1, H=16, W=16, cfg=True), dict(B=1, H=16, W=16, cfg=True), dict(B=1, H=8, W=8)]),
    "text_time": (lambda: synth(config.tiny_unet(sdxl_cond=True), 64),
                  [dict(B=2, H=16, W=16), dict(B=1, H=8, W=8, cfg=True), dict(B=2, H=16, W=16), dict(B=2, H=16, W=16),
                   dict(B=1, H=8, W=8, cfg=True)]),
    "five_time_ids": (refiner_weights,
                      [dict(B=2, H=16, W=16), dict(B=1, H=8, W=8), dict(B=2, H=16, W=16), dict(B=2, H=16, W=16),
                       dict(B=1, H=8, W=8)]),
    "timestep_cond": (lambda: synth(config.tiny_unet(time_cond=TC_DIM), 65),
                      [dict(B=2, H=16, W=16, tc=True), dict(B=2, H=16, W=16), dict(B=2, H=16, W=16, tc=True),
                       dict(B=2, H=16, W=16, tc=True), dict(B=1, H=16, W=16, cfg=True), dict(B=2, H=16, W=16),
                       dict(B=1, H=16, W=16, cfg=True)]),
}


@pytest.mark.parametrize("name", list(KINDS))
def test_every_call_kind_interleaved(engine_lib, name):
    """Note the plain sequence's cfg call next to the plain one with the same rows (B = 2): one key, so the second
    replays the graph the first captured -- the duplicated latents are an input like any other."""
    make, seq = KINDS[name]
    p = Pair(make())
    for k in seq:
        at = [i for i, s in enumerate(seq) if s == k]
        assert len(at) >= 2 and at[-1] - at[0] > 1, k
    bad = [i for i, k in enumerate(seq) if not p.call(**k)]
    assert not bad, f"calls not bitwise eager: {bad}"
    c, r = p.graph.graph_stats()
    assert c >= 2 and r >= 1 and c + r == len(seq)


# ------------------------------------------------------------------------------------------------ 4
def test_text_kv_cache_armed_loop(engine_lib):
    """sd_unet_text_kv_cache armed on a graph handle: one ehs tensor over the steps of a loop."""
    p = Pair(synth(config.tiny_unet(time_cond=TC_DIM), 66))
    p.graph.text_kv_cache(True)
    ehs = torch.randn(2, KV_L, p.cfg.cross_attention_dim, generator=p.g).half().cuda()
    ok = [p.call(2, 16, 16, ehs=ehs) for _ in range(4)]
    assert ok == [True] * 4, ok
    assert p.graph.graph_stats() == (1, 3)


def test_text_kv_cache_armed_recapture_keeps_no_stale_projection(engine_lib):
    """Three calls of one (B, H, W, L) with three ehs tensors, the cache armed once: without, with and without
    timestep_cond.  Each captures (the key's tcond flips), so each runs an eager pass on the staged copies; the staging
    address of ehs is the same in all three.  Before the capturing pass stayed clear of the pointer-keyed caches the
    handle failed here: see profiles/graph_replay_tests.txt."""
    p = Pair(synth(config.tiny_unet(time_cond=TC_DIM), 66))
    p.graph.text_kv_cache(True)
    ok = [p.call(2, 16, 16, L=KV_L), p.call(2, 16, 16, L=KV_L, tc=True), p.call(2, 16, 16, L=KV_L)]
    print(f"kv armed, tcond off/on/off: bitwise eager {ok}, stats {p.graph.graph_stats()}")
    assert ok == [True] * 3, ok
    assert p.graph.graph_stats() == (3, 0)
    assert p.call(2, 16, 16, L=KV_L) and p.graph.graph_stats() == (3, 1)


# ------------------------------------------------------------------------------------------------ 5
def test_refusals_leave_the_graph_alone(engine_lib):
    """Every setting graph mode refuses, tried on a handle with a captured graph: the documented code, an untouched
    output buffer, untouched counters; once the setting is undone the old key replays (no refusal grows anything:
    each returns before the plan), bitwise eager."""
    w = tiny_weights()
    h = Handle(w)
    p = Pair(w, graph=h.net, eager=Handle(w).net)
    lib, net, u = engine_lib, h.net, h.net._h
    assert p.call(2, 16, 16) and p.call(2, 16, 16)
    B, H, W, L = 2, 16, 16, 77
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 4, H, W, generator=g).half().cuda()
    t = torch.full((B,), 501.0).cuda()
    e = torch.randn(B, L, w["cfg"].cross_attention_dim, generator=g).half().cuda()
    emb = torch.randn(B, 1, D_IMG, generator=g).half().cuda()
    img = torch.rand(1, 3, 8 * H, 8 * W, generator=g).half().cuda()
    out = torch.full((3 * B, 4, H, W), SENTINEL).half().cuda()          # (forward_pag with CFG writes 3 B rows)
    tail = (B, H, W, stream())

    def plain():
        return lib.sd_unet_forward(u, P(x), P(t), P(e), L, None, None, P(out), *tail)

    def with_adapter():
        net.attach_ip_adapter(h.ad)
        try:
            return lib.sd_unet_forward_ex(u, P(x), P(t), P(e), L, None, None, P(emb), 1, P(out), *tail)
        finally:
            net.attach_ip_adapter(None)

    def with_controlnet():
        net.attach_controlnet(h.cn)
        try:
            return lib.sd_unet_forward_cn(u, P(x), P(t), P(e), L, None, None, None, 0, P(img), 1, 0.9, P(out), *tail)
        finally:
            net.attach_controlnet(None)

    def pag():
        return lib.sd_unet_forward_pag(u, P(x[:1]), P(t[:1]), P(e), L, None, None, IN_SCALE, 1, 1, P(out), 1, H, W, stream())

    def concat():
        return lib.sd_unet_forward_concat(u, P(x), B, 1.0, P(x), 4, B, B, P(t), P(e), L, None, None, P(out), *tail)

    def freeu():
        net.enable_freeu(0.9, 0.2, 1.2, 1.4)
        try:
            return plain()
        finally:
            net.disable_freeu()

    def deepcache_store():
        net.enable_deepcache(cache_interval=2, cache_depth=1).deep_cache_mode(net.DC_STORE)
        try:
            return plain()
        finally:
            net.deep_cache_mode(net.DC_PLAIN).disable_deepcache()

    def taps():
        _lib.check(lib.sd_unet_tap(u, 1), "sd_unet_tap")
        try:
            return plain()
        finally:
            _lib.check(lib.sd_unet_tap(u, 0), "sd_unet_tap")

    for attempt in (with_adapter, with_controlnet, pag, concat, freeu, deepcache_store, taps):
        stats, ws = net.graph_stats(), workspace(net)
        rc = attempt()
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (attempt.__name__, rc, lib.sd_last_error())
        assert torch.equal(out, torch.full_like(out, SENTINEL)), attempt.__name__
        assert net.graph_stats() == stats and workspace(net) == ws, attempt.__name__
        assert p.call(2, 16, 16), attempt.__name__                      # (counted by Pair.expect as a replay)
        assert net.graph_stats() == (stats[0], stats[1] + 1), attempt.__name__


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "one_element_off"])
def test_the_callers_memory(engine_lib, skew):
    """A capturing call and two replays through the C entry on buffers of the test's own: the inputs come back bitwise
    unchanged, the output lands in its B Cout H W elements and the guard elements on both sides keep their sentinel.
    skew = 1 starts every tensor one element past a 16-byte boundary (the staging copies are plain memcpys)."""
    p = Pair(synth(config.tiny_unet(), 67))
    lib, B, H, W, L, guard = engine_lib, 2, 8, 8, 77, 8 + skew
    n = B * 4 * H * W

    def placed(v):
        """`v` inside a buffer of its own dtype, `guard` sentinel elements before and after it."""
        buf = torch.full((v.numel() + 2 * guard,), SENTINEL, dtype=v.dtype).cuda()
        assert buf.data_ptr() % 16 == 0
        buf[guard:guard + v.numel()] = v.reshape(-1).cuda()
        return buf, buf[guard:guard + v.numel()]

    for i in range(3):
        d = p.tensors(B, H, W, L)
        want = p.eager(d["x"], d["t"], d["ehs"])[0]
        bufs = {k: placed(d[k]) for k in ("x", "t", "ehs")}
        before = {k: b.clone() for k, (b, _) in bufs.items()}
        obuf = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.float16).cuda()
        out = obuf[guard:guard + n]
        assert out.data_ptr() % 16 == (2 * skew)
        rc = lib.sd_unet_forward(p.graph._h, P(bufs["x"][1]), P(bufs["t"][1]), P(bufs["ehs"][1]), L, None, None, P(out),
                                 B, H, W, stream())
        assert rc == 0, lib.sd_last_error()
        torch.cuda.synchronize()
        p.expect((B, H, W, L, False))
        for k in bufs:
            assert torch.equal(bufs[k][0], before[k]), (i, k)
        assert torch.equal(out.view(B, 4, H, W), want), i
        assert torch.equal(obuf[:guard], torch.full_like(obuf[:guard], SENTINEL)), i
        assert torch.equal(obuf[guard + n:], torch.full_like(obuf[guard + n:], SENTINEL)), i
    assert p.graph.graph_stats() == (1, 2)


# ------------------------------------------------------------------------------------------------ 7
def _grown_between_replays(p, lib, how):
    assert p.call(2, 8, 8) and p.call(2, 8, 8)
    assert p.graph.graph_stats() == (1, 1)
    small = workspace(p.graph)
    d = p.tensors(2, 24, 16)
    want = p.eager(d["x"], d["t"], d["ehs"])[0]
    if how == "toggle":
        p.graph.use_graph(False)
        try:
            got = p.graph(d["x"], d["t"], d["ehs"])[0]
        finally:
            p.graph.use_graph(True)
    else:
        ents, cnt = (_lib.SdProfEntry * 512)(), C.c_int()
        lib.sd_prof_enable(1)
        try:
            got = p.graph(d["x"], d["t"], d["ehs"])[0]
            _lib.check(lib.sd_prof_collect(ents, 512, C.byref(cnt)), "sd_prof_collect")
        finally:
            lib.sd_prof_enable(0)
        assert cnt.value > 0                                            # the large forward ran launch by launch
    assert torch.equal(got, want)
    assert p.graph.graph_stats() == (1, 1)                              # neither went through the graph path
    assert workspace(p.graph) > small, "the workspace did not grow: the sequence proves nothing"
    p.regrown = True
    assert p.call(2, 8, 8), "the call after the workspace moved"        # (Pair.expect: a capture)
    assert p.graph.graph_stats() == (2, 1)
    assert p.call(2, 8, 8) and p.graph.graph_stats() == (2, 2)


def test_workspace_growth_between_replays_graph_switched_off_and_on(engine_lib):
    """Capture at (2, 8, 8); an eager (2, 24, 16) forward with replay switched off frees the slab the graph's addresses
    point into; the next (2, 8, 8) call has the old key and must capture again, the one after it replays."""
    _grown_between_replays(Pair(synth(config.tiny_unet(), 68)), engine_lib, "toggle")


def test_workspace_growth_between_replays_under_the_profiler(engine_lib):
    """The same with replay left on and the large forward run under sd_prof_enable, which takes the eager path."""
    _grown_between_replays(Pair(synth(config.tiny_unet(), 68)), engine_lib, "prof")


# ------------------------------------------------------------------------------------------------ 8
def test_fencing_on_a_side_stream(engine_lib):
    """Replays issued on a non-default stream with no device-wide synchronisation between them: each output is consumed
    on that stream (clone) and the input buffers are overwritten on it right after the call.  The staging copy has to be
    ordered before the overwrite and the output copy after the graph (ev_in / ev_out)."""
    p = Pair(synth(config.tiny_unet(), 69))
    B, H, W, steps = 2, 16, 16, 5
    src = [p.tensors(B, H, W) for _ in range(steps)]
    want = [p.eager(d["x"], d["t"], d["ehs"])[0] for d in src]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(s):
        x, t, e = (torch.empty_like(src[0][k]) for k in ("x", "t", "ehs"))
        for i in range(steps):
            for buf, k in ((x, "x"), (t, "t"), (e, "ehs")):
                buf.copy_(src[i][k], non_blocking=True)
            outs.append(p.graph(x, t, e)[0].clone())
            for buf in (x, t, e):
                buf.fill_(float("nan"))                                 # the caller's overwrite, right behind the call
    s.synchronize()
    torch.cuda.synchronize()
    assert p.graph.graph_stats() == (1, steps - 1)
    bad = [i for i in range(steps) if not torch.equal(outs[i], want[i])]
    assert not bad, f"steps not bitwise eager: {bad}"


# ------------------------------------------------------------------------------------------------ 9
def test_pipeline_calls_on_a_live_graph(engine_lib):
    """Two pipeline calls of the same shapes and different prompt embeddings, CFG on, the scheduler's step on the device,
    on a wrapper whose UNet replays and on one whose UNet does not: the latents of each call are bitwise equal.  The
    pipeline arms the text K/V cache in front of every loop; the second call finds the first one's graph."""
    ucfg, vcfg = config.tiny_unet(), config.tiny_vae()
    usd = _f16_round(weights.synth_state_dict(weights.unet_manifest(ucfg), 11))
    vae = HipAutoencoderKL(vcfg).load_state_dict(_f16_round(weights.synth_state_dict(weights.vae_manifest(vcfg), 12)))
    models = {on: SDModelWrapper(base=HipUNet2DConditionModel(ucfg).load_state_dict(usd).use_graph(on), vae=vae,
                                 scheduler=DDIMScheduler(), device="cuda") for on in (True, False)}
    pipe = StableDiffusionUnifiedPipeline(do_cfg=True, device="cuda", output_type="latents")
    g, steps = torch.Generator().manual_seed(3), 3
    for call in range(2):
        pos, neg = (torch.randn(2, 7, ucfg.cross_attention_dim, generator=g).half().cuda() for _ in range(2))
        lat0 = torch.randn(2, 4, 16, 16, generator=g).half().cuda()
        out = {on: pipe(m, prompt_embeds=pos.clone(), negative_prompt_embeds=neg.clone(), latents=lat0.clone(),
                        num_inference_steps=steps, guidance_scale=5.0, height=128, width=128) for on, m in models.items()}
        assert torch.isfinite(out[False].float()).all()
        assert torch.equal(out[True], out[False]), call
        assert models[True].base.graph_stats() == (1, steps * (call + 1) - 1), call
    assert models[False].base.graph_stats() == (0, 0)
