// AnimateDiff motion adapter (diffusers 0.27.2 MotionAdapter / TransformerTemporalModel, recalled) on the gfx950 kernels,
// run inside the UNet forward.
//
// A motion module sits behind every (resnet, transformer) pair of the down and up blocks and behind the mid block's
// transformer.  The UNet's batch is V videos of F consecutive frames; one module, on x of [V F, C, H, W]:
//   GroupNorm(32, eps 1e-6) over a group's channels and all F H W positions of one video -- in NHWC row order that is
//   the engine's GroupNorm on V images of (F H) x W -- proj_in, one transformer block
//       h += to_out(attn(LN1(h) + pe)),  h += to_out2(attn(LN2(h) + pe)),  h += FF_geglu(LN3(h)),
//   proj_out, + x.  Both attentions are self-attention over the F frames of one pixel (temporal_attention.hip).
// Everything but the attention is row-wise and runs on the launches the spatial transformer uses: the folded-LayerNorm
// q|k|v linear with the query pre-scale, the GEGLU projection, the residual epilogues.  The position rows enter as the
// per-frame table pe W^T (launch_motion_pos_bias, built here from the raw weights before the LayerNorm fold).
#include "model.h"

#include <cmath>
#include <cstdio>

namespace sd {

namespace {

void declare_module(WeightStore& ws, const std::string& p, int c) {
    ws.declare(p + ".norm.weight", {c});
    ws.declare(p + ".norm.bias", {c});
    ws.declare(p + ".proj_in.weight", {c, c});
    ws.declare(p + ".proj_in.bias", {c});
    const std::string b = p + ".transformer_blocks.0";
    for (const char* n : {".norm1", ".norm2", ".norm3"}) {
        ws.declare(b + n + ".weight", {c});
        ws.declare(b + n + ".bias", {c});
    }
    for (const char* a : {".attn1", ".attn2"}) {
        ws.declare(b + a + ".to_q.weight", {c, c});
        ws.declare(b + a + ".to_k.weight", {c, c});
        ws.declare(b + a + ".to_v.weight", {c, c});
        ws.declare(b + a + ".to_out.0.weight", {c, c});
        ws.declare(b + a + ".to_out.0.bias", {c});
    }
    ws.declare(b + ".ff.net.0.proj.weight", {8 * c, c});
    ws.declare(b + ".ff.net.0.proj.bias", {8 * c});
    ws.declare(b + ".ff.net.2.weight", {c, 4 * c});
    ws.declare(b + ".ff.net.2.bias", {c});
    ws.declare(p + ".proj_out.weight", {c, c});
    ws.declare(p + ".proj_out.bias", {c});
}

}  // namespace

MotionAdapter::MotionAdapter(const sd_motion_config& m) : mcfg(m) {
    const int nb = m.num_blocks;
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < m.layers_per_block; ++j)
            declare_module(ws, "down_blocks." + std::to_string(i) + ".motion_modules." + std::to_string(j), m.block_out_channels[i]);
    if (m.use_mid_block) declare_module(ws, "mid_block.motion_modules.0", m.block_out_channels[nb - 1]);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < m.layers_per_block + 1; ++j)
            declare_module(ws, "up_blocks." + std::to_string(i) + ".motion_modules." + std::to_string(j),
                           m.block_out_channels[nb - 1 - i]);
}

MotionAdapter::~MotionAdapter() {
    if (attached) attached->set_motion(nullptr);
}

int MotionAdapter::pack_module(const std::string& p, int heads, MotionModule* m) {
    int rc;
    if ((rc = ws.pack_norm(p + ".norm", &m->gn))) return rc;
    if ((rc = ws.pack_conv(p + ".proj_in", &m->pin))) return rc;
    if ((rc = ws.pack_conv(p + ".proj_out", &m->pout))) return rc;
    const int C = m->pin.cout;
    m->C = C; m->heads = heads;
    const std::string b = p + ".transformer_blocks.0";
    if ((rc = ws.pack_norm(b + ".norm1", &m->ln1))) return rc;
    if ((rc = ws.pack_norm(b + ".norm2", &m->ln2))) return rc;
    if ((rc = ws.pack_norm(b + ".norm3", &m->ln3))) return rc;
    // log2(e) / sqrt(d) rides on the query rows, as in the spatial transformer (pack_xformer): the kernel's prescaled path
    const float qs = 1.4426950408889634f / sqrtf((float)(C / heads));
    const int F = mcfg.max_seq_length;
    for (int a = 0; a < 2; ++a) {
        const std::string at = b + (a == 0 ? ".attn1" : ".attn2");
        ConvW* qkv = a == 0 ? &m->qkv1 : &m->qkv2;
        if ((rc = ws.pack_rows({at + ".to_q.weight", at + ".to_k.weight", at + ".to_v.weight"}, {}, qkv))) return rc;
        if ((rc = ws.pack_conv(at + ".to_out.0", a == 0 ? &m->out1 : &m->out2))) return rc;
        // the position term of this attention: pe_f W^T per frame from the UNFOLDED weights (pe is added after the
        // LayerNorm's affine), the query columns with the pre-scale
        float* tab = static_cast<float*>(ws.dmalloc((size_t)F * 3 * C * sizeof(float)));
        if (!tab) { set_error("hipMalloc failed (motion position table)"); return 3; }
        const char* const names[3] = {".to_q.weight", ".to_k.weight", ".to_v.weight"};
        for (int k = 0; k < 3; ++k)
            if ((rc = launch_motion_pos_bias(ws.raw(at + names[k])->dev, C, C, F, k == 0 ? qs : 1.f, k == 0 ? C : 0, tab + k * C,
                                             3L * C, 0)))
                return rc;
        (a == 0 ? m->pb1 : m->pb2) = tab;
        if ((rc = ws.fold_ln(qkv, a == 0 ? m->ln1 : m->ln2, C, qs))) return rc;
    }
    if ((rc = ws.pack_geglu(b + ".ff.net.0.proj", &m->ff1))) return rc;
    if ((rc = ws.fold_ln(&m->ff1, m->ln3, 0, 1.0f))) return rc;
    return ws.pack_conv(b + ".ff.net.2", &m->ff2);
}

int MotionAdapter::finalize() {
    if (finalized) return 0;
    std::string missing;
    if (!ws.complete(&missing)) { set_error("motion adapter finalize: weight not set: " + missing); return 2; }
    const int nb = mcfg.num_blocks;
    int rc;
    down.assign((size_t)nb, {}); up.assign((size_t)nb, {});
    for (int i = 0; i < nb; ++i) {
        down[(size_t)i].resize((size_t)mcfg.layers_per_block);
        for (int j = 0; j < mcfg.layers_per_block; ++j)
            if ((rc = pack_module("down_blocks." + std::to_string(i) + ".motion_modules." + std::to_string(j), mcfg.num_heads[i],
                                  &down[(size_t)i][(size_t)j])))
                return rc;
    }
    if (mcfg.use_mid_block && (rc = pack_module("mid_block.motion_modules.0", mcfg.num_heads[nb - 1], &mid))) return rc;
    for (int i = 0; i < nb; ++i) {
        up[(size_t)i].resize((size_t)mcfg.layers_per_block + 1);
        for (int j = 0; j < mcfg.layers_per_block + 1; ++j)
            if ((rc = pack_module("up_blocks." + std::to_string(i) + ".motion_modules." + std::to_string(j),
                                  mcfg.num_heads[nb - 1 - i], &up[(size_t)i][(size_t)j])))
                return rc;
    }
    SD_HIP_CHECK(hipDeviceSynchronize());
    ws.free_raw();
    finalized = true;
    return 0;
}

void op_temporal_attention(Ctx& c, View qkv, const float* bias, View out, int V, int F, int HW, int heads, int d) {
    if (c.dry || c.err) return;
    const int C = heads * d;
    if (prof_enabled()) {
        static thread_local char name[40];
        snprintf(name, sizeof(name), "temporal_attn_kernel<%d,%d>", d, F <= 16 ? 1 : 2);
        prof_open(c.stream, name, 4.0 * V * HW * heads * (double)F * F * d, 2.0 * V * F * (double)HW * 4 * C);
    }
    c.err = launch_temporal_attention(qkv.p, qkv.p + C, qkv.p + 2 * C, out.p, bias, qkv.ld, qkv.ld, qkv.ld, out.ld, 3L * C, V, F, HW,
                                      heads, d, 1, c.stream);
    prof_close(c.stream);
}

void run_motion(Ctx& c, const MotionModule& m, View x, int N, int F, int H, int W, View out, const GnOut& out_stats, int G_out) {
    Arena& a = *c.arena;
    const size_t mk = a.mark();
    const int C = m.C, T = H * W, V = N / F, d = C / m.heads;
    const long M = (long)N * T;
    View hn(a.alloc_h(M * C), C, C);
    // statistics over a group's channels and all F H W positions of one video: V images of F T pixels.  (The summaries
    // the producer of x left are per frame; this norm runs its own statistics pass.)
    op_groupnorm(c, m.gn, x, hn, V, (long)F * T, 32, 1e-6f, 0, nullptr);
    View cur(a.alloc_h(M * C), C, C), t2(a.alloc_h(M * C), C, C), t3(a.alloc_h(M * C), C, C);
    RowStat st_cur, st_t2, st_t3;
    st_cur.p = a.alloc_f(rowstat_floats(M, C));
    st_t2.p = a.alloc_f(rowstat_floats(M, C));
    st_t3.p = a.alloc_f(rowstat_floats(M, C));
    ConvArgs f_cur, f_t2, f_t3, f_ln1, f_ln2, f_ln3;
    f_cur.stat_out = &st_cur; f_t2.stat_out = &st_t2; f_t3.stat_out = &st_t3;
    f_ln1.ln_in = &st_cur; f_ln2.ln_in = &st_t2; f_ln3.ln_in = &st_t3;
    f_ln1.ln_eps = f_ln2.ln_eps = f_ln3.ln_eps = 1e-5f;
    f_ln3.geglu = 1;
    op_conv(c, m.pin, hn, N, H, W, cur, f_cur);
    View qkv(a.alloc_h(M * 3 * C), 3 * C, 3 * C), att(a.alloc_h(M * C), C, C);
    op_conv(c, m.qkv1, cur, N, H, W, qkv, f_ln1);
    op_temporal_attention(c, qkv, m.pb1, att, V, F, T, m.heads, d);
    op_conv(c, m.out1, att, N, H, W, t2, conv_res(cur, f_t2));
    op_conv(c, m.qkv2, t2, N, H, W, qkv, f_ln2);
    op_temporal_attention(c, qkv, m.pb2, att, V, F, T, m.heads, d);
    op_conv(c, m.out2, att, N, H, W, t3, conv_res(t2, f_t3));
    View g(a.alloc_h(M * 4 * C), 4 * C, 4 * C);
    op_conv(c, m.ff1, t3, N, H, W, g, f_ln3);
    op_conv(c, m.ff2, g, N, H, W, cur, conv_res(t3));
    // the module's last launch writes the caller's view (a skip, a concatenation's hidden half) and leaves the GroupNorm
    // summaries of what it wrote for the resnet that reads it next
    ConvArgs fo;
    gn_out_resolve(c, out_stats, T, C, G_out, &fo);
    op_conv(c, m.pout, cur, N, H, W, out, conv_res(x, fo));
    a.release(mk);
}

}  // namespace sd
