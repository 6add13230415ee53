// CLIP vision tower graph (transformers CLIPVisionModelWithProjection) on the gfx950 kernels: the image side of an
// IP-Adapter prompt.  One launch builds the embeddings from the NCHW pixels (vit.hip), pre_layrnorm writes
// hidden_states[0], the layer stack is the text encoder's (run_clip_layers) without the causal mask, and the head is
// post_layernorm of the class token followed by visual_projection.
//
// Head dims the attention kernels lack (ViT-bigG/14: 1664 / 16 = 104) are handled at pack time: every head's q / k / v
// rows and biases are zero-padded to the next supported dim, out_proj's columns likewise, and softmax's
// log2(e) / sqrt(d_true) is folded into the query rows so the attention runs `prescaled` at the padded dim.  Padded
// query / key columns add 0 to every score and padded value columns produce 0, which out_proj's zero columns ignore.
#include <algorithm>
#include <cmath>

#include "model.h"

namespace sd {

namespace {
std::string vkey(int i, const char* rest) { return "vision_model.encoder.layers." + std::to_string(i) + "." + rest; }
long round_up(long a, long b) { return (a + b - 1) / b * b; }

int upload_bias(WeightStore& ws, const std::vector<float>& host, float** dst) {
    const long padded = round_up((long)host.size(), kWeightRowPad);
    std::vector<float> buf((size_t)padded, 0.f);
    std::copy(host.begin(), host.end(), buf.begin());
    *dst = static_cast<float*>(ws.dmalloc((size_t)padded * sizeof(float)));
    if (!*dst) { set_error("hipMalloc failed (bias)"); return 3; }
    SD_HIP_CHECK(hipMemcpy(*dst, buf.data(), (size_t)padded * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int host_bias(const WeightStore& ws, const std::string& key, int n, std::vector<float>* out) {
    const RawTensor* t = ws.raw(key);
    if (!t || t->numel != n) { set_error("missing weight: " + key); return 2; }
    std::vector<half_t> h((size_t)n);
    SD_HIP_CHECK(hipMemcpy(h.data(), t->dev, (size_t)n * sizeof(half_t), hipMemcpyDeviceToHost));
    out->resize((size_t)n);
    for (int i = 0; i < n; ++i) (*out)[(size_t)i] = (float)h[(size_t)i];
    return 0;
}
}  // namespace

int clip_vision_padded_head_dim(int d) {
    if (d <= 0) return 0;
    if (attention_supported(d)) return d;
    for (int p = d + 1; p <= 128; ++p)
        if (attention_supported(p)) return p;
    return 0;
}

CLIPVision::CLIPVision(const sd_clip_vision_config& c) : cfg(c) {
    const int H = cfg.hidden_size, I = cfg.intermediate_size, P = cfg.patch_size, G = cfg.image_size / cfg.patch_size;
    tokens = 1 + G * G;
    d = H / cfg.num_heads;
    dp = clip_vision_padded_head_dim(d);
    ws.declare("vision_model.embeddings.class_embedding", {H});
    ws.declare("vision_model.embeddings.patch_embedding.weight", {H, 3, P, P});
    ws.declare("vision_model.embeddings.position_embedding.weight", {tokens, H});
    ws.declare("vision_model.pre_layrnorm.weight", {H});
    ws.declare("vision_model.pre_layrnorm.bias", {H});
    for (int i = 0; i < cfg.num_layers; ++i) {
        for (const char* n : {"self_attn.k_proj", "self_attn.v_proj", "self_attn.q_proj", "self_attn.out_proj"}) {
            ws.declare(vkey(i, n) + ".weight", {H, H});
            ws.declare(vkey(i, n) + ".bias", {H});
        }
        ws.declare(vkey(i, "layer_norm1.weight"), {H});
        ws.declare(vkey(i, "layer_norm1.bias"), {H});
        ws.declare(vkey(i, "mlp.fc1.weight"), {I, H});
        ws.declare(vkey(i, "mlp.fc1.bias"), {I});
        ws.declare(vkey(i, "mlp.fc2.weight"), {H, I});
        ws.declare(vkey(i, "mlp.fc2.bias"), {H});
        ws.declare(vkey(i, "layer_norm2.weight"), {H});
        ws.declare(vkey(i, "layer_norm2.bias"), {H});
    }
    ws.declare("vision_model.post_layernorm.weight", {H});
    ws.declare("vision_model.post_layernorm.bias", {H});
    ws.declare("visual_projection.weight", {cfg.projection_dim, H});
}

// The attention linears of layer i with every head at dp columns: the fused [q | k | v] matrix ([3 heads dp][H]) and
// out_proj ([H][heads dp]), both zero-filled up to the packed sizes (rows to kWeightRowPad, K to 64).
int CLIPVision::pack_attn(int i, ClipLayer* l) {
    const int H = cfg.hidden_size, heads = cfg.num_heads;
    const int A = heads * dp;
    const long Kq = round_up(H, 64), Ko = round_up(A, 64);
    const bool padded = dp != d;
    const float qs = 1.4426950408889634f / sqrtf((float)d);

    ConvW& q = l->qkv;
    const long qrows = round_up(3L * A, kWeightRowPad);
    q.cin = H; q.cout = 3 * A; q.ks = 1; q.K = Kq;
    q.w = static_cast<half_t*>(ws.dmalloc((size_t)qrows * Kq * sizeof(half_t)));
    if (!q.w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(q.w, 0, (size_t)qrows * Kq * sizeof(half_t), 0));
    std::vector<float> qb((size_t)3 * A, 0.f), b;
    const char* names[3] = {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"};
    for (int j = 0; j < 3; ++j) {
        const RawTensor* w = ws.raw(vkey(i, names[j]) + ".weight");
        if (!w) { set_error("missing weight: " + vkey(i, names[j]) + ".weight"); return 2; }
        int rc = host_bias(ws, vkey(i, names[j]) + ".bias", H, &b);
        if (rc) return rc;
        for (int h = 0; h < heads; ++h) {
            // head h: d rows of H values each, into rows [j A + h dp, + d) of the packed matrix
            SD_HIP_CHECK(hipMemcpy2DAsync(q.w + ((long)j * A + (long)h * dp) * Kq, (size_t)Kq * sizeof(half_t),
                                          w->dev + (long)h * d * H, (size_t)H * sizeof(half_t), (size_t)H * sizeof(half_t),
                                          (size_t)d, hipMemcpyDeviceToDevice, 0));
            for (int e = 0; e < d; ++e)
                qb[(size_t)j * A + (size_t)h * dp + e] = b[(size_t)h * d + e] * (padded && j == 0 ? qs : 1.f);
        }
    }
    // one more fp16 rounding of the query rows, as for the UNet's pre-scaled projections
    if (padded) { int rc = launch_scale_f16(q.w, (long)A * Kq, qs, 0); if (rc) return rc; }
    int rc = upload_bias(ws, qb, &q.bias);
    if (rc) return rc;

    ConvW& o = l->out;
    const RawTensor* w = ws.raw(vkey(i, "self_attn.out_proj.weight"));
    if (!w) { set_error("missing weight: " + vkey(i, "self_attn.out_proj.weight")); return 2; }
    const long orows = round_up(H, kWeightRowPad);
    o.cin = A; o.cout = H; o.ks = 1; o.K = Ko;
    o.w = static_cast<half_t*>(ws.dmalloc((size_t)orows * Ko * sizeof(half_t)));
    if (!o.w) { set_error("hipMalloc failed (weights)"); return 3; }
    SD_HIP_CHECK(hipMemsetAsync(o.w, 0, (size_t)orows * Ko * sizeof(half_t), 0));
    for (int h = 0; h < heads; ++h)
        SD_HIP_CHECK(hipMemcpy2DAsync(o.w + (long)h * dp, (size_t)Ko * sizeof(half_t), w->dev + (long)h * d,
                                      (size_t)H * sizeof(half_t), (size_t)d * sizeof(half_t), (size_t)H,
                                      hipMemcpyDeviceToDevice, 0));
    if ((rc = host_bias(ws, vkey(i, "self_attn.out_proj.bias"), H, &b))) return rc;
    return upload_bias(ws, b, &o.bias);
}

int CLIPVision::finalize() {
    if (finalized) return 0;
    std::string missing;
    if (!ws.complete(&missing)) { set_error("finalize: weight not set: " + missing); return 2; }
    auto keep = [&](const std::string& key, half_t** dst) -> int {
        const RawTensor* r = ws.raw(key);
        if (!r) { set_error("missing weight: " + key); return 2; }
        *dst = static_cast<half_t*>(ws.dmalloc((size_t)r->numel * sizeof(half_t)));
        if (!*dst) { set_error("hipMalloc failed"); return 3; }
        SD_HIP_CHECK(hipMemcpy(*dst, r->dev, (size_t)r->numel * sizeof(half_t), hipMemcpyDeviceToDevice));
        return 0;
    };
    int rc;
    if ((rc = keep("vision_model.embeddings.class_embedding", &cls))) return rc;
    if ((rc = keep("vision_model.embeddings.patch_embedding.weight", &patch))) return rc;
    if ((rc = keep("vision_model.embeddings.position_embedding.weight", &pos))) return rc;
    if ((rc = keep("visual_projection.weight", &proj))) return rc;
    if ((rc = ws.pack_norm("vision_model.pre_layrnorm", &pre_ln))) return rc;
    layers.assign((size_t)cfg.num_layers, ClipLayer());
    for (int i = 0; i < cfg.num_layers; ++i) {
        ClipLayer& l = layers[(size_t)i];
        if ((rc = ws.pack_norm(vkey(i, "layer_norm1"), &l.ln1))) return rc;
        if ((rc = pack_attn(i, &l))) return rc;
        if ((rc = ws.pack_norm(vkey(i, "layer_norm2"), &l.ln2))) return rc;
        if ((rc = ws.pack_conv(vkey(i, "mlp.fc1"), &l.fc1))) return rc;
        if ((rc = ws.pack_conv(vkey(i, "mlp.fc2"), &l.fc2))) return rc;
    }
    if ((rc = ws.pack_norm("vision_model.post_layernorm", &post_ln))) return rc;
    SD_HIP_CHECK(hipDeviceSynchronize());
    ws.free_raw();
    finalized = true;
    return 0;
}

int CLIPVision::run(Ctx& c, const half_t* pixels, half_t* hidden_states, half_t* last_hidden, half_t* pooled,
                    half_t* image_embeds, int B) {
    Arena& a = *c.arena;
    const int H = cfg.hidden_size, L = cfg.num_layers, T = tokens;
    const long M = (long)B * T;
    hipStream_t s = c.stream;
    const bool go = !c.dry;

    // residual stream: the caller's hidden_states slabs, or two ping-pong buffers (the last layer writes last_hidden
    // itself when that is asked for without the slabs)
    half_t* pp[2] = {nullptr, nullptr};
    if (!hidden_states) { pp[0] = a.alloc_h(M * H); pp[1] = a.alloc_h(M * H); }
    std::function<half_t*(int)> slab = [&](int l) -> half_t* {
        if (hidden_states) return hidden_states + (long)l * M * H;
        if (l == L && last_hidden) return last_hidden;
        return pp[l & 1];
    };

    half_t* emb = a.alloc_h(M * H);
    if (go && !c.err) {
        prof_open(s, "vit_patch_embed_kernel", 2.0 * B * (T - 1) * (double)H * 3 * cfg.patch_size * cfg.patch_size,
                  2.0 * ((double)B * 3 * cfg.image_size * cfg.image_size + M * (double)H));
        c.err = launch_vit_patch_embed(pixels, patch, cls, pos, emb, H, B, cfg.image_size, cfg.patch_size, H, s);
        prof_close(s);
    }
    op_layernorm(c, pre_ln, View(emb, H, H), View(slab(0), H, H), M, cfg.layer_norm_eps);

    ClipStack g;
    g.H = H; g.I = cfg.intermediate_size; g.heads = cfg.num_heads; g.d = dp;
    g.act = cfg.hidden_act == 0 ? 1 : 2;
    g.eps = cfg.layer_norm_eps;
    g.causal = 0;
    g.prescaled = dp != d ? 1 : 0;
    run_clip_layers(c, layers, g, slab, B, T);

    if (hidden_states && last_hidden && go && !c.err) {
        hipError_t e = hipMemcpyAsync(last_hidden, slab(L), (size_t)M * H * sizeof(half_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { set_error(std::string("clip_vision: hipMemcpyAsync: ") + hipGetErrorString(e)); c.err = 3; }
    }
    if (pooled || image_embeds) {
        // pooler_output = post_layernorm(last_hidden[:, 0]): one row per image, T rows apart
        half_t* p16 = pooled ? pooled : a.alloc_h((long)B * H);
        op_layernorm(c, post_ln, View(slab(L), (long)T * H, H), View(p16, H, H), B, cfg.layer_norm_eps);
        if (image_embeds) {
            float* p32 = a.alloc_f((long)B * H);
            float* e32 = a.alloc_f((long)B * cfg.projection_dim);
            if (go && !c.err) c.err = launch_f16_to_f32(p16, p32, (long)B * H, s);
            if (go && !c.err) c.err = launch_small_linear(p32, H, proj, nullptr, e32, cfg.projection_dim, B, H,
                                                          cfg.projection_dim, 0, 0, s);
            if (go && !c.err) c.err = launch_f32_to_f16(e32, image_embeds, (long)B * cfg.projection_dim, s);
        }
    }
    return c.err;
}

int CLIPVision::forward(const half_t* pixels, half_t* hidden_states, half_t* last_hidden, half_t* pooled,
                        half_t* image_embeds, int B, hipStream_t stream) {
    if (!finalized) { set_error("clip_vision: forward before finalize"); return 2; }
    if (B <= 0) { set_error("clip_vision: bad batch size"); return 1; }
    const long key = ((long)B << 8) ^ (hidden_states ? 1 : 0) ^ (last_hidden ? 2 : 0) ^ (pooled ? 4 : 0) ^
                     (image_embeds ? 8 : 0);
    return plan_and_run(arena, stream, planned_key, key, "clip_vision", [&](Ctx& c) {
        return run(c, pixels, hidden_states, last_hidden, pooled, image_embeds, B);
    });
}

}  // namespace sd
