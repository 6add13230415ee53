// UNet2DConditionModel graph on the gfx950 kernels.
//
// What it computes: diffusers 0.27.2 UNet2DConditionModel.forward as the reference calls it at
// /root/reference/pipelines/sd_unified_pipeline.py:475-482 (structure: SURVEY.md §3.3; weight names:
// /root/reference/scripts/convert_from_A1111.py:283-441).  How it runs is native to MI355X:
// NHWC fp16 activations, skip connections written straight into the concatenation buffers of the
// up path (no torch.cat copies), fused qkv / GEGLU / residual / time-embedding epilogues, one
// stacked GEMV for all 22 time_emb_proj layers, and a stack-discipline workspace arena.
#include <algorithm>
#include <vector>

#include "model.h"
#include <cmath>
#include <cstdlib>

namespace sd {

void declare_resnet(WeightStore& ws, const std::string& p, int cin, int cout, int temb) {
    ws.declare(p + ".norm1.weight", {cin});
    ws.declare(p + ".norm1.bias", {cin});
    ws.declare(p + ".conv1.weight", {cout, cin, 3, 3});
    ws.declare(p + ".conv1.bias", {cout});
    if (temb) {
        ws.declare(p + ".time_emb_proj.weight", {cout, temb});
        ws.declare(p + ".time_emb_proj.bias", {cout});
    }
    ws.declare(p + ".norm2.weight", {cout});
    ws.declare(p + ".norm2.bias", {cout});
    ws.declare(p + ".conv2.weight", {cout, cout, 3, 3});
    ws.declare(p + ".conv2.bias", {cout});
    if (cin != cout) {
        ws.declare(p + ".conv_shortcut.weight", {cout, cin, 1, 1});
        ws.declare(p + ".conv_shortcut.bias", {cout});
    }
}

namespace {

void declare_xformer(WeightStore& ws, const std::string& p, int c, int depth, int ctx, bool linear) {
    ws.declare(p + ".norm.weight", {c});
    ws.declare(p + ".norm.bias", {c});
    if (linear) ws.declare(p + ".proj_in.weight", {c, c}); else ws.declare(p + ".proj_in.weight", {c, c, 1, 1});
    ws.declare(p + ".proj_in.bias", {c});
    for (int d = 0; d < depth; ++d) {
        const std::string b = p + ".transformer_blocks." + std::to_string(d);
        ws.declare(b + ".norm1.weight", {c});
        ws.declare(b + ".norm1.bias", {c});
        ws.declare(b + ".attn1.to_q.weight", {c, c});
        ws.declare(b + ".attn1.to_k.weight", {c, c});
        ws.declare(b + ".attn1.to_v.weight", {c, c});
        ws.declare(b + ".attn1.to_out.0.weight", {c, c});
        ws.declare(b + ".attn1.to_out.0.bias", {c});
        ws.declare(b + ".norm2.weight", {c});
        ws.declare(b + ".norm2.bias", {c});
        ws.declare(b + ".attn2.to_q.weight", {c, c});
        ws.declare(b + ".attn2.to_k.weight", {c, ctx});
        ws.declare(b + ".attn2.to_v.weight", {c, ctx});
        ws.declare(b + ".attn2.to_out.0.weight", {c, c});
        ws.declare(b + ".attn2.to_out.0.bias", {c});
        ws.declare(b + ".norm3.weight", {c});
        ws.declare(b + ".norm3.bias", {c});
        ws.declare(b + ".ff.net.0.proj.weight", {8 * c, c});
        ws.declare(b + ".ff.net.0.proj.bias", {8 * c});
        ws.declare(b + ".ff.net.2.weight", {c, 4 * c});
        ws.declare(b + ".ff.net.2.bias", {c});
    }
    if (linear) ws.declare(p + ".proj_out.weight", {c, c}); else ws.declare(p + ".proj_out.weight", {c, c, 1, 1});
    ws.declare(p + ".proj_out.bias", {c});
}

}  // namespace

void Encoder::declare_encoder() {
    const int nb = cfg.num_blocks;
    const int* boc = cfg.block_out_channels;
    const int temb = boc[0] * 4;
    const int ctx = cfg.cross_attention_dim;
    const bool lin = cfg.use_linear_projection != 0;
    ws.declare("conv_in.weight", {boc[0], cfg.in_channels, 3, 3});
    ws.declare("conv_in.bias", {boc[0]});
    ws.declare("time_embedding.linear_1.weight", {temb, boc[0]});
    ws.declare("time_embedding.linear_1.bias", {temb});
    ws.declare("time_embedding.linear_2.weight", {temb, temb});
    ws.declare("time_embedding.linear_2.bias", {temb});
    if (cfg.time_cond_proj_dim > 0) ws.declare("time_embedding.cond_proj.weight", {boc[0], cfg.time_cond_proj_dim});
    if (cfg.addition_time_embed_dim > 0) {
        ws.declare("add_embedding.linear_1.weight", {temb, cfg.projection_class_embeddings_input_dim});
        ws.declare("add_embedding.linear_1.bias", {temb});
        ws.declare("add_embedding.linear_2.weight", {temb, temb});
        ws.declare("add_embedding.linear_2.bias", {temb});
    }
    int out_ch = boc[0];
    for (int i = 0; i < nb; ++i) {
        const int in_ch = out_ch;
        out_ch = boc[i];
        for (int j = 0; j < cfg.layers_per_block; ++j) {
            const std::string p = "down_blocks." + std::to_string(i);
            declare_resnet(ws, p + ".resnets." + std::to_string(j), j == 0 ? in_ch : out_ch, out_ch, temb);
            if (cfg.down_block_has_attn[i])
                declare_xformer(ws, p + ".attentions." + std::to_string(j), out_ch, cfg.transformer_layers[i], ctx, lin);
        }
        if (i != nb - 1) {
            ws.declare("down_blocks." + std::to_string(i) + ".downsamplers.0.conv.weight", {out_ch, out_ch, 3, 3});
            ws.declare("down_blocks." + std::to_string(i) + ".downsamplers.0.conv.bias", {out_ch});
        }
    }
    const int mid = boc[nb - 1];
    declare_resnet(ws, "mid_block.resnets.0", mid, mid, temb);
    declare_xformer(ws, "mid_block.attentions.0", mid, cfg.transformer_layers[nb - 1], ctx, lin);
    declare_resnet(ws, "mid_block.resnets.1", mid, mid, temb);
}

UNet::UNet(const sd_unet_config& c) : Encoder(c) {
    declare_encoder();
    const int nb = cfg.num_blocks;
    const int* boc = cfg.block_out_channels;
    const int temb = boc[0] * 4;
    const int ctx = cfg.cross_attention_dim;
    const bool lin = cfg.use_linear_projection != 0;
    int out_ch;
    out_ch = boc[nb - 1];
    for (int i = 0; i < nb; ++i) {
        const int prev = out_ch;
        out_ch = boc[nb - 1 - i];
        const int in_ch = boc[nb - 1 - (i + 1 < nb ? i + 1 : nb - 1)];
        const std::string p = "up_blocks." + std::to_string(i);
        for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
            const int skip = (j == cfg.layers_per_block) ? in_ch : out_ch;
            const int rin = (j == 0) ? prev : out_ch;
            declare_resnet(ws, p + ".resnets." + std::to_string(j), rin + skip, out_ch, temb);
            if (cfg.up_block_has_attn[i])
                declare_xformer(ws, p + ".attentions." + std::to_string(j), out_ch,
                                cfg.transformer_layers[nb - 1 - i], ctx, lin);
        }
        if (i != nb - 1) {
            ws.declare(p + ".upsamplers.0.conv.weight", {out_ch, out_ch, 3, 3});
            ws.declare(p + ".upsamplers.0.conv.bias", {out_ch});
        }
    }
    ws.declare("conv_norm_out.weight", {boc[0]});
    ws.declare("conv_norm_out.bias", {boc[0]});
    ws.declare("conv_out.weight", {cfg.out_channels, boc[0], 3, 3});
    ws.declare("conv_out.bias", {cfg.out_channels});
}

int Encoder::pack_resnet(const std::string& p, Resnet* r, std::vector<std::string>* tw, std::vector<std::string>* tb) {
    int rc;
    if ((rc = ws.pack_norm(p + ".norm1", &r->n1))) return rc;
    if ((rc = ws.pack_conv(p + ".conv1", &r->c1))) return rc;
    if ((rc = ws.pack_norm(p + ".norm2", &r->n2))) return rc;
    if ((rc = ws.pack_conv(p + ".conv2", &r->c2))) return rc;
    r->cin = r->c1.cin; r->cout = r->c1.cout;
    r->has_sc = ws.raw(p + ".conv_shortcut.weight") != nullptr;
    if (r->has_sc && (rc = ws.pack_conv(p + ".conv_shortcut", &r->sc))) return rc;
    if (tw) {
        r->temb_off = temb_total;
        temb_total += r->cout;
        tw->push_back(p + ".time_emb_proj.weight");
        tb->push_back(p + ".time_emb_proj.bias");
    }
    return 0;
}

int Encoder::pack_xformer(const std::string& p, Xformer* x, int heads, int depth) {
    int rc;
    if ((rc = ws.pack_norm(p + ".norm", &x->gn))) return rc;
    if ((rc = ws.pack_conv(p + ".proj_in", &x->pin))) return rc;
    if (depth == 0 && (rc = ws.pack_conv(p + ".proj_out", &x->pout))) return rc;
    x->C = x->pin.cout;
    x->heads = heads;
    x->blocks.resize((size_t)depth);
    for (int d = 0; d < depth; ++d) {
        TBlock& b = x->blocks[(size_t)d];
        const std::string q = p + ".transformer_blocks." + std::to_string(d);
        if ((rc = ws.pack_norm(q + ".norm1", &b.ln1))) return rc;
        if ((rc = ws.pack_norm(q + ".norm2", &b.ln2))) return rc;
        if ((rc = ws.pack_norm(q + ".norm3", &b.ln3))) return rc;
        if ((rc = ws.pack_rows({q + ".attn1.to_q.weight", q + ".attn1.to_k.weight", q + ".attn1.to_v.weight"}, {}, &b.qkv))) return rc;
        if ((rc = ws.pack_conv(q + ".attn1.to_out.0", &b.out1))) return rc;
        if ((rc = ws.pack_conv(q + ".attn2.to_q", &b.q2, false))) return rc;
        // fold softmax's log2(e)/sqrt(d) into both query projections (rows [0, C) of the fused q|k|v
        // matrix and all of attn2.to_q; neither has a bias): the attention kernel then runs its
        // `prescaled` path.  One extra fp16 rounding of weights that were fp16-rounded already.
        const float qs = 1.4426950408889634f / sqrtf((float)(x->C / heads));
        // text K/V projections depend only on encoder_hidden_states: all of them are stacked into
        // one GEMM (kv_all) issued once per forward instead of one small launch per block
        b.kv_off = kv_total;
        b.ip_kv_off = kv_total;          // IPAdapter::kv_all stacks its sites in this same order and width
        kv_total += 2 * x->C;
        kv_keys.push_back(q + ".attn2.to_k.weight");
        kv_keys.push_back(q + ".attn2.to_v.weight");
        if ((rc = ws.pack_conv(q + ".attn2.to_out.0", &b.out2))) return rc;
        if ((rc = ws.pack_geglu(q + ".ff.net.0.proj", &b.ff1))) return rc;
        const bool last = d + 1 == depth;
        if (!last && (rc = ws.pack_conv(q + ".ff.net.2", &b.ff2))) return rc;
        // The three LayerNorms feed one linear each (norm1 -> q|k|v, norm2 -> attn2.to_q, norm3 -> the GEGLU
        // projection): their affine is folded into those weights here and their statistics come out of the
        // epilogue of the GEMM that produces the normalised tensor, so a forward launches no LayerNorm
        // kernel (48 launches, 0.55 ms of the C2 forward in round 1).  SD_NO_LN_FOLD=1 keeps the kernels.
        static const bool no_fold = getenv("SD_NO_LN_FOLD") != nullptr;
        b.fold = !no_fold;
        if (b.fold) {
            if ((rc = ws.fold_ln(&b.qkv, b.ln1, x->C, qs))) return rc;
            if ((rc = ws.fold_ln(&b.q2, b.ln2, x->C, qs))) return rc;
            if ((rc = ws.fold_ln(&b.ff1, b.ln3, 0, 1.0f))) return rc;
        } else {
            if ((rc = launch_scale_f16(b.qkv.w, (long)x->C * b.qkv.K, qs, 0))) return rc;
            if ((rc = launch_scale_f16(b.q2.w, (long)x->C * b.q2.K, qs, 0))) return rc;
        }
        if (last && (rc = pack_xformer_tail(ws, p + ".proj_out", q + ".ff.net.2", x, &b))) return rc;
    }
    return 0;
}

// proj_out follows the last block's ff.net.2 with nothing but that linear's residual in between:
//     out = proj_out(ff2(g) + b_ff2 + t3) + b_po + x = [g | t3] [W_po W_ff2 | W_po]^T + (W_po b_ff2 + b_po) + x
// so the two launches become one with K = hidden + C: same FLOPs and weight bytes, one launch and one round trip of an
// [M, C] tensor (and its fp16 rounding) less.  Kept as two launches where ffn.hip can take the feed-forward (its kernel
// has no proj_out slabs), with the LayerNorm fold off, and under SD_NO_POUT_FOLD=1 (the A/B switch).
int pack_xformer_tail(WeightStore& ws, const std::string& proj_out, const std::string& ff2, Xformer* x, TBlock* last) {
    static const bool off = getenv("SD_NO_POUT_FOLD") != nullptr;
    const RawTensor* w2 = ws.raw(ff2 + ".weight");
    const RawTensor* wo = ws.raw(proj_out + ".weight");
    const int C = x->C;
    const long hidden = w2 && w2->shape.size() == 2 ? w2->shape[1] : 0;
    x->pout_fold = !off && last->fold && w2 && wo && hidden > 0 && w2->shape[0] == C && wo->shape[0] == C && wo->shape[1] == C &&
                   (hidden + C) % 64 == 0 && last->ff1.cout == 2 * hidden && !ffn_fused_width(C, (int)hidden);
    if (x->pout_fold) return ws.fold_linear(proj_out, ff2, &x->ff2p);
    int rc;
    if ((rc = ws.pack_conv(ff2, &last->ff2))) return rc;
    return ws.pack_conv(proj_out, &x->pout);
}

int Encoder::pack_encoder(std::vector<std::string>* tw, std::vector<std::string>* tb) {
    const int nb = cfg.num_blocks;
    int rc;
    if ((rc = ws.pack_conv("conv_in", &conv_in))) return rc;
    if ((rc = ws.pack_conv("time_embedding.linear_1", &te1))) return rc;
    if ((rc = ws.pack_conv("time_embedding.linear_2", &te2))) return rc;
    if (cfg.time_cond_proj_dim > 0 && (rc = ws.pack_conv("time_embedding.cond_proj", &tcp, false))) return rc;
    if (cfg.addition_time_embed_dim > 0) {
        if ((rc = ws.pack_conv("add_embedding.linear_1", &ae1))) return rc;
        if ((rc = ws.pack_conv("add_embedding.linear_2", &ae2))) return rc;
    }
    down_res.assign((size_t)nb, {}); down_att.assign((size_t)nb, {}); down_ds.assign((size_t)nb, ConvW());
    for (int i = 0; i < nb; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        down_res[i].resize((size_t)cfg.layers_per_block);
        if (cfg.down_block_has_attn[i]) down_att[i].resize((size_t)cfg.layers_per_block);
        for (int j = 0; j < cfg.layers_per_block; ++j) {
            if ((rc = pack_resnet(p + ".resnets." + std::to_string(j), &down_res[i][j], tw, tb))) return rc;
            if (cfg.down_block_has_attn[i] &&
                (rc = pack_xformer(p + ".attentions." + std::to_string(j), &down_att[i][j], cfg.num_heads[i],
                                   cfg.transformer_layers[i]))) return rc;
        }
        if (i != nb - 1 && (rc = ws.pack_conv(p + ".downsamplers.0.conv", &down_ds[i]))) return rc;
    }
    if ((rc = pack_resnet("mid_block.resnets.0", &mid_r0, tw, tb))) return rc;
    if ((rc = pack_xformer("mid_block.attentions.0", &mid_att, cfg.num_heads[nb - 1], cfg.transformer_layers[nb - 1]))) return rc;
    if ((rc = pack_resnet("mid_block.resnets.1", &mid_r1, tw, tb))) return rc;
    return 0;
}

int UNet::finalize() {
    if (finalized) return 0;
    std::string missing;
    if (!ws.complete(&missing)) { set_error("finalize: weight not set: " + missing); return 2; }
    const int nb = cfg.num_blocks;
    int rc;
    std::vector<std::string> tw, tb;
    temb_total = 0;
    kv_total = 0;
    kv_keys.clear();
    if ((rc = pack_encoder(&tw, &tb))) return rc;
    up_res.assign((size_t)nb, {}); up_att.assign((size_t)nb, {}); up_us.assign((size_t)nb, ConvW());
    for (int i = 0; i < nb; ++i) {
        const std::string p = "up_blocks." + std::to_string(i);
        up_res[i].resize((size_t)cfg.layers_per_block + 1);
        if (cfg.up_block_has_attn[i]) up_att[i].resize((size_t)cfg.layers_per_block + 1);
        for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
            if ((rc = pack_resnet(p + ".resnets." + std::to_string(j), &up_res[i][j], &tw, &tb))) return rc;
            if (cfg.up_block_has_attn[i] &&
                (rc = pack_xformer(p + ".attentions." + std::to_string(j), &up_att[i][j], cfg.num_heads[nb - 1 - i],
                                   cfg.transformer_layers[nb - 1 - i]))) return rc;
        }
        if (i != nb - 1 && (rc = ws.pack_conv(p + ".upsamplers.0.conv", &up_us[i], true, true))) return rc;
    }
    if ((rc = ws.pack_norm("conv_norm_out", &norm_out))) return rc;
    if ((rc = ws.pack_conv("conv_out", &conv_out))) return rc;
    if ((rc = ws.pack_rows(tw, tb, &temb_stack))) return rc;
    if (!kv_keys.empty() && (rc = ws.pack_rows(kv_keys, {}, &kv_all))) return rc;
    kv_keys.clear();
    SD_HIP_CHECK(hipDeviceSynchronize());
    ws.free_raw();
    finalized = true;
    int site = 0;
    for (auto& st : xformer_sites()) { st.second->tome_site0 = site; site += (int)st.second->blocks.size(); }
    return 0;
}

// ------------------------------------------------------------------------------------------ IP-Adapter
std::vector<std::pair<std::string, int>> unet_xattn_sites(const sd_unet_config& cfg, bool mid_last) {
    const int nb = cfg.num_blocks;
    const int* boc = cfg.block_out_channels;
    std::vector<std::pair<std::string, int>> down, up, mid;
    auto add = [](std::vector<std::pair<std::string, int>>& v, const std::string& p, int depth, int C) {
        for (int k = 0; k < depth; ++k) v.emplace_back(p + ".transformer_blocks." + std::to_string(k), C);
    };
    for (int i = 0; i < nb; ++i)
        if (cfg.down_block_has_attn[i])
            for (int j = 0; j < cfg.layers_per_block; ++j)
                add(down, "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), cfg.transformer_layers[i], boc[i]);
    add(mid, "mid_block.attentions.0", cfg.transformer_layers[nb - 1], boc[nb - 1]);
    for (int i = 0; i < nb; ++i)
        if (cfg.up_block_has_attn[i])
            for (int j = 0; j < cfg.layers_per_block + 1; ++j)
                add(up, "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j),
                    cfg.transformer_layers[nb - 1 - i], boc[nb - 1 - i]);
    std::vector<std::pair<std::string, int>> all = down;
    const auto& second = mid_last ? up : mid;
    const auto& third = mid_last ? mid : up;
    all.insert(all.end(), second.begin(), second.end());
    all.insert(all.end(), third.begin(), third.end());
    return all;
}

namespace {
const char* kIpProj = "encoder_hid_proj.image_projection_layers.0";
std::string rs_layer_key(int i, const char* rest) { return std::string(kIpProj) + ".layers." + std::to_string(i) + "." + rest; }
}

IPAdapter::IPAdapter(const sd_unet_config& c, const sd_ip_projection_config& p)
    : cfg(c), kind(p.kind), d_img(p.image_embed_dim), n_tok(p.num_tokens) {
    const int ctx = cfg.cross_attention_dim;
    const std::string pre = kIpProj;
    if (kind == SD_IP_PROJ_RESAMPLER) {
        dim = p.dim; heads = p.heads; depth = p.depth; ff_mult = p.ff_mult;
        const int64_t A = (int64_t)heads * 64, F = (int64_t)ff_mult * dim;
        // the original file's names under the diffusers prefix (stablediffusion_amd/ip_adapter.py)
        ws.declare(pre + ".latents", {1, n_tok, dim});
        ws.declare(pre + ".proj_in.weight", {dim, d_img});
        ws.declare(pre + ".proj_in.bias", {dim});
        ws.declare(pre + ".proj_out.weight", {ctx, dim});
        ws.declare(pre + ".proj_out.bias", {ctx});
        ws.declare(pre + ".norm_out.weight", {ctx});
        ws.declare(pre + ".norm_out.bias", {ctx});
        for (int i = 0; i < depth; ++i) {
            for (const char* n : {"0.norm1", "0.norm2"}) {
                ws.declare(rs_layer_key(i, n) + ".weight", {dim});
                ws.declare(rs_layer_key(i, n) + ".bias", {dim});
            }
            ws.declare(rs_layer_key(i, "0.to_q.weight"), {A, dim});
            ws.declare(rs_layer_key(i, "0.to_kv.weight"), {2 * A, dim});
            ws.declare(rs_layer_key(i, "0.to_out.weight"), {dim, A});
            ws.declare(rs_layer_key(i, "1.0.weight"), {dim});
            ws.declare(rs_layer_key(i, "1.0.bias"), {dim});
            ws.declare(rs_layer_key(i, "1.1.weight"), {F, dim});
            ws.declare(rs_layer_key(i, "1.3.weight"), {dim, F});
        }
    } else {
        ws.declare(pre + ".image_embeds.weight", {(int64_t)n_tok * ctx, d_img});
        ws.declare(pre + ".image_embeds.bias", {(int64_t)n_tok * ctx});
        ws.declare(pre + ".norm.weight", {ctx});
        ws.declare(pre + ".norm.bias", {ctx});
    }
    for (const auto& site : unet_xattn_sites(cfg, true)) {
        ws.declare(site.first + ".attn2.processor.to_k_ip.0.weight", {site.second, ctx});
        ws.declare(site.first + ".attn2.processor.to_v_ip.0.weight", {site.second, ctx});
    }
}

int IPAdapter::finalize() {
    if (finalized) return 0;
    std::string missing;
    if (!ws.complete(&missing)) { set_error("ip adapter finalize: weight not set: " + missing); return 2; }
    const std::string p = kIpProj;
    int rc;
    if (kind == SD_IP_PROJ_RESAMPLER) {
        const RawTensor* lt = ws.raw(p + ".latents");
        if (!lt) { set_error("missing weight: " + p + ".latents"); return 2; }
        latents = static_cast<half_t*>(ws.dmalloc((size_t)lt->numel * sizeof(half_t)));
        if (!latents) { set_error("hipMalloc failed"); return 3; }
        SD_HIP_CHECK(hipMemcpy(latents, lt->dev, (size_t)lt->numel * sizeof(half_t), hipMemcpyDeviceToDevice));
        if ((rc = ws.pack_conv(p + ".proj_in", &proj_in))) return rc;
        if ((rc = ws.pack_conv(p + ".proj_out", &proj_out))) return rc;
        if ((rc = ws.pack_norm(p + ".norm_out", &norm))) return rc;
        layers.assign((size_t)depth, ResamplerLayer());
        // softmax's log2(e) / sqrt(64) goes into the query rows, as in the UNet's projections (pack_xformer)
        const float qs = 1.4426950408889634f / 8.0f;
        for (int i = 0; i < depth; ++i) {
            ResamplerLayer& l = layers[(size_t)i];
            if ((rc = ws.pack_norm(rs_layer_key(i, "0.norm1"), &l.norm1))) return rc;
            if ((rc = ws.pack_norm(rs_layer_key(i, "0.norm2"), &l.norm2))) return rc;
            if ((rc = ws.pack_conv(rs_layer_key(i, "0.to_q"), &l.to_q, false))) return rc;
            if ((rc = launch_scale_f16(l.to_q.w, (long)l.to_q.cout * l.to_q.K, qs, 0))) return rc;
            if ((rc = ws.pack_conv(rs_layer_key(i, "0.to_kv"), &l.to_kv, false))) return rc;
            if ((rc = ws.pack_conv(rs_layer_key(i, "0.to_out"), &l.to_out, false))) return rc;
            if ((rc = ws.pack_norm(rs_layer_key(i, "1.0"), &l.ff_ln))) return rc;
            if ((rc = ws.pack_conv(rs_layer_key(i, "1.1"), &l.ff1, false))) return rc;
            if ((rc = ws.pack_conv(rs_layer_key(i, "1.3"), &l.ff2, false))) return rc;
        }
    } else {
        if ((rc = ws.pack_conv(p + ".image_embeds", &proj))) return rc;
        if ((rc = ws.pack_norm(p + ".norm", &norm))) return rc;
    }
    // stacked in the UNet's kv_all order, so that a block's ip_kv_off equals its kv_off
    std::vector<std::string> keys;
    kv_total = 0;
    for (const auto& site : unet_xattn_sites(cfg, false)) {
        keys.push_back(site.first + ".attn2.processor.to_k_ip.0.weight");
        keys.push_back(site.first + ".attn2.processor.to_v_ip.0.weight");
        kv_total += 2 * site.second;
    }
    if ((rc = ws.pack_rows(keys, {}, &kv_all))) return rc;
    SD_HIP_CHECK(hipDeviceSynchronize());
    ws.free_raw();
    finalized = true;
    return 0;
}

void IPAdapter::run_tokens(Ctx& c, const half_t* image_embeds, long rows, half_t* tok) {
    Arena& a = *c.arena;
    hipStream_t s = c.stream;
    const bool go = !c.dry;
    const int ctx = cfg.cross_attention_dim;
    if (kind != SD_IP_PROJ_RESAMPLER) {
        const long ntc = (long)n_tok * ctx;
        float* e32 = a.alloc_f(rows * d_img);
        float* p32 = a.alloc_f(rows * ntc);
        half_t* p16 = a.alloc_h(rows * ntc);
        if (go && !c.err) c.err = launch_f16_to_f32(image_embeds, e32, rows * d_img, s);
        if (go && !c.err) {
            prof_open(s, "small_linear_kernel", 2.0 * rows * ntc * d_img, 2.0 * ntc * d_img);
            c.err = launch_small_linear(e32, d_img, proj.w, proj.bias, p32, ntc, (int)rows, d_img, (int)ntc, 0, 0, s);
            prof_close(s);
        }
        if (go && !c.err) c.err = launch_f32_to_f16(p32, p16, rows * ntc, s);
        op_layernorm(c, norm, View(p16, ctx, ctx), View(tok, ctx, ctx), rows * n_tok, 1e-5f);
        return;
    }
    // ---- Resampler: R = rows images, T features and n_tok latents each.  Per layer 10 launches: 3 LayerNorms, to_q and
    //      to_kv of the latents, to_kv of the features (to_kv is row-wise: no concatenation), the attention, to_out
    //      (+ latents), W1 (+ GELU), W2 (+ residual). ----
    const int R = (int)rows, T = t_feat, A = heads * 64, F = ff_mult * dim;
    const long Mx = rows * T, Ml = rows * n_tok;
    View x(a.alloc_h(Mx * dim), dim, dim), xn(a.alloc_h(Mx * dim), dim, dim), kvx(a.alloc_h(Mx * 2 * A), 2 * A, 2 * A);
    View lat(a.alloc_h(Ml * dim), dim, dim), lat2(a.alloc_h(Ml * dim), dim, dim), ln(a.alloc_h(Ml * dim), dim, dim);
    View q(a.alloc_h(Ml * A), A, A), kvl(a.alloc_h(Ml * 2 * A), 2 * A, 2 * A), att(a.alloc_h(Ml * A), A, A);
    View f(a.alloc_h(Ml * F), F, F), po(a.alloc_h(Ml * ctx), ctx, ctx);
    op_conv(c, proj_in, View(const_cast<half_t*>(image_embeds), d_img, d_img), R, T, 1, x);
    ConvArgs gelu;
    gelu.act = 2;
    if (go && !c.err) {
        prof_open(s, "tile_rows_f16_kernel", 0.0, 4.0 * Ml * dim);
        c.err = launch_tile_rows_f16(latents, n_tok, lat.p, Ml, dim, s);
        prof_close(s);
    }
    for (const ResamplerLayer& l : layers) {
        op_layernorm(c, l.norm1, x, xn, Mx, 1e-5f);
        op_layernorm(c, l.norm2, lat, ln, Ml, 1e-5f);
        op_conv(c, l.to_q, ln, R, n_tok, 1, q);
        op_conv(c, l.to_kv, xn, R, T, 1, kvx);
        op_conv(c, l.to_kv, ln, R, n_tok, 1, kvl);
        op_resampler_attention(c, q, kvx.slice(0, A), kvx.slice(A, A), kvl.slice(0, A), kvl.slice(A, A), att, R, n_tok, T,
                               heads);
        op_conv(c, l.to_out, att, R, n_tok, 1, lat2, conv_res(lat));
        op_layernorm(c, l.ff_ln, lat2, ln, Ml, 1e-5f);
        op_conv(c, l.ff1, ln, R, n_tok, 1, f, gelu);
        op_conv(c, l.ff2, f, R, n_tok, 1, lat, conv_res(lat2));
    }
    op_conv(c, proj_out, lat, R, n_tok, 1, po);
    op_layernorm(c, norm, po, View(tok, ctx, ctx), Ml, 1e-5f);
}

int IPAdapter::project(const half_t* image_embeds, long rows, half_t* tok, hipStream_t stream) {
    if (!finalized) { set_error("ip adapter: project before finalize"); return 2; }
    if (rows < 1 || rows > 4096) { set_error("ip adapter: project takes 1..4096 images"); return 1; }
    const long key = rows * 1024 + t_feat;
    return plan_and_run(arena, stream, planned_rows, key, "ip adapter", [&](Ctx& c) {
        run_tokens(c, image_embeds, rows, tok);
        return c.err;
    });
}

void UNet::set_ip_adapter(IPAdapter* a) {
    if (ip == a) return;
    if (ip) ip->attached = nullptr;
    if (a) {
        if (a->attached && a->attached != this) a->attached->set_ip_adapter(nullptr);
        a->attached = this;
    }
    ip = a;
    ipkv_tag.clear();
    dc_tag.clear();
    reset_plans();
}

int UNet::set_motion(MotionAdapter* m) {
    if (motion == m) return 0;
    if (motion) motion->attached = nullptr;
    if (m) {
        if (m->attached && m->attached != this) m->attached->set_motion(nullptr);
        m->attached = this;
    }
    motion = m;
    dc_tag.clear();
    reset_plans();
    return 0;
}

int UNet::motion_refuse(const UNetCall& call, int frames_rows, bool pag_or_concat) {
    const int F = call.num_frames;
    if (F == 0) return 0;
    if (F < 0) { set_error("unet: num_frames is negative"); return 1; }
    if (!motion) { set_error("unet: num_frames given but no motion adapter is attached"); return 1; }
    const char* why = nullptr;
    if (pag_or_concat) why = "forward_pag / forward_concat";
    else if (graph_enabled) why = "graph replay";
    else if (dc_mode != SD_DC_PLAIN) why = "a DeepCache store / reuse mode";
    else if (tome.ratio > 0.0) why = "token merging";
    else if (hypertile.tile_size > 0) why = "HyperTile";
    else if (region_R) why = "regional prompts";
    else if (cn) why = "an attached ControlNet";
    else if (ip && ip_scale != 0.f) why = "an IP-Adapter at a non-zero scale";
    else if (freeu_on) why = "FreeU";
    // (timestep_cond cannot meet frames: sd_unet_forward_tc names none, and the entries that do take no timestep_cond)
    else if (cfg.addition_time_embed_dim > 0) why = "a text_time UNet";
    if (why) { set_error(std::string("unet: a motion adapter runs (num_frames >= 1): ") + why + " is not supported with it"); return 4; }
    if (F > motion->mcfg.max_seq_length) {
        set_error("unet: num_frames " + std::to_string(F) + " exceeds the adapter's max_seq_length " +
                  std::to_string(motion->mcfg.max_seq_length));
        return 1;
    }
    if (frames_rows <= 0 || frames_rows % F != 0) { set_error("unet: the batch is no multiple of num_frames"); return 1; }
    return 0;
}

// ------------------------------------------------------------------------------------------ blocks
namespace {
// Debug taps (engine.h: TapSink) around one block, named by its diffusers prefix: "<grp>.<i>.<kind>.<j>", or
// "<grp>.<kind>.<j>" with i < 0 (the mid block).  Without a sink neither builds the name.
std::string tap_name(const char* grp, int i, const char* kind, int j) {
    return std::string(grp) + (i < 0 ? "" : "." + std::to_string(i)) + "." + kind + "." + std::to_string(j);
}
inline void tap_begin(Ctx& c, const char* grp, int i, const char* kind, int j, View in, int N, int H, int W, View out,
                      int Ho, int Wo) {
    if (c.tap) ctx_tap_begin(c, tap_name(grp, i, kind, j), in, N, H, W, out, Ho, Wo);
}
inline void tap_end(Ctx& c, const char* grp, int i, const char* kind, int j, View out, int N, int Ho, int Wo) {
    if (c.tap) ctx_tap(c, tap_name(grp, i, kind, j), kTapOut, out, N, Ho, Wo);
}
}  // namespace

void run_resnet(Ctx& c, const Resnet& r, View x, int N, int H, int W, View out, int G, float eps,
                const float* tproj, int tproj_ld, const GnStatBuf* x_stats, const GnOut& out_stats, float stream_scale) {
    Arena& a = *c.arena;
    const size_t mk = a.mark();
    const long M = (long)N * H * W;
    const float s = stream_scale, eps_s = eps * s * s;
    View h2(a.alloc_h(M * r.cout), r.cout, r.cout);
    // Both GroupNorm + SiLU pairs run inside the convolution that consumes them where the launch allows (op_gn_conv);
    // conv1's epilogue leaves the GroupNorm summaries of h2 for norm2, conv2's those of `out` for whoever normalises it.
    const long HW = (long)H * W;
    ConvArgs f1;
    f1.gn_out = gn_wants_stats(HW, r.cout, G) ? ctx_gnbuf(c) : nullptr;
    f1.gn_groups = G;
    f1.acc_scale = s; f1.bias_scale = s;
    f1.rowadd = tproj ? tproj + r.temb_off : nullptr; f1.rowadd_ld = tproj_ld;
    op_gn_conv(c, r.n1, r.c1, x, N, H, W, h2, G, eps_s, 1, x_stats, f1);
    ConvArgs f2 = conv_res(x);
    if (r.has_sc) {
        f2.res = View(a.alloc_h(M * r.cout), r.cout, r.cout);
        ConvArgs fs;
        fs.bias_scale = s;                       // (its input carries the stream's scale already)
        op_conv(c, r.sc, x, N, H, W, f2.res, fs);
    }
    gn_out_resolve(c, out_stats, HW, r.cout, G, &f2);
    f2.acc_scale = s; f2.bias_scale = s;
    op_gn_conv(c, r.n2, r.c2, h2, N, H, W, out, G, eps_s, 1, f1.gn_out, f2);
    a.release(mk);
}

// Does block `bi` of `t`, on an H x W map, take part in HyperTile in this forward?  Then *u holds its site, level and this
// step's division, and u->copied whether any candidate division has nw > 1 (the site's gather buffers are then planned).
static bool hypertile_site(const Ctx& c, const Xformer& t, int bi, int H, int W, HyperTileUsed* u) {
    const HyperTileRun* hr = c.hypertile;
    if (!hr || hr->tile_size <= 0) return false;
    int lvl = 0;
    while ((hr->H0 >> lvl) > H) ++lvl;
    if ((hr->H0 >> lvl) != H || (hr->W0 >> lvl) != W || lvl > hr->max_depth) return false;
    HyperTileGeom g;
    const int site = t.tome_site0 + bi;
    if (hypertile_plan(H, W, hr->tile_size, hr->swap_size, hr->seed, hr->step, (uint32_t)site, &g)) return false;
    int cw[kHyperTileMaxSwap];
    const int kw = hypertile_counts(W, hr->tile_size, hr->swap_size, cw);
    u->site = site; u->H = H; u->W = W; u->nh = g.nh; u->nw = g.nw; u->level = lvl;
    u->copied = kw > 1 || cw[0] > 1;
    return true;
}

void run_xformer(Ctx& c, const Xformer& t, View x, int N, int H, int W, View out, int G, View text_kv, int L,
                 const GnStatBuf* x_stats, const GnOut& out_stats, const CfgShare* share) {
    Arena& a = *c.arena;
    const size_t mk = a.mark();
    const int C = t.C;
    const int T = H * W;
    const long M = (long)N * T;
    const int d = C / t.heads;
    const bool fold = !t.blocks.empty() && t.blocks[0].fold;
    // Shared CFG prefix: x holds N / 2 images, and so does everything up to the first block's attn2 query.  Buffers keep
    // their N-image size (the arena plan is the unshared forward's); Np / Mp are what the prefix launches run on.
    // forward_pag: Nl images exist on entry (ctx_live); the buffers are N images wide all the same.
    PagState* pg = c.pag;
    const bool perturb = pg && t.pag;
    int Nl = ctx_live(c, N);
    long Ml = (long)Nl * T;
    if (perturb && share) { set_error("run_xformer: a perturbed transformer inside the shared CFG prefix"); c.err = 2; return; }
    int Np = share ? Nl / 2 : Nl;
    long Mp = (long)Np * T;
    View hn(a.alloc_h(M * C), C, C);
    op_groupnorm(c, t.gn, x, hn, Np, T, G, 1e-6f, 0, x_stats);
    View cur(a.alloc_h(M * C), C, C), nxt(a.alloc_h(M * C), C, C);
    // row statistics of the residual stream at the three LayerNorm sites (cur -> ln1, t2 -> ln2, t3 -> ln3)
    RowStat st_cur, st_t2, st_t3;
    // producers of / consumers at the three LayerNorm sites: without the fold they ask for nothing, and the consumers
    // read `n`, the output of the LayerNorm's own launch
    ConvArgs f_cur, f_t2, f_t3, f_ln1, f_ln2, f_ln3;
    if (fold) {
        st_cur.p = a.alloc_f(rowstat_floats(M, C));
        st_t2.p = a.alloc_f(rowstat_floats(M, C));
        st_t3.p = a.alloc_f(rowstat_floats(M, C));
        f_cur.stat_out = &st_cur; f_t2.stat_out = &st_t2; f_t3.stat_out = &st_t3;
        f_ln1.ln_in = &st_cur; f_ln2.ln_in = &st_t2; f_ln3.ln_in = &st_t3;
        f_ln1.ln_eps = f_ln2.ln_eps = f_ln3.ln_eps = 1e-5f;
    }
    f_ln3.geglu = 1;                                           // (ff1, with the fold or behind norm3's own launch)
    op_conv(c, t.pin, hn, Np, H, W, cur, f_cur);
    ConvArgs fo;                                               // the launch that writes `out`
    gn_out_resolve(c, out_stats, T, C, G, &fo);
    for (size_t bi = 0; bi < t.blocks.size(); ++bi) {
        const TBlock& b = t.blocks[bi];
        const bool more = bi + 1 < t.blocks.size();
        const size_t mb = a.mark();
        View n(fold ? nullptr : a.alloc_h(M * C), C, C);
        View qkv(a.alloc_h(M * 3 * C), 3 * C, 3 * C);
        if (!fold) op_layernorm(c, b.ln1, cur, n, Mp, 1e-5f);
        op_conv(c, b.qkv, fold ? cur : n, Np, H, W, qkv, f_ln1);
        View att(a.alloc_h(M * C), C, C);
        View t2(a.alloc_h(M * C), C, C);
        const int tsite = t.tome_site0 + (int)bi;
        HyperTileUsed ht;
        const long tome_off = c.tome && !perturb && tsite < (int)c.tome->plan_off.size() ? c.tome->plan_off[(size_t)tsite] : -1;
        if (tome_off >= 0) {
            // Token merging: the match reads the residual stream norm1 reads; the projections are linear, so the mean of
            // the projected rows is the projection of the mean of the normalised rows, and the q|k|v launch above and
            // out1 below stay as they are.  Attention runs on T' rows; its output is copied back through the unmerge map.
            const TomeRun& tr = *c.tome;
            TomeGeom g;
            if (tome_geom(H, W, tr.sx, tr.sy, tr.ratio, tr.use_rand, tr.seed, tr.step, (uint32_t)tsite, &g) || g.r < 1) {
                set_error("run_xformer: token merging planned for a block that cannot merge"); c.err = 2; return;
            }
            void* plan = tr.buf + tome_off;
            if (c.tap) ctx_tap(c, "tome." + std::to_string(tsite), kTapIn, cur, Np, H, W);     // what the match reads
            View qm(a.alloc_h((long)N * g.Tm * 3 * C), 3 * C, 3 * C), am(a.alloc_h((long)N * g.Tm * C), C, C);
            if (!c.dry && !c.err) {
                hipStream_t s = c.stream;
                static const char* const stage_name[3] = {"tome_prep_kernel", "tome_match_kernel", "tome_select_kernel"};
                for (int st = 1; st <= 3 && !c.err; ++st) {
                    prof_open(s, stage_name[st - 1], st == 2 ? 2.0 * Np * g.Ns * g.Nd * C : 0.0, st == 3 ? 24.0 * Mp : 2.0 * Mp * C);
                    c.err = launch_tome_match(cur.p, cur.ld, Np, C, g, plan, s, st);
                    prof_close(s);
                }
                if (!c.err) {
                    prof_open(s, "tome_merge_kernel", 0.0, 2.0 * (Mp + (double)Np * g.Tm) * 3 * C);
                    c.err = launch_tome_merge(qkv.p, qkv.ld, 3 * C, plan, Np, T, g.Tm, qm.p, qm.ld, s);
                    prof_close(s);
                }
                if (tr.used) {
                    TomeUsed u;
                    u.site = tsite; u.H = H; u.W = W; u.r = g.r; u.Tm = g.Tm; u.B = Np; u.plan_off = tome_off;
                    tr.used->push_back(u);
                }
            }
            op_attention(c, qm.slice(0, C), qm.slice(C, C), qm.slice(2 * C, C), am, Np, g.Tm, g.Tm, t.heads, d, 0, 1);
            if (!c.dry && !c.err) {
                prof_open(c.stream, "tome_unmerge_kernel", 0.0, 4.0 * Mp * C);
                c.err = launch_tome_unmerge(am.p, am.ld, C, plan, Np, T, att.p, att.ld, c.stream);
                prof_close(c.stream);
            }
            op_conv(c, b.out1, att, Np, H, W, t2, conv_res(cur, f_t2));
        } else if (!perturb && hypertile_site(c, t, (int)bi, H, W, &ht)) {
            // HyperTile: attention within the tiles of this step's division; every other launch of the block is row-wise
            // and stays in raster order.  (ht.copied says whether a candidate nw > 1 exists: then the gather buffers are
            // planned, whatever this step drew.)
            const bool plan_copy = ht.copied != 0;
            ht.copied = ht.nw > 1;
            ht.B = Np;
            View qg(plan_copy ? a.alloc_h(M * 3 * C) : nullptr, 3 * C, 3 * C), ag(plan_copy ? a.alloc_h(M * C) : nullptr, C, C);
            if (!c.dry && !c.err && c.hypertile->used) c.hypertile->used->push_back(ht);
            if (ht.nw == 1) {
                // horizontal bands (the whole map when nh == 1: the plain launch): contiguous row ranges, nothing to copy
                op_attention(c, qkv.slice(0, C), qkv.slice(C, C), qkv.slice(2 * C, C), att, Np * ht.nh, T / ht.nh, T / ht.nh,
                             t.heads, d, 0, 1);
            } else {
                if (!c.dry && !c.err) {
                    prof_open(c.stream, "hypertile_gather_kernel", 0.0, 2.0 * Mp * 3 * C * 2);
                    c.err = launch_hypertile_gather(qkv.p, qkv.ld, 3 * C, Np, H, W, ht.nh, ht.nw, qg.p, qg.ld, c.stream);
                    prof_close(c.stream);
                }
                const int tt = T / (ht.nh * ht.nw);
                op_attention(c, qg.slice(0, C), qg.slice(C, C), qg.slice(2 * C, C), ag, Np * ht.nh * ht.nw, tt, tt, t.heads, d,
                             0, 1);
                if (!c.dry && !c.err) {
                    prof_open(c.stream, "hypertile_scatter_kernel", 0.0, 2.0 * Mp * C * 2);
                    c.err = launch_hypertile_scatter(ag.p, ag.ld, C, Np, H, W, ht.nh, ht.nw, att.p, att.ld, c.stream);
                    prof_close(c.stream);
                }
            }
            op_conv(c, b.out1, att, Np, H, W, t2, conv_res(cur, f_t2));
        } else if (!perturb) {
            op_attention(c, qkv.slice(0, C), qkv.slice(C, C), qkv.slice(2 * C, C), att, Np, T, T, t.heads, d, 0, 1);
            op_conv(c, b.out1, att, Np, H, W, t2, conv_res(cur, f_t2));
        } else {
            // Perturbed self-attention: the attention and its out-projection on the Nq un-perturbed images; the perturbed
            // group's map is the identity, so its out-projection reads the V columns of qkv in place (no attention launch,
            // no copy; its Q / K columns were computed with the others' and are never read).  Before the widening the
            // group is still its source: V and the residual are the source images' rows.
            const int Nq = pg->Nq, Ng = N - Nq;
            const long Mq = (long)Nq * T, src0 = pg->widened ? Mq : (long)(Nq - Ng) * T;
            op_attention(c, qkv.slice(0, C), qkv.slice(C, C), qkv.slice(2 * C, C), att, Nq, T, T, t.heads, d, 0, 1);
            RowStat sa, sb;
            ConvArgs fa = conv_res(cur, f_t2), fb = f_t2;
            sa.p = st_t2.p;
            if (fold) { fa.stat_out = &sa; fb.stat_out = &sb; }
            op_conv(c, b.out1, att, Nq, H, W, t2, fa);
            sb.p = st_t2.p ? st_t2.p + Mq * sa.parts * 2 : nullptr;
            const View vp(qkv.p + src0 * qkv.ld + 2 * C, qkv.ld, C), rp(cur.p + src0 * cur.ld, cur.ld, C);
            op_conv(c, b.out1, vp, Ng, H, W, View(t2.p + Mq * t2.ld, t2.ld, C), conv_res(rp, fb));
            if (fold) {
                // the row statistics of t2 across the two launches: side by side when both picked one layout, else one
                // statistics pass over all N images
                st_t2.parts = sa.parts; st_t2.width = sa.width;
                if (sa.parts != sb.parts || sa.width != sb.width) {
                    st_t2.parts = 1; st_t2.width = C;
                    if (!c.dry && !c.err) {
                        prof_open(c.stream, "row_stats_kernel", 0.0, 2.0 * M * C);
                        c.err = launch_row_stats(t2.p, t2.ld, st_t2.p, M, C, c.stream);
                        prof_close(c.stream);
                    }
                }
            }
            if (!pg->widened) {
                // from here on the perturbed group differs: give it rows in everything the remainder reads -- this
                // transformer's input (proj_out's residual) and the caller's tensors -- in one launch.  (cur and qkv were
                // read through the source rows above and are dead after this block's out1.)
                std::vector<RowDupSeg> segs;
                if (pg->caller_segs) pg->caller_segs(segs);
                RowDupSeg g;
                g.src = x.p + src0 * x.ld; g.dst = x.p + Mq * x.ld;
                g.ld_bytes = x.ld * 2; g.row_bytes = (long)x.C * 2; g.rows = (long)Ng * T;
                segs.push_back(g);
                if (!c.dry && !c.err) {
                    double bytes = 0;
                    for (const RowDupSeg& sg : segs) bytes += 2.0 * sg.rows * sg.row_bytes;
                    prof_open(c.stream, "row_dup_kernel", 0.0, bytes);
                    c.err = launch_row_dup(segs.data(), (int)segs.size(), c.stream);
                    prof_close(c.stream);
                }
                pg->widened = true;
                Nl = Np = N; Ml = Mp = M;
            }
        }
        View q(a.alloc_h(M * C), C, C);
        if (!fold) op_layernorm(c, b.ln2, t2, n, Mp, 1e-5f);
        op_conv(c, b.q2, fold ? t2 : n, Np, H, W, q, f_ln2);
        if (Np != Nl) {
            // the text enters here: from now on the halves differ.  Widen what the N-image remainder reads -- the
            // query, t2 (out2's residual), x (proj_out's residual) and the caller's tensors -- in one launch.
            std::vector<RowDupSeg> segs = share->segs;
            for (const View& v : {q, t2, x}) {
                RowDupSeg g;
                g.src = v.p; g.dst = v.p + Mp * v.ld;
                g.ld_bytes = v.ld * 2; g.row_bytes = (long)v.C * 2; g.rows = Mp;
                segs.push_back(g);
            }
            if (!c.dry && !c.err) {
                double bytes = 0;
                for (const RowDupSeg& g : segs) bytes += 2.0 * g.rows * g.row_bytes;
                prof_open(c.stream, "row_dup_kernel", 0.0, bytes);
                c.err = launch_row_dup(segs.data(), (int)segs.size(), c.stream);
                prof_close(c.stream);
            }
            Np = Nl; Mp = Ml;
        }
        // Regional prompts: the R segments of the text K / V, weighted per query by this level's weights, in one launch
        if (c.region_w) {
            int lvl = 0;
            while ((c.region_H >> lvl) > H) ++lvl;
            if ((c.region_H >> lvl) != H || (c.region_W >> lvl) != W || L % c.region_R != 0) {
                set_error("run_xformer: no regional weights for a " + std::to_string(H) + " x " + std::to_string(W) + " map");
                c.err = 2;
                return;
            }
            op_region_attention(c, q, text_kv.slice(b.kv_off, C), text_kv.slice(b.kv_off + C, C),
                                c.region_w + region_level_offset(c.region_Bw, c.region_R, c.region_H, c.region_W, lvl), att, Nl,
                                T, L / c.region_R, c.region_R, t.heads, d, c.region_Bw);
        }
        // IP-Adapter attached: text and image attention in one launch (scale 0: the text attention alone, as without one)
        else if (c.ip_kv.p && c.ip_scale != 0.f)
            op_ip_attention(c, q, text_kv.slice(b.kv_off, C), text_kv.slice(b.kv_off + C, C), c.ip_kv.slice(b.ip_kv_off, C),
                            c.ip_kv.slice(b.ip_kv_off + C, C), att, Nl, T, L, c.ip_T, t.heads, d, c.ip_scale);
        else
            op_attention(c, q, text_kv.slice(b.kv_off, C), text_kv.slice(b.kv_off + C, C), att, Nl, T, L, t.heads, d, 0, 1);
        View t3 = more ? View(a.alloc_h(M * C), C, C) : xformer_tail_t3(a, t, M);
        op_conv(c, b.out2, att, Nl, H, W, t3, conv_res(t2, f_t3));
        if (more) {
            // norm3 -> GEGLU feed-forward -> + residual: the projection with its GEGLU epilogue and the output linear with
            // its residual epilogue
            View g(a.alloc_h(M * 4 * C), 4 * C, 4 * C);
            if (!fold) op_layernorm(c, b.ln3, t3, n, Ml, 1e-5f);
            op_conv(c, b.ff1, fold ? t3 : n, Nl, H, W, g, f_ln3);
            op_conv(c, b.ff2, g, Nl, H, W, nxt, conv_res(t3, f_cur));
        } else {
            // the last block: its feed-forward and proj_out
            run_xformer_tail(c, t, t3, st_t3, n, nxt, x, Nl, H, W, out, fo);
        }
        a.release(mb);
        View tmp = cur; cur = nxt; nxt = tmp;
    }
    if (t.blocks.empty()) op_conv(c, t.pout, cur, Nl, H, W, out, conv_res(x, fo));
    a.release(mk);
}

View xformer_tail_t3(Arena& a, const Xformer& t, long M) {
    if (!t.pout_fold) return View(a.alloc_h(M * t.C), t.C, t.C);
    const long ld = t.ff2p.cin;             // hidden + C
    return View(a.alloc_h(M * ld) + (ld - t.C), ld, t.C);
}

bool run_xformer_tail(Ctx& c, const Xformer& t, View t3, const RowStat& st_t3, View n, View nxt, View x, int N, int H, int W,
                      View out, const ConvArgs& fo) {
    Arena& a = *c.arena;
    const TBlock& b = t.blocks.back();
    const int C = t.C;
    const long M = (long)N * H * W;
    const int hidden = b.ff1.cout / 2;
    const bool fold = b.fold;
    ConvArgs f_ln3;                         // ff1: GEGLU, on the folded norm3 where the block folds it
    f_ln3.geglu = 1;
    if (fold || t.pout_fold) { f_ln3.ln_in = &st_t3; f_ln3.ln_eps = 1e-5f; }
    if (t.pout_fold) {
        if (t3.ld != hidden + C || t.ff2p.cin != hidden + C) { set_error("run_xformer_tail: t3 is not xformer_tail_t3's view"); c.err = 1; return false; }
        View gt(t3.p - hidden, t3.ld, hidden + C);          // [g | t3]
        op_conv(c, b.ff1, t3, N, H, W, gt.slice(0, hidden), f_ln3);
        // K = hidden + C is in no tuned table: the tile measured for ff.net.2 alone (same M and N, K = hidden) is the
        // nearest measured answer, and keeps the table's split-K where it has one
        ConvArgs f = conv_res(x, fo);
        int v, sp;
        if (igemm2_tuned_pointwise((int)M, C, hidden, &v, &sp)) { f.tile_variant = v; f.tile_splits = sp; }
        op_conv(c, t.ff2p, gt, N, H, W, out, f);
        return false;
    }
    // norm3 -> GEGLU feed-forward -> + residual: one launch with the 4C-wide hidden tensor kept on the CU where the
    // problem fits it (the 64 x 64 level: ffn.hip), otherwise the projection with its GEGLU epilogue and the output
    // linear with its residual epilogue
    const bool fused = fold && op_ffn_fused(c, b.ff1, b.ff2, t3, st_t3, 1e-5f, M, nxt);
    if (!fused) {
        const size_t mk = a.mark();
        View g(a.alloc_h(M * hidden), hidden, hidden);
        if (!fold) op_layernorm(c, b.ln3, t3, n, M, 1e-5f);
        op_conv(c, b.ff1, fold ? t3 : n, N, H, W, g, f_ln3);
        op_conv(c, b.ff2, g, N, H, W, nxt, conv_res(t3));
        a.release(mk);
    }
    op_conv(c, t.pout, nxt, N, H, W, out, conv_res(x, fo));
    return fused;
}

// ----------------------------------------------------------------------------------------- forward
int Encoder::run_temb(Ctx& c, const float* timesteps, const half_t* add_text, const float* add_time_ids, int B,
                      float** tproj_out, int rows_alloc, const float* tcond) {
    Arena& a = *c.arena;
    const int* boc = cfg.block_out_channels;
    const int temb = boc[0] * 4;
    hipStream_t s = c.stream;
    const bool go = !c.dry;
    // ---- time embedding (fp32, batch-sized GEMVs) ----
    float* sinus = a.alloc_f((long)B * boc[0]);
    float* e1 = a.alloc_f((long)B * temb);
    float* emb = a.alloc_f((long)B * temb);
    float* tproj = a.alloc_f((long)std::max(B, rows_alloc) * temb_total);
    *tproj_out = tproj;
    // (a guidance-embedded UNet: sinusoid + cond_proj(timestep_cond) from one launch in the sinusoid's place)
    if (go && !c.err)
        c.err = tcond ? launch_timestep_cond(timesteps, tcond, tcp.w, tcp.K, sinus, B, boc[0], cfg.time_cond_proj_dim,
                                             cfg.flip_sin_to_cos, cfg.freq_shift, s)
                      : launch_timestep_sinusoid(timesteps, 1, sinus, B, boc[0], cfg.flip_sin_to_cos, cfg.freq_shift, boc[0], s);
    if (go && !c.err) c.err = launch_small_linear(sinus, boc[0], te1.w, te1.bias, e1, temb, B, boc[0], temb, 0, 1, s);
    // (without text_time conditioning the SiLU every resnet applies to the embedding rides on this launch)
    const bool aug_path = cfg.addition_time_embed_dim > 0;
    if (go && !c.err) c.err = launch_small_linear(e1, temb, te2.w, te2.bias, emb, temb, B, temb, temb, 0, aug_path ? 0 : 1, s);
    if (aug_path) {
        const int ad = cfg.addition_time_embed_dim;
        const int pin = cfg.projection_class_embeddings_input_dim;
        const int nid = num_time_ids();
        const int tdim = pin - nid * ad;        // pooled text embedding width
        if (!add_text || !add_time_ids) { set_error("unet: add_text / add_time_ids required for text_time conditioning"); return 1; }
        // (rows as wide as add_embedding.linear_1's packed K: pin itself with six ids, zero padded otherwise)
        const int kin = nid == 6 ? pin : (int)ae1.K;
        float* addin = a.alloc_f((long)B * kin);
        float* a1 = a.alloc_f((long)B * temb);
        float* aug = a.alloc_f((long)B * temb);
        if (nid != 6) {
            if (go && !c.err) c.err = launch_text_time_input(add_text, add_time_ids, addin, B, tdim, ad, nid,
                                                             cfg.flip_sin_to_cos, cfg.freq_shift, kin, s);
        } else {
            // six ids (SDXL base) keep the launch sequence they always had
            float* txt = a.alloc_f((long)B * tdim);
            if (go && !c.err) c.err = launch_f16_to_f32(add_text, txt, (long)B * tdim, s);
            if (go && !c.err) {
                hipError_t e = hipMemcpy2DAsync(addin, (size_t)pin * 4, txt, (size_t)tdim * 4, (size_t)tdim * 4, (size_t)B,
                                                hipMemcpyDeviceToDevice, s);
                if (e != hipSuccess) { set_error(hipGetErrorString(e)); c.err = 3; }
            }
            // time_ids.flatten() -> [B*6] scalars -> sinusoid(ad) each -> [B, 6*ad] placed after the text
            if (go && !c.err) {
                for (int j = 0; j < 6 && !c.err; ++j)
                    c.err = launch_timestep_sinusoid(add_time_ids + j, 6, addin + tdim + j * ad, B, ad,
                                                             cfg.flip_sin_to_cos, cfg.freq_shift, pin, s);
            }
        }
        if (go && !c.err) c.err = launch_small_linear(addin, kin, ae1.w, ae1.bias, a1, temb, B, kin, temb, 0, 1, s);
        if (go && !c.err) c.err = launch_small_linear(a1, temb, ae2.w, ae2.bias, aug, temb, B, temb, temb, 0, 0, s);
        if (go && !c.err) c.err = launch_add_f32(emb, aug, (long)B * temb, 1, s);      // silu(emb + aug_emb)
    }
    // every resnet consumes the embedding only as time_emb_proj(silu(emb)): the SiLU is applied once
    // here instead of inside the weight-bandwidth-bound stacked GEMV
    if (c.tap) ctx_tap_f32(c, "emb", emb, B, temb);             // (what exists on the device: silu(emb))
    if (go && !c.err) c.err = launch_small_linear(emb, temb, temb_stack.w, temb_stack.bias, tproj, temb_total, B, temb, temb_total, 0, 0, s);

    return c.err;
}

void Encoder::run_conv_in(Ctx& c, const half_t* sample, int B, int H, int W, View y0, GnStatBuf* gb, const View* res,
                          GnStatBuf** xs, const UNetCall* cat) {
    Arena& a = *c.arena;
    const int* boc = cfg.block_out_channels;
    const int G = cfg.norm_num_groups;
    hipStream_t s = c.stream;
    const bool go = !c.dry;
    const size_t mk = a.mark();
    const long M = (long)B * H * W;
    auto head_stats = [&](float* out) {
        if (!gb) return;
        gb->st = GnStats();
        if (out) { gb->st.part = gb->buf; gb->st.rows = 128; gb->st.S = (int)((long)H * W / 128); }
    };
    if (cat) {
        Head2Params h2;
        h2.a = sample; h2.Na = cat->lat_rows; h2.Ca = cfg.in_channels - cat->extra_channels; h2.in_scale = cat->in_scale;
        h2.b = cat->extra; h2.Nb = cat->extra_rows; h2.Cb = cat->extra_channels; h2.zero_from = cat->zero_from;
        h2.w = conv_in.w; h2.K = conv_in.K; h2.bias = conv_in.bias; h2.y = y0.p; h2.ldy = y0.ld;
        h2.gnstat_out = (gb && gb->buf) ? gb->buf : nullptr; h2.G = G;
        h2.N = B; h2.H = H; h2.W = W; h2.Cout = boc[0];
        if (!res && conv_head2_supported(h2)) {
            head_stats(h2.gnstat_out);
            if (go && !c.err) {
                prof_open(s, "conv_head2_kernel", 2.0 * M * boc[0] * 9.0 * cfg.in_channels, 2.0 * M * (boc[0] + cfg.in_channels));
                c.err = launch_conv_head2(h2, s);
                prof_close(s);
            }
            *xs = gb;
            a.release(mk);
            return;
        }
        half_t* full = a.alloc_h(M * cfg.in_channels);
        if (go && !c.err) {
            prof_open(s, "concat_sample_kernel", 0.0, 4.0 * M * cfg.in_channels);
            c.err = launch_concat_sample(h2.a, h2.Na, h2.Ca, h2.in_scale, h2.b, h2.Nb, h2.Cb, h2.zero_from, full, B, (long)H * W, s);
            prof_close(s);
        }
        sample = full;
    }
    HeadParams hp;
    hp.x_nchw = sample; hp.w = conv_in.w; hp.K = conv_in.K; hp.bias = conv_in.bias; hp.y = y0.p; hp.ldy = y0.ld;
    hp.gnstat_out = (gb && gb->buf) ? gb->buf : nullptr; hp.G = G;
    hp.N = B; hp.Cin = cfg.in_channels; hp.H = H; hp.W = W; hp.Cout = boc[0];
    if (!res && conv_head_supported(hp)) {
        head_stats(hp.gnstat_out);
        if (go && !c.err) {
            prof_open(s, "conv_head_kernel", 2.0 * M * boc[0] * 9.0 * cfg.in_channels, 2.0 * M * (boc[0] + cfg.in_channels));
            c.err = launch_conv_head(hp, s);
            prof_close(s);
        }
        *xs = gb;
    } else {
        half_t* col = a.alloc_h(M * conv_in.K);
        if (go && !c.err) {
            prof_open(s, "im2col_nchw3x3_kernel", 0.0, 2.0 * M * (conv_in.K + cfg.in_channels));
            c.err = launch_im2col_nchw3x3(sample, col, B, cfg.in_channels, H, W, (int)conv_in.K, s);
            prof_close(s);
        }
        ConvW pw = conv_in; pw.ks = 1;
        ConvArgs f;
        f.gn_out = gb;
        f.gn_groups = G;
        if (res) f.res = *res;
        op_conv(c, pw, View(col, conv_in.K, (int)conv_in.K), B, H, W, y0, f);
        *xs = f.gn_out;
    }
    a.release(mk);
}

View Encoder::run_down(Ctx& c, View x, GnStatBuf*& xs, int B, int& h, int& w, View text_kv, int L, const float* tproj,
                       const SkipDst& skip_view, const SkipStat& skip_stat, const CfgShare* share, int stop_after) {
    Arena& a = *c.arena;
    const int nb = cfg.num_blocks;
    const int G = cfg.norm_num_groups;
    const float eps = cfg.norm_eps;
    int skip_i = 1;
    for (int i = 0; i < nb; ++i) {
        // (stop_after >= 0, a DeepCache reuse step: that many layers of block 0 and nothing below them)
        const int nl = stop_after >= 0 ? std::min(stop_after, cfg.layers_per_block) : cfg.layers_per_block;
        for (int j = 0; j < nl; ++j) {
            const Resnet& r = down_res[i][j];
            if (cfg.down_block_has_attn[i]) {
                const size_t mk = a.mark();
                View tmp(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout);
                GnStatBuf* rs = nullptr;
                const CfgShare* sh = (i == 0 && j == 0) ? share : nullptr;
                const int Bl = ctx_live(c, B);
                tap_begin(c, "down_blocks", i, "resnets", j, x, B, h, w, tmp, h, w);
                run_resnet(c, r, x, sh ? Bl / 2 : Bl, h, w, tmp, G, eps, tproj, temb_total, xs, &rs);
                tap_end(c, "down_blocks", i, "resnets", j, tmp, B, h, w);
                View dst = skip_view(skip_i);
                if (c.pag) c.pag->skips_done = skip_i;
                // (a motion module behind the pair: the transformer writes a temporary, the module's last launch the skip)
                const MotionModule* mm = c.motion ? &c.motion->down[(size_t)i][(size_t)j] : nullptr;
                const View xo = mm ? View(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout) : dst;
                const GnOut skip_out(&xs, skip_stat(skip_i, (long)h * w, r.cout));
                tap_begin(c, "down_blocks", i, "attentions", j, tmp, B, h, w, xo, h, w);
                run_xformer(c, down_att[i][j], tmp, B, h, w, xo, G, text_kv, L, rs, mm ? GnOut() : skip_out, sh);
                tap_end(c, "down_blocks", i, "attentions", j, xo, B, h, w);
                if (mm) {
                    tap_begin(c, "down_blocks", i, "motion_modules", j, xo, B, h, w, dst, h, w);
                    run_motion(c, *mm, xo, B, c.motion_frames, h, w, dst, skip_out, G);
                    tap_end(c, "down_blocks", i, "motion_modules", j, dst, B, h, w);
                }
                a.release(mk);
                x = dst;
            } else {
                View dst = skip_view(skip_i);
                const MotionModule* mm = c.motion ? &c.motion->down[(size_t)i][(size_t)j] : nullptr;
                const size_t mk = a.mark();
                const View xo = mm ? View(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout) : dst;
                const GnOut skip_out(&xs, skip_stat(skip_i, (long)h * w, r.cout));
                tap_begin(c, "down_blocks", i, "resnets", j, x, B, h, w, xo, h, w);
                run_resnet(c, r, x, ctx_live(c, B), h, w, xo, G, eps, tproj, temb_total, xs, mm ? GnOut() : skip_out);
                tap_end(c, "down_blocks", i, "resnets", j, xo, B, h, w);
                if (mm) {
                    tap_begin(c, "down_blocks", i, "motion_modules", j, xo, B, h, w, dst, h, w);
                    run_motion(c, *mm, xo, B, c.motion_frames, h, w, dst, skip_out, G);
                    tap_end(c, "down_blocks", i, "motion_modules", j, dst, B, h, w);
                }
                a.release(mk);
                x = dst;
            }
            ++skip_i;
        }
        if (stop_after >= 0) return x;
        if (i != nb - 1) {
            ConvArgs f;
            f.stride = 2;
            f.gn_out = skip_stat(skip_i, (long)(h / 2) * (w / 2), down_ds[i].cout);
            View dst = skip_view(skip_i++);
            f.gn_groups = G;
            tap_begin(c, "down_blocks", i, "downsamplers", 0, x, B, h, w, dst, h / 2, w / 2);
            op_conv(c, down_ds[i], x, ctx_live(c, B), h, w, dst, f);
            tap_end(c, "down_blocks", i, "downsamplers", 0, dst, B, h / 2, w / 2);
            xs = f.gn_out;
            h /= 2; w /= 2;
            x = dst;
        }
    }

    return x;
}

void Encoder::run_mid(Ctx& c, View x, GnStatBuf* xs, int B, int h, int w, View text_kv, int L, const float* tproj,
                      View dst) {
    Arena& a = *c.arena;
    const int nb = cfg.num_blocks;
    const int* boc = cfg.block_out_channels;
    const int G = cfg.norm_num_groups;
    const float eps = cfg.norm_eps;
    const int C = boc[nb - 1];
    const long M = (long)B * h * w;
    View m0(a.alloc_h(M * C), C, C), m1(a.alloc_h(M * C), C, C);
    GnStatBuf *s0 = nullptr, *s1 = nullptr;
    tap_begin(c, "mid_block", -1, "resnets", 0, x, B, h, w, m0, h, w);
    run_resnet(c, mid_r0, x, ctx_live(c, B), h, w, m0, G, eps, tproj, temb_total, xs, &s0);
    tap_end(c, "mid_block", -1, "resnets", 0, m0, B, h, w);
    tap_begin(c, "mid_block", -1, "attentions", 0, m0, B, h, w, m1, h, w);
    run_xformer(c, mid_att, m0, B, h, w, m1, G, text_kv, L, s0, &s1);
    tap_end(c, "mid_block", -1, "attentions", 0, m1, B, h, w);
    if (c.motion && c.motion->mcfg.use_mid_block) {
        // behind the transformer, before the second resnet, which reads the module's own summaries
        View m2(a.alloc_h(M * C), C, C);
        tap_begin(c, "mid_block", -1, "motion_modules", 0, m1, B, h, w, m2, h, w);
        run_motion(c, c.motion->mid, m1, B, c.motion_frames, h, w, m2, GnOut(&s1), G);
        tap_end(c, "mid_block", -1, "motion_modules", 0, m2, B, h, w);
        m1 = m2;
    }
    tap_begin(c, "mid_block", -1, "resnets", 1, m1, B, h, w, dst, h, w);
    run_resnet(c, mid_r1, m1, ctx_live(c, B), h, w, dst, G, eps, tproj, temb_total, s1);   // output joins a concat: no consumer
    tap_end(c, "mid_block", -1, "resnets", 1, dst, B, h, w);
}

int Encoder::num_skips() const { return 1 + cfg.num_blocks * cfg.layers_per_block + (cfg.num_blocks - 1); }

int UNet::run(Ctx& c, const UNetCall& call, int dc) {
    const half_t* sample = call.sample;
    const half_t* const ehs = call.ehs;
    const half_t* const image_embeds = call.image_embeds;
    half_t* const out = call.out;
    const int L = call.L, B = call.B, H = call.H, W = call.W, n_img = call.n_img;
    const float cn_scale = call.cn_scale;
    const CfgIn* const cfg_in = call.cfg_in;
    const PagIn* const pag = call.pag;
    Arena& a = *c.arena;
    const int nb = cfg.num_blocks;
    const int* boc = cfg.block_out_channels;
    const int G = cfg.norm_num_groups;
    const float eps = cfg.norm_eps;
    hipStream_t s = c.stream;
    const bool go = !c.dry;
    const bool reuse = dc == SD_DC_REUSE;

    // ---- shared CFG prefix (forward_cfg): B = 2 Bp images from Bp latents and Bp timesteps.  conv_in, the first
    //      resnet and the first transformer up to its attn2 query run on Bp images; run_xformer widens what the rest
    //      reads.  The scaled latents get their buffer whatever the scale, so every step of a loop keeps one plan. ----
    // ---- perturbed-attention guidance (forward_pag): the last Ng of the B images are the perturbed group, copies of the
    //      Ng in front of them (the text group).  ehs / add_text / add_time_ids hold Nq = B - Ng rows.  Late: the group
    //      does not exist until the first flagged transformer (PagState); otherwise `sample` holds all B images. ----
    PagState pgs;
    const int Ng = pag ? B / (pag->groups + 1) : 0, Nq = B - Ng;
    if (pag) {
        pgs.N = B; pgs.Nq = Nq;
        pgs.widened = !pag->late;
        c.pag = &pgs;
    }
    // ---- two-source mode (forward_concat): B images from lat_rows latents and timesteps, group by group.  The time
    //      embedding runs on the lat_rows and is widened like the shared CFG prefix's, conv_in reads both sources. ----
    const UNetCall* const cat = call.extra ? &call : nullptr;
    const int Bp = cat ? call.lat_rows : cfg_in ? Nq / 2 : Nq;
    CfgShare share;
    if (cfg_in) {
        const long n = (long)Bp * cfg.in_channels * H * W;
        half_t* scaled = a.alloc_h(n);
        sample = cfg_in->latents;
        if (cfg_in->in_scale != 1.f) {
            if (go && !c.err) c.err = launch_scale_copy_f16(cfg_in->latents, scaled, n, cfg_in->in_scale, s);
            sample = scaled;
        }
    }

    float* tproj = nullptr;
    if (int rc = run_temb(c, call.timesteps, call.add_text, call.add_time_ids, Bp, &tproj, B, call.tcond)) return rc;
    if (cfg_in) {
        RowDupSeg g;
        g.src = tproj; g.dst = tproj + (long)Bp * temb_total;
        g.ld_bytes = g.row_bytes = (long)Bp * temb_total * 4; g.rows = 1;
        share.segs.push_back(g);
    }
    if (cat && B > Bp) {
        std::vector<RowDupSeg> segs;
        for (int g0 = Bp; g0 < B; g0 += Bp) {
            RowDupSeg g;
            g.src = tproj; g.dst = tproj + (long)g0 * temb_total;
            g.ld_bytes = g.row_bytes = (long)Bp * temb_total * 4; g.rows = 1;
            segs.push_back(g);
        }
        if (go && !c.err) {
            prof_open(s, "row_dup_kernel", 0.0, 2.0 * (B - Bp) * temb_total * 4);
            c.err = launch_row_dup(segs.data(), (int)segs.size(), s);
            prof_close(s);
        }
    }

    // ---- text K/V of every cross-attention block in one GEMM: [B*L, ctx] x [ctx, sum 2C] ----
    //      (forward_pag: projected for the Nq rows of ehs; the perturbed group gets a copy of the text group's rows, which
    //      the cache keeps with the rest.  That copy, and up front the group's tproj rows, are one row_dup launch here.)
    const bool kv_cached = ptr_caches_live() && kv_cache.h() != nullptr;
    View text_kv(kv_cached ? kv_cache.h() : a.alloc_h((long)B * L * kv_total), kv_total, kv_total);
    std::vector<RowDupSeg> pag_now;
    if (!(kv_cached && kv_tag.matches(ehs, B, L, Ng))) {
        op_conv(c, kv_all, View(const_cast<half_t*>(ehs), cfg.cross_attention_dim, cfg.cross_attention_dim), Nq, L, 1, text_kv);
        if (kv_cached && go && !c.err) kv_tag.set(ehs, B, L, Ng);
        if (pag) {
            RowDupSeg g;
            g.src = text_kv.p + (long)(Nq - Ng) * L * kv_total; g.dst = text_kv.p + (long)Nq * L * kv_total;
            g.ld_bytes = g.row_bytes = (long)Ng * L * kv_total * 2; g.rows = 1;
            pag_now.push_back(g);
        }
    }
    RowDupSeg pag_tproj;
    if (pag) {
        pag_tproj.src = tproj + (long)(Nq - Ng) * temb_total; pag_tproj.dst = tproj + (long)Nq * temb_total;
        pag_tproj.ld_bytes = pag_tproj.row_bytes = (long)Ng * temb_total * 4; pag_tproj.rows = 1;
        if (!pag->late) pag_now.push_back(pag_tproj);
    }
    if (!pag_now.empty() && go && !c.err) {
        double bytes = 0;
        for (const RowDupSeg& g : pag_now) bytes += 2.0 * g.rows * g.row_bytes;
        prof_open(s, "row_dup_kernel", 0.0, bytes);
        c.err = launch_row_dup(pag_now.data(), (int)pag_now.size(), s);
        prof_close(s);
    }

    // ---- IP-Adapter: image tokens = LayerNorm(image_embeds W_proj^T + b), or the Resampler's (IPAdapter::run_tokens),
    //      [B n_img n_tok, ctx], then their K / V for every cross-attention block in one GEMM:
    //      [B T_ip, ctx] x [ctx, sum 2C] ----
    if (ip && image_embeds) {
        const int ctx = cfg.cross_attention_dim, T_ip = n_img * ip->n_tok;
        const long rows = (long)B * n_img, ntc = (long)ip->n_tok * ctx;
        const bool ip_cached = ptr_caches_live() && ipkv_cache.h() != nullptr;
        View ip_kv(ip_cached ? ipkv_cache.h() : a.alloc_h((long)B * T_ip * ip->kv_total), ip->kv_total, ip->kv_total);
        // the planning pass always takes the computing branch: its temporaries live between mark and release, so the
        // live pass skipping them (cache hit) allocates less and every later tensor keeps its planned address
        const bool hit = ip_cached && ipkv_tag.matches(image_embeds, B, n_img);
        if (c.dry || !hit) {
            const size_t mk = a.mark();
            half_t* tok = a.alloc_h(rows * ntc);
            ip->run_tokens(c, image_embeds, rows, tok);
            op_conv(c, ip->kv_all, View(tok, ctx, ctx), B, T_ip, 1, ip_kv);
            a.release(mk);
            if (ip_cached && go && !c.err) ipkv_tag.set(image_embeds, B, n_img);
        }
        c.ip_kv = ip_kv;
        c.ip_T = T_ip;
        c.ip_scale = ip_scale;
    }

    // ---- skip / concat buffer plan ----
    // Skip tensors are produced in down-path order and consumed by the up path in reverse; each
    // up resnet k reads cat_k = [hidden (C1) | skip (C2)].  Allocate every cat_k up front so the
    // down-path producers write their outputs directly into the skip half.
    // DeepCache (store / reuse): cats[dc_k] is the handle's persistent buffer, whose hidden half a store forward leaves
    // behind for the reuse forwards after it.  A reuse forward reads no concatenation before that one.
    struct Cat { half_t* p; int c1, c2, h, w; };
    std::vector<Cat> cats;
    const int dc_k = dc != SD_DC_PLAIN ? num_skips() - 1 - dc_depth : -1;
    {
        int out_ch = boc[nb - 1];
        int h = H >> (nb - 1), w = W >> (nb - 1);
        for (int i = 0; i < nb; ++i) {
            const int prev = out_ch;
            out_ch = boc[nb - 1 - i];
            const int in_ch = boc[nb - 1 - (i + 1 < nb ? i + 1 : nb - 1)];
            for (int j = 0; j < cfg.layers_per_block + 1; ++j) {
                Cat ct;
                ct.c2 = (j == cfg.layers_per_block) ? in_ch : out_ch;
                ct.c1 = (j == 0) ? prev : out_ch;
                ct.h = h; ct.w = w;
                const int kc = (int)cats.size();
                ct.p = kc == dc_k ? dc_buf.h() : (reuse && kc < dc_k) ? nullptr : a.alloc_h((long)B * h * w * (ct.c1 + ct.c2));
                cats.push_back(ct);
            }
            if (i != nb - 1) { h *= 2; w *= 2; }
        }
    }
    const int nskip = (int)cats.size();
    int skip_i = 0;   // index of the next skip to produce; consumer is cats[nskip-1-skip_i]
    auto skip_view = [&](int si) {
        const Cat& ct = cats[(size_t)(nskip - 1 - si)];
        return View(ct.p, ct.c1 + ct.c2, ct.c1 + ct.c2).slice(ct.c1, ct.c2);
    };

    // ---- GroupNorm summaries travel from the convolution that writes a tensor to the GroupNorm that reads
    //      it (big maps only); `xs` = those of the current x, nullptr when nobody produced them ----
    ctx_gnpool_init(c, B, (long)H * W, G);
    GnStatBuf* xs = nullptr;
    // A skip connection's summaries are read twice: by the next layer of the down path and, much later, by the up block
    // that concatenates it -- they get buffers of their own instead of ring slots.  `hid` receives those of a tensor that
    // becomes the HIDDEN half of a concatenation, over the sub-groups gn_cat_unit prescribes (up to 128 of them).
    std::vector<GnStatBuf> sst((size_t)nskip);
    GnStatBuf hid;
    if (c.gnpool[0].buf) {
        for (auto& b : sst) b.buf = a.alloc_f(gnstat_floats(B, (long)H * W, G));
        hid.buf = a.alloc_f(gnstat_floats(B, (long)H * W, 128));
    }
    auto skip_stat = [&](int si, long HWs, int C) -> GnStatBuf* {
        return (sst[(size_t)si].buf && gn_wants_stats(HWs, C, G)) ? &sst[(size_t)si] : nullptr;
    };

    // ---- ControlNet: its encoder on the same sample, timestep and text.  The pre-zero-conv hidden tensors of every
    //      skip and of the mid block live above the concatenation buffers (released after the residual adds); the
    //      ControlNet runs on a GroupNorm ring of its own, this forward's ring is restored after it ----
    //      With n_act >= 2 running nets (MultiControlNet) every site is one wide buffer [rows, n_act C] and net k's encoder
    //      writes the column slice [k C, (k + 1) C): the operand of one K-concatenated residual GEMM per site.
    const bool use_cn = cn && call.control && cn_scale != 0.f && !cfg_in;
    const int n_act = !use_cn ? 0 : call.cn_active > 1 ? call.cn_active : 1;
    const size_t cn_mark = a.mark();
    std::vector<View> cn_sites;
    std::vector<int> cn_rows;
    View cn_mid;
    if (use_cn) {
        int hh = H, ww = W;
        auto site = [&](int C) {
            cn_sites.emplace_back(a.alloc_h((long)B * hh * ww * n_act * C), (long)n_act * C, n_act * C);
            cn_rows.push_back(B * hh * ww);
        };
        site(boc[0]);
        for (int i = 0; i < nb; ++i) {
            for (int j = 0; j < cfg.layers_per_block; ++j) site(boc[i]);
            if (i != nb - 1) { hh /= 2; ww /= 2; site(boc[i]); }
        }
        cn_mid = View(a.alloc_h((long)B * hh * ww * n_act * boc[nb - 1]), (long)n_act * boc[nb - 1], n_act * boc[nb - 1]);
        cn_rows.push_back(B * hh * ww);
        GnStatBuf ring[Ctx::kGnPool];
        for (int i = 0; i < Ctx::kGnPool; ++i) ring[i] = c.gnpool[i];
        const int ring_next = c.gn_next, ring_groups = c.gn_groups;
        TapSink* const tap = c.tap;         // (the ControlNet's encoder shares run_down / run_mid: its blocks are not tapped)
        c.tap = nullptr;
        const TomeRun* const tome_run = c.tome;     // (and they run without token merging)
        c.tome = nullptr;
        const HyperTileRun* const ht_run = c.hypertile;
        c.hypertile = nullptr;
        if (n_act == 1) {
            if (int rc = run_controlnet(c, call, call.cn_idx, cn_sites, cn_mid)) return rc;
        } else {
            // one net after the other, each on its own image, embedding and text K / V; a net's temporaries are dead when
            // its encoder has run
            for (int k = 0; k < n_act; ++k) {
                const int net = call.cn_act[k];
                UNetCall one = call;
                one.control = call.mc_control[net]; one.n_ctrl = call.mc_n_ctrl[net];
                std::vector<View> sl;
                for (const View& v : cn_sites) sl.push_back(v.slice(k * (v.C / n_act), v.C / n_act));
                const size_t mk = a.mark();
                if (int rc = run_controlnet(c, one, net, sl, cn_mid.slice(k * (cn_mid.C / n_act), cn_mid.C / n_act))) return rc;
                a.release(mk);
            }
        }
        c.tome = tome_run;
        c.hypertile = ht_run;
        c.tap = tap;
        for (int i = 0; i < Ctx::kGnPool; ++i) c.gnpool[i] = ring[i];
        c.gn_next = ring_next; c.gn_groups = ring_groups;
    }

    // ---- conv_in: one launch straight from the NCHW latents (edge.hip); otherwise (inpainting's 9 channels, odd maps)
    //      im2col into a 64-wide K, then the GEMM kernel ----
    int h = H, w = W;
    if (c.tap) ctx_tap(c, "conv_in", kTapPre, skip_view(skip_i), B, H, W);      // (its input is the caller's sample)
    run_conv_in(c, sample, cfg_in ? Bp : ctx_live(c, B), H, W, skip_view(skip_i), skip_stat(skip_i, (long)H * W, boc[0]),
                nullptr, &xs, cat);
    View x = skip_view(skip_i++);
    if (c.tap) ctx_tap(c, "conv_in", kTapOut, x, B, H, W);
    if (pag) {
        // what the late widening copies besides the flagged transformer's own input: tproj, and every skip that is
        // written and still to be read by the up path
        pgs.skips_done = 1;
        pgs.caller_segs = [&](std::vector<RowDupSeg>& v) {
            v.push_back(pag_tproj);
            const int n = std::min(pgs.skips_done, nskip - pgs.cats_consumed);
            for (int si = 0; si < n; ++si) {
                const Cat& ct = cats[(size_t)(nskip - 1 - si)];
                const View sv = skip_view(si);
                const long px = (long)ct.h * ct.w;
                RowDupSeg g;
                g.src = sv.p + (Nq - Ng) * px * sv.ld; g.dst = sv.p + Nq * px * sv.ld;
                g.ld_bytes = sv.ld * 2; g.row_bytes = (long)sv.C * 2; g.rows = Ng * px;
                v.push_back(g);
            }
        };
    }
    if (cfg_in) {
        // skip 0 is read again by the last up resnet, on all B images.  (Its GroupNorm summaries are not: their only
        // reader besides the first resnet is the SD_GN_CAT merge, which forward_cfg does not share under.)
        RowDupSeg g;
        g.src = x.p; g.dst = x.p + (long)Bp * H * W * x.ld;
        g.ld_bytes = x.ld * 2; g.row_bytes = (long)x.C * 2; g.rows = (long)Bp * H * W;
        share.segs.push_back(g);
    }

    // ---- down path ----
    // (a reuse step stops after dc_depth layers of block 0, the last of which wrote the skip half of cats[dc_k])
    x = run_down(c, x, xs, B, h, w, text_kv, L, tproj, [&](int si) { return skip_view(si); },
                 [&](int si, long HWs, int C) { return skip_stat(si, HWs, C); }, cfg_in ? &share : nullptr,
                 reuse ? dc_depth : -1);

    // ---- mid block ----
    if (pag) pgs.skips_done = nskip;
    if (!reuse) run_mid(c, x, xs, B, h, w, text_kv, L, tproj, View(cats[0].p, cats[0].c1 + cats[0].c2, cats[0].c1));

    // ---- ControlNet residuals: skip_i += s (h_i W_i^T + b_i) in the skip half of every concatenation and
    //      mid += s (h_mid W_mid^T + b_mid) in the hidden half of the first, one GEMM per site with the scale and the
    //      residual in its epilogue.  After the mid block: the skips were the down path's inputs too, and diffusers adds
    //      the residuals only to what the up path reads.  (The grouped cn_residual_kernel is slower than these launches
    //      today: DESIGN.md §4.)  Then the ControlNet's tensors and the mid block's temporaries are dead. ----
    //      Two or more running nets: y += [h_1 | ... | h_n] [s_1 W_1 | ... | s_n W_n]^T + sum s_k b_k, one GEMM per site
    //      with K = n C on the folded weights (UNet::cn_fold: refolded only when the running nets or a scale changed) --
    //      or, with the K-concatenated form switched off (cn_kcat_on), one GEMM per net and site on its column slice.
    if (use_cn) {
        const bool kcat = n_act > 1 && cn_kcat_on();
        if (kcat && go && !c.err) {
            float sc[kCnMaxNets];
            for (int k = 0; k < n_act; ++k) sc[k] = call.mc_scale[call.cn_act[k]];
            c.err = cn_fold(call.cn_act, sc, n_act, s);
        }
        for (int si = 0; si <= nskip; ++si) {
            const View xh = si < nskip ? cn_sites[(size_t)si] : cn_mid;
            const View y = si < nskip ? skip_view(si) : View(cats[0].p, cats[0].c1 + cats[0].c2, cats[0].c1);
            if (n_act == 1) {
                ConvArgs f;
                f.acc_scale = cn_scale; f.bias_scale = cn_scale;
                op_conv(c, cn_zero(call.cn_idx, si), xh, 1, cn_rows[(size_t)si], 1, y, conv_res(y, f));
            } else if (kcat) {
                const ConvW& z0 = cn_zero(call.cn_act[0], si);
                ConvW zw;
                zw.w = cn_wcat.h() + cn_wcat_off[(size_t)si];
                zw.bias = reinterpret_cast<float*>(cn_bcat.data()) + cn_bcat_off[(size_t)si];
                zw.cin = n_act * z0.cin; zw.cout = z0.cout; zw.ks = 1; zw.K = n_act * z0.K;
                op_conv(c, zw, xh, 1, cn_rows[(size_t)si], 1, y, conv_res(y));
            } else {
                const int C = xh.C / n_act;
                for (int k = 0; k < n_act; ++k) {
                    ConvArgs f;
                    f.acc_scale = f.bias_scale = call.mc_scale[call.cn_act[k]];
                    op_conv(c, cn_zero(call.cn_act[k], si), xh.slice(k * C, C), 1, cn_rows[(size_t)si], 1, y, conv_res(y, f));
                }
            }
        }
    }
    if (use_cn) a.release(cn_mark);

    // ---- up path ----
    View final_x;
    int k = 0;
    // Summaries of the hidden half of cats[k], when its producer (the previous layer's last convolution or the upsample
    // convolution) left them, and over how many sub-groups.  Off unless SD_GN_CAT=1: measured a wash on the C2 forward
    // (10.07-10.13 ms with, 10.04-10.10 without, alternating runs on one box: the statistics passes it removes, five
    // launches, cost about what the five producers' extra epilogue work and the merge launches cost --
    // profiles/r03_groupnorm_apply.txt); every concatenation's norm1 then runs its own statistics pass.
    const GnStatBuf* hid_ready = nullptr;
    int hid_groups = 0;
    // (with a ControlNet the skips' summaries predate the residual add: norm1 always runs its own statistics pass)
    static const bool no_cat_env = getenv("SD_GN_CAT") == nullptr;
    // (forward_pag likewise: a skip's summaries may cover fewer images than the concatenation that reads it)
    const bool no_cat_stats = no_cat_env || use_cn || pag;
    for (int i = 0; i < nb; ++i) {
        for (int j = 0; j < cfg.layers_per_block + 1; ++j, ++k) {
            if (reuse && k < dc_k) continue;     // (h, w stayed H, W: the layers that remain are the last block's)
            const Cat& ct = cats[(size_t)k];
            const Resnet& r = up_res[i][j];
            View xin(ct.p, ct.c1 + ct.c2, ct.c1 + ct.c2);
            const bool last_in_block = (j == cfg.layers_per_block);
            // FreeU (diffusers apply_freeu, up blocks 0 and 1): scale the first half of the hidden channels and filter
            // the skip, in place in the concatenation, after the ControlNet's residuals and before norm1 reads it.  Both
            // producers' GroupNorm summaries are stale afterwards: norm1 of such a resnet runs its own statistics pass,
            // and nobody emits summaries into a hidden half that FreeU will rescale (fu_next).
            const bool fu = freeu_on && i < 2;
            const bool fu_next = freeu_on && (last_in_block ? i + 1 : i) < 2;
            const int Bl = ctx_live(c, B);      // images this layer's concatenation holds
            if (pag) pgs.cats_consumed = k + 1;
            if (fu && go && !c.err) {
                const double elems = (double)Bl * h * w * (ct.c1 / 2 + ct.c2);
                prof_open(s, "freeu_kernel", 16.0 * Bl * h * w * ct.c2, 4.0 * elems);
                c.err = launch_freeu(xin.p, xin.ld, Bl, h, w, ct.c1, ct.c2, i == 0 ? freeu_b1 : freeu_b2,
                                     i == 0 ? freeu_s1 : freeu_s2, s);
                prof_close(s);
            }
            const bool last = last_in_block && i == nb - 1;
            // destination of this layer's output: next cat's hidden half, an upsample input, or the tail
            View dst;
            const size_t mk = a.mark();
            if (!last_in_block) {
                const Cat& nx = cats[(size_t)k + 1];
                dst = View(nx.p, nx.c1 + nx.c2, nx.c1);
            } else {
                dst = View(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout);
            }
            // The input is a concatenation [hidden | skip] written by two producers.  On the big maps both left summaries
            // (the hidden half's over sub-groups narrow enough that no group of the concatenation straddles one:
            // gn_cat_unit): one small launch merges them per group and norm1 runs its apply pass only.  Otherwise norm1
            // computes its own statistics.
            const long HWc = (long)h * w;
            const int Ccat = ct.c1 + ct.c2, si = nskip - 1 - k;
            GnStatBuf catst;
            const GnStatBuf* xin_stats = nullptr;
            if (!no_cat_stats && !fu && hid_ready && hid_ready->st.part && sst[(size_t)si].st.part && gn_wants_stats(HWc, Ccat, G) &&
                ct.c2 % G == 0 && (Ccat / G) % (ct.c2 / G) == 0 && ct.c1 % (ct.c2 / G) == 0) {
                float* fin = a.alloc_f((long)B * G * 2);
                if (go && !c.err) {
                    prof_open(s, "gn_cat_finalize_kernel", 0.0, 8.0 * B * (hid_ready->st.S * hid_groups + sst[(size_t)si].st.S * G));
                    c.err = launch_gn_cat_finalize(hid_ready->st, hid_groups, ct.c1, sst[(size_t)si].st, G, ct.c2, fin, B, HWc, G, s);
                    prof_close(s);
                }
                catst.buf = fin;
                catst.st.part = fin; catst.st.S = 1; catst.st.rows = HWc;
                xin_stats = &catst;
            }
            hid_ready = nullptr;
            // what the NEXT concatenation's norm1 needs from this layer's output (or from the upsample convolution after it)
            int nx_groups = 0;
            if (!last && hid.buf && !no_cat_stats && !fu_next) {
                const Cat& nx = cats[(size_t)k + 1];
                const int u = gn_cat_unit(nx.c1, nx.c2, G);
                if (gn_wants_stats(last_in_block ? HWc * 4 : HWc, nx.c1 + nx.c2, G) && (u >= 8 || u == 4) && nx.c1 / u <= 128) nx_groups = nx.c1 / u;
            }
            const bool hid_here = nx_groups > 0 && !last_in_block;       // this layer's last convolution writes the hidden half
            GnStatBuf* outp = nullptr;
            xs = nullptr;
            // the last layer's summaries go to the tail, a hidden half's into `hid`; nobody reads any other output's
            const GnOut summ = last ? GnOut(&xs) : hid_here ? GnOut(&outp, &hid, nx_groups) : GnOut();
            // (a motion module behind the layer: it writes `dst`, with the summaries asked of the layer's last launch)
            const MotionModule* mm = c.motion ? &c.motion->up[(size_t)i][(size_t)j] : nullptr;
            const View xo = mm ? View(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout) : dst;
            if (cfg.up_block_has_attn[i]) {
                View tmp(a.alloc_h((long)B * h * w * r.cout), r.cout, r.cout);
                GnStatBuf* rs = nullptr;
                tap_begin(c, "up_blocks", i, "resnets", j, xin, B, h, w, tmp, h, w);
                run_resnet(c, r, xin, Bl, h, w, tmp, G, eps, tproj, temb_total, xin_stats, &rs);
                tap_end(c, "up_blocks", i, "resnets", j, tmp, B, h, w);
                tap_begin(c, "up_blocks", i, "attentions", j, tmp, B, h, w, xo, h, w);
                run_xformer(c, up_att[i][j], tmp, B, h, w, xo, G, text_kv, L, rs, mm ? GnOut() : summ);
                tap_end(c, "up_blocks", i, "attentions", j, xo, B, h, w);
            } else {
                tap_begin(c, "up_blocks", i, "resnets", j, xin, B, h, w, xo, h, w);
                run_resnet(c, r, xin, Bl, h, w, xo, G, eps, tproj, temb_total, xin_stats, mm ? GnOut() : summ);
                tap_end(c, "up_blocks", i, "resnets", j, xo, B, h, w);
            }
            if (mm) {
                tap_begin(c, "up_blocks", i, "motion_modules", j, xo, B, h, w, dst, h, w);
                run_motion(c, *mm, xo, B, c.motion_frames, h, w, dst, summ, G);
                tap_end(c, "up_blocks", i, "motion_modules", j, dst, B, h, w);
            }
            if (last) {
                final_x = dst;   // the temporary stays alive for the tail
            } else {
                if (last_in_block) {
                    const Cat& nx = cats[(size_t)k + 1];
                    View up_dst(nx.p, nx.c1 + nx.c2, nx.c1);
                    ConvArgs fu;
                    fu.up = 1;
                    fu.gn_out = nx_groups > 0 ? &hid : nullptr;
                    fu.gn_groups = nx_groups;
                    tap_begin(c, "up_blocks", i, "upsamplers", 0, dst, B, h, w, up_dst, 2 * h, 2 * w);
                    op_conv(c, up_us[i], dst, ctx_live(c, B), h, w, up_dst, fu);
                    tap_end(c, "up_blocks", i, "upsamplers", 0, up_dst, B, 2 * h, 2 * w);
                    outp = fu.gn_out;
                    h *= 2; w *= 2;
                }
                hid_ready = outp;
                hid_groups = nx_groups;
                a.release(mk);
            }
        }
    }

    // ---- tail: GN + SiLU + conv_out, back to NCHW ----
    if (pag && !pgs.widened) { set_error("unet: forward_pag reached the tail without a perturbed transformer"); return 2; }
    {
        const int C = boc[0];
        const long M = (long)B * h * w;
        if (c.tap) ctx_tap(c, "tail", kTapIn, final_x, B, h, w);                // (its output is the forward's)
        TailParams tp;
        tp.x = final_x.p; tp.ldx = final_x.ld;
        if (xs && xs->st.part) { tp.gn_part = xs->st.part; tp.gn_S = xs->st.S; tp.gn_rows = xs->st.rows; }
        tp.G = G; tp.eps = eps; tp.gamma = norm_out.gamma; tp.beta = norm_out.beta; tp.silu = 1;
        tp.w = conv_out.w; tp.K = conv_out.K; tp.bias = conv_out.bias; tp.y = out;
        tp.N = B; tp.H = h; tp.W = w; tp.C = C; tp.Cout = cfg.out_channels;
        // (dry run: xs->st is only filled by real launches; the fused tail allocates nothing, so both plans fit)
        if (go && !c.err && conv_tail_supported(tp)) {
            // GroupNorm + SiLU + convolution + NCHW in one launch (edge.hip)
            prof_open(s, "conv_tail_kernel", 2.0 * M * cfg.out_channels * 9.0 * C, 2.0 * M * (C + cfg.out_channels));
            c.err = launch_conv_tail(tp, s);
            prof_close(s);
            return c.err;
        }
        View hn(a.alloc_h(M * C), C, C);
        op_groupnorm(c, norm_out, final_x, hn, B, (long)h * w, G, eps, 1, xs);
        if (cfg.out_channels <= 4 && conv_out.ks == 3 && conv_out.K == 9L * C && M >= kSmallCoutMinPixels) {
            // dedicated HBM-bound kernel, writes NCHW directly (kernels.h: launch_conv3x3_small_cout)
            if (go && !c.err) {
                prof_open(s, "conv3x3_small_cout_kernel", 2.0 * M * cfg.out_channels * 9.0 * C, 2.0 * M * (C + cfg.out_channels));
                c.err = launch_conv3x3_small_cout(hn.p, hn.ld, conv_out.w, conv_out.K, conv_out.bias, out, B, h, w, C,
                                                  cfg.out_channels, s);
                prof_close(s);
            }
        } else {
            View y(a.alloc_h(M * cfg.out_channels), cfg.out_channels, cfg.out_channels);
            op_conv(c, conv_out, hn, B, h, w, y);
            if (go && !c.err) c.err = launch_nhwc_to_nchw(y.p, y.ld, out, B, (long)h * w, cfg.out_channels, s);
        }
    }
    return c.err;
}

// A persistent buffer grows before the pass that uses it: a growth leaves the contents undefined, so it clears the tag
// that says what they hold (a CacheTag, or the key of the captured graph that reads the staging buffer).
template <class Tag>
static int reserve_cache(DeviceBuf& buf, size_t bytes, Tag& tag) {
    bool grew = false;
    const int rc = buf.reserve(bytes, &grew);
    if (grew) tag = Tag();
    return rc;
}

UNet::~UNet() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (gstream) (void)hipStreamDestroy(gstream);
    if (ip) ip->attached = nullptr;
    for (ControlNet* n : cns) n->attached = nullptr;
    if (motion) motion->attached = nullptr;
}

// Graph path: stage I/O through engine-owned buffers, capture the forward once per shape on an
// engine-owned stream, afterwards replay it with one hipGraphLaunch fenced against the caller's
// stream by two events.
int UNet::forward_graph(const UNetCall& call, hipStream_t stream) {
    const int B = call.B, H = call.H, W = call.W, L = call.L;
    const float* const tcond = call.tcond;
    const bool sdxl = cfg.addition_time_embed_dim > 0;
    const int pdim = sdxl ? cfg.projection_class_embeddings_input_dim - num_time_ids() * cfg.addition_time_embed_dim : 0;
    const int nid = sdxl ? num_time_ids() : 0;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t n_sample = up((size_t)B * cfg.in_channels * H * W * 2), n_t = up((size_t)B * 4);
    const size_t n_ehs = up((size_t)B * L * cfg.cross_attention_dim * 2), n_text = up((size_t)B * pdim * 2);
    const size_t n_ids = up((size_t)B * nid * 4), n_out = up((size_t)B * cfg.out_channels * H * W * 2);
    const size_t n_tc = tcond ? up((size_t)B * cfg.time_cond_proj_dim * 4) : 0;
    const size_t need = n_sample + n_t + n_ehs + n_text + n_ids + n_tc + n_out;
    if (!gstream) {
        SD_HIP_CHECK(hipStreamCreateWithFlags(&gstream, hipStreamNonBlocking));
        SD_HIP_CHECK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        SD_HIP_CHECK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    }
    if (int rc = reserve_cache(io_slab, need, graph_key)) return rc;
    char* ptr = io_slab.data();
    half_t* g_sample = reinterpret_cast<half_t*>(ptr); ptr += n_sample;
    float* g_t = reinterpret_cast<float*>(ptr); ptr += n_t;
    half_t* g_ehs = reinterpret_cast<half_t*>(ptr); ptr += n_ehs;
    half_t* g_text = sdxl ? reinterpret_cast<half_t*>(ptr) : nullptr; ptr += n_text;
    float* g_ids = sdxl ? reinterpret_cast<float*>(ptr) : nullptr; ptr += n_ids;
    float* g_tc = tcond ? reinterpret_cast<float*>(ptr) : nullptr; ptr += n_tc;
    half_t* g_out = reinterpret_cast<half_t*>(ptr);
    SD_HIP_CHECK(hipMemcpyAsync(g_sample, call.sample, (size_t)B * cfg.in_channels * H * W * 2, hipMemcpyDeviceToDevice, stream));
    SD_HIP_CHECK(hipMemcpyAsync(g_t, call.timesteps, (size_t)B * 4, hipMemcpyDeviceToDevice, stream));
    SD_HIP_CHECK(hipMemcpyAsync(g_ehs, call.ehs, (size_t)B * L * cfg.cross_attention_dim * 2, hipMemcpyDeviceToDevice, stream));
    if (sdxl) {
        if (!call.add_text || !call.add_time_ids) { set_error("unet: add_text / add_time_ids required for text_time conditioning"); return 1; }
        SD_HIP_CHECK(hipMemcpyAsync(g_text, call.add_text, (size_t)B * pdim * 2, hipMemcpyDeviceToDevice, stream));
        SD_HIP_CHECK(hipMemcpyAsync(g_ids, call.add_time_ids, (size_t)B * nid * 4, hipMemcpyDeviceToDevice, stream));
    }
    if (tcond) SD_HIP_CHECK(hipMemcpyAsync(g_tc, tcond, (size_t)B * cfg.time_cond_proj_dim * 4, hipMemcpyDeviceToDevice, stream));
    GraphKey key;
    key.B = B; key.H = H; key.W = W; key.L = L; key.tcond = tcond != nullptr;
    // the same forward on the staged copies
    UNetCall staged;
    staged.sample = g_sample; staged.timesteps = g_t; staged.ehs = g_ehs; staged.L = L;
    staged.add_text = g_text; staged.add_time_ids = g_ids; staged.out = g_out;
    staged.B = B; staged.H = H; staged.W = W; staged.tcond = g_tc;
    int rc = 0;
    const GraphDeps now{arena.base(), arena.capacity(), io_slab.data()};
    if (!graph_may_replay(key, now, graph_key, graph_deps, gexec != nullptr)) {
        // (re)plan + one eager run on the caller's stream: sets every kernel's LDS attribute (not
        // allowed while capturing) and produces this call's result.  It reads the staged copies, so it stays clear of
        // the pointer-keyed caches (graph_pass), like the captured pass after it.
        graph_enabled = false;
        graph_pass = true;
        rc = forward(staged, stream);
        graph_pass = false;
        graph_enabled = true;
        if (rc) return rc;
        if (gexec) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
        hipGraph_t graph = nullptr;
        SD_HIP_CHECK(hipStreamBeginCapture(gstream, hipStreamCaptureModeRelaxed));
        Ctx ctx{&arena, gstream, false};
        arena.begin(false);
        rc = run(ctx, staged);
        hipError_t e = hipStreamEndCapture(gstream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) { set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e)); return 3; }
        if (arena.overflow()) { (void)hipGraphDestroy(graph); set_error("unet: workspace overflow while capturing (planner bug)"); return 2; }
        e = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { gexec = nullptr; set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e)); return 3; }
        graph_key = key;
        graph_deps = GraphDeps{arena.base(), arena.capacity(), io_slab.data()};     // (the eager pass may have grown the arena)
        ++graph_captures;
    } else {
        SD_HIP_CHECK(hipEventRecord(ev_in, stream));
        SD_HIP_CHECK(hipStreamWaitEvent(gstream, ev_in, 0));
        SD_HIP_CHECK(hipGraphLaunch(gexec, gstream));
        ++graph_replays;
        SD_HIP_CHECK(hipEventRecord(ev_out, gstream));
        SD_HIP_CHECK(hipStreamWaitEvent(stream, ev_out, 0));
    }
    SD_HIP_CHECK(hipMemcpyAsync(call.out, g_out, (size_t)B * cfg.out_channels * H * W * 2, hipMemcpyDeviceToDevice, stream));
    return 0;
}

int UNet::forward(const UNetCall& in, hipStream_t stream) {
    // the one copy both passes of run() receive: n_img, n_ctrl and cn_scale are normalised on it below
    UNetCall call = in;
    const int B = call.B, H = call.H, W = call.W, L = call.L;
    // MultiControlNet: the list's images / counts / scales onto the single net's fields (UNetCall::mcn)
    bool mcn_idle = false;
    call.cn_active = 0; call.cn_idx = 0;
    if (call.mcn) {
        if (call.n_nets != (int)cns.size()) { set_error("unet: forward_mcn: n_nets differs from the attached ControlNets"); return 1; }
        call.control = nullptr; call.n_ctrl = 0; call.cn_scale = 0.f;
        for (int i = 0; i < call.n_nets; ++i) {
            if (!(call.mc_scale[i] == call.mc_scale[i])) { set_error("unet: conditioning scale is NaN"); return 1; }
            if (call.mc_scale[i] == 0.f) continue;
            if (!call.mc_control[i]) { set_error("unet: forward_mcn: control image required for a ControlNet at a non-zero scale"); return 1; }
            if (call.mc_n_ctrl[i] < 1 || B <= 0 || B % call.mc_n_ctrl[i] != 0) { set_error("unet: the control image count must divide the batch"); return 1; }
            call.cn_act[call.cn_active++] = i;
        }
        mcn_idle = call.cn_active == 0;
        if (!mcn_idle) {
            const int i = call.cn_act[0];
            call.control = call.mc_control[i]; call.n_ctrl = call.mc_n_ctrl[i];
            call.cn_scale = call.cn_active == 1 ? call.mc_scale[i] : 1.f;
            call.cn_idx = i;
        }
    } else if (cns.size() > 1) {
        set_error("unet: more than one ControlNet is attached: sd_unet_forward_mcn takes their images and scales");
        return 1;
    }
    const half_t* const image_embeds = call.image_embeds;
    const half_t* const control = call.control;
    const float* const tcond = call.tcond;
    const CfgIn* const cfg_in = call.cfg_in;
    const PagIn* const pag = call.pag;
    if (!finalized) { set_error("unet: forward before finalize"); return 2; }
    if (int rc = regions_refuse(call, B, pag || call.extra)) return rc;
    if (int rc = motion_refuse(call, cfg_in ? B / 2 : B, pag || call.extra)) return rc;
    const bool motion_on = motion && call.num_frames >= 1;
    if (int rc = tap_refuses(graph_enabled || cfg_in || pag || call.extra || dc_mode != SD_DC_PLAIN)) return rc;
    if (pag && (B % (pag->groups + 1) != 0 || graph_enabled || control || image_embeds || tcond || dc_mode != SD_DC_PLAIN)) {
        set_error("unet: perturbed-attention forward not available for this call");
        return 2;
    }
    if (tcond && cfg.time_cond_proj_dim <= 0) { set_error("unet: timestep_cond given but the UNet has no time_cond_proj_dim"); return 1; }
    if (tcond && cfg_in) { set_error("unet: timestep_cond with the shared CFG prefix (a guidance-embedded UNet runs without CFG)"); return 1; }
    if (tcond && cn) { set_error("unet: timestep_cond with a ControlNet attached is not supported"); return 4; }
    if (cfg_in && ((pag ? B - B / 3 : B) % 2 != 0 || graph_enabled || control || !unet_cfg_share_eligible(cfg))) {
        set_error("unet: shared CFG prefix not available for this call");
        return 2;
    }
    const int div = 1 << (cfg.num_blocks - 1);
    if (B <= 0 || H % div != 0 || W % div != 0) { set_error("unet: H and W must be divisible by 2^(blocks-1)"); return 1; }
    // (forward_pag and forward_concat run with an attached adapter only at scale 0, where the text attention runs alone)
    // (so does a motion forward: sd_unet_forward_motion takes no image_embeds, and motion_refuse let scale 0 alone through)
    const bool text_only = pag || call.extra || (motion_on && !image_embeds);
    if (ip && !image_embeds && !text_only) { set_error("unet: an IP-Adapter is attached: image_embeds required"); return 1; }
    if (!ip && image_embeds) { set_error("unet: image_embeds given but no IP-Adapter is attached"); return 1; }
    if (ip && !text_only) {
        if (call.n_img < 1 || call.n_img * ip->n_tok > 64) { set_error("unet: images per prompt x adapter tokens must be in [1, 64]"); return 4; }
        // (with regional prompts set the adapter is at scale 0 and its kernel does not run: regions_refuse has the limit)
        if (!region_R && (L < 1 || L > 160)) { set_error("unet: with an IP-Adapter the text length must be in [1, 160]"); return 4; }
        if (graph_enabled) { set_error("unet: graph replay with an IP-Adapter attached is not supported"); return 4; }
    } else {
        call.n_img = 0;
    }
    if (cn && !control && !mcn_idle) { set_error("unet: a ControlNet is attached: control image required"); return 1; }
    if (!cn && control) { set_error("unet: control image given but no ControlNet is attached"); return 1; }
    if (cn) {
        if (!mcn_idle && (call.n_ctrl < 1 || B % call.n_ctrl != 0)) { set_error("unet: the control image count must divide the batch"); return 1; }
        if (!(call.cn_scale == call.cn_scale)) { set_error("unet: conditioning scale is NaN"); return 1; }
        if (graph_enabled) { set_error("unet: graph replay with a ControlNet attached is not supported"); return 4; }
    } else {
        call.n_ctrl = 0;
        call.cn_scale = 0.f;
    }
    const bool use_cn = cn && call.cn_scale != 0.f;
    if (freeu_on && graph_enabled) { set_error("unet: graph replay with FreeU enabled is not supported"); return 4; }
    // token merging: which blocks merge at this shape, and their plan buffers, before anything is launched
    const bool tome_on = tome.ratio > 0.0;
    tome.plan_off.clear();
    tome.buf = nullptr;
    if (tome_on) {
        if (graph_enabled) { set_error("unet: graph replay with token merging enabled is not supported"); return 4; }
        if (pag) { set_error("unet: forward_pag with token merging enabled is not supported"); return 4; }
        if (call.extra) { set_error("unet: forward_concat with token merging enabled is not supported"); return 4; }
        // (no test composes these with token merging yet: refused, not silently trusted)
        if (freeu_on) { set_error("unet: FreeU with token merging enabled is not supported"); return 4; }
        if (cn) { set_error("unet: a ControlNet attached with token merging enabled is not supported"); return 4; }
        if (ip) { set_error("unet: an IP-Adapter attached with token merging enabled is not supported"); return 4; }
        std::vector<TomeUsed> sites;
        size_t bytes = 0;
        if (int rc = tome_layout(B, H, W, &sites, &bytes)) return rc;
        bool grew = false;
        if (int rc = tome_buf.reserve(bytes > 0 ? bytes : 256, &grew)) return rc;
        tome.buf = tome_buf.data();
        for (const TomeUsed& u : sites) {
            if ((size_t)u.site >= tome.plan_off.size()) tome.plan_off.resize((size_t)u.site + 1, -1);
            tome.plan_off[(size_t)u.site] = u.plan_off;
        }
        tome_used.clear();
        tome.used = &tome_used;
    }
    // HyperTile: refused before anything is launched where the division cannot change per step or attn1 is not an attention
    const bool ht_on = hypertile.tile_size > 0;
    if (ht_on) {
        if (tome_on) { set_error("unet: HyperTile with token merging enabled is not supported"); return 4; }
        if (graph_enabled) { set_error("unet: graph replay with HyperTile enabled is not supported"); return 4; }
        if (pag) { set_error("unet: forward_pag with HyperTile enabled is not supported"); return 4; }
        hypertile.H0 = H; hypertile.W0 = W;
        hypertile_used.clear();
        hypertile.used = &hypertile_used;
    }
    const int dc = dc_mode;
    if (dc != SD_DC_PLAIN) {
        if (dc_depth <= 0) { set_error("unet: DeepCache store / reuse mode while the depth is 0"); return 2; }
        if (graph_enabled) { set_error("unet: graph replay with a DeepCache store / reuse mode is not supported"); return 4; }
        if (use_cn) { set_error("unet: a DeepCache store / reuse mode with a running ControlNet is not supported"); return 4; }
        if (freeu_on && cfg.num_blocks < 3) {
            set_error("unet: DeepCache with FreeU needs at least three blocks (FreeU would touch the cached block)");
            return 4;
        }
        if (dc == SD_DC_REUSE && !(dc_buf.h() && dc_tag.matches(nullptr, B, H, W, cfg_in != nullptr))) {
            set_error("unet: DeepCache reuse forward without a stored step of this shape");
            return 2;
        }
        // persistent concatenation buffer [B H W, C1 + C0] of layer L-d of the last (full-resolution) up block
        const int* boc = cfg.block_out_channels;
        const int c1 = dc_depth == cfg.layers_per_block ? boc[cfg.num_blocks > 1 ? 1 : 0] : boc[0];
        if (int rc = reserve_cache(dc_buf, (size_t)B * H * W * (c1 + boc[0]) * sizeof(half_t), dc_tag)) return rc;
        if (dc == SD_DC_STORE) dc_tag.clear();       // (until this forward has run)
    }
    if (graph_enabled && !prof_enabled()) return forward_graph(call, stream);
    // persistent buffers for the text K/V and its like (outside the per-forward arena; not in forward_graph's eager pass)
    const bool caches = kv_cache_on && !graph_pass;
    if (caches) {
        if (int rc = reserve_cache(kv_cache, (size_t)B * L * kv_total * sizeof(half_t), kv_tag)) return rc;
        if (ip && !text_only)
            if (int rc = reserve_cache(ipkv_cache, (size_t)B * call.n_img * ip->n_tok * ip->kv_total * sizeof(half_t), ipkv_tag)) return rc;
        for (int k = 0; use_cn && k < (call.cn_active > 1 ? call.cn_active : 1); ++k) {
            const int i = call.cn_active > 1 ? call.cn_act[k] : call.cn_idx;
            const ControlNet* n = cns[(size_t)i];
            if (int rc = reserve_cache(cond_cache[i], (size_t)B * H * W * n->cfg.block_out_channels[0] * sizeof(half_t), cond_tag[i])) return rc;
            if (int rc = reserve_cache(cnkv_cache[i], (size_t)B * L * n->kv_total * sizeof(half_t), cnkv_tag[i])) return rc;
        }
    }
    // set_ip_adapter, set_controlnet, set_pag_layers and sd_ip_adapter_set_feature_tokens change what a key stands for:
    // they reset the plans
    PlanKey key;
    key.B = B; key.H = H; key.W = W; key.L = L;
    key.kv_cache = caches;
    key.ip_tokens = ip ? call.n_img * ip->n_tok : 0;
    key.cfg_share = cfg_in != nullptr;
    if (pag) { key.pag_groups = pag->groups; key.pag_late = pag->late; }
    key.n_ctrl = use_cn ? call.n_ctrl : 0;
    if (use_cn && call.cn_active > 1) for (int k = 0; k < call.cn_active; ++k) key.cn_n[call.cn_act[k]] = call.mc_n_ctrl[call.cn_act[k]];
    else if (use_cn) key.cn_n[call.cn_idx] = call.n_ctrl;
    key.dc_depth = dc != SD_DC_PLAIN ? dc_depth : 0;
    key.cat_rows = call.extra ? call.lat_rows : 0;
    if (tome_on) { key.tome_ratio = tome.ratio; key.tome_ds = tome_max_ds; key.tome_sx = tome.sx; key.tome_sy = tome.sy; }
    if (ht_on) { key.ht_tile = hypertile.tile_size; key.ht_swap = hypertile.swap_size; key.ht_depth = hypertile.max_depth; }
    key.motion_frames = motion_on ? call.num_frames : 0;
    if (taps.on) taps.clear();              // one forward's records at a time
    if (region_R && region_stale) {
        // the level weights were overwritten (sd_unet_poison_workspace): rebuild them from the kept copy
        if (int rc = launch_region_pyramid(reinterpret_cast<const float*>(region_src.data()),
                                           reinterpret_cast<float*>(region_buf.data()), region_Bw, region_R, region_H, region_W,
                                           cfg.num_blocks, stream))
            return rc;
        region_stale = false;
    }
    const int rc = plan_and_run(arena, stream, planned[dc], key, "unet", [&](Ctx& c) {
        c.tap = taps.on ? &taps : nullptr;
        c.tome = tome_on ? &tome : nullptr;
        c.hypertile = ht_on ? &hypertile : nullptr;
        c.motion = motion_on ? motion : nullptr;
        c.motion_frames = motion_on ? call.num_frames : 0;
        if (region_R) {
            c.region_w = reinterpret_cast<const float*>(region_buf.data());
            c.region_R = region_R; c.region_Bw = region_Bw; c.region_H = region_H; c.region_W = region_W;
        }
        return run(c, call, dc);
    });
    if (!rc && dc == SD_DC_STORE) dc_tag.set(nullptr, B, H, W, cfg_in != nullptr);
    return rc;
}

int UNet::set_regions(const float* weights, int Bw, int R, int H, int W, hipStream_t stream) {
    if (!weights || R == 0) {
        region_R = region_Bw = region_H = region_W = 0;
        region_stale = false;
        dc_tag.clear();                 // (a DeepCache feature stored with regions is stale)
        if (int rc = region_src.release()) return rc;
        return region_buf.release();
    }
    if (!finalized) { set_error("unet: set_regions before finalize"); return 2; }
    if (R < 1 || R > 8) { set_error("unet: set_regions: more than 8 regions (or fewer than 1)"); return 4; }
    const int div = 1 << (cfg.num_blocks - 1);
    if (Bw < 1 || H < 1 || W < 1 || H % div != 0 || W % div != 0) {
        set_error("unet: set_regions: Bw >= 1 and H, W divisible by 2^(blocks-1) required");
        return 1;
    }
    for (auto& st : xformer_sites()) {
        const Xformer& t = *st.second;
        if (!t.blocks.empty() && !ip_attention_supported(t.C / t.heads)) {
            set_error("unet: set_regions: head dim " + std::to_string(t.C / t.heads) + " at " + st.first +
                      " is not one the regional cross-attention runs at (32, 40, 64, 80, 160)");
            return 4;
        }
    }
    const size_t n = (size_t)Bw * R * H * W;
    bool grew = false;
    if (int rc = region_src.reserve(n * sizeof(float), &grew)) return rc;
    if (int rc = region_buf.reserve((size_t)region_level_offset(Bw, R, H, W, cfg.num_blocks) * sizeof(float), &grew)) return rc;
    SD_HIP_CHECK(hipMemcpyAsync(region_src.data(), weights, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (int rc = launch_region_pyramid(reinterpret_cast<const float*>(region_src.data()), reinterpret_cast<float*>(region_buf.data()),
                                       Bw, R, H, W, cfg.num_blocks, stream))
        return rc;
    region_R = R; region_Bw = Bw; region_H = H; region_W = W;
    region_stale = false;
    dc_tag.clear();
    return 0;
}

int UNet::regions_refuse(const UNetCall& call, int B, bool pag_or_concat) {
    if (region_R == 0) return 0;
    const char* why = nullptr;
    if (pag_or_concat) why = "forward_pag / forward_concat";
    else if (graph_enabled) why = "graph replay";
    else if (cn) why = "an attached ControlNet";
    else if (ip && ip_scale != 0.f) why = "an IP-Adapter at a non-zero scale";
    else if (call.tcond) why = "timestep_cond (forward_tc)";
    else if (tome.ratio > 0.0) why = "token merging";
    else if (dc_mode != SD_DC_PLAIN) why = "a DeepCache store / reuse mode";
    if (why) { set_error(std::string("unet: regional prompts are set: ") + why + " is not supported with them"); return 4; }
    if (call.L % region_R != 0) { set_error("unet: regional prompts: ehs_len is no multiple of the regions"); return 1; }
    if (B % region_Bw != 0) { set_error("unet: regional prompts: the weights' batch does not divide the batch"); return 1; }
    if (call.H != region_H || call.W != region_W) { set_error("unet: regional prompts: H / W differ from the ones set"); return 1; }
    if (call.L / region_R > 160) { set_error("unet: regional prompts: more than 160 tokens per region"); return 4; }
    return 0;
}

int UNet::tap_refuses(bool mode) {
    if (!taps.on || !mode) return 0;
    set_error("unet: debug taps are on (sd_unet_tap): graph replay, the shared CFG prefix, forward_pag, forward_concat and "
              "the DeepCache store / reuse modes do not run; their suites prove them against the plain forward");
    return 4;
}

int UNet::set_deep_cache(int depth) {
    if (depth < 0 || depth > cfg.layers_per_block) {
        set_error("unet: DeepCache depth must be in [0, layers_per_block]");
        return 1;
    }
    dc_depth = depth;
    dc_mode = SD_DC_PLAIN;
    dc_tag.clear();
    return depth == 0 ? dc_buf.release() : 0;
}

int UNet::set_tome(double ratio, int max_downsample, int sx, int sy, int use_rand, uint32_t seed) {
    if (!(ratio >= 0.0 && ratio <= 0.75)) { set_error("unet: token merging ratio must be in [0, 0.75]"); return 1; }
    if (ratio == 0.0) {
        dc_tag.clear();                 // (a DeepCache feature stored under other settings is stale)
        tome.ratio = 0.0;
        tome_used.clear();
        return tome_buf.release();
    }
    if (hypertile.tile_size > 0) { set_error("unet: token merging while HyperTile is on is not supported (both rewrite attn1's rows)"); return 4; }
    if (sx < 1 || sx > 8 || sy < 1 || sy > 8) { set_error("unet: token merging cell sizes sx, sy must be in 1..8"); return 1; }
    if (max_downsample != 1 && max_downsample != 2 && max_downsample != 4 && max_downsample != 8) {
        set_error("unet: token merging max_downsample must be 1, 2, 4 or 8");
        return 1;
    }
    dc_tag.clear();
    tome.ratio = ratio; tome.sx = sx; tome.sy = sy; tome.use_rand = use_rand ? 1 : 0; tome.seed = seed;
    tome_max_ds = max_downsample;
    tome_used.clear();
    return 0;
}

int UNet::set_hypertile(int tile_size, int swap_size, int max_depth, uint32_t seed) {
    if (tile_size < 0) { set_error("unet: HyperTile tile_size must be >= 0 (0: off)"); return 1; }
    if (tile_size == 0) {
        dc_tag.clear();                 // (a DeepCache feature stored under other settings is stale)
        hypertile.tile_size = 0;
        hypertile_used.clear();
        return 0;
    }
    if (swap_size < 1 || swap_size > kHyperTileMaxSwap) { set_error("unet: HyperTile swap_size must be in 1..8"); return 1; }
    if (max_depth < 0 || max_depth > 3) { set_error("unet: HyperTile max_depth must be in 0..3"); return 1; }
    if (tome.ratio > 0.0) { set_error("unet: HyperTile while token merging is on is not supported (both rewrite attn1's rows)"); return 4; }
    dc_tag.clear();
    hypertile.tile_size = tile_size; hypertile.swap_size = swap_size; hypertile.max_depth = max_depth; hypertile.seed = seed;
    hypertile_used.clear();
    return 0;
}

int UNet::tome_layout(int B, int H, int W, std::vector<TomeUsed>* sites, size_t* bytes) {
    const int nb = cfg.num_blocks;
    size_t at = 0;
    int rc = 0;
    auto visit = [&](const Xformer& t, int level) {
        const int h = H >> level, w = W >> level;
        if ((1 << level) > tome_max_ds || rc) return;
        for (size_t bi = 0; bi < t.blocks.size(); ++bi) {
            TomeGeom g;
            if ((rc = tome_geom(h, w, tome.sx, tome.sy, tome.ratio, tome.use_rand, tome.seed, tome.step,
                                (uint32_t)(t.tome_site0 + (int)bi), &g)))
                return;
            if (g.r < 1) continue;                                  // nothing to merge: the plain path, bit for bit
            if (!tome_supported(g)) {
                set_error("unet: token merging on a " + std::to_string(h) + " x " + std::to_string(w) +
                          " map is not supported (more than 16384 tokens, or no whole cell)");
                rc = 4;
                return;
            }
            TomeUsed u;
            u.site = t.tome_site0 + (int)bi; u.H = h; u.W = w; u.r = g.r; u.Tm = g.Tm; u.B = B; u.plan_off = (long)at;
            sites->push_back(u);
            at += ((size_t)tome_plan_bytes(B, g.T) + 255) & ~size_t(255);
        }
    };
    for (int i = 0; i < nb && i < (int)down_att.size(); ++i)
        for (const Xformer& t : down_att[(size_t)i]) visit(t, i);
    visit(mid_att, nb - 1);
    for (int i = 0; i < nb && i < (int)up_att.size(); ++i)
        for (const Xformer& t : up_att[(size_t)i]) visit(t, nb - 1 - i);
    *bytes = at;
    return rc;
}

bool unet_cfg_share_eligible(const sd_unet_config& cfg) {
    return cfg.addition_time_embed_dim == 0 && cfg.num_blocks >= 1 && cfg.down_block_has_attn[0] != 0 &&
           cfg.transformer_layers[0] >= 1;
}

bool UNet::cfg_share_active(bool share) const {
    // read once per process, like the other A/B switches
    static const bool off = getenv("SD_NO_CFG_SHARE") != nullptr;
    static const bool gn_cat = getenv("SD_GN_CAT") != nullptr;
    // (an attached ControlNet needs its control image: forward() says so)
    return share && !off && !gn_cat && !graph_enabled && !cn && unet_cfg_share_eligible(cfg);
}

int UNet::forward_cfg(const UNetCall& lat, float in_scale, bool share, hipStream_t stream) {
    const int B = lat.B, H = lat.H, W = lat.W;
    if (!finalized) { set_error("unet: forward before finalize"); return 2; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("unet: forward_cfg: empty batch"); return 1; }
    // (not shared it is the plain forward on the duplicated latents, which taps; under graph replay forward() refuses,
    // and nothing may be launched before it does)
    if (int rc = regions_refuse(lat, 2 * B, false)) return rc;
    if (int rc = motion_refuse(lat, B, false)) return rc;
    if (int rc = tap_refuses(cfg_share_active(share) || graph_enabled)) return rc;
    UNetCall call = lat;
    call.B = 2 * B;
    if (cfg_share_active(share)) {
        CfgIn in;
        in.latents = lat.sample;
        in.in_scale = in_scale;
        call.sample = nullptr;
        call.cfg_in = &in;
        return forward(call, stream);
    }
    // not shared: cat([latents * in_scale] * 2) and the doubled timesteps in a buffer of the engine's, then the forward
    // every caller ran before.  (One buffer: calls on one stream are ordered by it, like the graph path's staging.)
    const size_t n = (size_t)B * cfg.in_channels * H * W;
    const size_t lat_bytes = (2 * n * sizeof(half_t) + 255) & ~size_t(255);
    bool grew = false;
    if (int rc = cfg_slab.reserve(lat_bytes + 2 * (size_t)B * sizeof(float), &grew)) return rc;
    half_t* lat2 = cfg_slab.h();
    float* ts2 = reinterpret_cast<float*>(cfg_slab.data() + lat_bytes);
    if (int rc = launch_cfg_duplicate(lat.sample, lat2, (long)n, in_scale, stream)) return rc;
    if (int rc = launch_dup_f32(lat.timesteps, ts2, B, stream)) return rc;
    call.sample = lat2;
    call.timesteps = ts2;
    return forward(call, stream);
}

// ------------------------------------------------------------------------------- two-source forward (InstructPix2Pix)
int UNet::forward_concat(const UNetCall& call, hipStream_t stream) {
    const int B = call.B, Bl = call.lat_rows;
    if (!finalized) { set_error("unet: forward before finalize"); return 2; }
    if (B <= 0 || call.H <= 0 || call.W <= 0 || Bl <= 0) { set_error("unet: forward_concat: empty batch"); return 1; }
    if (int rc = regions_refuse(call, B, true)) return rc;
    // (this entry cannot name frames: with an adapter attached it would silently run without the modules)
    if (motion) { set_error("unet: forward_concat with a motion adapter attached is not supported"); return 4; }
    if (int rc = tap_refuses(true)) return rc;
    // (what the handle is set up for comes first: a ControlNet only attaches to a 4-channel UNet, which the channel check below
    // would turn away with another code)
    if (graph_enabled) { set_error("unet: forward_concat under graph replay is not supported"); return 4; }
    if (cn) { set_error("unet: forward_concat with a ControlNet attached is not supported"); return 4; }
    if (dc_mode != SD_DC_PLAIN) { set_error("unet: forward_concat in a DeepCache store / reuse mode is not supported"); return 4; }
    if (ip && ip_scale != 0.f) { set_error("unet: forward_concat with an IP-Adapter at a non-zero scale is not supported"); return 4; }
    if (cfg.time_cond_proj_dim > 0) { set_error("unet: forward_concat on a guidance-embedded UNet (timestep_cond) is not supported"); return 4; }
    // (the time embedding is computed for the B_lat latents and tiled: text_time conditioning differs per group)
    if (cfg.addition_time_embed_dim > 0) { set_error("unet: forward_concat on a text_time UNet (add_text / add_time_ids per row) is not supported"); return 4; }
    if (!call.extra || call.extra_rows < 1) { set_error("unet: forward_concat: the second source is missing"); return 1; }
    if (call.extra_channels < 1 || call.extra_channels >= cfg.in_channels || cfg.in_channels - call.extra_channels != 4) {
        set_error("unet: forward_concat: 4 latent channels + extra_channels " + std::to_string(call.extra_channels) +
                  " != in_channels " + std::to_string(cfg.in_channels));
        return 1;
    }
    if (B % Bl != 0) { set_error("unet: forward_concat: the latents must divide the batch (B % B_lat != 0)"); return 1; }
    if (B / Bl - 1 > kRowDupMax) { set_error("unet: forward_concat: more than " + std::to_string(kRowDupMax + 1) + " groups"); return 1; }
    if (call.zero_from < 0 || call.zero_from > B) { set_error("unet: forward_concat: zero_from outside [0, B]"); return 1; }
    if (!(call.in_scale == call.in_scale)) { set_error("unet: forward_concat: in_scale is NaN"); return 1; }
    return forward(call, stream);
}

// ------------------------------------------------------------------------------- perturbed-attention guidance
std::vector<std::pair<std::string, Xformer*>> UNet::xformer_sites() {
    std::vector<std::pair<std::string, Xformer*>> v;
    for (size_t i = 0; i < down_att.size(); ++i)
        for (size_t j = 0; j < down_att[i].size(); ++j)
            v.emplace_back("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), &down_att[i][j]);
    v.emplace_back("mid_block.attentions.0", &mid_att);
    for (size_t i = 0; i < up_att.size(); ++i)
        for (size_t j = 0; j < up_att[i].size(); ++j)
            v.emplace_back("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), &up_att[i][j]);
    return v;
}

int UNet::set_pag_layers(const char* const* keys, int count) {
    if (!finalized) { set_error("unet: set_pag_layers before finalize"); return 2; }
    if (count < 0 || (count > 0 && !keys)) { set_error("unet: set_pag_layers: bad arguments"); return 1; }
    auto sites = xformer_sites();
    std::vector<Xformer*> pick;
    for (int k = 0; k < count; ++k) {
        Xformer* hit = nullptr;
        for (auto& st : sites)
            if (keys[k] && st.first == keys[k]) hit = st.second;
        if (!hit || hit->blocks.empty()) {
            set_error(std::string("unet: set_pag_layers: no transformer block at '") + (keys[k] ? keys[k] : "(null)") + "'");
            return 1;
        }
        pick.push_back(hit);
    }
    for (auto& st : sites) st.second->pag = false;
    for (Xformer* x : pick) x->pag = true;
    kv_tag.clear();
    reset_plans();
    return 0;
}

int UNet::forward_pag(const UNetCall& lat, float in_scale, bool cfg_on, bool share, hipStream_t stream) {
    const int B = lat.B, H = lat.H, W = lat.W;
    if (!finalized) { set_error("unet: forward before finalize"); return 2; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("unet: forward_pag: empty batch"); return 1; }
    if (int rc = regions_refuse(lat, B, true)) return rc;
    if (motion) { set_error("unet: forward_pag with a motion adapter attached is not supported"); return 4; }
    if (int rc = tap_refuses(true)) return rc;
    if (cn) { set_error("unet: forward_pag with a ControlNet attached is not supported"); return 4; }
    if (ip && ip_scale != 0.f) { set_error("unet: forward_pag with an IP-Adapter at a non-zero scale is not supported"); return 4; }
    if (dc_mode != SD_DC_PLAIN) { set_error("unet: forward_pag in a DeepCache store / reuse mode is not supported (a reuse step has no perturbed branch)"); return 4; }
    if (graph_enabled) { set_error("unet: forward_pag under graph replay is not supported"); return 4; }
    if (cfg.time_cond_proj_dim > 0) { set_error("unet: forward_pag on a guidance-embedded UNet (timestep_cond) is not supported"); return 4; }
    // the flagged transformers in execution order: late widening needs the first of them behind the network's first
    int first_flagged = -1, idx = 0;
    for (auto& st : xformer_sites()) {
        if (st.second->pag && first_flagged < 0) first_flagged = idx;
        ++idx;
    }
    if (first_flagged < 0) { set_error("unet: forward_pag without perturbed layers (sd_unet_set_pag_layers)"); return 1; }
    static const bool off = getenv("SD_NO_PAG_SHARE") != nullptr;
    static const bool gn_cat = getenv("SD_GN_CAT") != nullptr;
    PagIn pag;
    pag.groups = cfg_on ? 2 : 1;
    pag.late = share && !off && !gn_cat && first_flagged > 0;
    const int G = pag.groups, N = (G + 1) * B;
    UNetCall call = lat;
    call.B = N;
    call.pag = &pag;
    if (pag.late && cfg_on && cfg_share_active(true)) {
        // B latents -> 2B at the first cross-attention (the CFG-shared start) -> 3B at the first flagged transformer
        CfgIn in;
        in.latents = lat.sample;
        in.in_scale = in_scale;
        call.sample = nullptr;
        call.cfg_in = &in;
        return forward(call, stream);
    }
    // the scaled latents and the timesteps once per group, in the buffer forward_cfg's duplicate path uses (late: the
    // un-perturbed groups only are read)
    const size_t n = (size_t)B * cfg.in_channels * H * W;
    const size_t lat_bytes = ((G + 1) * n * sizeof(half_t) + 255) & ~size_t(255);
    bool grew = false;
    if (int rc = cfg_slab.reserve(lat_bytes + (size_t)N * sizeof(float), &grew)) return rc;
    half_t* latN = cfg_slab.h();
    float* ts = reinterpret_cast<float*>(cfg_slab.data() + lat_bytes);
    if (int rc = launch_cfg_duplicate(lat.sample, latN, (long)n, in_scale, stream)) return rc;
    if (int rc = launch_dup_f32(lat.timesteps, ts, B, stream)) return rc;
    if (G == 2) {
        if (int rc = launch_scale_copy_f16(lat.sample, latN + 2 * n, (long)n, in_scale, stream)) return rc;
        SD_HIP_CHECK(hipMemcpyAsync(ts + 2 * B, lat.timesteps, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    call.sample = latN;
    call.timesteps = ts;
    return forward(call, stream);
}

}  // namespace sd
