// ControlNetModel (diffusers 0.27.2) on the gfx950 kernels, run inside the UNet forward.
//
// The ControlNet is an encoder copy of the UNet topology (Encoder: conv_in, time / add embedding, down path, mid block)
// whose conv_in output is offset by the conditioning embedding of the control image, plus one 1x1 "zero conv" per skip
// and one for the mid block.  The UNet runs it after its own time embedding and text K / V, keeps its pre-zero-conv
// hidden tensors in the arena, and adds s (h W^T + b) into its skips and mid-block output after its own mid block,
// before the up path reads them (UNet::run).
#include "model.h"

namespace sd {

namespace {
const char* kCond = "controlnet_cond_embedding";
// ControlNetConditioningEmbedding with conditioning_embedding_out_channels = (16, 32, 96, 256)
const int kCondOut[ControlNet::kCondLayers] = {16, 16, 32, 32, 96, 96, 256};
const int kCondStride[ControlNet::kCondLayers] = {1, 1, 2, 1, 2, 1, 2};
std::string cond_name(int l) { return l == 0 ? std::string(kCond) + ".conv_in" : std::string(kCond) + ".blocks." + std::to_string(l - 1); }
}  // namespace

ControlNet::ControlNet(const sd_unet_config& c, int conditioning_channels) : Encoder(c), cond_channels(conditioning_channels) {
    declare_encoder();
    int cin = cond_channels;
    for (int l = 0; l < kCondLayers; ++l) {
        cond_cin[l] = cin; cond_cout[l] = kCondOut[l]; cond_stride[l] = kCondStride[l];
        ws.declare(cond_name(l) + ".weight", {kCondOut[l], cin, 3, 3});
        ws.declare(cond_name(l) + ".bias", {kCondOut[l]});
        cin = kCondOut[l];
    }
    const int c0 = cfg.block_out_channels[0];
    ws.declare(std::string(kCond) + ".conv_out.weight", {c0, cin, 3, 3});
    ws.declare(std::string(kCond) + ".conv_out.bias", {c0});
    // one zero conv per skip, in down-path order (conv_in, every resnet / transformer output, every downsampler)
    int si = 0;
    auto zc = [&](int C) {
        const std::string p = "controlnet_down_blocks." + std::to_string(si++);
        ws.declare(p + ".weight", {C, C, 1, 1});
        ws.declare(p + ".bias", {C});
    };
    zc(c0);
    for (int i = 0; i < cfg.num_blocks; ++i) {
        for (int j = 0; j < cfg.layers_per_block; ++j) zc(cfg.block_out_channels[i]);
        if (i != cfg.num_blocks - 1) zc(cfg.block_out_channels[i]);
    }
    const int mid = cfg.block_out_channels[cfg.num_blocks - 1];
    ws.declare("controlnet_mid_block.weight", {mid, mid, 1, 1});
    ws.declare("controlnet_mid_block.bias", {mid});
}

ControlNet::~ControlNet() {
    if (attached) attached->drop_controlnet(this);
}

int ControlNet::finalize() {
    if (finalized) return 0;
    std::string missing;
    if (!ws.complete(&missing)) { set_error("controlnet finalize: weight not set: " + missing); return 2; }
    int rc;
    std::vector<std::string> tw, tb;
    temb_total = 0;
    kv_total = 0;
    kv_keys.clear();
    if ((rc = pack_encoder(&tw, &tb))) return rc;
    for (int l = 0; l < kCondLayers; ++l) {
        cond_w[l] = static_cast<float*>(ws.dmalloc((size_t)cond_cout[l] * cond_cin[l] * 9 * sizeof(float)));
        cond_b[l] = static_cast<float*>(ws.dmalloc((size_t)cond_cout[l] * sizeof(float)));
        if (!cond_w[l] || !cond_b[l]) return 3;
        if ((rc = launch_cn_pack_cond(ws.raw(cond_name(l) + ".weight")->dev, cond_w[l], cond_cout[l], cond_cin[l], 0))) return rc;
        if ((rc = launch_f16_to_f32(ws.raw(cond_name(l) + ".bias")->dev, cond_b[l], cond_cout[l], 0))) return rc;
    }
    if ((rc = ws.pack_conv(std::string(kCond) + ".conv_out", &cond_out))) return rc;
    zero.assign((size_t)num_skips(), ConvW());
    for (int si = 0; si < num_skips(); ++si)
        if ((rc = ws.pack_conv("controlnet_down_blocks." + std::to_string(si), &zero[(size_t)si]))) return rc;
    if ((rc = ws.pack_conv("controlnet_mid_block", &zero_mid))) return rc;
    if ((rc = ws.pack_rows(tw, tb, &temb_stack))) return rc;
    if (!kv_keys.empty() && (rc = ws.pack_rows(kv_keys, {}, &kv_all))) return rc;
    kv_keys.clear();
    SD_HIP_CHECK(hipDeviceSynchronize());
    ws.free_raw();
    finalized = true;
    return 0;
}

void ControlNet::run_cond_embed(Ctx& c, const half_t* image, int n, int H, int W, View out) {
    Arena& a = *c.arena;
    const size_t mk = a.mark();
    const half_t* x = image;
    int ih = 8 * H, iw = 8 * W;
    for (int l = 0; l < kCondLayers; ++l) {
        CnCondConvParams p;
        p.x = x; p.nchw = l == 0;
        p.w = cond_w[l]; p.bias = cond_b[l];
        p.N = n; p.IH = ih; p.IW = iw; p.Cin = cond_cin[l]; p.Cout = cond_cout[l]; p.stride = cond_stride[l]; p.silu = 1;
        p.OH = (ih - 1) / p.stride + 1; p.OW = (iw - 1) / p.stride + 1;
        half_t* y = a.alloc_h((long)n * p.OH * p.OW * p.Cout);
        p.y = y;
        if (!c.dry && !c.err) {
            const double M = (double)n * p.OH * p.OW;
            prof_open(c.stream, "cn_cond_conv_kernel", 2.0 * M * p.Cout * 9.0 * p.Cin, 2.0 * (M * p.Cout + (double)n * ih * iw * p.Cin));
            c.err = launch_cn_cond_conv(p, c.stream);
            prof_close(c.stream);
        }
        x = y; ih = p.OH; iw = p.OW;
    }
    // (ih, iw) == (H, W): 8H halves three times
    op_conv(c, cond_out, View(const_cast<half_t*>(x), cond_cout[kCondLayers - 1], cond_cout[kCondLayers - 1]), n, H, W, out);
    a.release(mk);
}

int ControlNet::run(Ctx& c, const UNetCall& call, View text_kv, View emb, const std::vector<View>& sites, View mid) {
    const int B = call.B, H = call.H, W = call.W, L = call.L;
    Arena& a = *c.arena;
    const int G = cfg.norm_num_groups;
    const size_t mk = a.mark();
    float* tproj = nullptr;
    if (int rc = run_temb(c, call.timesteps, call.add_text, call.add_time_ids, B, &tproj)) return rc;
    // GroupNorm summaries: every hidden tensor is read by the next layer only (the zero conv needs none), so the ring
    ctx_gnpool_init(c, B, (long)H * W, G);
    auto stat = [&](int, long HW, int C) -> GnStatBuf* { return gn_wants_stats(HW, C, G) ? ctx_gnbuf(c) : nullptr; };
    GnStatBuf* xs = nullptr;
    // conv_in(sample) + conditioning embedding in one GEMM (the embedding rides on the residual epilogue)
    run_conv_in(c, call.sample, B, H, W, sites[0], stat(0, (long)H * W, cfg.block_out_channels[0]), &emb, &xs);
    int h = H, w = W;
    View x = run_down(c, sites[0], xs, B, h, w, text_kv, L, tproj, [&](int si) { return sites[(size_t)si]; }, stat);
    run_mid(c, x, xs, B, h, w, text_kv, L, tproj, mid);
    a.release(mk);
    return c.err;
}

int UNet::set_controlnets(ControlNet* const* nets, int count) {
    const std::vector<ControlNet*> want(nets, nets + count);
    if (want == cns) return 0;
    // the folded weights of every site, sized for all the nets of the list (one net folds nothing)
    std::vector<long> woff, boff;
    long wtot = 0, btot = 0;
    if (count > 1) {
        const int nsites = num_skips() + 1;
        for (int si = 0; si < nsites; ++si) {
            const ConvW& z = si < nsites - 1 ? want[0]->zero[(size_t)si] : want[0]->zero_mid;
            const long rows = weight_rows(z.cout);
            woff.push_back(wtot); boff.push_back(btot);
            wtot += rows * count * z.K;
            btot += rows;
        }
        bool grew = false;
        if (int rc = cn_wcat.reserve((size_t)wtot * sizeof(half_t), &grew)) return rc;
        if (int rc = cn_bcat.reserve((size_t)btot * sizeof(float), &grew)) return rc;
    }
    for (ControlNet* o : cns) o->attached = nullptr;
    for (ControlNet* n : want) {
        if (n->attached && n->attached != this) n->attached->drop_controlnet(n);
        n->attached = this;
    }
    cns = want;
    cn = cns.empty() ? nullptr : cns[0];
    cn_wcat_off = woff; cn_bcat_off = boff;
    cn_fold_tag = CnFoldTag();
    clear_cn_tags();
    dc_tag.clear();
    reset_plans();
    return 0;
}

void UNet::drop_controlnet(ControlNet* n) {
    std::vector<ControlNet*> rest;
    for (ControlNet* o : cns)
        if (o != n) rest.push_back(o);
    n->attached = nullptr;
    (void)set_controlnets(rest.data(), (int)rest.size());      // (a shorter list needs no larger buffer: it cannot fail)
}

const ConvW& UNet::cn_zero(int i, int si) const {
    const ControlNet* n = cns[(size_t)i];
    return si < (int)n->zero.size() ? n->zero[(size_t)si] : n->zero_mid;
}

int UNet::cn_fold(const int* idx, const float* scale, int n, hipStream_t s) {
    bool same = cn_fold_tag.valid && cn_fold_tag.n == n;
    for (int j = 0; j < n && same; ++j) same = cn_fold_tag.idx[j] == idx[j] && cn_fold_tag.scale[j] == scale[j];
    if (same) return 0;
    CnFoldParams fp;
    fp.n = n;
    const int nsites = num_skips() + 1;
    for (int si = 0; si < nsites; ++si) {
        CnFoldSite& q = fp.s[fp.count++];
        const ConvW& z0 = cn_zero(idx[0], si);
        for (int j = 0; j < n; ++j) { q.w[j] = cn_zero(idx[j], si).w; q.bias[j] = cn_zero(idx[j], si).bias; }
        q.w_cat = cn_wcat.h() + cn_wcat_off[(size_t)si];
        q.b_cat = reinterpret_cast<float*>(cn_bcat.data()) + cn_bcat_off[(size_t)si];
        q.rows = (int)weight_rows(z0.cout); q.C = (int)z0.K;
        q.first = fp.total;
        fp.total += cn_fold_blocks(q.rows, q.C, n);
    }
    for (int j = 0; j < n; ++j) fp.scale[j] = scale[j];
    cn_fold_tag.valid = false;
    prof_open(s, "cn_fold_scales_kernel", 0.0, 0.0);
    const int rc = launch_cn_fold_scales(fp, s);
    prof_close(s);
    if (rc) return rc;
    cn_fold_tag.valid = true; cn_fold_tag.n = n;
    for (int j = 0; j < n; ++j) { cn_fold_tag.idx[j] = idx[j]; cn_fold_tag.scale[j] = scale[j]; }
    ++cn_fold_count;
    return 0;
}

int UNet::run_controlnet(Ctx& c, const UNetCall& call, int net, const std::vector<View>& sites, View mid) {
    ControlNet* const cn = cns[(size_t)net];
    DeviceBuf& cond_cache = this->cond_cache[net];
    DeviceBuf& cnkv_cache = this->cnkv_cache[net];
    CacheTag& cond_tag = this->cond_tag[net];
    CacheTag& cnkv_tag = this->cnkv_tag[net];
    const half_t* const ehs = call.ehs;
    const half_t* const control = call.control;
    const int B = call.B, H = call.H, W = call.W, L = call.L, n_ctrl = call.n_ctrl;
    Arena& a = *c.arena;
    const bool go = !c.dry;
    hipStream_t s = c.stream;
    const int C0 = cn->cfg.block_out_channels[0];
    const long HWC = (long)H * W * C0;
    // ---- conditioning embedding [B H W, C0]: n_ctrl images computed once, sample b reads image b mod n_ctrl (diffusers'
    //      cat([image] * 2) under CFG); kept across the loop like the text K / V.  The planning pass always takes the
    //      computing branch (see the IP-Adapter's K / V). ----
    const bool cached = ptr_caches_live() && cond_cache.h() != nullptr;
    half_t* cond = cached ? cond_cache.h() : a.alloc_h((long)B * HWC);
    const bool hit = cached && cond_tag.matches(control, B, n_ctrl, H, W);
    if (c.dry || !hit) {
        cn->run_cond_embed(c, control, n_ctrl, H, W, View(cond, C0, C0));
        for (int b = n_ctrl; b < B && go && !c.err; b += n_ctrl) {
            const hipError_t e = hipMemcpyAsync(cond + (long)b * HWC, cond, (size_t)n_ctrl * HWC * sizeof(half_t),
                                                hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { set_error(hipGetErrorString(e)); c.err = 3; }
        }
        if (cached && go && !c.err) cond_tag.set(control, B, n_ctrl, H, W);
    }
    // ---- the ControlNet's own text K / V ----
    const int ctx = cfg.cross_attention_dim;
    const bool kc = ptr_caches_live() && cnkv_cache.h() != nullptr;
    View kv(kc ? cnkv_cache.h() : a.alloc_h((long)B * L * cn->kv_total), cn->kv_total, cn->kv_total);
    const bool khit = kc && cnkv_tag.matches(ehs, B, L);
    if (c.dry || !khit) {
        op_conv(c, cn->kv_all, View(const_cast<half_t*>(ehs), ctx, ctx), B, L, 1, kv);
        if (kc && go && !c.err) cnkv_tag.set(ehs, B, L);
    }
    // ---- the encoder, without IP-Adapter image attention (diffusers' ControlNet attention processors are plain) ----
    const View ip_kv = c.ip_kv;
    c.ip_kv = View();
    const int rc = cn->run(c, call, kv, View(cond, C0, C0), sites, mid);
    c.ip_kv = ip_kv;
    return rc;
}

}  // namespace sd
