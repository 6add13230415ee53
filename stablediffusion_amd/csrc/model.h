// Model graphs (UNet2DConditionModel, AutoencoderKL) assembled from the gfx950 kernels.
#pragma once
#include "../../include/sd_engine.h"
#include "engine.h"

#include <functional>

namespace sd {

const std::string& last_error();

struct Resnet {
    NormW n1, n2;
    ConvW c1, c2, sc;
    bool has_sc = false;
    int temb_off = -1;
    int cin = 0, cout = 0;
};
struct TBlock {
    NormW ln1, ln2, ln3;
    ConvW qkv, out1, q2, out2, ff1, ff2;
    int kv_off = 0;     // column offset of this block's [K | V] text projection in UNet::kv_all
    int ip_kv_off = 0;  // column offset of its [K_ip | V_ip] image projection in IPAdapter::kv_all (same site order)
    bool fold = false;  // ln1 / ln2 / ln3 are folded into qkv / q2 / ff1 (no LayerNorm launches)
};
struct Xformer {
    NormW gn;
    ConvW pin, pout;
    std::vector<TBlock> blocks;
    int C = 0, heads = 1;
    // proj_out folded over the last block's ff.net.2 (pack_xformer_tail): ff2p = [W_po W_ff2 | W_po] is packed INSTEAD of
    // that block's ff2 and of pout, and run_xformer_tail issues one GEMM over [g | t3] where two ran.
    bool pout_fold = false;
    ConvW ff2p;
    // perturbed-attention guidance (sd_unet_set_pag_layers): in a forward_pag call the perturbed group's attn1 of every
    // block here is to_out(to_v(norm1(x))), the identity attention map
    bool pag = false;
    // ordinal of blocks[0] among all BasicTransformerBlocks of the UNet in execution order (UNet::finalize): the `site` of
    // token merging's destination draw
    int tome_site0 = 0;
};
struct VaeAttn {
    NormW gn;
    ConvW qkv, out;
    int C = 0;
};

// x_stats: GroupNorm summaries of x left by the convolution that produced it (or nullptr);
// out_stats: where the block leaves the summaries of `out` for the GroupNorm that consumes it next (GnOut below).
// stream_scale s (a power of two, the VAE encoder's range-scaled form): x and out hold s times the block's true input /
// output.  GroupNorm is invariant to the scale of its input up to eps, so norm1 / norm2 run with eps * s^2, conv1 /
// conv2 emit s * (conv + bias), the shortcut (whose input carries s already) only scales its bias: the block computes the
// same function, with every stored activation s times smaller.
// Shared CFG prefix (UNet::run with a CfgIn): the N images are the two halves of a classifier-free-guidance batch built
// from the same N / 2 latents, and up to the first cross-attention of the first transformer nothing tells the halves
// apart.  The layers before it run on the first N / 2 images only; `segs` are the tensors the caller wants widened to N
// images (second half = first half) in the one copy launch run_xformer issues in front of that cross-attention, together
// with its own (its input, which proj_out adds back, t2 and the attn2 query).
struct CfgShare {
    std::vector<RowDupSeg> segs;
};

// The GroupNorm summaries of `out` that a block asks of its last launch, for the GroupNorm that reads `out` next.
struct GnOut {
    // receives the buffer the launch is asked to write them into, or nullptr where it is asked for none (a map whose
    // GroupNorm takes no summaries: gn_wants_stats).  nullptr here: nobody reads them, the launch is asked for none.
    GnStatBuf** report;
    GnStatBuf* buf;     // that buffer, instead of the next ring slot: a skip's summaries live until the up path reads them
    // instead of G groups: an output that becomes the hidden half of a concatenation is summarised over the sub-groups
    // that concatenation's GroupNorm can merge (gn_cat_unit)
    int groups;
    GnOut(GnStatBuf** report_ = nullptr, GnStatBuf* buf_ = nullptr, int groups_ = 0) : report(report_), buf(buf_), groups(groups_) {}
};
// `o` as the request of the launch that writes HW pixels of C channels per image (a->gn_out, a->gn_groups); reports the buffer
inline void gn_out_resolve(Ctx& c, const GnOut& o, long HW, int C, int G, ConvArgs* a) {
    a->gn_out = (o.report && gn_wants_stats(HW, C, G)) ? (o.buf ? o.buf : ctx_gnbuf(c)) : nullptr;
    a->gn_groups = o.groups > 0 ? o.groups : G;
    if (o.report) *o.report = a->gn_out;
}

void run_resnet(Ctx& c, const Resnet& r, View x, int N, int H, int W, View out, int G, float eps,
                const float* tproj, int tproj_ld, const GnStatBuf* x_stats = nullptr, const GnOut& out_stats = GnOut(),
                float stream_scale = 1.f);
void run_xformer(Ctx& c, const Xformer& t, View x, int N, int H, int W, View out, int G, View text_kv, int L,
                 const GnStatBuf* x_stats = nullptr, const GnOut& out_stats = GnOut(), const CfgShare* share = nullptr);

// The end of a transformer, from the residual stream after attn2 (t3, row statistics st_t3 when the LayerNorms are
// folded) to its output: out = proj_out(t3 + ff(norm3(t3))) + x, with `fo` (the GroupNorm-summary request) on the launch
// that writes `out`.  Packed by pack_xformer_tail (after the last block's ff1), in one of two forms:
//   folded (t.pout_fold): t3 is the view xformer_tail_t3 returned, the last C columns of an [M, hidden + C] buffer; the
//     GEGLU projection writes g into the columns in front and one GEMM with K = hidden + C does ff.net.2, its residual
//     and proj_out, on the tile the tuned table holds for the unfolded ff.net.2 of the same M;
//   unfolded: the feed-forward (one fused launch where ffn.hip takes it, else two GEMMs) into nxt, then proj_out.
// n: scratch [M, C] for the unfolded LayerNorm (SD_NO_LN_FOLD), nxt: scratch [M, C].  Returns whether ffn.hip ran.
int pack_xformer_tail(WeightStore& ws, const std::string& proj_out, const std::string& ff2, Xformer* x, TBlock* last);
View xformer_tail_t3(Arena& a, const Xformer& t, long M);
bool run_xformer_tail(Ctx& c, const Xformer& t, View t3, const RowStat& st_t3, View n, View nxt, View x, int N, int H, int W,
                      View out, const ConvArgs& fo);

struct UNet;
struct UNetCall;

// AnimateDiff motion adapter (motion.cpp; diffusers 0.27.2 MotionAdapter, recalled): one module per (resnet, transformer)
// pair of the down and up blocks and, optionally, one in the mid block.  A module is GroupNorm(32) over a whole video,
// proj_in, one transformer block whose two attentions are self-attention over the frames of a pixel, proj_out, + x.
struct MotionModule {
    NormW gn, ln1, ln2, ln3;            // (the LayerNorms are folded into qkv1 / qkv2 / ff1)
    ConvW pin, pout, qkv1, out1, qkv2, out2, ff1, ff2;
    float* pb1 = nullptr;               // position tables [max_seq_length][3C] fp32 of attn1 / attn2 (launch_motion_pos_bias)
    float* pb2 = nullptr;
    int C = 0, heads = 1;
};
struct MotionAdapter {
    explicit MotionAdapter(const sd_motion_config& m);
    ~MotionAdapter();
    int finalize();

    sd_motion_config mcfg;
    WeightStore ws;
    bool finalized = false;
    std::vector<std::vector<MotionModule>> down, up;
    MotionModule mid;
    UNet* attached = nullptr;

  private:
    int pack_module(const std::string& p, int heads, MotionModule* m);
};
// out = module(x) on N = V F frames of H x W, the frames of a video consecutive; out_stats / G_out: the GroupNorm
// summaries its last launch leaves (GnOut).  x and out may not overlap.
void run_motion(Ctx& c, const MotionModule& m, View x, int N, int F, int H, int W, View out, const GnOut& out_stats, int G_out);
void op_temporal_attention(Ctx& c, View qkv, const float* bias, View out, int V, int F, int HW, int heads, int d);

// Every attn2 of a UNet topology as (transformer block prefix, channels): diffusers' attn_processors order
// (down, up, mid) with mid_last, the engine's kv_all order (down, mid, up) without.
std::vector<std::pair<std::string, int>> unet_xattn_sites(const sd_unet_config& cfg, bool mid_last);

// IP-Adapter image prompt bound to a UNet topology (diffusers 0.27.2 ImageProjection + IPAdapterAttnProcessor2_0):
// tokens = LayerNorm(reshape(image_embeds x W_proj^T + b, [n_tok, ctx])), then at every attn2
// o = SDPA(q, K_text, V_text) + scale * SDPA(q, tokens W_k_ip^T, tokens W_v_ip^T).
//
// IP-Adapter Plus (kind SD_IP_PROJ_RESAMPLER) replaces the projection by the perceiver Resampler of the IP-Adapter
// repository: n_tok learned latents attend, over `depth` layers, to the tower's penultimate hidden states
// [T_feat, d_img] per image and to themselves (one softmax over both), each layer followed by an erf-GELU
// feed-forward; tokens = LayerNorm(proj_out(latents)).  Everything after the tokens is the same.
struct ResamplerLayer {
    NormW norm1, norm2, ff_ln;          // of the features, of the latents, in front of the feed-forward
    ConvW to_q, to_kv, to_out, ff1, ff2;    // no biases; to_q carries log2(e) / 8
};
struct IPAdapter {
    IPAdapter(const sd_unet_config& c, const sd_ip_projection_config& p);
    int finalize();
    // image_embeds -> tok [rows n_tok, ctx] (rows = B n_img): image_embeds is [rows, d_img] for the linear kind,
    // [rows, t_feat, d_img] for the Resampler.  Temporaries come from c.arena; the caller marks and releases.
    void run_tokens(Ctx& c, const half_t* image_embeds, long rows, half_t* tok);
    // run_tokens on the adapter's own arena (sd_ip_adapter_project: tests and tools)
    int project(const half_t* image_embeds, long rows, half_t* tok, hipStream_t stream);

    sd_unet_config cfg;
    int kind = SD_IP_PROJ_LINEAR;
    int d_img = 0, n_tok = 0;
    WeightStore ws;
    bool finalized = false;
    ConvW proj;                         // image_embeds linear [n_tok ctx][d_img]
    NormW norm;                         // LayerNorm over ctx, eps 1e-5 (the Resampler's norm_out)
    ConvW kv_all;                       // every to_k_ip / to_v_ip, row-concatenated in UNet::kv_all's site order
    int kv_total = 0;
    UNet* attached = nullptr;           // the UNet it is attached to (sd_unet_set_ip_adapter), if any
    // Resampler
    int dim = 0, heads = 0, depth = 0, ff_mult = 0;
    int t_feat = 257;                   // feature tokens per image (sd_ip_adapter_set_feature_tokens)
    half_t* latents = nullptr;          // [n_tok][dim]
    ConvW proj_in, proj_out;
    std::vector<ResamplerLayer> layers;
    Arena arena;                        // project()'s workspace
    long planned_rows = -1;
};

// conv_in, time / add embedding, down path and mid block of a UNet2DConditionModel topology: the part a UNet and a
// ControlNet (its encoder copy) share -- weight declaration, packing and the forward pieces.
struct Encoder {
    explicit Encoder(const sd_unet_config& c) : cfg(c) {}

    sd_unet_config cfg;
    WeightStore ws;
    ConvW conv_in, te1, te2, ae1, ae2, temb_stack;
    ConvW tcp;                          // time_embedding.cond_proj (time_cond_proj_dim > 0: guidance-embedded UNets), no bias
    ConvW kv_all;                       // every attn2.to_k / to_v of the model, row-concatenated
    std::vector<std::string> kv_keys;   // (finalize only)
    std::vector<std::vector<Resnet>> down_res;
    std::vector<std::vector<Xformer>> down_att;
    std::vector<ConvW> down_ds;
    Resnet mid_r0, mid_r1;
    Xformer mid_att;
    int temb_total = 0;
    int kv_total = 0;

    // columns of add_time_ids (text_time conditioning): 6 for SDXL base and for a zero field, 5 for the SDXL refiner
    int num_time_ids() const { return cfg.num_time_ids ? cfg.num_time_ids : 6; }

    // Skip tensors the down path produces, in order: conv_in's output, every down resnet / transformer output, every
    // downsampler output (the residual sites of a ControlNet, the skips of a UNet).
    int num_skips() const;
    // where skip `si` goes and which GroupNorm-summary buffer its producer fills (nullptr: a ring slot or none)
    using SkipDst = std::function<View(int si)>;
    using SkipStat = std::function<GnStatBuf*(int si, long HW, int C)>;

  protected:
    void declare_encoder();
    int pack_encoder(std::vector<std::string>* tw, std::vector<std::string>* tb);
    int pack_resnet(const std::string& p, Resnet* r, std::vector<std::string>* tw, std::vector<std::string>* tb);
    int pack_xformer(const std::string& p, Xformer* x, int heads, int depth);
    // time (+ text_time) embedding -> every resnet's time_emb_proj(silu(emb)) in one GEMV: [B, temb_total] fp32
    // (rows_alloc > B: the buffer is sized for that many rows, the first B are written)
    // tcond [B, time_cond_proj_dim] fp32 (or nullptr): cond_proj(tcond) is added to the sinusoid, in its launch
    int run_temb(Ctx& c, const float* timesteps, const half_t* add_text, const float* add_time_ids, int B, float** tproj,
                 int rows_alloc = 0, const float* tcond = nullptr);
    // conv_in into y0: straight from the NCHW latents when the edge kernel takes it and there is no residual, else
    // im2col + GEMM with `res` added in its epilogue.  *xs = the GroupNorm summaries of y0 it left (or nullptr).
    // cat (a call in two-source mode): `sample` holds the latents alone; one launch from both sources where
    // conv_head2_supported, otherwise the concatenated sample is built in the arena and takes the path above.
    void run_conv_in(Ctx& c, const half_t* sample, int B, int H, int W, View y0, GnStatBuf* gb, const View* res,
                     GnStatBuf** xs, const UNetCall* cat = nullptr);
    // down path from x = skip 0 (summaries xs) at h x w: writes skips 1.. through dst / stat, returns the last one.
    // share: x, xs and tproj hold the first B / 2 images; the first resnet and the start of the first transformer run on
    // those (CfgShare), everything after on all B.
    View run_down(Ctx& c, View x, GnStatBuf*& xs, int B, int& h, int& w, View text_kv, int L, const float* tproj,
                  const SkipDst& dst, const SkipStat& stat, const CfgShare* share = nullptr, int stop_after = -1);
    void run_mid(Ctx& c, View x, GnStatBuf* xs, int B, int h, int w, View text_kv, int L, const float* tproj, View dst);
};

// ControlNet (diffusers 0.27.2 ControlNetModel): its own encoder copy of the UNet topology, the conditioning
// embedding of the control image, and one zero-conv (1x1, C -> C) per skip plus one for the mid block.
struct ControlNet : Encoder {
    ControlNet(const sd_unet_config& c, int conditioning_channels);
    ~ControlNet();
    int finalize();

    int cond_channels = 3;
    bool finalized = false;
    static constexpr int kCondLayers = 7;          // conv_in, blocks.0-5 (3x3, SiLU after each)
    float* cond_w[kCondLayers] = {};                // [Cout / 16][9 Cin][16] fp32 (launch_cn_pack_cond)
    float* cond_b[kCondLayers] = {};                // [Cout] fp32
    int cond_cin[kCondLayers] = {}, cond_cout[kCondLayers] = {}, cond_stride[kCondLayers] = {};
    ConvW cond_out;                                 // 256 -> block_out_channels[0], 3x3, through igemm2
    std::vector<ConvW> zero;                        // controlnet_down_blocks.i, one per skip
    ConvW zero_mid;                                 // controlnet_mid_block
    UNet* attached = nullptr;

    // the conditioning embedding of n control images [n, cond_channels, 8H, 8W] f16 into out [n H W, C0] (NHWC)
    void run_cond_embed(Ctx& c, const half_t* image, int n, int H, int W, View out);
    // the encoder on (sample, timestep, text) with emb added after conv_in: the pre-zero-conv hidden tensors of every
    // skip (sites[i]) and of the mid block (mid), all [B h w, C] in the arena
    // (of the call: sample, timesteps, L, add_text, add_time_ids, B, H, W; text_kv = the ControlNet's own projection)
    int run(Ctx& c, const UNetCall& call, View text_kv, View emb, const std::vector<View>& sites, View mid);
};

// Whether a UNet topology allows the shared CFG prefix: no per-sample additional embedding (text_time makes the time
// embedding differ between the halves) and a transformer in down block 0 (where the text first enters).
bool unet_cfg_share_eligible(const sd_unet_config& cfg);

// Input of a forward in shared-CFG mode: the un-duplicated latents [B / 2, C, H, W] and the scheduler's input scale;
// the timesteps argument then holds B / 2 entries and `sample` is unused.
struct CfgIn {
    const half_t* latents = nullptr;
    float in_scale = 1.f;
};

// A forward_pag call: `groups` un-perturbed groups (2: [uncond ; text], 1: [text]) followed by the perturbed copy of the
// last one; late = that copy is made at the first flagged transformer (PagState), not up front.
struct PagIn {
    int groups = 2;
    bool late = false;
};

// One forward of a UNet: what every entry (the six sd_unet_forward* functions, forward_cfg, forward_pag, the graph path)
// hands to UNet::forward and what forward hands, unchanged, to the planning pass and the live pass of UNet::run.  The
// defaults are "feature not used".
struct UNetCall {
    const half_t* sample = nullptr;         // [B, C, H, W] (unused with cfg_in)
    const float* timesteps = nullptr;       // [B] ([B / 2] with cfg_in)
    const half_t* ehs = nullptr;            // [B, L, cross_attention_dim]
    int L = 0;
    const half_t* add_text = nullptr;       // text_time conditioning: [B, pooled] and [B, num_time_ids]
    const float* add_time_ids = nullptr;
    half_t* out = nullptr;                  // [B, C_out, H, W]
    int B = 0, H = 0, W = 0;
    const half_t* image_embeds = nullptr;   // IP-Adapter: n_img image prompts per sample
    int n_img = 0;
    const half_t* control = nullptr;        // ControlNet: n_ctrl control images [n_ctrl, 3, 8H, 8W] and the residuals' scale
    int n_ctrl = 0;
    float cn_scale = 0.f;
    // MultiControlNet (sd_unet_forward_mcn): mcn = the call names one image / count / scale per attached net, by index.
    // UNet::forward normalises: cn_active = the nets that run (scale != 0); with one, control / n_ctrl / cn_scale are its
    // and cn_idx says which; with two or more, cn_act[] lists them and control / n_ctrl are the first one's.
    bool mcn = false;
    int n_nets = 0;
    const half_t* mc_control[kCnMaxNets] = {};
    int mc_n_ctrl[kCnMaxNets] = {};
    float mc_scale[kCnMaxNets] = {};
    int cn_idx = 0, cn_active = 0, cn_act[kCnMaxNets] = {};
    const float* tcond = nullptr;           // timestep_cond [B, time_cond_proj_dim] of a guidance-embedded UNet
    const CfgIn* cfg_in = nullptr;          // shared-CFG mode (forward_cfg)
    int num_frames = 0;                     // motion adapter: the B images are B / num_frames videos (0: the modules do not run)
    const PagIn* pag = nullptr;             // perturbed-attention mode (forward_pag)
    // Two-source mode (forward_concat): the sample is cat([fp16(sample[n % lat_rows] * in_scale), n < zero_from ?
    // extra[n % extra_rows] : 0], dim 1) and is never handed over as a tensor; `sample` holds the lat_rows latents
    // [lat_rows, in_channels - extra_channels, H, W], `timesteps` lat_rows entries (repeated per group on the device).
    const half_t* extra = nullptr;          // [extra_rows, extra_channels, H, W]
    int extra_channels = 0, extra_rows = 0, zero_from = 0, lat_rows = 0;
    float in_scale = 1.f;
};

// What the arena plan of a forward depends on.  Compared field by field: a plan is redone exactly when one differs from
// the last one planned in the same DeepCache mode.
struct PlanKey {
    int B = 0, H = 0, W = 0, L = 0;         // (B = 0: nothing planned)
    bool kv_cache = false;                  // the text K/V live in their persistent buffer, not in the arena
    int ip_tokens = 0;                      // image tokens per sample of the attached IP-Adapter, 0 without
    bool cfg_share = false;
    int pag_groups = 0;                     // forward_pag: 1 or 2, and whether the perturbed group is widened late
    bool pag_late = false;
    int n_ctrl = 0;                         // control images of a ControlNet that runs, 0 when none does
    int cn_n[kCnMaxNets] = {0, 0, 0, 0};    // ... of every attached net that runs, by its index (0: it does not)
    int dc_depth = 0;                       // DeepCache depth of a store / reuse forward (the plain one ignores it)
    int cat_rows = 0;                       // forward_concat: the latents the B images are built from, 0 otherwise
    double tome_ratio = 0.0;                // token merging: what the merged rows per block depend on (0: off)
    int tome_ds = 0, tome_sx = 0, tome_sy = 0;
    int ht_tile = 0, ht_swap = 0, ht_depth = 0; // HyperTile: what the gather buffers of the sites depend on (0: off)
    int motion_frames = 0;                  // frames per video when a motion adapter runs, 0 otherwise
    bool operator==(const PlanKey& o) const {
        return B == o.B && H == o.H && W == o.W && L == o.L && kv_cache == o.kv_cache && ip_tokens == o.ip_tokens &&
               cfg_share == o.cfg_share && pag_groups == o.pag_groups && pag_late == o.pag_late && n_ctrl == o.n_ctrl && cn_n[0] == o.cn_n[0] &&
               cn_n[1] == o.cn_n[1] && cn_n[2] == o.cn_n[2] && cn_n[3] == o.cn_n[3] &&
               dc_depth == o.dc_depth && cat_rows == o.cat_rows && tome_ratio == o.tome_ratio && tome_ds == o.tome_ds &&
               tome_sx == o.tome_sx && tome_sy == o.tome_sy && ht_tile == o.ht_tile && ht_swap == o.ht_swap &&
               ht_depth == o.ht_depth && motion_frames == o.motion_frames;
    }
};
// What a captured graph depends on (timestep_cond's width is the configuration's: its presence changes the launches).
struct GraphKey {
    int B = 0, H = 0, W = 0, L = 0;
    bool tcond = false;
    bool operator==(const GraphKey& o) const { return B == o.B && H == o.H && W == o.W && L == o.L && tcond == o.tcond; }
};
// The device addresses a captured graph has baked in: every activation lies in the arena's slab, every input and the
// output in the staging slab.  Either slab is freed when it grows (Arena::reserve, DeviceBuf::reserve), and the arena
// grows under any larger forward the handle runs eagerly in between (graph replay switched off and on again, the
// profiler on, an adapter or a ControlNet attached), so the key alone does not say that a graph may run.
struct GraphDeps {
    const void* arena_base = nullptr;
    size_t arena_cap = 0;
    const void* io_base = nullptr;
    bool operator==(const GraphDeps& o) const {
        return arena_base == o.arena_base && arena_cap == o.arena_cap && io_base == o.io_base;
    }
};
// May the captured graph be launched for this call?  Only when there is one, it was captured for this key, and both
// slabs are where (and as large as) they were at the capture; otherwise forward_graph captures again.
inline bool graph_may_replay(const GraphKey& key, const GraphDeps& now, const GraphKey& captured_key,
                             const GraphDeps& captured, bool have_exec) {
    return have_exec && key == captured_key && now == captured;
}

struct UNet : Encoder {
    explicit UNet(const sd_unet_config& c);
    int finalize();
    // forward_pag / forward_cfg take the call of the UN-duplicated latents: lat.sample [B, C, H, W], lat.timesteps [B],
    // lat.B = B, while ehs / add_text / add_time_ids / image_embeds / out hold the rows of the forward they build.
    // Perturbed-attention guidance.  One forward on [uncond ; text ; perturbed] (cfg) or [text ; perturbed] from B
    // latents and timesteps; ehs / add_text / add_time_ids hold the un-perturbed groups' rows, the perturbed group takes
    // the text group's.  share: widen to the perturbed group at the first flagged transformer where it is not the
    // network's first (after the CFG-shared start where forward_cfg would take it); otherwise, and under
    // SD_NO_PAG_SHARE, duplicate up front.
    int forward_pag(const UNetCall& lat, float in_scale, bool cfg_on, bool share, hipStream_t stream);
    // The forward of a call in two-source mode (UNetCall::extra): sd_unet_forward_concat's checks, then forward().
    int forward_concat(const UNetCall& call, hipStream_t stream);
    int set_pag_layers(const char* const* site_keys, int count);
    // every transformer in execution order with its site key ("down_blocks.i.attentions.j", "mid_block.attentions.0", ...)
    std::vector<std::pair<std::string, Xformer*>> xformer_sites();
    // The forward on cat([latents * in_scale] * 2) with both halves at the same timesteps [B]: ehs / image_embeds / out
    // hold 2B rows, negative half first.  Runs the CFG-shared prefix once per latent when `share`, the topology and the
    // engine's state allow (unet_cfg_share_eligible, no graph replay, no ControlNet, SD_GN_CAT and SD_NO_CFG_SHARE unset);
    // otherwise duplicates into a buffer of its own and runs forward(): bit for bit what callers did before.
    int forward_cfg(const UNetCall& lat, float in_scale, bool share, hipStream_t stream);
    bool cfg_share_active(bool share) const;
    DeviceBuf cfg_slab;                 // forward_cfg's / forward_pag's duplicated latents + timesteps when they do not share
    int forward(const UNetCall& call, hipStream_t stream);
    void set_ip_adapter(IPAdapter* a);
    int set_controlnet(ControlNet* n) { return set_controlnets(&n, n ? 1 : 0); }

    Arena arena;
    bool finalized = false;
    // the last planned key of each DeepCache mode: a loop alternates store / reuse steps, and one key would make a dry
    // pass at every switch (the arena only grows, so a plan made for one mode stays good while another runs)
    PlanKey planned[3];
    void reset_plans() { for (PlanKey& k : planned) k = PlanKey(); }

    // ---- optional hipGraph replay of the whole forward (sd_unet_use_graph) ----
    // One captured graph per input shape; inputs / output are staged through engine-owned buffers so
    // the captured pointers stay valid whatever tensors the caller passes.  The ~480 launches of a
    // forward then cost the host one hipGraphLaunch (CPU time per step 2 ms -> ~0.02 ms); GPU time is
    // unchanged (kernel boundaries cost the same under a graph, MI355X_MICROARCH.md price list).
    // The handle holds one graph; graph_may_replay says per call whether it is launched or captured anew.
    bool graph_enabled = false;
    hipStream_t gstream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraphExec_t gexec = nullptr;
    GraphKey graph_key;
    GraphDeps graph_deps;               // (of the capture gexec came from: graph_may_replay)
    DeviceBuf io_slab;
    // forward_graph's eager pass runs with graph_enabled off; this says it is one.  The pointer-keyed caches below see
    // the staging slab's addresses there, which name no caller tensor, so they neither read nor fill under it.
    bool graph_pass = false;
    bool ptr_caches_live() const { return kv_cache_on && !graph_enabled && !graph_pass; }
    int64_t graph_captures = 0, graph_replays = 0;      // since creation (sd_unet_graph_stats)
    int forward_graph(const UNetCall& call, hipStream_t stream);
    ~UNet();

    // ---- text K/V kept across the forwards of one denoise loop (sd_unet_text_kv_cache) ----
    // encoder_hidden_states is constant over the loop, so the stacked to_k / to_v projection of every
    // cross-attention block is computed by the first forward and reused by the other 49.
    // Valid for one (pointer, batch, length); the caller invalidates when the CONTENTS behind the pointer change.
    bool kv_cache_on = false;
    DeviceBuf kv_cache;
    CacheTag kv_tag;                    // (ehs; B, L, images of the perturbed group whose copy it holds (forward_pag) or 0)

    // ---- IP-Adapter (sd_unet_set_ip_adapter): nullptr = plain cross-attention, the forward as without the feature.
    // Its stacked K / V of the image tokens follow the text K / V's cache rules: kept across the forwards of one loop
    // for one (pointer, batch, images per prompt), invalidated by every sd_unet_text_kv_cache call, not under graphs.
    IPAdapter* ip = nullptr;
    float ip_scale = 1.f;
    DeviceBuf ipkv_cache;
    CacheTag ipkv_tag;                  // (image_embeds; B, n_img)

    // ---- ControlNet (sd_unet_set_controlnet): nullptr = the forward as without the feature.  Its conditioning
    // embedding ([B H W, C0], sample b from control image b mod n_ctrl) and its text K / V follow the text K / V's cache
    // rules: kept across the forwards of one loop for one (pointer, B, n_ctrl, H, W) / (pointer, B, L), invalidated by
    // every sd_unet_text_kv_cache call and by set_controlnet, not under graphs.
    // MultiControlNet (sd_unet_set_controlnets): up to kCnMaxNets nets in `cns`, every cache per net (by its index in the
    // list); cn = cns[0] or nullptr is what every "a ControlNet is attached" check reads, so a list is refused wherever
    // one net is.  One running net (the others at scale 0) takes the single-net path; two or more write their hidden
    // tensors into column slices of one wide buffer per site and add their residuals with one GEMM per site on the
    // folded weights cn_wcat / cn_bcat ([rows][n C] fp16 / [rows] fp32 per site, sized for all attached nets at attach,
    // refolded when the (running nets, scales) tag changes) -- or, with cn_kcat_on() false, one GEMM per net and site.
    ControlNet* cn = nullptr;
    std::vector<ControlNet*> cns;
    DeviceBuf cond_cache[kCnMaxNets], cnkv_cache[kCnMaxNets];
    CacheTag cond_tag[kCnMaxNets];      // (control; B, n_ctrl, H, W)
    CacheTag cnkv_tag[kCnMaxNets];      // (ehs; B, L)
    void clear_cn_tags() { for (int i = 0; i < kCnMaxNets; ++i) { cond_tag[i].clear(); cnkv_tag[i].clear(); } }
    DeviceBuf cn_wcat, cn_bcat;
    std::vector<long> cn_wcat_off, cn_bcat_off;     // per site (skips, then mid), in elements
    struct CnFoldTag {
        bool valid = false;
        int n = 0, idx[kCnMaxNets] = {};
        float scale[kCnMaxNets] = {};
    } cn_fold_tag;
    int64_t cn_fold_count = 0;          // fold launches since creation (sd_unet_cn_fold_count)
    int set_controlnets(ControlNet* const* nets, int count);
    void drop_controlnet(ControlNet* n);    // (a net being destroyed: the others stay attached)
    // zero-conv of attached net `i` at site si (si == number of skips: the mid block's)
    const ConvW& cn_zero(int i, int si) const;
    // fold the running nets' zero-convs for one K-concatenated GEMM per site, unless the tag says they are folded
    int cn_fold(const int* idx, const float* scale, int n, hipStream_t s);

    // ---- FreeU (sd_unet_set_freeu): off = the forward as without the feature.  On, every resnet of up blocks 0 and 1
    // gets one in-place launch on its concatenation buffer before norm1 reads it: (b1, s1) in block 0, (b2, s2) in
    // block 1.  It allocates nothing, so the arena plan does not depend on it; not under graphs.
    bool freeu_on = false;
    float freeu_s1 = 1.f, freeu_s2 = 1.f, freeu_b1 = 1.f, freeu_b2 = 1.f;

    // ---- DeepCache (sd_unet_set_deep_cache / sd_unet_deep_cache_mode): depth 0 = off, the forward as without the
    // feature.  With depth d in 1..layers_per_block the concatenation buffer cats[nskip-1-d] of run() -- whose hidden half
    // is the input of layer L-d of the last up block -- lives in dc_buf instead of the arena (grown like kv_cache).  A
    // store forward is the full forward and leaves that hidden half behind; a reuse forward runs conv_in, d layers of
    // down block 0 (rewriting the buffer's skip half), layers L-d..L of the last up block and the tail.  Valid for one
    // (B, H, W, shared CFG prefix or not); not under graphs, not with a running ControlNet.
    int dc_depth = 0, dc_mode = 0;
    DeviceBuf dc_buf;
    CacheTag dc_tag;                    // (no pointer; B, H, W, shared CFG prefix or not) of the stored step
    int set_deep_cache(int depth);

    // ---- token merging (sd_unet_set_tome): ratio 0 = off, the forward as without the feature.  On, attn1 of every
    // transformer block whose map is at most tome_max_ds times smaller than the sample runs on T' = T - r merged rows:
    // match on the block's input (tome.hip: three launches), merge of the q|k|v rows, the attention at T', unmerge of its
    // output; the q|k|v and out-projection GEMMs stay full-size.  The plan buffers of all merging blocks live in tome_buf
    // (grown like kv_cache; the unmerge maps of the last forward are read from it).  Not under graphs, not in
    // forward_pag / forward_concat; a ControlNet's encoder runs without it.
    TomeRun tome;
    int tome_max_ds = 1;
    DeviceBuf tome_buf;
    std::vector<TomeUsed> tome_used;    // the merging blocks of the last forward, in execution order
    int set_tome(double ratio, int max_downsample, int sx, int sy, int use_rand, uint32_t seed);
    // the blocks that merge for an H x W sample, in execution order of the full forward, with their plan offsets
    int tome_layout(int B, int H, int W, std::vector<TomeUsed>* sites, size_t* bytes);

    // ---- HyperTile (sd_unet_set_hypertile): tile_size 0 = off, the forward as without the feature.  On, attn1 of every
    // transformer block of a level <= max_depth draws a division nh x nw of its map per step (kernels.h: hypertile_plan)
    // and attends within the tiles: (1, 1) runs the plain launches; nw == 1 cuts the NHWC rows into contiguous bands, so
    // the attention runs on qkv / att in place with batch B nh; otherwise the q|k|v rows are gathered into tile order,
    // the attention runs with batch B nh nw and its output is scattered back (hypertile.hip).  The gather buffers are
    // arena scratch, planned for every site that has a candidate nw > 1, whatever a step draws.  Not together with token
    // merging (both rewrite attn1's rows), not under graphs (the division changes per step), not in forward_pag; a
    // ControlNet's encoder runs without it.
    HyperTileRun hypertile;
    std::vector<HyperTileUsed> hypertile_used;  // the participating sites of the last forward, in execution order
    int set_hypertile(int tile_size, int swap_size, int max_depth, uint32_t seed);

    // ---- regional prompts (sd_unet_set_regions): region_R = 0 is off, the forward as without the feature.  On, every
    // attn2 of forward / forward_cfg runs region_xattn_kernel on the R segments of an encoder_hidden_states of R * L
    // tokens, weighted per query by the level's weights.  region_src keeps the caller's [Bw, R, H, W] weights; region_buf
    // is every level's [Bw, T_l, R] (one region_pyramid_kernel launch), scratch that the next forward rebuilds from
    // region_src when sd_unet_poison_workspace has overwritten it (region_stale).  Not under graphs, not with a
    // ControlNet, an IP-Adapter at a non-zero scale, token merging, a DeepCache store / reuse mode, timestep_cond,
    // forward_pag or forward_concat: regions_refuse says so before anything is launched.
    int region_R = 0, region_Bw = 0, region_H = 0, region_W = 0;
    DeviceBuf region_src, region_buf;
    bool region_stale = false;
    int set_regions(const float* weights, int Bw, int R, int H, int W, hipStream_t stream);
    // 0 when regions are off or the call may run with them; else the code (1 / 4) with the message set.  B is the batch of
    // the forward the call builds (2 B of forward_cfg's latents).
    int regions_refuse(const UNetCall& call, int B, bool pag_or_concat);

    // ---- motion adapter (sd_unet_set_motion): nullptr = the forward as without the feature.  Attached, a call with
    // num_frames >= 1 runs a module behind every (resnet, transformer) pair; what is not composed with frames is refused
    // before anything is launched (motion_refuse).
    MotionAdapter* motion = nullptr;
    int set_motion(MotionAdapter* m);
    // 0 when no module runs for this call or it may run; else the code (1 / 4) with the message set.  frames_rows: the
    // rows the frames must divide (the latents of forward_cfg, the batch otherwise).
    int motion_refuse(const UNetCall& call, int frames_rows, bool pag_or_concat);

    // ---- debug taps (sd_unet_tap; engine.h: TapSink): on, the plain forward records the input and output view of
    // every block; the modes whose launches differ from the plain forward's are refused (tap_refuses: 4 when `mode`).
    TapSink taps;
    int tap_refuses(bool mode);

    ConvW conv_out;
    NormW norm_out;
    std::vector<std::vector<Resnet>> up_res;
    std::vector<std::vector<Xformer>> up_att;
    std::vector<ConvW> up_us;

  private:
    // dc: the DeepCache mode of this forward (SD_DC_*)
    int run(Ctx& c, const UNetCall& call, int dc = 0);
    // ControlNet step of run(): its hidden tensors into sites / mid (allocated by the caller)
    // (net = its index in cns; call.control / n_ctrl are that net's)
    int run_controlnet(Ctx& c, const UNetCall& call, int net, const std::vector<View>& sites, View mid);
};

struct VAE {
    explicit VAE(const sd_vae_config& c);
    int finalize();
    int decode(const half_t* z, half_t* img, int B, int h, int w, hipStream_t stream);
    int encode(const half_t* img, half_t* moments, int B, int H, int W, hipStream_t stream);
    // diffusers' tiled_decode / tiled_encode (vae_tiles.hip): tiles of one shape run stacked through decode / encode in
    // chunks of tile_batch images, one gather launch per chunk, one merge launch per canvas
    int decode_tiled(const half_t* z, half_t* img, int B, int h, int w, int tile_latent, double f, int tile_batch,
                     hipStream_t stream);
    int encode_tiled(const half_t* img, half_t* moments, int B, int H, int W, int tile_latent, double f, int tile_batch,
                     hipStream_t stream);
    DeviceBuf tile_in, tile_stack;      // a chunk's gathered tiles; every tile's output, for the merge
    // The encoder with every inter-layer activation stored 2^-k times smaller (same function: see run_resnet): the
    // engine's answer to `config.force_upcast` (sd_unified_pipeline.py:1020-1036 runs such VAEs in fp32 around encode
    // because their activations leave fp16's range).  0 = plain fp16 storage.
    int encode_shift = 0;
    TapSink taps;                       // debug taps of the next decode / encode (sd_vae_tap; engine.h)

    sd_vae_config cfg;
    WeightStore ws;
    Arena arena;
    bool finalized = false;
    long planned_key = -1;

    // decoder
    half_t* pq_w = nullptr; float* pq_b = nullptr;      // post_quant_conv (pointwise, NCHW)
    ConvW d_conv_in, d_conv_out;
    NormW d_norm_out;
    Resnet d_mid0, d_mid1;
    VaeAttn d_attn;
    std::vector<std::vector<Resnet>> d_up;
    std::vector<ConvW> d_us;
    // encoder
    half_t* q_w = nullptr; float* q_b = nullptr;        // quant_conv
    ConvW e_conv_in, e_conv_out;
    NormW e_norm_out;
    Resnet e_mid0, e_mid1;
    VaeAttn e_attn;
    std::vector<std::vector<Resnet>> e_down;
    std::vector<ConvW> e_ds;

  private:
    int pack_resnet(const std::string& p, Resnet* r);
    int pack_attn(const std::string& p, VaeAttn* a);
    int pack_pointwise(const std::string& p, half_t** w, float** b);
    void run_attn(Ctx& c, const VaeAttn& a, View x, int N, int H, int W, View out, const GnStatBuf* x_stats,
                  GnStatBuf** out_stats, float stream_scale = 1.f);
    int run_decode(Ctx& c, const half_t* z, half_t* img, int B, int h, int w);
    int run_encode(Ctx& c, const half_t* img, half_t* moments, int B, int H, int W, float stream_scale);
    int run_tiled(bool enc, const sd_vae_tiles& p, const half_t* in, half_t* out, int B, int tile_batch, hipStream_t stream);
};

// Tiled VAE (vae_tiles.hip).  The plan is sd_vae_tile_plan's (include/sd_engine.h), host only.  vae_tile_stack lays the
// tiles' outputs out for the merge -- [class][tile, raster order][b][C][th][tw] -- and returns the stack's elements;
// class_off (optional) takes the offset of each of the plan's classes.
constexpr int VAE_TILE_MAX_BATCH = 32;
struct VaeGatherList {          // image i of a gathered chunk: canvas image b[i], tile start (ys[i], xs[i]); by value
    int b[VAE_TILE_MAX_BATCH];
    int ys[VAE_TILE_MAX_BATCH];
    int xs[VAE_TILE_MAX_BATCH];
};
struct VaeMergeGeom {           // output space; nfy / nfx = full-size tiles in front on each axis (then at most two more)
    int Ho, Wo, T, blend, limit, nfy, nfx, B, C;
    long cls_off[9];            // stack offset of shape class (cy, cx), c = 0 full, 1 + k = k-th tile behind the full ones
};
int vae_tile_plan(int encode, int h, int w, int tile_sample, int tile_latent, double f, sd_vae_tiles* out);
bool vae_tile_plan_valid(const sd_vae_tiles& p);        // p is, field for field, what the plan function builds
long vae_tile_stack(const sd_vae_tiles& p, int B, int C, VaeMergeGeom* g, long* class_off);
// stack[i, c, y, x] = canvas[b_i, c, ys_i + y, xs_i + x], canvas [.., C, Hc, .] with row stride ld; n <= VAE_TILE_MAX_BATCH
int launch_vae_tile_gather(const half_t* canvas, long ld, half_t* stack, const VaeGatherList& l, int n, int C, int Hc,
                           int th, int tw, hipStream_t s);
// canvas [B, C, Ho, Wo] (row stride ld) from the raw tiles in `tiles`, every pixel written once (vae_tiles.hip)
int launch_vae_tile_merge(const half_t* tiles, half_t* canvas, long ld, const VaeMergeGeom& g, hipStream_t s);

// CLIP text encoder (transformers CLIPTextModel / CLIPTextModelWithProjection): the text side of
// encode_prompt, /root/reference/pipelines/sd_unified_pipeline.py:583-608.
struct ClipLayer {
    NormW ln1, ln2;
    ConvW qkv, out, fc1, fc2;
};
// The pre-LN layer stack both CLIP towers run.  Per layer: LN -> fused q|k|v GEMM -> attention -> out-proj GEMM
// (+residual) -> LN -> fc1 GEMM (+activation) -> fc2 GEMM (+residual); layer l reads slab(l) and writes slab(l + 1)
// ([B T, H], row stride H).  d is the head dim the attention runs at: the fused q|k|v matrix has 3 heads d rows and
// out-proj heads d columns, which is more than H where the vision tower padded its heads at pack time.  Scratch rows
// that feed a GEMM are as wide as its packed K (a multiple of 64); columns past the real width are zeroed once per call.
struct ClipStack {
    int H = 0, I = 0, heads = 1, d = 0;
    int act = 0;                // IGemmParams::act of fc1
    float eps = 1e-5f;
    int causal = 0, prescaled = 0;
};
void run_clip_layers(Ctx& c, const std::vector<ClipLayer>& layers, const ClipStack& g,
                     const std::function<half_t*(int)>& slab, int B, int T);

struct CLIP {
    explicit CLIP(const sd_clip_config& c);
    int finalize();
    int forward(const int* ids, const int* eos_index, half_t* hidden_states, half_t* last_hidden, half_t* pooled,
                half_t* text_embeds, int B, int T, hipStream_t stream);
    int final_layer_norm(const half_t* x, half_t* y, long rows, hipStream_t stream);

    sd_clip_config cfg;
    WeightStore ws;
    Arena arena;
    bool finalized = false;
    long planned_key = -1;
    half_t* tok = nullptr;      // [vocab][H]
    half_t* pos = nullptr;      // [max_positions][H]
    half_t* proj = nullptr;     // [projection_dim][H], no bias
    std::vector<ClipLayer> layers;
    NormW final_ln;

  private:
    int run(Ctx& c, const int* ids, const int* eos_index, half_t* hidden_states, half_t* last_hidden, half_t* pooled,
            half_t* text_embeds, int B, int T);
};

// Head dim the attention runs at for a model head dim d: d itself where attention_supported, else the next supported
// one up to 128 (the heads are zero-padded at pack time), 0 when there is none.
int clip_vision_padded_head_dim(int d);

// CLIP vision tower (transformers CLIPVisionModelWithProjection): patch / class / position embedding, pre_layrnorm, the
// non-causal layer stack, post_layernorm of the class token, visual_projection.
struct CLIPVision {
    explicit CLIPVision(const sd_clip_vision_config& c);
    int finalize();
    int forward(const half_t* pixels, half_t* hidden_states, half_t* last_hidden, half_t* pooled, half_t* image_embeds, int B,
                hipStream_t stream);

    sd_clip_vision_config cfg;
    int tokens = 0;             // 1 + (image_size / patch_size)^2
    int d = 0, dp = 0;          // head dim of the model / the one the attention runs at (dp > d: zero-padded heads)
    WeightStore ws;
    Arena arena;
    bool finalized = false;
    long planned_key = -1;
    half_t* cls = nullptr;      // [H]
    half_t* patch = nullptr;    // [H][3 P P]
    half_t* pos = nullptr;      // [tokens][H]
    half_t* proj = nullptr;     // [projection_dim][H], no bias
    std::vector<ClipLayer> layers;
    NormW pre_ln, post_ln;

  private:
    int pack_attn(int i, ClipLayer* l);
    int run(Ctx& c, const half_t* pixels, half_t* hidden_states, half_t* last_hidden, half_t* pooled, half_t* image_embeds,
            int B);
};

}  // namespace sd
