// Host-side runtime of the denoise engine: device memory arena, packed-weight store and the
// execution context shared by the UNet and VAE graphs.  Plain C++ + HIP runtime; no torch.
#pragma once
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"

namespace sd {

// Activation view: NHWC fp16 tensor living at `p` with row (pixel) stride `ld` elements.
struct View {
    half_t* p = nullptr;
    long ld = 0;
    int C = 0;
    int c0 = 0;         // column of `p` inside its row (slice keeps it): what a debug tap needs to copy whole rows
    View() {}
    View(half_t* p_, long ld_, int C_) : p(p_), ld(ld_), C(C_) {}
    View slice(int c, int n) const { View v(p + c, ld, n); v.c0 = c0 + c; return v; }
};

// Bump allocator over one hipMalloc'ed slab with stack-style mark/release.  In "dry" mode no memory
// is attached and only the peak is recorded; the real slab is sized from that.
class Arena {
  public:
    ~Arena();
    int reserve(size_t bytes);            // (re)allocate the slab if smaller than `bytes`
    void begin(bool dry) { dry_ = dry; off_ = 0; if (dry) peak_ = 0; }
    void* alloc(size_t bytes);
    half_t* alloc_h(long n) { return static_cast<half_t*>(alloc((size_t)n * sizeof(half_t))); }
    float* alloc_f(long n) { return static_cast<float*>(alloc((size_t)n * sizeof(float))); }
    size_t mark() const { return off_; }
    void release(size_t m) { off_ = m; }
    size_t peak() const { return peak_; }
    size_t capacity() const { return cap_; }
    const char* base() const { return base_; }      // (with capacity(): what a captured graph's addresses depend on)
    bool dry() const { return dry_; }
    bool overflow() const { return overflow_; }

  private:
    char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0, peak_ = 0;
    bool dry_ = false, overflow_ = false;
};

// A device buffer a handle keeps across calls, outside the per-call arena: it only grows.  Growing frees the old block,
// which launches enqueued earlier may still read, so the device is synchronised first; the contents are undefined
// afterwards, which is why reserve() reports it -- the caller clears whatever says the contents are valid (CacheTag).
// SD_DEVICEBUF_HOST_ALLOC (the host-only bookkeeping test) swaps the three HIP calls for malloc / free.
class DeviceBuf {
  public:
    DeviceBuf() {}
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { if (p_) dev_free(p_); }
    // at least `bytes`; *grew = the buffer was reallocated (set before the allocation: it stays true when that fails,
    // and the buffer is then empty)
    int reserve(size_t bytes, bool* grew) {
        *grew = bytes > cap_;
        if (!*grew) return 0;
        if (int rc = dev_sync()) return rc;
        if (p_) dev_free(p_);
        p_ = nullptr; cap_ = 0;
        if (int rc = dev_alloc(&p_, bytes)) return rc;
        cap_ = bytes;
        return 0;
    }
    int release() {
        if (!p_) return 0;
        if (int rc = dev_sync()) return rc;
        dev_free(p_);
        p_ = nullptr; cap_ = 0;
        return 0;
    }
    char* data() const { return static_cast<char*>(p_); }
    half_t* h() const { return static_cast<half_t*>(p_); }
    size_t capacity() const { return cap_; }

  private:
#ifdef SD_DEVICEBUF_HOST_ALLOC
    static int dev_sync() { return 0; }
    static void dev_free(void* p) { free(p); }
    static int dev_alloc(void** p, size_t bytes) { *p = malloc(bytes); return *p ? 0 : 3; }
#else
    static int dev_sync() { SD_HIP_CHECK(hipDeviceSynchronize()); return 0; }
    static void dev_free(void* p) { (void)hipFree(p); }
    static int dev_alloc(void** p, size_t bytes) { SD_HIP_CHECK(hipMalloc(p, bytes)); return 0; }
#endif
    void* p_ = nullptr;
    size_t cap_ = 0;
};

// What the contents of a cache were computed from: the source pointer and up to four dims (each cache says which).  A
// cache is read when matches() holds and filled -- then set() -- when it does not; clear() is every invalidation.
struct CacheTag {
    bool valid = false;
    const void* src = nullptr;
    int d[4] = {0, 0, 0, 0};
    bool matches(const void* s, int d0, int d1 = 0, int d2 = 0, int d3 = 0) const {
        return valid && src == s && d[0] == d0 && d[1] == d1 && d[2] == d2 && d[3] == d3;
    }
    void set(const void* s, int d0, int d1 = 0, int d2 = 0, int d3 = 0) {
        valid = true; src = s; d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3;
    }
    void clear() { valid = false; }
};

// rows of a packed weight matrix of `cout` outputs (zero rows up to a multiple of kWeightRowPad)
inline long weight_rows(long cout) { return (cout + kWeightRowPad - 1) / kWeightRowPad * kWeightRowPad; }
struct ConvW {          // conv or linear, packed [rows_pad][K] fp16 + fp32 bias (padded)
    half_t* w = nullptr;
    float* bias = nullptr;
    int cin = 0, cout = 0, ks = 1;
    long K = 0;         // packed K (>= ks*ks*cin, multiple of 64)
    float* wsum = nullptr;   // row sums of the packed weights: set when a LayerNorm was folded in (fold_ln)
    // the folded pack of a conv that follows a nearest-2x upsample (pack_conv(fold_up2x): four parity panels
    // [rows_pad][4 cin], kernels.h: launch_fold_upconv), next to the 9-tap pack: op_conv picks per launch
    half_t* w_up = nullptr;
};
// Per-row (mean, M2) parts of an activation tensor, `parts` pairs per row, part k over the columns
// [k width, min((k + 1) width, C)): written by the GEMM that produced the tensor (or by launch_row_stats,
// one part of width C), consumed by the GEMM that applies the folded LayerNorm (IGemmParams::rowstat_out / ln_stat).
struct RowStat {
    float* p = nullptr;
    int parts = 0;
    int width = 0;
};
// GroupNorm summaries of an activation tensor written by the convolution that produced it: `buf` is
// caller-allocated (gnstat_floats), `st` is filled in by op_conv when the launch really emits them
// (st.part == nullptr otherwise: the GroupNorm then runs its own statistics pass).
struct GnStatBuf {
    float* buf = nullptr;
    GnStats st;
};
// Everything optional about an op_conv launch: the geometry besides the weights' own, what the epilogue adds and what
// the launch fuses.  A default-constructed one asks for nothing: a stride-1 convolution (or linear) with its bias.
struct ConvArgs {
    // conv_problem's: up = 1 upsamples the input 2x (nearest) first, pad = -1 is the kernel size's default
    int stride = 1, up = 0, pad = -1;
    const float* rowadd = nullptr;      // fp32 row per image ([N][rowadd_ld]) added to every pixel (the time embedding)
    int rowadd_ld = 0;
    View res;                           // residual added in the epilogue, by value (p == nullptr: none)
    int geglu = 0, act = 0;             // GEGLU pack (y = hidden * gelu(gate), cout / 2 columns); IGemmParams::act
    const RowStat* ln_in = nullptr;     // LayerNorm of the INPUT, folded into this linear (ConvW::wsum set)
    float ln_eps = 0.f;
    RowStat* stat_out = nullptr;        // row statistics of the OUTPUT for the LayerNorm that follows
    GnStatBuf* gn_out = nullptr;        // GroupNorm summaries of the OUTPUT for the GroupNorm that follows
    int gn_groups = 0;
    // GroupNorm (+ SiLU) of the INPUT applied inside the convolution (set by op_gn_conv_fused):
    const struct NormW* gn_in = nullptr;
    GnStats gn_in_stats;                // (mean, M2) summaries of the input
    int gn_in_groups = 0;
    float gn_in_eps = 0.f;
    int gn_in_silu = 0;
    // y = acc_scale * (x W^T) + bias_scale * bias + ...: the range-scaled VAE encoder (powers of two; VAE::run_encode)
    float acc_scale = 1.f, bias_scale = 1.f;
    // tile hint of this launch (IGemmRequest::hint_variant / hint_splits): -1 = none
    int tile_variant = -1, tile_splits = 0;
};
// `base` (by default nothing) plus the residual `res`: a copy, since residuals differ per launch where a struct is shared
inline ConvArgs conv_res(View res, const ConvArgs& base = ConvArgs()) { ConvArgs a = base; a.res = res; return a; }
struct NormW {
    float* gamma = nullptr;
    float* beta = nullptr;
    float* gb = nullptr;     // [C / 64][64 gamma | 64 beta]: what the fused GroupNorm's DMA piece reads (C % 64 == 0)
    int C = 0;
};

// Raw tensors handed over through sd_*_set_weight, kept on device as fp16 until finalize().
struct RawTensor {
    std::vector<int64_t> shape;
    half_t* dev = nullptr;
    long numel = 0;
};

class WeightStore {
  public:
    ~WeightStore();
    void declare(const std::string& key, std::vector<int64_t> shape);
    int set(const std::string& key, const void* data, const int64_t* shape, int ndim, int dtype);
    bool complete(std::string* missing) const;
    const RawTensor* raw(const std::string& key) const;
    // packing helpers (device work on the null stream; finalize() synchronises once).  Each comes in two forms: by key
    // (the model load: the raw tensors of `prefix`) and on the operands themselves (fp16 device weights, fp32 host bias /
    // gamma / beta; bias_host may be nullptr: no bias), which the first resolves to and the single-operator entries call.
    // fold_up2x: the conv follows a nearest-2x upsample (upsamplers.0.conv): also build the folded pack (ConvW::w_up)
    int pack_conv(const std::string& prefix, ConvW* out, bool has_bias = true, bool fold_up2x = false);
    int pack_conv(const half_t* w_oihw_dev, int O, int I, int KH, int KW, const float* bias_host, ConvW* out,
                  bool fold_up2x = false);
    int pack_rows(const std::vector<std::string>& weight_keys, const std::vector<std::string>& bias_keys,
                  ConvW* out);                                  // row-concatenated linears
    int pack_geglu(const std::string& prefix, ConvW* out);      // [8C][C] -> 64-row interleave
    int pack_geglu(const half_t* w_dev, long O, long I, const float* bias_host, ConvW* out);
    int pack_norm(const std::string& prefix, NormW* out);
    int pack_norm(const float* gamma_host, const float* beta_host, int C, NormW* out);
    // Fold LayerNorm `ln` (applied to the GEMM's input) into the packed linear `w`: W <- W diag(gamma)
    // (rows < rows_scaled additionally times row_scale), bias <- bias + W beta, w->wsum = row sums.
    int fold_ln(ConvW* w, const NormW& ln, int rows_scaled, float row_scale);
    // Fold the linear (or 1x1 conv) `outer` over the linear `inner` it follows with nothing in between, as one packed
    // linear on [inner's input | inner's residual]: W' = [W_o W_i | W_o] ([O][K_i + J]), b' = W_o b_i + b_o.  The product
    // is accumulated in fp32 on the device and rounded to fp16 once; pack_conv's padding rules.
    int fold_linear(const std::string& outer, const std::string& inner, ConvW* out);
    void free_raw();
    void* dmalloc(size_t bytes);                                // tracked device allocation
    int64_t packed_bytes() const { return packed_bytes_; }

    std::vector<std::string> order;                             // manifest order
    std::unordered_map<std::string, RawTensor> tensors;

  private:
    int host_floats(const std::string& key, std::vector<float>* out) const;
    std::vector<void*> owned_;
    int64_t packed_bytes_ = 0;
};

// Perturbed-attention guidance (UNet::forward_pag): the forward's N images are the Nq un-perturbed ones followed by the
// perturbed group, N - Nq copies of the last N - Nq of them whose flagged transformers (Xformer::pag) replace the
// self-attention map by the identity.  Until the first flagged transformer nothing tells the perturbed group from the
// group it copies, so with late widening it does not exist before: every launch runs on Nq images inside buffers planned
// for N, and run_xformer issues one row_dup launch at that transformer's first attn1 -- its own input plus whatever
// `caller_segs` adds (UNet::run: tproj and the skips written and not yet read).
struct PagState {
    int N = 0, Nq = 0;
    bool widened = false;               // the perturbed group's rows exist (from the start when duplicated up front)
    int skips_done = 0;                 // skips the down path has written so far
    int cats_consumed = 0;              // concatenations the up path has read so far
    std::function<void(std::vector<RowDupSeg>&)> caller_segs;
};

// Token merging (UNet::set_tome) as one forward sees it: the settings, the plan buffer of every transformer block that
// merges at this forward's shape (by the block's ordinal among all BasicTransformerBlocks in execution order of the full
// forward; -1: the block runs the plain path) and the list of the blocks that did merge, filled by the live pass.
struct TomeUsed {
    int site = 0, H = 0, W = 0, r = 0, Tm = 0, B = 0;
    long plan_off = 0;
};
struct TomeRun {
    double ratio = 0.0;
    int sx = 2, sy = 2, use_rand = 1;
    uint32_t seed = 0, step = 0;
    char* buf = nullptr;                // the plan buffers (UNet::tome_buf)
    std::vector<long> plan_off;
    std::vector<TomeUsed>* used = nullptr;
};

// HyperTile (UNet::set_hypertile) as one forward sees it: the settings, the sample's size (a site's level is read off its
// map) and the list of the participating sites (level <= max_depth) of the live pass with the division each drew.
struct HyperTileUsed {
    int site = 0, H = 0, W = 0, nh = 1, nw = 1, B = 0, copied = 0, level = 0;
};
struct HyperTileRun {
    int tile_size = 0;                  // 0: off
    int swap_size = 2, max_depth = 0;
    uint32_t seed = 0, step = 0;
    int H0 = 0, W0 = 0;                 // the forward's sample
    std::vector<HyperTileUsed>* used = nullptr;
};

// Debug taps (sd_unet_tap / sd_vae_tap): copies of the activation views at block boundaries of ONE forward, for the
// per-block tests.  Off (Ctx::tap == nullptr, the default) a forward does no tap work at all: no launch, no allocation,
// the arena plan and the profile are what they are without the facility.  On, the live pass copies each tapped view on
// the forward's stream into a buffer of the sink's own (hipMalloc, outside the arena; the planning pass records
// nothing, so no plan depends on it).  A view narrower than its row is copied with its whole rows (View::c0 says
// where they start): the test sees the row stride the block read or wrote through, and, for an output, the
// neighbouring columns before (kind kTapPre) and after the block.
enum { kTapIn = 0, kTapOut = 1, kTapPre = 2 };
struct TapEntry {
    std::string name;   // diffusers prefix of the block ("down_blocks.0.resnets.1", "conv_in", "tail", "emb")
    int kind = kTapIn;
    int f32 = 0;        // elements are float (the time embedding) instead of half
    int N = 0, H = 0, W = 0, C = 0, c0 = 0;
    long ld = 0;        // row stride of the copy in elements: rows N H W, columns [c0, c0 + C) are the view
    void* dev = nullptr;
    size_t bytes = 0;
};
struct TapSink {
    bool on = false;
    float scale = 1.f;  // stream scale the activations carry (VAE::run_encode: 2^-encode_shift), 1 otherwise
    std::vector<TapEntry> entries;
    ~TapSink() { clear(); }
    void clear();       // synchronises the device when there is something to free
};

// Execution context of one forward call.
struct Ctx {
    Arena* arena;
    hipStream_t stream;
    bool dry;
    int err = 0;
    // Ring of GroupNorm-summary buffers (ctx_gnpool_init at the top of a forward): a convolution whose
    // output goes into a GroupNorm takes the next slot (ctx_gnbuf) and the GroupNorm reads it one or two
    // launches later, long before the ring comes round again.
    static constexpr int kGnPool = 4;
    GnStatBuf gnpool[kGnPool];
    int gn_next = 0;
    int gn_groups = 0;
    // IP-Adapter image K / V of this forward ([B T_ip, sum 2C], TBlock::ip_kv_off) when an adapter is attached:
    // run_xformer then issues the fused decoupled cross-attention instead of the text-only one
    View ip_kv;
    int ip_T = 0;
    float ip_scale = 1.f;
    PagState* pag = nullptr;            // forward_pag only
    TapSink* tap = nullptr;             // debug taps of this forward (nullptr: off)
    // token merging of this forward (nullptr: off, and always inside a ControlNet's encoder: tomesd patches the UNet only)
    const TomeRun* tome = nullptr;
    // HyperTile of this forward (nullptr: off, and always inside a ControlNet's encoder, as token merging)
    const HyperTileRun* hypertile = nullptr;
    // motion adapter of this forward (nullptr: off, and always inside a ControlNet's encoder): its modules run behind the
    // blocks of run_down / run_mid / the up path on videos of motion_frames consecutive images
    const struct MotionAdapter* motion = nullptr;
    int motion_frames = 0;
    // Regional prompts of this forward (nullptr: off): the handle's weight pyramid (UNet::region_buf) for a
    // region_H x region_W sample, region_R regions in an encoder_hidden_states of region_R * (L / region_R) tokens,
    // weight batch region_Bw.  run_xformer then issues region_xattn_kernel at every attn2 instead of the plain launch.
    const float* region_w = nullptr;
    int region_R = 0, region_Bw = 0, region_H = 0, region_W = 0;
};
// Record view `v` ([N H W, v.C] fp16, kind kTap*) under `name`; nothing on a dry or failed context.  Callers guard with
// `if (c.tap)` so that a forward without taps does not even build the name.
void ctx_tap(Ctx& c, const std::string& name, int kind, View v, int N, int H, int W);
void ctx_tap_f32(Ctx& c, const std::string& name, const float* p, int rows, int cols);
// a block's boundary: before it runs, its input and (where the output view is narrower than its row) the rows it will
// write into; after it, the output
inline void ctx_tap_begin(Ctx& c, const std::string& name, View in, int N, int H, int W, View out, int Ho, int Wo) {
    ctx_tap(c, name, kTapIn, in, N, H, W);
    if (out.C != out.ld) ctx_tap(c, name, kTapPre, out, N, Ho, Wo);
}
// images a launch over an N-image tensor runs on right now: all of them, or the un-perturbed ones in front while the
// perturbed group of a forward_pag call does not exist yet
inline int ctx_live(const Ctx& c, int N) { return c.pag && !c.pag->widened ? c.pag->Nq : N; }
void ctx_gnpool_init(Ctx& c, int N, long HW_max, int G);
GnStatBuf* ctx_gnbuf(Ctx& c);       // next ring slot with `st` cleared; nullptr when the pool is not set up

// One call of a model on its arena.  `body(ctx)` issues the model's launches, or, on a dry context, only its allocations.
// When `key` is not the one `planned` remembers, a dry pass sizes the arena first: an error of that pass returns before
// anything is allocated; growing the slab frees the old one, so the device is synchronised first (nothing enqueued
// earlier may still use it); then the key is remembered, whatever the live pass returns.  The arena only grows, so a
// remembered plan stays good while calls with other keys run.  Returns body's result, or 2 when the live pass asked for
// more than was planned.
template <class Key, class Body>
int plan_and_run(Arena& arena, hipStream_t stream, Key& planned, const Key& key, const char* model, Body body) {
    if (!(key == planned)) {
        Ctx dry{&arena, stream, true};
        arena.begin(true);
        int rc = body(dry);
        if (rc) return rc;
        if (arena.peak() > arena.capacity()) {
            SD_HIP_CHECK(hipDeviceSynchronize());
            if ((rc = arena.reserve(arena.peak()))) return rc;
        }
        planned = key;
    }
    Ctx ctx{&arena, stream, false};
    arena.begin(false);
    const int rc = body(ctx);
    if (!rc && arena.overflow()) { set_error(std::string(model) + ": workspace overflow (planner bug)"); return 2; }
    return rc;
}

// ---- optional per-launch timing (bench.py's live roofline): HIP events on the launch stream ----
struct ProfAgg { double flops = 0, bytes = 0, ms = 0; long launches = 0; };
void prof_enable(bool on);
bool prof_enabled();
void prof_open(hipStream_t s, const char* kernel, double flops, double bytes);
void prof_close(hipStream_t s);
int prof_collect(std::map<std::string, ProfAgg>* out);   // synchronises, aggregates by kernel name

// ---- op wrappers: skip the launch in dry mode, latch the first error ----
// A convolution launch as conv_prepare leaves it: the problem, its plan, the split-K workspace (arena), whether
// row_stats_kernel runs behind it (statistics asked for that the epilogue does not write), the weights' real channels.
struct ConvLaunch {
    IGemmParams p;
    IGemmPlan plan;
    float* partial = nullptr;
    bool stats_after = false;
    int cin = 0;
};
// op_conv = conv_prepare + conv_launch.  conv_prepare poses and plans the launch, refuses what the planned kernel cannot
// do, fills in what the plan leaves of the requested statistics (a.gn_out->st, a.stat_out's layout) and takes the
// workspace from the arena -- all of it the same in the planning and the live pass; false when there is nothing to launch
// (planning pass, or an error latched).  conv_launch issues it (stat_out: ConvArgs::stat_out).
bool conv_prepare(Ctx& c, const ConvW& w, View x, int N, int H, int W, View y, const ConvArgs& a, ConvLaunch* out);
void conv_launch(Ctx& c, const ConvLaunch& l, View y, RowStat* stat_out);
void op_conv(Ctx& c, const ConvW& w, View x, int N, int H, int W, View y, const ConvArgs& a = ConvArgs());
// floats a RowStat buffer needs for an [M, C] tensor whatever tile the producer picks
inline long rowstat_floats(long M, int C) { return M * ((C + 63) / 64) * 2; }
// floats a GnStatBuf needs for N images of HW pixels (tiles of >= 64 pixels) and G groups
// (a split-K reduction kernel leaves up to 64 summaries per image whatever the map size)
inline long gnstat_floats(int N, long HW, int G) { const long t = (HW + 63) / 64; return (long)N * (t > 64 ? t : 64) * G * 2; }
void op_groupnorm(Ctx& c, const NormW& n, View x, View y, int N, long HW, int G, float eps, int silu,
                  const GnStatBuf* pre = nullptr);
// y = conv(act(GroupNorm(x))): GroupNorm kernel + convolution, or, under SD_GN_FUSE=1, op_gn_conv_fused where it takes
// the problem.  `pre` = the summaries of x its producer left (or nullptr: a statistics pass runs); `a` as op_conv's,
// but for its stride, up, pad, geglu and act: the convolution behind a GroupNorm is posed with their defaults.
void op_gn_conv(Ctx& c, const NormW& n, const ConvW& w, View x, int N, int H, int W, View y, int G, float eps, int silu,
                const GnStatBuf* pre, const ConvArgs& a = ConvArgs());
// The same inside the convolution: the launch applies the norm to its halo tiles in LDS and the normalised tensor never
// exists.  Returns false -- nothing launched or allocated -- when the launch cannot take the norm (no per-64 pack of
// gamma / beta, n.C != Cin, !igemm2_gn_fusable) or SD_NO_GN_FUSE is set.  `prepared` (the timed operator entry): the
// statistics launches are issued, the convolution is only prepared into it and its arena allocations stay for the
// caller's conv_launch.
bool op_gn_conv_fused(Ctx& c, const NormW& n, const ConvW& w, View x, int N, int H, int W, View y, int G, float eps,
                      int silu, const GnStatBuf* pre, const ConvArgs& a = ConvArgs(), ConvLaunch* prepared = nullptr);
void op_layernorm(Ctx& c, const NormW& n, View x, View y, long rows, float eps);
// y = x + GEGLU(LN(x) ff1) ff2 in one launch (ffn.hip) when the problem fits it (C = 320, LayerNorm folded into ff1, the
// row statistics of x at hand); returns false -- nothing launched -- when it does not: the caller runs the two GEMMs.
bool op_ffn_fused(Ctx& c, const ConvW& ff1, const ConvW& ff2, View x, const RowStat& x_stat, float ln_eps, long M, View y);
void op_attention(Ctx& c, View q, View k, View v, View out, int B, int Tq, int Tk, int heads, int d, int causal = 0,
                  int prescaled = 0);
// out = softmax(q k^T) v + ip_scale softmax(q k_ip^T) v_ip (prescaled queries, ip_attention.hip)
void op_ip_attention(Ctx& c, View q, View k, View v, View k_ip, View v_ip, View out, int B, int Tq, int L, int T_ip,
                     int heads, int d, float ip_scale);
// out[n, t] = sum_r w[n % Bw, t, r] softmax(q k_r^T) v_r over the R segments of L keys each (prescaled queries,
// region_attention.hip)
void op_region_attention(Ctx& c, View q, View k, View v, const float* w, View out, int B, int Tq, int L, int R, int heads,
                         int d, int Bw);
// out = softmax(q [kx ; kl]^T) [vx ; vl], head dim 64, prescaled queries (resampler.hip)
void op_resampler_attention(Ctx& c, View q, View kx, View vx, View kl, View vl, View out, int B, int n_q, int T_feat,
                            int heads);

}  // namespace sd
