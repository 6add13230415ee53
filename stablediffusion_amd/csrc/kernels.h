// Host-side launchers of the HIP kernels (definitions in *.hip).  All tensors are device memory,
// activations are NHWC fp16 "views": a base pointer plus a row stride (`ld`, in elements) so a
// tensor can live inside a wider buffer (zero-copy skip concatenation).
#pragma once
#include "common.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution / linear (igemm.hip)
//   y[m, co] = bias[co] + rowadd[n(m), co] + res[m, co] + sum_k A[m, k] * Wp[co, k]
//   m = (n, oh, ow);  k = (kh, kw, ci);  A gathered on the fly from x (zero padding, stride,
//   optional nearest-2x upsample of the input).  Wp is the packed weight [rows >= Cout][K].
// ---------------------------------------------------------------------------------------------
struct IGemmParams {
    const half_t* x; long ldx;
    const half_t* w;
    const float* bias;
    const float* rowadd; int rowadd_ld;
    const half_t* res; long ldres;
    half_t* y; long ldy;
    int N, H, W, Cin;       // input geometry (before the optional 2x upsample)
    int OH, OW, Cout;       // output geometry; Cout = GEMM columns (2x the stored width for GEGLU)
    int KS, stride, pad, up;
    int M, K;
    int geglu;              // 1: y[m, j] = hidden_j * gelu(gate_j), weights interleaved per 64
    // Block -> tile order.  Each XCD (own 4 MB L2) works through a contiguous range of block ids; 0: the
    // N tiles of one M tile are neighbours (the activation rows are fetched into one L2, every L2 pulls
    // all the weights), 1: the M tiles of one N tile are neighbours (each weight panel goes to one L2,
    // the activations to all).  Set by the launcher: 1 when the weights outweigh the activations.
    int mfast = 0;
    int act = 0;            // activation after bias, before residual (LDS-DMA kernels, no split-K):
                            // 0 none, 1 quick_gelu x*sigmoid(1.702x) (CLIP-L MLP), 2 exact-erf gelu (OpenCLIP MLP)
    // ---- LayerNorm folded across the GEMM (LDS-DMA kernels, pointwise, no split-K) ----
    // Producer side: the epilogue also writes, per output row and per column tile of this launch, the mean and
    // M2 = sum (v - mean)^2 of the fp16 values it stores: rowstat_out[(m * rowstat_parts + tile_n) * 2 + {0,1}].
    float* rowstat_out = nullptr;
    int rowstat_parts = 0;          // = column tiles of the launch (filled in by the launcher)
    // Consumer side: y = LN(x) W^T + b with LN's affine folded into the weights at pack time
    // (W' = W diag(gamma), b' = b + W beta, wsum_n = sum_k W'_nk) becomes
    //     y[m, n] = rstd_m * (acc[m, n] - mean_m * wsum[n]) + b'[n],   acc = x W'^T on the raw x
    // with mean / rstd of row m from the producer's (mean, M2) parts: ln_parts of them, part k over the columns
    // [k ln_part_w, min((k + 1) ln_part_w, ln_C)).
    const float* ln_stat = nullptr;
    int ln_parts = 0, ln_C = 0, ln_part_w = 0;
    float ln_eps = 0.f;
    const float* ln_wsum = nullptr;
    // ---- GroupNorm statistics of the output, for the GroupNorm that follows (LDS-DMA kernels, no split-K,
    //      every tile inside one image, group boundaries on tile boundaries: IGemmPlan::gnstats) ----
    // gnstat_out[((img * tiles_per_image + tile) * gn_groups + g) * 2 + {0,1}] = (mean, M2) of the tile's rows
    // x the group's channels (the GnStats layout of launch_groupnorm)
    float* gnstat_out = nullptr;
    int gn_groups = 0;
    // ---- GroupNorm (+ SiLU) of the INPUT, applied inside the convolution (conv3x3_halo_kernel<BN, true>: the halo
    //      tile of every 64-channel slab is normalised in LDS after its DMA has landed; igemm2_gn_fusable) ----
    // gni_part: (mean, M2) summaries of x in the GnStats layout, gni_S of them per image over gni_rows pixels each;
    // gni_gb: the norm's affine packed per 64 channels [Cin / 64][64 gamma | 64 beta] (NormW::gb).
    const float* gni_part = nullptr;
    int gni_S = 0;
    long gni_rows = 0;
    int gni_groups = 0;
    float gni_eps = 0.f;
    int gni_silu = 0;
    const float* gni_gb = nullptr;
    int dbg_unchecked = 0;          // tests: wsgemm's residual descriptor without its range check
    // ---- y = acc_scale * (x W^T) + bias_scale * bias (+ rowadd + res): the VAE encoder's range-scaled form (LDS-DMA
    //      kernels and their split-K reductions; IGemmPlan::scales_ok).  Scales are powers of two.  See VAE::run_encode. ----
    float acc_scale = 1.f, bias_scale = 1.f;
};
// The geometry of a convolution over an [N, H, W, Cin] input (nearest-2x upsampled first when up = 1), everything else
// left zero: pad < 0 takes the kernel size's default (1 for 3x3, 0 for 1x1); an explicit pad of 0 under a stride is the
// VAE encoder's Downsample2D (F.pad (0,1,0,1), then the strided conv with padding 0: the right / bottom zero column is
// the gather's ordinary bounds check).  K = ks ks Cin; a caller whose pack pads K sets its own.
inline IGemmParams conv_problem(int N, int H, int W, int Cin, int Cout, int ks, int stride, int up, int pad) {
    IGemmParams p{};
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.KS = ks; p.stride = stride; p.up = up;
    p.pad = pad >= 0 ? pad : (ks == 3 ? 1 : 0);
    const int IH = H << up, IW = W << up;
    if (stride == 1) { p.OH = IH; p.OW = IW; }
    else if (pad == 0) { p.OH = (IH + 1 - ks) / stride + 1; p.OW = (IW + 1 - ks) / stride + 1; }
    else { p.OH = (IH + 2 * p.pad - ks) / stride + 1; p.OW = (IW + 2 * p.pad - ks) / stride + 1; }
    p.M = N * p.OH * p.OW; p.K = ks * ks * Cin;
    return p;
}
// Whether launch_igemm2 can apply a GroupNorm of `groups` groups to this problem's input (p.gni_* set by the caller).
bool igemm2_gn_fusable(const IGemmParams& p, int groups);
int launch_igemm(const IGemmParams& p, hipStream_t s);
const char* igemm_variant(const IGemmParams& p);   // name of the tile variant launch_igemm picks
// LDS-DMA pipeline variants (igemm2.hip)
bool igemm2_supported(const IGemmParams& p);
void igemm2_force(int variant, int splits);            // tuner / tests: -1 restores the heuristic
// What a launch's caller may ask for on top of the problem: buffers the launch should fill if it can.
struct IGemmRequest {
    float* rowstat = nullptr;       // row statistics of the output (IGemmParams::rowstat_out)
    float* gnstat = nullptr;        // GroupNorm summaries of the output for gn_groups groups (IGemmParams::gnstat_out)
    int gn_groups = 0;
    bool no_workspace = false;      // no split-K workspace will be passed: the launch runs unsplit
    // Tile hint of this launch: taken ahead of the tuned table (behind sd_igemm_force), with the force override's
    // validity fallbacks; -1 = none, the plan as without the field.  hint_splits < 1 runs unsplit.
    int hint_variant = -1, hint_splits = 0;
};
// The tuned table's row for a plain pointwise problem (ks 1, stride 1, no upsample, no GEGLU), if it has one.
bool igemm2_tuned_pointwise(int M, int N, int K, int* variant, int* splits);
// How one launch runs, decided once (conv_plan; igemm2_plan for a linear) and handed to launch_igemm2.
constexpr int kKindPgemmGeglu = 100;    // geglu_persist_kernel (pgemm.hip)
constexpr int kKindIgemm1 = -1;         // not an LDS-DMA problem (!igemm2_supported): launch_igemm
constexpr int kKindBadVariant = -2;     // a forced variant id outside the table: the launch fails
constexpr int kKindHalo80 = 80;         // conv3x3_halo_kernel<80>: conv_plan's second stage, not a row of the table
constexpr int kKindUpconvFold = 220;    // conv3x3_halo_up2x2_kernel on the folded pack: conv_plan's first stage
struct IGemmPlan {
    int kind = kKindIgemm1;         // the kernel that runs: a variant id of igemm2.hip's table, or one of the above
    int variant = -1;               // the tile the choice landed on (differs from kind where pgemm / igemm3 / its fallback take over)
    int splits = 1;                 // split-K slices
    long partial_floats = 0;        // fp32 workspace the caller passes as `partial` (0: none)
    int bm = 0, bn = 0;             // the tile
    bool rowstats = false;          // the epilogue writes the row statistics; otherwise the caller runs launch_row_stats
    int rs_parts = 1, rs_part_w = 0;    // their layout either way: parts per row, columns per part (the last one ragged)
    bool gnstats = false;           // the epilogue, or the split-K reduction, leaves the GroupNorm summaries
    int gn_rows = 0;                // pixels per summary (GnStats::rows)
    bool scales_ok = false;         // acc_scale / bias_scale are honoured (not the GEGLU / weight-stationary forms)
    char name[64] = "";             // the kernel as rocprofv3 names it
};
// The table stage: plans the launch of p among the rows of the variant table.  Requests are resolved in the order GroupNorm
// summaries, row statistics, workspace (each granted one can change the tile, and with it the next answer);
// p.gnstat_out / p.gn_groups / p.rowstat_out are set to the buffers the launch will fill and left null for the rest.
// Host code only.  A linear calls it directly; a convolution goes through conv_plan.
IGemmPlan igemm2_plan(IGemmParams& p, const IGemmRequest& rq = IGemmRequest());
// The whole decision for a convolution launch, the one predicate of the planning and the live pass.  In this order:
//   1. the folded upsample (kKindUpconvFold), when p.up == 1 and a folded pack is given: nearest-2x upsample + 3x3 conv
//      run as four 2x2 convs on the input map, one per output parity, on weights folded at pack time (launch_fold_upconv;
//      conv3x3_halo_up2x2_kernel): 4/9 of the 9-tap kernel's MACs.  Takes what upconv_fold_supported admits; row add,
//      residual, GEGLU, activation, LayerNorm fold, fused input GroupNorm and row statistics stay on the 9-tap kernels.
//      p is rewritten to the folded problem: w = w_fold, K = 4 Cin, KS = 2;
//   2. the 80-column halo tile (kKindHalo80; conv3x3_halo_kernel<80>: 256 pixels x 80 columns, waves 8 x 1): twice the
//      blocks of the 160-column tile on the same halo tiles, for the launches whose 128- / 160-column grid leaves CUs idle
//      (M = 8192 x Cout = 640 is 32 x 5 tiles of 128 columns on 256 CUs, and 32 x 8 of these).  cus: the CU count its
//      rule fills (0: the device's).  SD_NO_HALO80=1 (read once) turns it off.  The rule is stated at the definition;
//   3. the table (igemm2_plan), whose answer the rule of stage 2 reads: it is computed once per launch.
// Every route sets p.gnstat_out / p.gn_groups / p.rowstat_out to what the launch will fill.  Host only, pure.
IGemmPlan conv_plan(IGemmParams& p, const half_t* w_fold, const IGemmRequest& rq, int cus = 0);
// Runs p as planned, every kind of plan; plans it itself by the table (requests = p's own rowstat_out / gnstat_out) when
// no plan is passed.  A table plan that splits K needs `partial` of plan->partial_floats; without it the launch is
// planned again and runs unsplit.
int launch_igemm2(const IGemmParams& p, float* partial, hipStream_t s, const IGemmPlan* plan = nullptr);
// The shape part of stage 1 (and SD_NO_UPCONV_FOLD unset): Cin % 64, Cout % 8, a 256-pixel patch (64 / 32 / 16 columns
// wide) tiles the H x W INPUT map, operands within 2 GB.  Host only.
bool upconv_fold_supported(int N, int H, int W, int Cin, int Cout, long ldx);
// tests / tools: -1 the rule, 0 never, 1 whenever the kernel takes the problem (split-K until the grid covers the CUs)
void halo80_force(int mode);
// The folded pack of a [O][I][3][3] fp16 weight: four parity panels (dy, dx), each [rows][4 I] with rows = O padded
// to kWeightRowPad (wp zeroed by the caller), K order [I / 64][a][b][64]; rows dy = 0: W'[a=0] = W[kh=0],
// W'[a=1] = W[1] + W[2]; dy = 1: W'[0] = W[0] + W[1], W'[1] = W[2]; columns likewise.  Taps are summed in fp32
// (kh-major, kw inside) and rounded to fp16 once.  I % 64 == 0.
int launch_fold_upconv(const half_t* w_oihw, half_t* wp, int O, int I, hipStream_t s);
// Most row-statistics parts per row (IGemmParams::ln_parts) a folded-LayerNorm launch takes; launch_igemm2 fails beyond.
int igemm2_max_ln_parts();
// What the calling thread's last launch_igemm2 launched on top of the plan: the split-K slices after the launcher's
// collapse (cdiv(slabs, cdiv(slabs, plan.splits)), at most plan.splits) and the reduction kernel behind them.
struct IGemmLaunchNote {
    int splits = 1;
    int reducer = 0;                // 0 none, 1 splitk_epilogue_kernel, 2 splitk_epilogue_gs_kernel
};
IGemmLaunchNote igemm2_last_launch();
// Pointwise 128 x 80 tile with the activation operand fetched straight into registers (igemm3.hip): launch_igemm2 takes
// it instead of the 128 x 80 LDS-DMA variants when the problem allows (no split-K, GEGLU, row add, GroupNorm summaries).
bool igemm3_supported(const IGemmParams& p);
int launch_igemm3(const IGemmParams& p, int mfast, hipStream_t s);
// Rows the packed weight matrix must be padded to (zero rows), so tile loads need no masks.
constexpr int kWeightRowPad = 256;
// Weight-stationary persistent GEMM for the K = 320 pointwise problems of the 64x64 level (wsgemm.hip):
// igemm2 variants 13 (plain, 128x160) and 14 (GEGLU, 128x128); launch_igemm2 routes to it.
bool wsgemm_supported(const IGemmParams& p);
int wsgemm_rowstat_parts(const IGemmParams& p);         // column partials per row it writes to rowstat_out
int launch_wsgemm(const IGemmParams& p, hipStream_t s);
// Persistent GEGLU projection for the K >= 128 pointwise problems with >= 512 tiles of 256 x 128 (pgemm.hip): one block
// per CU owns an M tile and a run of N tiles, its LDS-DMA ring runs across the tile boundaries; launch_igemm2 routes to it.
bool pgemm_geglu_supported(const IGemmParams& p);
int launch_pgemm_geglu(const IGemmParams& p, hipStream_t s);

// Fused GEGLU feed-forward (ffn.hip): out = x + GEGLU(LN(x) W1^T + b1) W2^T + b2 with the 4C-wide hidden tensor kept in
// LDS / registers (C = 320: the 64 x 64 level of the SD1.5 UNet).  W1 / b1 / wsum1 are the LayerNorm-folded, GEGLU-packed
// projection (WeightStore::pack_geglu + fold_ln), W2 / b2 the packed output linear; ln_stat the row statistics of x.
struct FfnParams {
    const half_t* x; long ldx;          // [M, C]: input of the block and its residual
    half_t* y; long ldy;                // [M, C]
    const half_t* w1; const float* b1; const float* wsum1; int w1_rows;     // [w1_rows >= 8C][C]
    const half_t* w2; const float* b2; int w2_rows;                          // [w2_rows >= 384][4C]
    const float* ln_stat; int ln_parts; float ln_eps;
    int M, C, hidden;
    int ln_part_w;                      // columns per ln_stat part (IGemmParams::ln_part_w)
};
bool ffn_fused_supported(const FfnParams& p);
// The part of that answer known at pack time: the widths the kernel is built for (and SD_NO_FFN_FUSE unset).
bool ffn_fused_width(int C, int hidden);
int launch_ffn_fused(const FfnParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Normalisation (norm.hip)
// ---------------------------------------------------------------------------------------------
// GroupNorm over NHWC: x [N, HW, C] (ld), groups G.  `scratch` must hold gn_scratch_floats().
long gn_scratch_floats(int N, long HW, int C, int G);
// Statistics some earlier kernel already computed for x: per (sample, slab of `rows` consecutive pixels,
// group) the pair (mean, M2 = sum (x - mean)^2), part[((n * S + slab) * G + g) * 2 + {0,1}].  Written by
// a convolution's epilogue (IGemmParams::gnstat_out); launch_groupnorm then skips its own pass over x.
struct GnStats {
    const float* part = nullptr;
    int S = 0;
    long rows = 0;
};
// false for the small maps the single-kernel GroupNorm handles (it reads x once anyway)
bool gn_wants_stats(long HW, int C, int G);
// What a GroupNorm launch does (norm_plan: the one function launch_groupnorm, launch_gn_stats and sd_norm_plan decide by).
struct NormPlan {
    bool valid = false;     // C % 8 == 0, C % G == 0, G <= 256
    int stats = 0;          // statistics kernel: 0 none, 1 gn_stats_kernel, 2 gn_stats2_kernel
    bool stats2 = false;    // the statistics pass, when one runs (launch_gn_stats: always), is gn_stats2_kernel
    int apply = 0;          // 0 gn_fused_kernel<T, NV>, 1 gn_apply_kernel, 2 gn_apply2_kernel<NV>
    int T = 0, NV = 0;      // template arguments of the fused / apply2 kernel
    int unit = 0;           // channels per block of the fused kernel
    bool use_pre = false;   // caller's summaries are used (they are ignored where the fused kernel runs anyway)
    bool finalize = false;  // gn_finalize_kernel merges them first (more than 64 per image)
    int S = 0;              // summaries per image the statistics pass writes, or the caller's
    long rows = 0;          // pixels per summary
    int CB = 0;             // channels per block of the statistics and apply2 kernels
    long apply_rows = 0;    // pixels per block of the apply kernel
    long scratch = 0;       // gn_scratch_floats
};
NormPlan norm_plan(int N, long HW, int C, int G, bool have_summaries, int S_pre, long rows_pre);
int launch_groupnorm(const half_t* x, long ldx, const float* gamma, const float* beta,
                     half_t* y, long ldy, int N, long HW, int C, int G, float eps, int silu,
                     float* scratch, hipStream_t s, const GnStats* pre = nullptr, NormPlan* ran = nullptr);
// Statistics pass alone: (mean, M2) summaries of x into `scratch` (gn_scratch_floats), described by *st.
int launch_gn_stats(const half_t* x, long ldx, int N, long HW, int C, int G, float* scratch, GnStats* st, hipStream_t s);
// Merges the st.S summaries per image into one (into `out`, N * G * 2 floats) and rewrites *st to describe that.
int launch_gn_finalize(GnStats* st, float* out, int N, long HW, int C, int G, hipStream_t s);
// GroupNorm over a channel concatenation [A | B] from its two producers' summaries (norm.hip: gn_cat_finalize_kernel):
// sa / sb describe summaries over Ga / Gb sub-groups of the Ca / Cb channels; out (N * G * 2 floats) receives one
// (mean, M2) per image and group of the concatenation = GnStats{out, 1, HW}.  gn_cat_unit: the sub-group width A's
// producer has to use; B's own width must divide both the channels per group and Ca.
int gn_cat_unit(int Ca, int Cb, int G);
int launch_gn_cat_finalize(const GnStats& sa, int Ga, int Ca, const GnStats& sb, int Gb, int Cb, float* out, int N, long HW, int G,
                           hipStream_t s);
int launch_layernorm(const half_t* x, long ldx, const float* gamma, const float* beta,
                     half_t* y, long ldy, long rows, int C, float eps, hipStream_t s);
// stat[m * 2 + {0,1}] = (mean, M2 = sum (x - mean)^2) of row m (the one-part form of IGemmParams::rowstat_out)
int launch_row_stats(const half_t* x, long ldx, float* stat, long rows, int C, hipStream_t s);
// Pack-time LayerNorm fold of a [rows][K] fp16 weight matrix, in place (rows < rows_scaled are also
// multiplied by row_scale: the attention query pre-scale):  w[n][k] <- fp16(w[n][k] * gamma[k] * s_n),
// wsum[n] = sum_k of the ROUNDED new row, bias[n] <- s_n * (bias_in[n] + sum_k w_old[n][k] * beta[k]).
// bias_in may be null (no bias); bias / wsum are fp32 arrays of `rows` entries.
int launch_ln_fold(half_t* w, long K, int rows, const float* gamma, const float* beta, const float* bias_in,
                   float* bias, float* wsum, int rows_scaled, float row_scale, hipStream_t s);

// Pack-time fold of an outer linear wo [O][J] over an inner one wi [J][K] (both fp16, row-major) into the rows of a
// packed matrix wp [>= O rows][Kp >= K + J]: wp[n] = [fp16(wo[n] wi) | wo[n]] (fp32 accumulation, one rounding); columns
// from K + J up are left as they are (the pack's zero padding).
int launch_fold_linear(const half_t* wo, const half_t* wi, half_t* wp, int O, int J, int K, long Kp, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Attention (attention.hip): out = softmax(q k^T / sqrt(d)) v per (batch, head)
// ---------------------------------------------------------------------------------------------
int launch_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out,
                     int B, int Tq, int Tk, int heads, int d,
                     long ldq, long ldk, long ldv, long ldo, hipStream_t s, int causal = 0, int prescaled = 0);
// prescaled = 1: q already carries log2(e)/sqrt(d) (the UNet folds it into its query projections at
// pack time, launch_scale_f16), which lets the kernel drop its per-score scale-and-subtract FMA.
bool attention_supported(int d);
// Which attn_kernel<D, QT, KT, PRESC, NWV> launch_attention runs for a problem: head dim, 16-query subtiles per wave,
// keys per tile, accumulator-start form for pre-scaled queries, waves per block (16 * QT * NWV queries per block).
// D == 0: unsupported head dim.  Host only; launch_attention dispatches on it.
struct AttnPlan { int D, QT, KT, PRESC, NWV; };
AttnPlan attention_plan(int B, int Tq, int Tk, int heads, int d, int causal, int prescaled);
// IP-Adapter decoupled cross-attention (ip_attention.hip), one launch:
//   out = softmax(s q k^T) v + ip_scale * softmax(s q k_ip^T) v_ip,   s = 1/sqrt(d) (or 1 with prescaled)
// q [B,Tq,heads*d], k / v [B,L,..], k_ip / v_ip [B,Tip,..] with their own row strides; 1 <= L <= 160,
// 1 <= Tip <= 64; ip_scale = 0 skips the image keys.  Returns 4 for unsupported shapes / head dims.
int launch_ip_attention(const half_t* q, const half_t* k, const half_t* v, const half_t* kip, const half_t* vip,
                        half_t* out, int B, int Tq, int L, int Tip, int heads, int d, long ldq, long ldk, long ldv,
                        long ldki, long ldvi, long ldo, float ip_scale, int prescaled, hipStream_t s);
bool ip_attention_supported(int d);
// ip_attention_plan: the launch's shape -- a block tile of `tile_rows` queries, `qtiles` of them per (batch, head),
// `qblocks` blocks per (batch, head) (a block walks the tiles qblk, qblk + qblocks, ... when qblocks < qtiles) and
// `lds_bytes` of dynamic LDS.  Returns the launch's codes for L, Tip, a NaN scale and d; all zero counts for an empty
// problem.  Host only; launch_ip_attention takes its grid and LDS size from it.
struct IpPlan { int tile_rows = 0, qtiles = 0, qblocks = 0, lds_bytes = 0; };
int ip_attention_plan(int B, int Tq, int L, int Tip, int heads, int d, float ip_scale, IpPlan* pl);
int launch_axpy_f16(half_t* y, long ldy, const half_t* x, long ldx, long rows, int cols, float a, hipStream_t s);
// Regional prompts (region_attention.hip), one launch:
//   out[n, t] = sum_r w[n % Bw, t, r] softmax(s q[n, t] k[n, rL:(r+1)L]^T) v[n, rL:(r+1)L],   s as above
// q / out [B, Tq, heads*d], k / v [B, R L, ..] with their own row strides (% 8); w [Bw, Tq, R] fp32, Bw divides B;
// d as ip_attention_supported, 1 <= R <= 8, 1 <= L <= 160 (4 otherwise; 1 for null pointers, strides, Bw).
// region_plan: how the launch holds the R segments in LDS -- `groups` groups of at most `seg_per_group` segments of
// `seg_bytes` each, `lds_bytes` of dynamic LDS; groups == 1: all resident, a block walks several query tiles; more: one
// query tile per block, K / V restaged between groups.  Host only; launch_region_attention dispatches on it.
struct RegionPlan { int seg_per_group = 0, groups = 0, lds_bytes = 0, seg_bytes = 0; };
int region_plan(int R, int L, int d, RegionPlan* pl);
int launch_region_attention(const half_t* q, const half_t* k, const half_t* v, const float* w, half_t* out, int B, int Tq,
                            int L, int R, int heads, int d, long ldq, long ldk, long ldv, long ldo, int Bw, int prescaled,
                            hipStream_t s);
// The weights of every UNet level from the sample-resolution ones w [Bw, R, H, W] fp32, one launch: level l of `out` is
// [Bw, (H >> l)(W >> l), R] (the layout launch_region_attention reads), the 2x2 mean of level l - 1, at float offset
// region_level_offset(.., l); levels in [1, 4], H and W divisible by 2^(levels-1) (1 otherwise).
long region_level_offset(int Bw, int R, int H, int W, int level);
int launch_region_pyramid(const float* w, float* out, int Bw, int R, int H, int W, int levels, hipStream_t s);
// Perceiver attention of the IP-Adapter Plus Resampler (resampler.hip), one launch, head dim 64:
//   out = softmax(s q [kx ; kl]^T) [vx ; vl],   s = 1/8 (or 1 with prescaled)
// q / out [B, n_q, heads*64], kx / vx [B, T_feat, ..], kl / vl [B, n_q, ..], every view with its own row stride (% 8,
// 16-byte aligned); 1 <= n_q <= 16, 1 <= T_feat, T_feat + n_q <= resampler_max_keys() = 320.  Returns 4 for
// unsupported shapes.
int launch_resampler_attention(const half_t* q, const half_t* kx, const half_t* vx, const half_t* kl, const half_t* vl,
                               half_t* out, int B, int n_q, int T_feat, int heads, long ldq, long ldkx, long ldvx, long ldkl,
                               long ldvl, long ldo, int prescaled, hipStream_t s);
int resampler_max_keys();
// dst[r] = src[r % src_rows] for r < rows, rows of `cols` halves (cols % 8 == 0, dense): the Resampler's latents per image
int launch_tile_rows_f16(const half_t* src, long src_rows, half_t* dst, long rows, int cols, hipStream_t s);
// dst[b][r] = r < Tx ? x[b][r] : l[b][r - Tx] over `cols` halves (cols and strides % 8 == 0): timing baseline only
int launch_concat_rows_f16(const half_t* x, long ldx, int Tx, const half_t* l, long ldl, int Tl, half_t* dst, long ldd, long B,
                           int cols, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// ControlNet (controlnet.hip)
// ---------------------------------------------------------------------------------------------
// Grouped zero-convs: for every problem i, y_i[m, :C] = fp16(y_i[m, :C] + scale (x_i[m, :] W_i^T + b_i)), one launch.
// W_i packed [>= C rows][C] (WeightStore::pack_conv of a 1x1 conv), bias fp32 (16-byte aligned), x / y NHWC views with
// their own row strides (ldx % 8 == 0, ldy % 4 == 0); y's columns past C are not touched.  C % 64 == 0, any M >= 1.
// first = the problem's first tile in the joint list (cn_residual_tiles of the ones before it), total = all tiles.
// scale == 0 launches nothing.
constexpr int kCnMaxProblems = 16;
struct CnResProblem {
    const half_t* x = nullptr; long ldx = 0;
    const half_t* w = nullptr;
    const float* bias = nullptr;
    half_t* y = nullptr; long ldy = 0;
    int M = 0, C = 0;
    int first = 0;
};
struct CnResParams {
    CnResProblem p[kCnMaxProblems];
    int count = 0, total = 0;
    float scale = 1.f;
};
int cn_residual_tiles(int M, int C);
bool cn_residual_supported(const CnResParams& p);
int launch_cn_residual(const CnResParams& p, hipStream_t s);
// MultiControlNet: the zero-convs of n nets at one residual site folded into one linear on the column-concatenated
// hidden tensors [h_1 | ... | h_n], for every site in one launch:
//   w_cat[o, i C + k] = fp16(float(w_i[o, k]) * scale[i])     (one fp32 multiply, round to nearest)
//   b_cat[o]          = sum_i scale[i] * bias_i[o]            (fp32, in net order, no contraction)
// w_i packed [rows][C] (WeightStore::pack_conv of a 1x1 conv: rows = weight_rows(C), zero past C), bias_i fp32 [rows],
// w_cat [rows][n C], b_cat [rows]; C % 8 == 0, rows % 4 == 0, every pointer 16-byte aligned.  first = the site's first
// 256-thread block in the joint list (cn_fold_blocks of the ones before it), total = all blocks.
constexpr int kCnMaxNets = 4;
struct CnFoldSite {
    const half_t* w[kCnMaxNets] = {};
    const float* bias[kCnMaxNets] = {};
    half_t* w_cat = nullptr;
    float* b_cat = nullptr;
    int rows = 0, C = 0;
    int first = 0;
};
struct CnFoldParams {
    CnFoldSite s[kCnMaxProblems];
    float scale[kCnMaxNets] = {};
    int n = 0, count = 0, total = 0;
};
int cn_fold_blocks(int rows, int C, int n);
bool cn_fold_supported(const CnFoldParams& p);
int launch_cn_fold_scales(const CnFoldParams& p, hipStream_t s);
// sd_cn_kcat_force: how two or more running ControlNets add their residuals: -1 the default (SD_NO_CN_KCAT=1 in the
// environment selects the chained form), 0 chained per-net launches per site, 1 one K-concatenated GEMM per site
void cn_kcat_force(int mode);
bool cn_kcat_on();
// One layer of ControlNetConditioningEmbedding: y = act(conv3x3(x) + bias), stride 1 or 2, pad 1.  x NCHW fp16 with
// Cin = 3 (nchw = 1: the control image) or NHWC fp16 with Cin in {16, 32, 96}; y NHWC fp16 [N, OH, OW, Cout],
// Cout % 16 == 0; w from launch_cn_pack_cond, bias fp32 [Cout]; silu = 1 applies SiLU.
struct CnCondConvParams {
    const half_t* x = nullptr; int nchw = 0;
    const float* w = nullptr; const float* bias = nullptr;
    half_t* y = nullptr;
    int N = 0, IH = 0, IW = 0, Cin = 0, OH = 0, OW = 0, Cout = 0, stride = 1, silu = 1;
};
bool cn_cond_conv_supported(const CnCondConvParams& p);
int launch_cn_cond_conv(const CnCondConvParams& p, hipStream_t s);
// OIHW fp16 [O][I][3][3] -> [O / 16][3][3][I][16] fp32 (the weight layout cn_cond_conv_kernel reads)
int launch_cn_pack_cond(const half_t* w_oihw, float* out, int O, int I, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// FreeU (freeu.hip)
// ---------------------------------------------------------------------------------------------
// In place on a concatenation view x [N, H W, ld] fp16, hidden = columns [0, C1), skip = [C1, C1 + C2):
//   hidden[:, :C1 / 2] *= b;   skip = fourier_filter(skip, threshold 1, scale s) over (H, W)
// (diffusers 0.27.2 apply_freeu), one launch for both halves and all N images; fp32 moments and correction, one
// rounding to fp16.  C1 even, C2 >= 1, ld >= C1 + C2; columns past C1 + C2 and hidden[:, C1 / 2:] are not touched.
// Returns 1 for arguments outside that domain or non-finite factors, 4 for H + W > 4096.
int launch_freeu(half_t* x, long ld, int N, int H, int W, int C1, int C2, float b, float s, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Small / elementwise kernels (misc.hip)
// ---------------------------------------------------------------------------------------------
// out[b, :] = [cos(t_b f_i) | sin(t_b f_i)] (flip) or [sin | cos]; f_i = exp(-ln(1e4) i/(half-shift))
int launch_timestep_sinusoid(const float* t, int t_stride, float* out, int count, int dim, int flip, float shift,
                             long out_ld, hipStream_t s);
// The input of add_embedding.linear_1: out[b] = [f32(text[b, :P]) | sinusoid(ids[b, 0]) | .. | sinusoid(ids[b, n - 1]) | 0 ..],
// rows out_ld >= P + n * ad floats apart (the rest zeroed), one launch; the sinusoids are launch_timestep_sinusoid's
// bits.  ad even, n >= 1.
int launch_text_time_input(const half_t* text, const float* ids, float* out, int B, int P, int ad, int n, int flip,
                           float shift, int out_ld, hipStream_t s);
// out[b, j] = sinusoid(t_b)[j] + sum_k w[j, k] cond[b, k]: launch_timestep_sinusoid (t_stride 1, out_ld dim) with the
// cond_proj of a guidance-embedded UNet added, one launch.  w [dim rows][ldw] f16, cond [count, cond_dim] f32.
int launch_timestep_cond(const float* t, const float* cond, const half_t* w, long ldw, float* out, int count, int dim,
                         int cond_dim, int flip, float shift, hipStream_t s);
// y[b, n] = bias[n] + sum_k act(x[b, k]) * W[n, k]  for small b (time-embedding MLPs); fp32 in/out.
int launch_small_linear(const float* x, long ldx, const half_t* w, const float* bias, float* y,
                        long ldy, int B, int K, int Nout, int silu_in, int silu_out, hipStream_t s);
// The kernel launch_small_linear runs (the one place that decides; sd_small_linear_plan reports it): 1 skinny_linear_kernel,
// 0 small_linear_kernel, -1 refused (K % 8).  Host only.
int small_linear_plan(int B, int K, int Nout);
int launch_add_f32(float* y, const float* x, long n, int silu, hipStream_t s);   // y = act(y + x), x may be null
int launch_f16_to_f32(const half_t* x, float* y, long n, hipStream_t s);
int launch_f32_to_f16(const float* x, half_t* y, long n, hipStream_t s);
// NCHW fp16 [N,C,H,W] -> im2col rows [N*H*W, Kpad] for a 3x3 pad-1 conv with tiny C (k=(kh,kw,c)).
int launch_im2col_nchw3x3(const half_t* x, half_t* col, int N, int C, int H, int W, int Kpad,
                          hipStream_t s);
// NHWC [M, C] (ld) -> NCHW [N, C, HW]
int launch_nhwc_to_nchw(const half_t* x, long ldx, half_t* y, int N, long HW, int C, hipStream_t s);
// NCHW [N,C,HW] -> NHWC [M, C] (ld)
int launch_nchw_to_nhwc(const half_t* x, half_t* y, long ldy, int N, long HW, int C, hipStream_t s);
// Pointwise CxC conv on NCHW with tiny C (VAE post_quant_conv / quant_conv).
int launch_pointwise_nchw(const half_t* x, const half_t* w, const float* bias, half_t* y, int N,
                          int Cin, int Cout, long HW, hipStream_t s);
// 3x3 / stride 1 / pad 1 conv to Cout <= 4 channels (conv_out): x NHWC f16 (row stride ldx), packed weights
// [>= Cout rows][K = 9 * Cin] (rows beyond Cout are the pack's zero padding), fp32 bias; output NCHW f16.
// Worth it from about 128 K output pixels (512-pixel blocks: fewer leave most CUs idle; measured on C2: the
// 32 K-pixel UNet conv_out is faster on the generic 64-column tile, the 1 M-pixel VAE conv_out 1.7x faster here).
constexpr long kSmallCoutMinPixels = 131072;
int launch_conv3x3_small_cout(const half_t* x, long ldx, const half_t* w, long K, const float* bias, half_t* y_nchw,
                              int N, int H, int W, int Cin, int Cout, hipStream_t s);
// ---- the two ends of the UNet (edge.hip) ----
// conv_in: x NCHW f16 [N, Cin, H, W] (9 Cin <= 64) -> y NHWC [N H W, 320] (row stride ldy) = conv3x3(x) + bias, packed
// weights [>= 320][64] (k = (kh, kw, ci), zero from 9 Cin up: WeightStore::pack_conv's layout).  gnstat_out != nullptr:
// also the GroupNorm summaries of y for G groups in the IGemmParams::gnstat_out layout with 128-row tiles
// (GnStats{part = gnstat_out, S = H W / 128, rows = 128}).
struct HeadParams {
    const half_t* x_nchw = nullptr;
    const half_t* w = nullptr; long K = 0;
    const float* bias = nullptr;
    half_t* y = nullptr; long ldy = 0;
    float* gnstat_out = nullptr; int G = 0;
    int N = 0, Cin = 0, H = 0, W = 0, Cout = 0;
};
bool conv_head_supported(const HeadParams& p);
int launch_conv_head(const HeadParams& p, hipStream_t s);
// conv_in from two sources, one launch (InstructPix2Pix's 8-channel sample, never materialised):
//   y[n] = conv3x3(cat(fp16(a[n % Na] * in_scale), n < zero_from ? b[n % Nb] : 0)) + bias
// a [Na, Ca, H, W] / b [Nb, Cb, H, W] NCHW f16, 9 (Ca + Cb) <= K, K = 64 or 128 (pack_conv's pack of [320, Ca + Cb, 3, 3]),
// N % Na == 0; the scaled latents are rounded to fp16 as launch_scale_copy_f16 rounds them; b is not read for the
// images from zero_from up.  Output, summaries and the remaining limits as launch_conv_head.
struct Head2Params {
    const half_t* a = nullptr; int Na = 0, Ca = 0; float in_scale = 1.f;
    const half_t* b = nullptr; int Nb = 0, Cb = 0; int zero_from = 0;
    const half_t* w = nullptr; long K = 0;
    const float* bias = nullptr;
    half_t* y = nullptr; long ldy = 0;
    float* gnstat_out = nullptr; int G = 0;
    int N = 0, H = 0, W = 0, Cout = 0;
};
bool conv_head2_supported(const Head2Params& p);
int launch_conv_head2(const Head2Params& p, hipStream_t s);
// The sample launch_conv_head2 reads, materialised: out [N, Ca + Cb, H W] NCHW f16 (the general conv_in path's input)
int launch_concat_sample(const half_t* a, int Na, int Ca, float in_scale, const half_t* b, int Nb, int Cb, int zero_from,
                         half_t* out, int N, long HW, hipStream_t s);
// norm_out -> SiLU -> conv_out: y NCHW f16 [N, Cout <= 4, H, W] = conv3x3(act(GroupNorm(x))) + bias; x NHWC (row stride
// ldx), GroupNorm summaries of x as (gn_part, gn_S, gn_rows) (GnStats), packed weights [>= Cout][K = 9 C] in
// pack_conv's K order [C / 64][kh][kw][64].
struct TailParams {
    const half_t* x = nullptr; long ldx = 0;
    const float* gn_part = nullptr; int gn_S = 0; long gn_rows = 0;
    int G = 0; float eps = 0.f; const float* gamma = nullptr; const float* beta = nullptr; int silu = 0;
    const half_t* w = nullptr; long K = 0; const float* bias = nullptr;
    half_t* y = nullptr;
    int N = 0, H = 0, W = 0, C = 0, Cout = 0;
};
bool conv_tail_supported(const TailParams& p);
int launch_conv_tail(const TailParams& p, hipStream_t s);
// Weight packing: OIHW -> [O][KH][KW][I(+pad)] rows; Kpad >= KH*KW*I.
int launch_pack_conv(const half_t* w_oihw, half_t* wp, int O, int I, int KH, int KW, long Kpad,
                     hipStream_t s);
int launch_cfg_duplicate(const half_t* lat, half_t* out, long n_total, float scale, hipStream_t s);
// Copies `rows` rows of row_bytes bytes (row stride ld_bytes) from src to dst for up to kRowDupMax tensors in one launch;
// everything 16-byte aligned.  The shared CFG prefix widens its B-row tensors to 2B rows with it (dst = src + B rows);
// the late-widened perturbed group of forward_pag takes up to 12 skips (SD1.5) + tproj + the transformer's input.
constexpr int kRowDupMax = 24;
struct RowDupSeg {
    const void* src = nullptr;
    void* dst = nullptr;
    long ld_bytes = 0, row_bytes = 0, rows = 0;
};
int launch_row_dup(const RowDupSeg* segs, int count, hipStream_t s);
int launch_scale_copy_f16(const half_t* x, half_t* out, long n, float scale, hipStream_t s);   // out = fp16(x * scale)
int launch_dup_f32(const float* x, float* out, long n, hipStream_t s);                         // out[0:n] = out[n:2n] = x
// CLIP text embeddings: out[b, t, :] = token_table[ids[b, t], :] + position_table[t, :]  (ids clamped to the table)
int launch_clip_embed(const int* ids, const half_t* tok, const half_t* pos, half_t* out, int B, int T, int H, int vocab,
                      hipStream_t s);
// CLIPVisionEmbeddings before pre_layrnorm (vit.hip), one launch: pixels [B,3,S,S] NCHW, w [H][3][P][P] (the raw conv
// weight, no bias), cls [H], pos [1 + (S/P)^2][H] -> out [B, 1 + (S/P)^2, H] with row stride ld (>= H, % 8 == 0).
int launch_vit_patch_embed(const half_t* pixels, const half_t* w, const half_t* cls, const half_t* pos, half_t* out, long ld,
                           int B, int S, int P, int H, hipStream_t s);
// out[b, :] = x[b * T + idx[b], :] as f16 (out16) and / or f32 (out32); idx clamped to [0, T)
int launch_gather_rows(const half_t* x, long ldx, const int* idx, half_t* out16, float* out32, int B, int T, int H,
                       hipStream_t s);
int launch_inpaint_blend(half_t* lat, const half_t* img, const half_t* noise, const half_t* mask, float a, float b, int B,
                         int C, long HW, hipStream_t s);
int launch_scale_f16(half_t* x, long n, float scale, hipStream_t s);     // x *= scale (fp32 multiply, one rounding)
int launch_image_to_uint8(const half_t* img, unsigned char* out, int B, int C, long HW, hipStream_t s);
int launch_cfg_linear(const half_t* eps2b, half_t* lat, float* hist, long n, float g, float cx, float ce, float ch,
                      float hx, float he, hipStream_t s);
// Perturbed-attention guidance: e = fp16(fma(s, t - p, fma(g, t - u, u))) of rows [u ; t ; p] (rows == 3) or
// fp16(fma(s, t - p, t)) of rows [t ; p] (rows == 2; s == 0 skips the outer fma).  launch_pag_linear: launch_cfg_linear's
// update on that e, one launch; launch_pag_combine: e itself into out [n].
int launch_pag_linear(const half_t* model_out, int rows, half_t* lat, float* hist, long n, float g, float sp, float cx,
                      float ce, float ch, float hx, float he, hipStream_t s);
int launch_pag_combine(const half_t* model_out, int rows, half_t* out, long n, float g, float sp, hipStream_t s);
// InstructPix2Pix's dual guidance over rows [text ; image ; uncond]: e = fp16(fma(gi, i - u, fma(gt, t - i, u))).
// launch_ip2p_linear: launch_cfg_linear's update on that e, one launch; launch_ip2p_combine: e itself into out [n].
int launch_ip2p_linear(const half_t* model_out, half_t* lat, float* hist, long n, float gt, float gi, float cx, float ce,
                       float ch, float hx, float he, hipStream_t s);
int launch_ip2p_combine(const half_t* model_out, half_t* out, long n, float gt, float gi, hipStream_t s);
// MultiDiffusion windows (views.hip).  A view v = iy * nx + ix is the [h, w] window of a [rows, C, Hc, Wc] canvas at
// (ys[iy], xs[ix]); with wrap_x its columns are taken modulo Wc.  The starts travel by value in the launch parameters.
constexpr int VIEW_MAX_STARTS = 64;
struct ViewStarts {
    int ys[VIEW_MAX_STARTS];
    int xs[VIEW_MAX_STARTS];
};
// windows[v * B + b, c, y, x] = canvas[b, c, ys + y, (xs + x) mod Wc]: a pure fp16 copy.
int launch_views_gather(const half_t* canvas, half_t* windows, int B, int C, int Hc, int Wc, int h, int w,
                        const ViewStarts& st, int ny, int nx, int wrap_x, hipStream_t s);
// eps[g * B + b, c, Y, X] = fp16(sum_v wt * out_{g,v,b} / sum_v wt) over the views that cover (Y, X), in ascending v, fp32
// sums, one rounding; wt [h, w] fp32 or NULL (all ones).  model_out holds the forwards of chunks of `vpc` views, laid out
// [chunk][group][view in chunk][b]: the row of (g, v, b) is (v / vpc) vpc G B + (g size + v % vpc) B + b with
// size = min(vpc, V - (v / vpc) vpc).  Every pixel must be covered by a view (the C entry checks it).
int launch_views_merge(const half_t* model_out, half_t* eps, const float* wt, int G, int B, int C, int Hc, int Wc, int h,
                       int w, const ViewStarts& st, int ny, int nx, int wrap_x, int vpc, hipStream_t s);
// Token merging (tome.hip; Bolya & Hoffman 2023, tomesd's bipartite_soft_matching_random2d).  The H x W map is cut into
// sy x sx cells; cell (cy, cx) of the hsy x wsx whole ones gives one destination token, (cy sy + k / sx, cx sx + k % sx) with
// k = 0 or mix32(seed, step, site, cell) % (sx sy); every other token is a source.  r = min(Ns, int(T ratio)) sources, those
// of largest cosine similarity to their best destination, are merged into it: T' = T - r rows, the unmerged sources in
// raster order, then the destinations in raster order (a destination row = the mean of itself and its merged sources).
// The counter hash of every per-step draw (token merging's destination tokens, HyperTile's divisions).
__host__ __device__ inline uint32_t mix32(uint32_t seed, uint32_t step, uint32_t site, uint32_t cell) {
    uint32_t h = seed ^ (step * 0x9E3779B9u) ^ (site * 0x85EBCA6Bu) ^ (cell * 0xC2B2AE35u);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
struct TomeGeom {
    int H, W, sx, sy, hsy, wsx, use_rand;
    uint32_t seed, step, site;
    int T, Nd, Ns, r, Tm;
};
// Fills *g; 1 for sx / sy outside 1..8, a ratio outside [0, 0.75] (or NaN), an empty map.  Host only, no device.
int tome_geom(int H, int W, int sx, int sy, double ratio, int use_rand, uint32_t seed, uint32_t step, uint32_t site, TomeGeom* g);
void tome_dst_tokens(const TomeGeom& g, int* dst_tok);          // [Nd] destination tokens in rank order (host)
bool tome_supported(const TomeGeom& g);                         // T <= 16384, Nd >= 1, the selection's keys fit the LDS
long tome_plan_bytes(int B, int T);                             // the opaque plan buffer of B images of T tokens
// Three launches (norms + rank tables, match, select) from x [B T, C] fp16 (row stride ldx % 8 == 0, C % 32 == 0, 16-byte
// aligned) into `plan`: the unmerge map, the member lists of every merged row, node_max / node_idx of every source.
// g.r >= 1.  Returns 4 where !tome_supported.  stage: 0 all three, in order; 1 / 2 / 3 that launch alone (the forward times
// them one by one).
int launch_tome_match(const half_t* x, long ldx, int B, int C, const TomeGeom& g, void* plan, hipStream_t s, int stage = 0);
// Copies of a plan's map [B, T] / node_max [B, Ns] / node_idx [B, Ns] into device arrays (each nullable), on the stream.
int tome_plan_fetch(const void* plan, int B, int T, int Ns, int* map_out, float* node_max, int* node_idx, hipStream_t s);
int tome_plan_read_map(const void* plan, int b, int T, int* map_host);      // synchronous copy to the host
// A plan from a caller's map [B, T] (host) onto T' rows: the member lists in ascending token index.  Every row of [0, T')
// needs a member.  Synchronises the stream.
int tome_plan_from_map(const int* map_host, int B, int T, int Tm, void* plan, hipStream_t s);
// dst [B T', ldd] <- per merged row the mean of src's [B T, lds] member rows over `cols` columns: fp32 sum in ascending
// token index, one IEEE divide by the member count, one rounding.  Tm_host: T' when the host knows it (0: the grid covers
// T rows and the kernel reads T' from the plan).  16-byte accesses when cols, both strides and both pointers allow.
int launch_tome_merge(const half_t* src, long lds, int cols, const void* plan, int B, int T, int Tm_host, half_t* dst, long ldd,
                      hipStream_t s);
// dst [B T, ldd] row t <- src [B T', lds] row map[t]: a pure copy of `cols` columns.
int launch_tome_unmerge(const half_t* src, long lds, int cols, const void* plan, int B, int T, half_t* dst, long ldd,
                        hipStream_t s);
// HyperTile (hypertile.hip; tfernd/HyperTile): the Hs x Ws map of a self-attention site is cut into nh x nw tiles of
// th x tw tokens and every token attends to the tokens of its own tile.  Per axis of n tokens the candidate tile extents
// are the first swap_size divisors e of n with e >= min(tile_size, n), in ascending order; counts[i] = n / e_i (most tiles
// first, never empty).  nh = counts_h[mix32(seed, step, site, 0) % len], nw = counts_w[mix32(seed, step, site, 1) % len].
constexpr int kHyperTileMaxSwap = 8;
struct HyperTileGeom {
    int Hs, Ws, nh, nw, th, tw;
};
// counts [<= 8] of one axis; returns how many (0: n < 1, tile_size < 1 or swap_size outside 1..8).  Host only.
int hypertile_counts(int n, int tile_size, int swap_size, int* counts);
// Fills *g with the draw; 1 for arguments hypertile_counts refuses or Hs Ws > 2^24.  Host only, no device.
int hypertile_plan(int Hs, int Ws, int tile_size, int swap_size, uint32_t seed, uint32_t step, uint32_t site, HyperTileGeom* g);
// gather: dst row ((b nh + ty) nw + tx) th tw + y tw + x <- src row (b Hs + ty th + y) Ws + tx tw + x over `cols` columns
// of [B Hs Ws] rows, a pure fp16 copy with 16 bytes per lane in one launch; scatter: the inverse map.  cols % 8 == 0, both
// row strides % 8 == 0 and >= cols, 16-byte aligned pointers, nh | Hs, nw | Ws, B, nh, nw >= 1: anything else returns 1 with
// nothing launched.  Columns past `cols` of dst are not written.
int launch_hypertile_gather(const half_t* src, long lds, int cols, int B, int Hs, int Ws, int nh, int nw, half_t* dst, long ldd,
                            hipStream_t s);
int launch_hypertile_scatter(const half_t* src, long lds, int cols, int B, int Hs, int Ws, int nh, int nw, half_t* dst, long ldd,
                             hipStream_t s);
// Temporal self-attention of a motion module (temporal_attention.hip), one launch: every pixel p of every video v attends
// over its F <= 32 frames; frame f of the pixel is row (v F + f) HW + p of q / k / v / out (their own row strides), heads
// split the columns as in launch_attention.  bias: fp32 [>= F][ldb] with the q | k | v position terms at columns
// 0 | C | 2C (C = heads d), added in fp32 before the operand is rounded to fp16; null: none.  d in {32, 40, 64, 80, 160}.
// Returns 1 (arguments) / 4 (F, d) with the message set, nothing launched.
struct TattnPlan { int D, FT, pixels, waves, pv_k, lds_bytes; long blocks; };   // D == 0: refused
// FT: 16-frame tiles per axis (1 or 2), pixels per block, waves per block, contraction of the PV MFMA (16x16x16 or
// 16x16x32), static LDS of a block, blocks of the launch.  Host only; launch_temporal_attention dispatches on it.
TattnPlan temporal_attention_plan(int V, int F, int HW, int heads, int d);
int launch_temporal_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, const float* bias, long ldq,
                              long ldk, long ldv, long ldo, long ldb, int V, int F, int HW, int heads, int d, int prescaled,
                              hipStream_t s);
// out[f, n] = (n < scale_rows ? scale : 1) * sum_c pe[f, c] w[n, c] for f < F, n < N: the sinusoidal position rows
// pe[f, 2i] = sin(f 10000^(-2i/C)), pe[f, 2i+1] = cos(same) pushed through a projection weight w [N][C] fp16 (float64
// inside, one rounding to fp32).  C % 8 == 0, C <= 4096.
int launch_motion_pos_bias(const half_t* w, int N, int C, int F, float scale, int scale_rows, float* out, long ldo, hipStream_t s);
// den = dx x + dout m, x <- pden den + pnoise noise (m: model_out, or its CFG combine when rows == 2); noise / denoised
// nullable.  The scheduler step of LCMScheduler in one launch.
int launch_lcm_step(const half_t* model_out, int rows, half_t* lat, const half_t* noise, half_t* denoised, long n, float g,
                    float dx, float dout, float pden, float pnoise, hipStream_t s);
// One scheduler step as up to three rows of fp64 coefficients over v = (x, m, z, h_0 .. h_3) (sd_step_plan, validated, with
// the unused rows and columns zeroed): lat <- fp16(out . v), bank[write_slot[j]] <- fp32(write[j] . v), all from the old
// values.  m as in launch_lcm_step; noise nullable when its column is zero; bank slots are `stride` floats apart.
constexpr int STEP_SLOTS = 4, STEP_WRITES = 2, STEP_COLS = 3 + STEP_SLOTS;
struct StepRows {
    double out[STEP_COLS];
    double write[STEP_WRITES][STEP_COLS];
    int n_writes;
    int write_slot[STEP_WRITES];
};
int launch_sched_affine_step(const half_t* model_out, int rows, half_t* lat, const half_t* noise, float* bank, long stride,
                             long n, float g, const StepRows& p, hipStream_t s);
// launch_cfg_linear on k_b * eps, k_b = 1 + phi (std(text_b) / std(eps_b) - 1) per sample b of n elements (guidance
// rescale): a statistics launch and an update launch; factors [B] (nullable) receives k_b
int launch_cfg_rescale_linear(const half_t* eps2b, half_t* lat, float* hist, int B, long n, float g, float phi, float cx,
                              float ce, float ch, float hx, float he, float* factors, hipStream_t s);

// Box probe (probe.hip): back-to-back 16x16x32 f16 MFMA loop (TFLOP/s) and a 16-byte-per-lane copy (GB/s, read + write)
int probe_mfma(int iters, float* tflops, hipStream_t s);
int probe_copy(long bytes, int iters, float* gbs, hipStream_t s);
// L2 -> LDS rate of the LDS-DMA path with every CU streaming (probe.hip); aggregate GB/s over all CUs
int probe_dma(long region_bytes, int passes, int depth, int shared, float* gbs, hipStream_t s);

}  // namespace sd
