// Temporal self-attention of an AnimateDiff motion module for gfx950 (CDNA4, wave64): every pixel of every video attends
// over its own F <= 32 frames,
//   out[(v F + f) HW + p, h] = softmax_g(s (q_f + bq_f)(k_g + bk_g)^T) (v_g + bv_g),   rows f, g of pixel p of video v
// with q | k | v read where the row-wise q|k|v GEMM left them (row (v F + f) HW + p, the frames of a pixel HW rows apart)
// and the output written in the same row order: no permuted copy on either side.  b* is the sinusoidal position term
// pushed through the projection at pack time (motion_pos_bias_kernel below): (LN(h) + pe_f) W^T = LN(h) W^T + pe_f W^T,
// a per-frame fp32 table [F_max][3C] added BEFORE the operand is rounded to fp16.
//
// Structure:
//   * one wave per (pixel, head) problem: the whole problem is one (F <= 16) or four (F <= 32) 16 x 16 score tiles, so
//     there is no key loop, no running maximum and no rescale: the softmax is exact over the F keys in one pass.
//   * a block of four waves takes kTattnPixels consecutive pixels of one video and all heads, head fastest: the waves
//     that run together read neighbouring d-wide pieces of the SAME activation rows, so the 128-byte lines of a row are
//     shared in the CU's L1 while they are hot; every byte of q|k|v is requested once and nothing else is read but the
//     table (L2-resident: 32 x 3C floats).
//   * "swapped" products as in attention.hip, so a query's softmax lives in one lane column: S^T = K Q^T with both
//     fragments loaded straight from global memory (16 bytes per lane: the MFMA A / B lane map IS a 16-byte piece of
//     one frame's row), O^T = V^T P^T with P^T taken from the S^T accumulators.  Only V needs a transpose: it is staged
//     in a wave-private LDS tile with odd-multiple-of-32-byte rows and read back with ds_read_b64_tr_b16.
//   * F <= 16 runs the PV product on 16x16x16 MFMAs (the accumulator layout of S^T is its B operand as it stands);
//     F <= 32 on 16x16x32 with the two key tiles as the halves of the contraction.
//   * probabilities are rounded to nearest fp16 and the denominator is summed from the SAME rounded values, so the
//     rounding cancels to first order in the weights; a single frame returns v + bv bit for bit.
//   * padded keys (g >= F) are never read (their rows belong to the next video), load as zeros and are masked to
//     -inf; padded queries are computed on zeros and never stored.
#include <cmath>

#include "kernels.h"

namespace sd {
namespace {

constexpr int kTattnWaves = 4;
constexpr int kTattnPixels = 2;       // pixels per block

constexpr int odd32_bytes(int bytes) { return ((((bytes + 31) / 32) | 1)) * 32; }
constexpr int tattn_vstr(int D) { return odd32_bytes((D + 15) / 16 * 16 * 2) / 2; }      // halves

// 8 halves of one row plus 8 table entries, added in fp32, rounded once
__device__ __forceinline__ h8 load_biased(const half_t* p, const float* b) {
    h8 x = *reinterpret_cast<const h8*>(p);
    if (b) {
        const f4 b0 = *reinterpret_cast<const f4*>(b), b1 = *reinterpret_cast<const f4*>(b + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = (half_t)((float)x[e] + b0[e]);
            x[e + 4] = (half_t)((float)x[e + 4] + b1[e]);
        }
    }
    return x;
}

// FT: 16-frame tiles (1: F <= 16, 2: F <= 32).  bias: [>= F][ldb] fp32 with q | k | v at columns 0 | C | 2C, or null.
template <int D, int FT>
__global__ __launch_bounds__(64 * kTattnWaves) void temporal_attn_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ k, const half_t* __restrict__ v, half_t* __restrict__ out,
    const float* __restrict__ bias, long ldq, long ldk, long ldv, long ldo, long ldb, int F, int HW, int heads,
    float scale_log2e, int pixblocks) {
    constexpr int KS = (D + 31) / 32;                    // 32-wide steps of the QK^T contraction (zero-padded)
    constexpr int DT = (D + 15) / 16;                    // 16-row tiles of O^T
    constexpr int CH = D / 8;                            // 16-byte chunks per row
    constexpr int KEYS = 16 * FT;
    constexpr int VSTR = tattn_vstr(D);
    constexpr int VSLOTS = (KEYS * CH + 63) / 64;
    __shared__ __attribute__((aligned(16))) half_t sV[kTattnWaves][KEYS * VSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int vid = blockIdx.x / pixblocks, p0 = (blockIdx.x - vid * pixblocks) * kTattnPixels;
    const int C = heads * D;
    const int nprob = kTattnPixels * heads;
    half_t* sv = sV[wave];

    for (int pr0 = 0; pr0 < nprob; pr0 += kTattnWaves) {         // block-uniform trip count
        const int prob = pr0 + wave;
        const int pp = prob / heads, h = prob - pp * heads;
        const int pix = p0 + pp;
        const bool live = prob < nprob && pix < HW;
        const long row0 = (long)vid * F * HW + pix;              // frame f of this pixel: row0 + f HW
        const int col = h * D;

        // ---- V (+ bv) -> the wave's LDS tile, rows >= F zero (they meet probabilities that are exactly 0).  Columns
        //      [D, 16 DT) (D = 40: 40..47) are never written: the transposed reads below return whatever LDS holds there as
        //      rows D.. of O^T, whose MFMA rows are independent of the others and are never stored (dd < D) ----
        // (the tile is this wave's own, so a wave-level LDS wait would order it as well as this block barrier does; the
        // barrier is what has run on the hardware, the trip count is block-uniform, and the change waits for a measurement)
        if (pr0 > 0) __syncthreads();                            // the tile's readers of the last round are done
#pragma unroll
        for (int i = 0; i < VSLOTS; ++i) {
            const int idx = i * 64 + lane;
            const int r = idx / CH, c = (idx - r * CH) * 8;
            if (idx < KEYS * CH) {
                h8 val = {0, 0, 0, 0, 0, 0, 0, 0};
                if (live && r < F)
                    val = load_biased(v + (row0 + (long)r * HW) * ldv + col + c,
                                      bias ? bias + (long)r * ldb + 2 * C + col + c : nullptr);
                *reinterpret_cast<h8*>(sv + r * VSTR + c) = val;
            }
        }

        // ---- K and Q fragments: lane holds row (frame) fr of its tile, columns 32 ks + 8 fq .. + 8 ----
        h8 kf[FT][KS], qf[FT][KS];
#pragma unroll
        for (int t = 0; t < FT; ++t) {
            const int f = t * 16 + fr;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int c = ks * 32 + fq * 8;
                h8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, qv = {0, 0, 0, 0, 0, 0, 0, 0};
                if (live && f < F && c < D) {
                    const long r = row0 + (long)f * HW;
                    const float* bf = bias ? bias + (long)f * ldb + col + c : nullptr;
                    kv = load_biased(k + r * ldk + col + c, bias ? bf + C : nullptr);
                    qv = load_biased(q + r * ldq + col + c, bf);
                }
                kf[t][ks] = kv;
                qf[t][ks] = qv;
            }
        }

        // ---- S^T = K Q^T: s[kt][qt], lane = query fr of tile qt, registers = keys 16 kt + 4 fq + j ----
        f4 s[FT][FT];
#pragma unroll
        for (int kt = 0; kt < FT; ++kt)
#pragma unroll
            for (int qt = 0; qt < FT; ++qt) s[kt][qt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int kt = 0; kt < FT; ++kt)
#pragma unroll
                for (int qt = 0; qt < FT; ++qt)
                    s[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][ks], qf[qt][ks], s[kt][qt], 0, 0, 0);

        // ---- exact softmax over the F keys of each query column ----
        h4 pf[FT][FT];                                           // [qt][kt]
        float inv[FT];
#pragma unroll
        for (int qt = 0; qt < FT; ++qt) {
            float x[FT][4];
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < FT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = kt * 16 + fq * 4 + j;
                    x[kt][j] = key < F ? s[kt][qt][j] * scale_log2e : -INFINITY;
                    m = fmaxf(m, x[kt][j]);
                }
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));                     // finite: key 0 exists
            float l = 0.f;
#pragma unroll
            for (int kt = 0; kt < FT; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const half_t ph = (half_t)__builtin_amdgcn_exp2f(x[kt][j] - m);      // round to nearest
                    pf[qt][kt][j] = ph;
                    l += (float)ph;
                }
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            inv[qt] = 1.0f / l;
        }

        __syncthreads();                                         // the V tile is written

        // ---- O^T = V^T P^T, normalise, store: lane holds 4 consecutive d of one query frame ----
#pragma unroll
        for (int i = 0; i < DT; ++i) {
            const half_t* a0 = sv + (fq * 4 + (fr >> 2)) * VSTR + i * 16 + (fr & 3) * 4;
            const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0));
            f4 o[FT];
            if constexpr (FT == 1) {
                o[0] = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4, lo), pf[0][0], f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            } else {
                const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0 + 16 * VSTR));
                union { struct { s4v a, b; } p; h8 v; } u;
                u.p.a = lo; u.p.b = hi;
#pragma unroll
                for (int qt = 0; qt < FT; ++qt) {
                    union { struct { h4 a, b; } p; h8 v; } pb;
                    pb.p.a = pf[qt][0]; pb.p.b = pf[qt][FT - 1];
                    o[qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u.v, pb.v, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                }
            }
            const int dd = i * 16 + fq * 4;
#pragma unroll
            for (int qt = 0; qt < FT; ++qt) {
                const int f = qt * 16 + fr;
                if (live && f < F && dd < D) {
                    const f4 val = o[qt] * inv[qt];
                    const h4 w = {(half_t)val[0], (half_t)val[1], (half_t)val[2], (half_t)val[3]};
                    *reinterpret_cast<h4*>(out + (row0 + (long)f * HW) * ldo + col + dd) = w;
                }
            }
        }
    }
}

template <int D, int FT>
int launch_tattn(const half_t* q, const half_t* k, const half_t* v, half_t* out, const float* bias, long ldq, long ldk,
                 long ldv, long ldo, long ldb, int V, int F, int HW, int heads, float scale_log2e, hipStream_t s) {
    const int pixblocks = cdiv(HW, kTattnPixels);
    hipLaunchKernelGGL((temporal_attn_kernel<D, FT>), dim3((unsigned)(V * pixblocks)), dim3(64 * kTattnWaves), 0, s, q, k, v, out,
                       bias, ldq, ldk, ldv, ldo, ldb, F, HW, heads, scale_log2e, pixblocks);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

// One block per frame: the frame's position row pe[C] in LDS (float64 closed form), then a thread per output column.
__global__ __launch_bounds__(256) void motion_pos_bias_kernel(const half_t* __restrict__ w, int N, int C, float scale, int scale_rows,
                                                              float* __restrict__ out, long ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* pe = reinterpret_cast<double*>(smem);
    const int f = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        const double ang = (double)f * exp(-(double)(c & ~1) * (9.210340371976184 / (double)C));     // ln 10000
        pe[c] = (c & 1) ? cos(ang) : sin(ang);
    }
    __syncthreads();
    const int n = blockIdx.y * 256 + threadIdx.x;
    if (n >= N) return;
    const half_t* row = w + (long)n * C;
    double acc = 0.0;
    for (int c = 0; c < C; c += 8) {
        const h8 x = *reinterpret_cast<const h8*>(row + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += pe[c + e] * (double)(float)x[e];
    }
    out[(long)f * ldo + n] = (float)(n < scale_rows ? acc * (double)scale : acc);
}

}  // namespace

// The one place that decides what a temporal attention runs (host only; sd_temporal_attention_plan exposes it and
// launch_temporal_attention dispatches on it).
TattnPlan temporal_attention_plan(int V, int F, int HW, int heads, int d) {
    TattnPlan pl{};
    if (V < 1 || HW < 1 || heads < 1 || F < 1 || F > 32) return pl;
    if (d != 32 && d != 40 && d != 64 && d != 80 && d != 160) return pl;
    pl.D = d;
    pl.FT = F <= 16 ? 1 : 2;
    pl.pixels = kTattnPixels;
    pl.waves = kTattnWaves;
    pl.pv_k = pl.FT == 1 ? 16 : 32;
    pl.lds_bytes = kTattnWaves * 16 * pl.FT * tattn_vstr(d) * 2;
    pl.blocks = (long)V * cdiv(HW, kTattnPixels);
    return pl;
}

int launch_temporal_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, const float* bias, long ldq,
                              long ldk, long ldv, long ldo, long ldb, int V, int F, int HW, int heads, int d, int prescaled,
                              hipStream_t s) {
    const TattnPlan pl = temporal_attention_plan(V, F, HW, heads, d);
    if (pl.D == 0) {
        set_error("temporal_attention: needs V, HW, heads >= 1, 1 <= F <= 32 and a head dim of 32, 40, 64, 80 or 160");
        return 4;
    }
    const long C = (long)heads * d;
    if (!q || !k || !v || !out || (ldq | ldk | ldv | ldo) % 8 != 0 || ldq < C || ldk < C || ldv < C || ldo < C ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
          reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias)) & 15) != 0 ||
        (bias && (ldb < 3 * C || ldb % 4 != 0))) {
        set_error("temporal_attention: row strides must be multiples of 8 and at least heads * d, pointers 16-byte aligned, "
                  "the table's stride a multiple of 4 and at least 3 heads * d");
        return 1;
    }
    if ((long)V * F * HW >= (1L << 31) || pl.blocks > 0x7fffffffL) { set_error("temporal_attention: too many rows for one launch"); return 1; }
    const float scale = prescaled ? 1.0f : 1.4426950408889634f / sqrtf((float)d);
    // one row per instantiation temporal_attention_plan can name
#define SD_TATTN_RUN(DD, TT) \
    if (pl.D == DD && pl.FT == TT) return launch_tattn<DD, TT>(q, k, v, out, bias, ldq, ldk, ldv, ldo, ldb, V, F, HW, heads, scale, s)
    SD_TATTN_RUN(32, 1); SD_TATTN_RUN(32, 2);
    SD_TATTN_RUN(40, 1); SD_TATTN_RUN(40, 2);
    SD_TATTN_RUN(64, 1); SD_TATTN_RUN(64, 2);
    SD_TATTN_RUN(80, 1); SD_TATTN_RUN(80, 2);
    SD_TATTN_RUN(160, 1); SD_TATTN_RUN(160, 2);
#undef SD_TATTN_RUN
    set_error("temporal_attention: no kernel for the planned instantiation");
    return 4;
}

int launch_motion_pos_bias(const half_t* w, int N, int C, int F, float scale, int scale_rows, float* out, long ldo, hipStream_t s) {
    if (!w || !out || N < 1 || C < 8 || C % 8 != 0 || C > 4096 || F < 1 || ldo < N || (reinterpret_cast<uintptr_t>(w) & 15) != 0 ||
        !std::isfinite(scale)) {
        set_error("motion_pos_bias: needs N, F >= 1, C a multiple of 8 up to 4096, a 16-byte aligned weight, ldo >= N and a "
                  "finite scale");
        return 1;
    }
    hipLaunchKernelGGL(motion_pos_bias_kernel, dim3((unsigned)F, (unsigned)cdiv(N, 256)), dim3(256), (size_t)C * sizeof(double), s, w, N,
                       C, scale, scale_rows, out, ldo);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
