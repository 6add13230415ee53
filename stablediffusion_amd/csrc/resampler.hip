// Perceiver attention of the IP-Adapter Plus Resampler for gfx950 (CDNA4, wave64), one launch per layer:
//   out = softmax(s q [K_x ; K_l]^T) [V_x ; V_l]
// q: the n_q <= 16 latent queries of one image, K_x / V_x: the T_feat projected image features, K_l / V_l: the n_q
// projected latents.  fp16 in/out, fp32 scores and accumulators, head dim 64.  The reference module concatenates the
// normalised features and latents and projects the concatenation; the projection is row-wise, so the graph projects
// each source into its own buffer and this kernel reads the two views (each with its own row stride) as one key set.
//
// One block per (image, head), four waves.  All T_feat + n_q <= 320 keys and values are staged into LDS once, features
// first, latents behind them, zero-padded to a multiple of 32 rows.  The 16 query rows are one MFMA tile, so the
// waves split the KEYS: wave w takes the 32-key steps w, w + 4, w + 8.  The softmax is exact and joint over both
// segments -- block-wide row maximum and row sum through LDS, no running maximum -- and the probabilities are
// normalised in fp32 before they are rounded to fp16 for the PV product.  Each wave's partial O^T goes through LDS and
// is summed in wave order, so the result does not depend on scheduling.
// Shared with ip_attention.hip: S^T = K Q^T (a query's scores sit in one lane column), P^T straight from the S^T
// accumulators as the B operand of O^T = V^T P^T, V^T read with ds_read_b64_tr_b16 from row-major V, odd multiples of
// 32 bytes as LDS row strides, 16x16x32 MFMAs.
#include "kernels.h"

namespace sd {
namespace {

constexpr int kRsD = 64;                // head dim
constexpr int kRsStr = 80;              // LDS row stride in halves: 160 bytes = 5 x 32
constexpr int kRsWaves = 4;
constexpr int kRsMaxKeys = 320;         // T_feat + n_q
constexpr int kRsSteps = (kRsMaxKeys / 32 + kRsWaves - 1) / kRsWaves;   // 32-key steps per wave: 3
constexpr int kRsRedFloats = 2 * kRsWaves * 16 + kRsWaves * 16 * kRsD;  // row max, row sum, partial outputs

__device__ __forceinline__ unsigned rs_pack_rte(float a, float b) {
    h2 v = {(half_t)a, (half_t)b};
    return __builtin_bit_cast(unsigned, v);
}

// Rows [r0, r0 + n) of the LDS tile from n rows of a [*, 64] head slice (row stride ld).
__device__ __forceinline__ void rs_stage(half_t* dst, int r0, const half_t* src, long ld, int n, int tid) {
    for (int idx = tid; idx < n * (kRsD / 8); idx += 64 * kRsWaves) {
        const int r = idx >> 3, c = (idx & 7) * 8;
        *reinterpret_cast<h8*>(dst + (r0 + r) * kRsStr + c) = *reinterpret_cast<const h8*>(src + (long)r * ld + c);
    }
}

__global__ __launch_bounds__(64 * kRsWaves) void resampler_attn_kernel(
    const half_t* __restrict__ q, const half_t* __restrict__ kx, const half_t* __restrict__ vx,
    const half_t* __restrict__ kl, const half_t* __restrict__ vl, half_t* __restrict__ out, int n_q, int T_feat, int heads,
    long ldq, long ldkx, long ldvx, long ldkl, long ldvl, long ldo, float scale_log2e) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int D = kRsD, STR = kRsStr, KS = D / 32, DT = D / 16;
    const int Tk = T_feat + n_q;
    const int nkk = (Tk + 31) / 32, rows = nkk * 32;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sK = reinterpret_cast<half_t*>(smem);
    half_t* sV = sK + rows * STR;
    float* sMax = reinterpret_cast<float*>(sV + rows * STR);    // [waves][16]
    float* sSum = sMax + kRsWaves * 16;                         // [waves][16]
    float* sO = sSum + kRsWaves * 16;                           // [waves][16 queries][64]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;

    rs_stage(sK, 0, kx + (long)b * T_feat * ldkx + h * D, ldkx, T_feat, tid);
    rs_stage(sV, 0, vx + (long)b * T_feat * ldvx + h * D, ldvx, T_feat, tid);
    rs_stage(sK, T_feat, kl + (long)b * n_q * ldkl + h * D, ldkl, n_q, tid);
    rs_stage(sV, T_feat, vl + (long)b * n_q * ldvl + h * D, ldvl, n_q, tid);
    for (int idx = tid; idx < (rows - Tk) * (D / 8); idx += 64 * kRsWaves) {
        const int r = Tk + (idx >> 3), c = (idx & 7) * 8;
        const h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        *reinterpret_cast<h8*>(sK + r * STR + c) = z;
        *reinterpret_cast<h8*>(sV + r * STR + c) = z;
    }

    // the query tile: rows >= n_q are zeros (their columns are computed and dropped)
    h8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        h8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (fr < n_q) val = *reinterpret_cast<const h8*>(q + ((long)b * n_q + fr) * ldq + h * D + ks * 32 + fq * 8);
        qf[ks] = val;
    }
    __syncthreads();

    // this wave's steps: kk = wave + 4 j, j < nst
    const int nst = nkk > wave ? (nkk - wave + kRsWaves - 1) / kRsWaves : 0;

    // ---- S^T = K Q^T: s[j][half] holds keys (wave + 4 j) * 32 + half * 16 + fq * 4 + e of query fr ----
    f4 s[kRsSteps][2];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kRsSteps; ++j) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            s[j][hf] = f4{0.f, 0.f, 0.f, 0.f};
            if (j < nst) {
                const int k0 = (wave + kRsWaves * j) * 32 + hf * 16;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const h8 kf = *reinterpret_cast<const h8*>(sK + (k0 + fr) * STR + ks * 32 + fq * 8);
                    s[j][hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[j][hf], 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (k0 + fq * 4 + e >= Tk) s[j][hf][e] = -INFINITY;     // padding keys never win and weigh 0
                    m = fmaxf(m, s[j][hf][e]);
                }
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    if (fq == 0) sMax[wave * 16 + fr] = m;
    __syncthreads();
    m = sMax[fr];
#pragma unroll
    for (int w = 1; w < kRsWaves; ++w) m = fmaxf(m, sMax[w * 16 + fr]);     // finite: key 0 is always real

    const float nm = -m * scale_log2e;
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < kRsSteps; ++j) {
        if (j < nst) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][hf][e], scale_log2e, nm));
                    s[j][hf][e] = p;
                    l += p;
                }
        }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (fq == 0) sSum[wave * 16 + fr] = l;
    __syncthreads();
    l = sSum[fr];
#pragma unroll
    for (int w = 1; w < kRsWaves; ++w) l += sSum[w * 16 + fr];
    const float inv = 1.f / l;

    // ---- O^T = V^T P^T over this wave's keys ----
    f4 o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kRsSteps; ++j) {
        if (j < nst) {
            union { unsigned w[4]; h8 v; } pb;
            pb.w[0] = rs_pack_rte(s[j][0][0] * inv, s[j][0][1] * inv);
            pb.w[1] = rs_pack_rte(s[j][0][2] * inv, s[j][0][3] * inv);
            pb.w[2] = rs_pack_rte(s[j][1][0] * inv, s[j][1][1] * inv);
            pb.w[3] = rs_pack_rte(s[j][1][2] * inv, s[j][1][3] * inv);
            const int k0 = (wave + kRsWaves * j) * 32;
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const half_t* a0 = sV + (k0 + fq * 4 + (fr >> 2)) * STR + i * 16 + (fr & 3) * 4;
                const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0));
                const s4v hi =
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0 + 16 * STR));
                union { struct { s4v a, b; } p; h8 v; } u;
                u.p.a = lo; u.p.b = hi;
                o[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u.v, pb.v, o[i], 0, 0, 0);
            }
        }
    }
    // lane holds 4 consecutive d of query fr
#pragma unroll
    for (int i = 0; i < DT; ++i) *reinterpret_cast<f4*>(sO + (wave * 16 + fr) * D + i * 16 + fq * 4) = o[i];
    __syncthreads();
    {
        const int qi = tid >> 4, d0 = (tid & 15) * 4;
        f4 acc = *reinterpret_cast<const f4*>(sO + qi * D + d0);
#pragma unroll
        for (int w = 1; w < kRsWaves; ++w) {
            const f4 t = *reinterpret_cast<const f4*>(sO + (w * 16 + qi) * D + d0);
            acc[0] += t[0]; acc[1] += t[1]; acc[2] += t[2]; acc[3] += t[3];
        }
        if (qi < n_q) {
            const h4 w = {(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
            *reinterpret_cast<h4*>(out + ((long)b * n_q + qi) * ldo + h * D + d0) = w;
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}

__global__ void tile_rows_f16_kernel(const half_t* __restrict__ src, long src_rows, half_t* __restrict__ dst, long rows,
                                     int cols) {
    const int cpr = cols / 8;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cpr) return;
    const long r = idx / cpr;
    const int c = (int)(idx - r * cpr) * 8;
    *reinterpret_cast<h8*>(dst + r * cols + c) = *reinterpret_cast<const h8*>(src + (r % src_rows) * cols + c);
}

// dst[b][r] = r < Tx ? x[b][r] : l[b][r - Tx]: the concatenation the composed form of sd_op_resampler_attention builds
__global__ void concat_rows_f16_kernel(const half_t* __restrict__ x, long ldx, int Tx, const half_t* __restrict__ l, long ldl,
                                       int Tl, half_t* __restrict__ dst, long ldd, long B, int cols) {
    const int cpr = cols / 8;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * (Tx + Tl) * cpr) return;
    const long row = idx / cpr;
    const int c = (int)(idx - row * cpr) * 8;
    const long b = row / (Tx + Tl);
    const int r = (int)(row - b * (Tx + Tl));
    const half_t* src = r < Tx ? x + (b * Tx + r) * ldx : l + (b * Tl + (r - Tx)) * ldl;
    *reinterpret_cast<h8*>(dst + row * ldd + c) = *reinterpret_cast<const h8*>(src + c);
}

}  // namespace

int resampler_max_keys() { return kRsMaxKeys; }

int launch_concat_rows_f16(const half_t* x, long ldx, int Tx, const half_t* l, long ldl, int Tl, half_t* dst, long ldd, long B,
                           int cols, hipStream_t s) {
    if (cols % 8 != 0 || (ldx | ldl | ldd) % 8 != 0) { set_error("concat_rows_f16: cols and strides must be multiples of 8"); return 1; }
    const long n = B * (Tx + Tl) * (cols / 8);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(concat_rows_f16_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, x, ldx, Tx, l, ldl, Tl, dst, ldd,
                       B, cols);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tile_rows_f16(const half_t* src, long src_rows, half_t* dst, long rows, int cols, hipStream_t s) {
    if (cols % 8 != 0 || src_rows < 1) { set_error("tile_rows_f16: cols must be a multiple of 8 and src_rows >= 1"); return 1; }
    const long n = rows * (cols / 8);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(tile_rows_f16_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, src, src_rows, dst, rows, cols);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_resampler_attention(const half_t* q, const half_t* kx, const half_t* vx, const half_t* kl, const half_t* vl,
                               half_t* out, int B, int n_q, int T_feat, int heads, long ldq, long ldkx, long ldvx, long ldkl,
                               long ldvl, long ldo, int prescaled, hipStream_t s) {
    if ((ldq | ldkx | ldvx | ldkl | ldvl | ldo) % 8 != 0) { set_error("resampler attention: row strides must be multiples of 8"); return 1; }
    if (((uintptr_t)q | (uintptr_t)kx | (uintptr_t)vx | (uintptr_t)kl | (uintptr_t)vl | (uintptr_t)out) % 16 != 0) {
        set_error("resampler attention: operands must be 16-byte aligned");
        return 1;
    }
    if (B < 0 || heads < 0) { set_error("resampler attention: negative batch or head count"); return 1; }
    if (n_q < 1 || n_q > 16) { set_error("resampler attention: queries must be in [1, 16]"); return 4; }
    if (T_feat < 1 || T_feat + n_q > kRsMaxKeys) { set_error("resampler attention: feature tokens + queries must be in [2, 320]"); return 4; }
    const long width = (long)heads * kRsD;
    if (ldq < width || ldkx < width || ldvx < width || ldkl < width || ldvl < width || ldo < width) {
        set_error("resampler attention: a row stride is smaller than heads x 64");
        return 1;
    }
    if (B == 0 || heads == 0) return 0;
    if ((long)B * heads > 0x7fffffffL) { set_error("resampler attention: too many (image, head) pairs"); return 4; }
    constexpr size_t lds_max = (size_t)kRsMaxKeys * kRsStr * 2 * 2 + (size_t)kRsRedFloats * 4;
    static_assert(lds_max <= 160 * 1024, "LDS");
    static_assert(kRsSteps * kRsWaves * 32 >= kRsMaxKeys, "every 32-key step needs a wave");
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&resampler_attn_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    }
    const int rows = 32 * ((T_feat + n_q + 31) / 32);
    const size_t lds = (size_t)rows * kRsStr * 2 * 2 + (size_t)kRsRedFloats * 4;
    const float scale_log2e = prescaled ? 1.0f : 1.4426950408889634f / 8.0f;
    hipLaunchKernelGGL(resampler_attn_kernel, dim3((unsigned)(B * heads)), dim3(64 * kRsWaves), lds, s, q, kx, vx, kl, vl, out,
                       n_q, T_feat, heads, ldq, ldkx, ldvx, ldkl, ldvl, ldo, scale_log2e);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
