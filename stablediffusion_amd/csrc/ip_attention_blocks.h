// Building blocks of the LDS-resident cross-attention kernels (ip_attention.hip, region_attention.hip) for gfx950:
// odd-multiple-of-32-byte LDS row strides, staging of a [rows, D] head slice, and one exact-softmax segment with the
// swapped products S^T = K Q^T and O^T = V^T P^T (V^T read with ds_read_b64_tr_b16), its coefficient folded into P
// before the fp16 rounding so that every segment accumulates into one set of fp32 output registers.
#pragma once
#include "kernels.h"

namespace sd {
namespace {

constexpr int ip_odd32_bytes(int bytes) { return ((((bytes + 31) / 32) | 1)) * 32; }
constexpr int ip_kstr(int D) { return ip_odd32_bytes((D + 31) / 32 * 32 * 2) / 2; }   // halves
constexpr int ip_vstr(int D) { return ip_odd32_bytes((D + 15) / 16 * 16 * 2) / 2; }   // halves
constexpr int kMaxTextSteps = 5;      // 32-key PV steps: L <= 160
constexpr int kMaxIpSteps = 2;        // T_ip <= 64

__device__ __forceinline__ unsigned pack_rte(float a, float b) {
    h2 v = {(half_t)a, (half_t)b};
    return __builtin_bit_cast(unsigned, v);
}

// Stage rows [0, n) of a [rows, D] head slice (row stride ld) into LDS rows of `str` halves, zero beyond n / D.
template <int D>
__device__ __forceinline__ void stage_rows(half_t* dst, int str, const half_t* src, long ld, int n, int rows, int tid,
                                           int nth) {
    const int cpr = str / 8;
    for (int idx = tid; idx < rows * cpr; idx += nth) {
        const int r = idx / cpr, c = (idx - r * cpr) * 8;
        h8 val = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < n && c < D) val = *reinterpret_cast<const h8*>(src + (long)r * ld + c);
        *reinterpret_cast<h8*>(dst + r * str + c) = val;
    }
}

// One softmax segment of one wave's 16 * QT queries: o += coef * softmax(scale q K^T) V over keys [0, n).
// nkk (<= NKK) 32-key steps are staged in cK / cV.  coef[t] is the lane's own query's coefficient in tile t (query
// t * 16 + fr): one value for all (ip_xattn_kernel's lambda) or one per query (region_xattn_kernel's weights).
template <int D, int QT, int NKK>
__device__ __forceinline__ void ip_segment(const half_t* cK, const half_t* cV, int n, int nkk, const float (&coef)[QT],
                                           float scale_log2e, const h8 (&qf)[QT][(D + 31) / 32],
                                           f4 (&o)[(D + 15) / 16][QT], int fr, int fq) {
    constexpr int KS = (D + 31) / 32;
    constexpr int DT = (D + 15) / 16;
    constexpr int KSTR = ip_kstr(D), VSTR = ip_vstr(D);
    constexpr int NSUB = 2 * NKK;
    const int nsub = 2 * nkk;

    // ---- S^T = K Q^T ----
    f4 s[NSUB][QT];
#pragma unroll
    for (int ksub = 0; ksub < NSUB; ++ksub)
#pragma unroll
        for (int t = 0; t < QT; ++t) s[ksub][t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ksub = 0; ksub < NSUB; ++ksub) {
        if (ksub < nsub) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const h8 kf = *reinterpret_cast<const h8*>(cK + (ksub * 16 + fr) * KSTR + ks * 32 + fq * 8);
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    s[ksub][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[t][ks], s[ksub][t], 0, 0, 0);
            }
        }
    }
    // ---- exact softmax per query (= per lane column): keys >= n never win and weigh 0 ----
    unsigned pf[QT][NKK][4];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float m = -INFINITY;
#pragma unroll
        for (int ksub = 0; ksub < NSUB; ++ksub) {
            if (ksub < nsub) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (ksub * 16 + fq * 4 + j >= n) s[ksub][t][j] = -INFINITY;
                    m = fmaxf(m, s[ksub][t][j]);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        const float nm = -m * scale_log2e;
        float l = 0.f;
#pragma unroll
        for (int ksub = 0; ksub < NSUB; ++ksub) {
            if (ksub < nsub) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[ksub][t][j], scale_log2e, nm));
                    s[ksub][t][j] = p;
                    l += p;
                }
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float w = coef[t] / l;
#pragma unroll
        for (int ksub = 0; ksub < NSUB; ++ksub) {
            if (ksub < nsub) {
                pf[t][ksub >> 1][(ksub & 1) * 2] = pack_rte(s[ksub][t][0] * w, s[ksub][t][1] * w);
                pf[t][ksub >> 1][(ksub & 1) * 2 + 1] = pack_rte(s[ksub][t][2] * w, s[ksub][t][3] * w);
            }
        }
    }
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        if (kk < nkk) {
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const half_t* a0 = cV + (kk * 32 + fq * 4 + (fr >> 2)) * VSTR + i * 16 + (fr & 3) * 4;
                const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0));
                const s4v hi =
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(a0 + 16 * VSTR));
                union { struct { s4v a, b; } p; h8 v; } u;
                u.p.a = lo; u.p.b = hi;
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    union { unsigned w[4]; h8 v; } pb;
#pragma unroll
                    for (int e = 0; e < 4; ++e) pb.w[e] = pf[t][kk][e];
                    o[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(u.v, pb.v, o[i][t], 0, 0, 0);
                }
            }
        }
    }
}

template <int D, int QT, int NKK>
__device__ __forceinline__ void ip_segment(const half_t* cK, const half_t* cV, int n, int nkk, float coef,
                                           float scale_log2e, const h8 (&qf)[QT][(D + 31) / 32],
                                           f4 (&o)[(D + 15) / 16][QT], int fr, int fq) {
    float coefs[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) coefs[t] = coef;
    ip_segment<D, QT, NKK>(cK, cV, n, nkk, coefs, scale_log2e, qf, o, fr, fq);
}

}  // namespace
}  // namespace sd
