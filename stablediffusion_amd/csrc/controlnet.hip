// ControlNet kernels for gfx950 (diffusers 0.27.2 ControlNetModel):
//
//   cn_residual_kernel   every zero-conv of a ControlNet and its scaled add into the UNet's skips, one launch:
//                        y_i = fp16(y_i + s (x_i W_i^T + b_i)) for up to 16 independent problems (K = N = C_i).
//   cn_cond_conv_kernel  one layer of ControlNetConditioningEmbedding: 3x3 conv, stride 1 or 2, pad 1, bias, SiLU,
//                        NHWC fp16 out (NCHW fp16 in for the first layer, which reads the control image).
//   cn_fold_scales_kernel  MultiControlNet: every site's zero-conv weights of the running nets, scaled and column-
//                        concatenated for one GEMM on [h_1 | ... | h_n]; one grouped launch.
#include <atomic>
#include <cstdlib>

#include "kernels.h"

namespace sd {

namespace {

// ------------------------------------------------------------------------------------ grouped zero-convs
// Tile 128 (rows) x 64 (columns); four waves, 32 rows each.  Both operands go straight from global memory into MFMA
// fragments (16 bytes per lane): the weight rows of a 64-column tile (<= 160 KB at C = 1280) stay in L2, and the
// 64-column tiles of one row tile are neighbours in the joint tile list, so its activation rows are fetched into one
// L2 and reused there.  acc = W x^T per 16 x 16 block: lane (fr, fq) ends with row fr, columns fq*4 .. fq*4+3 -- one
// 8-byte read-modify-write of y per block.  No split-K: every output element is read and written by one lane.
constexpr int kResBM = 128, kResBN = 64;

__global__ __launch_bounds__(256) void cn_residual_kernel(CnResParams P) {
    const int tile = blockIdx.x;
    // the problem of this block: the last one whose first tile is <= tile (block-uniform selects, no indexed loads)
    CnResProblem q = P.p[0];
#pragma unroll
    for (int i = 1; i < kCnMaxProblems; ++i)
        if (i < P.count && tile >= P.p[i].first) q = P.p[i];
    const int ntn = q.C / kResBN;
    const int t = tile - q.first;
    const int tm = t / ntn, tn = t - tm * ntn;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    const long m0 = (long)tm * kResBM + wave * 32;
    if (m0 >= q.M) return;
    const int n0 = tn * kResBN;
    // rows past M are clamped for the loads (in bounds) and skipped at the store
    const long r0 = m0 + fr < q.M ? m0 + fr : q.M - 1;
    const long r1 = m0 + 16 + fr < q.M ? m0 + 16 + fr : q.M - 1;
    const half_t* xa0 = q.x + r0 * q.ldx + fq * 8;
    const half_t* xa1 = q.x + r1 * q.ldx + fq * 8;
    const half_t* wb = q.w + (long)(n0 + fr) * q.C + fq * 8;
    const long wstep = 16L * q.C;
    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    h8 a[2], b[4];
    a[0] = *reinterpret_cast<const h8*>(xa0);
    a[1] = *reinterpret_cast<const h8*>(xa1);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const h8*>(wb + j * wstep);
    for (int k = 32; k <= q.C; k += 32) {
        // next K step's fragments in flight while this one's MFMAs run
        h8 na[2], nb[4];
        const int kk = k < q.C ? k : 0;
        na[0] = *reinterpret_cast<const h8*>(xa0 + kk);
        na[1] = *reinterpret_cast<const h8*>(xa1 + kk);
#pragma unroll
        for (int j = 0; j < 4; ++j) nb[j] = *reinterpret_cast<const h8*>(wb + j * wstep + kk);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[i][j], 0, 0, 0);
        a[0] = na[0]; a[1] = na[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = nb[j];
    }
    const float s = P.scale;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long row = m0 + i * 16 + fr;
        if (row >= q.M) continue;
        half_t* yr = q.y + row * q.ldy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + j * 16 + fq * 4;
            const f4 bias = *reinterpret_cast<const f4*>(q.bias + col);
            h4 old = *reinterpret_cast<const h4*>(yr + col);
            h4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)((float)old[e] + s * (acc[i][j][e] + bias[e]));
            *reinterpret_cast<h4*>(yr + col) = o;
        }
    }
}

// --------------------------------------------------------------------------- MultiControlNet scale fold
// One lane per 16-byte piece of an output: first the rows x n x C / 8 pieces of w_cat, then the rows / 4 pieces of
// b_cat.  Memory-bound copy with one multiply per element; the site of a block is found as cn_residual_kernel does.
__global__ __launch_bounds__(256) void cn_fold_scales_kernel(CnFoldParams P) {
    const int blk = blockIdx.x;
    CnFoldSite q = P.s[0];
#pragma unroll
    for (int i = 1; i < kCnMaxProblems; ++i)
        if (i < P.count && blk >= P.s[i].first) q = P.s[i];
    const long item = (long)(blk - q.first) * 256 + threadIdx.x;
    const int c8 = q.C >> 3;
    const long nw = (long)q.rows * P.n * c8;
    if (item < nw) {
        const int kc = (int)(item % c8);
        const long r = item / c8;
        const int net = (int)(r % P.n);
        const long o = r / P.n;
        const half_t* w = q.w[0];
        float s = P.scale[0];
#pragma unroll
        for (int j = 1; j < kCnMaxNets; ++j)
            if (net == j) { w = q.w[j]; s = P.scale[j]; }
        const h8 v = *reinterpret_cast<const h8*>(w + o * q.C + kc * 8);
        h8 out;
#pragma unroll
        for (int e = 0; e < 8; ++e) out[e] = (half_t)((float)v[e] * s);
        *reinterpret_cast<h8*>(q.w_cat + o * ((long)P.n * q.C) + (long)net * q.C + kc * 8) = out;
    } else if (item - nw < (q.rows >> 2)) {
#pragma clang fp contract(off)
        const long o4 = (item - nw) * 4;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kCnMaxNets; ++j) {
            if (j >= P.n) break;
            const f4 b = *reinterpret_cast<const f4*>(q.bias[j] + o4);
            const float s = P.scale[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = s * b[e];
                acc[e] = j == 0 ? t : acc[e] + t;
            }
        }
        *reinterpret_cast<f4*>(q.b_cat + o4) = acc;
    }
}

// ------------------------------------------------------------------------------- conditioning embedding
// VALU form: one lane per output pixel, 16 output channels per block row (blockIdx.y).  The weights of those 16
// channels are read at block-uniform addresses ([Cout / 16][9 Cin][16] fp32), so they come in through the scalar
// cache and every multiply-add takes its weight as an SGPR operand; the input value is loaded once per (tap,
// channel) and reused 16 times.  Out-of-image taps read a clamped pixel and multiply by zero (no divergence).
template <int CIN, bool NCHW>
__global__ __launch_bounds__(256) void cn_cond_conv_kernel(CnCondConvParams p) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)p.N * p.OH * p.OW;
    if (pix >= total) return;
    const int cb = blockIdx.y;
    const long ohw = (long)p.OH * p.OW;
    const int n = (int)(pix / ohw);
    const int rem = (int)(pix - (long)n * ohw);
    const int oy = rem / p.OW, ox = rem - oy * p.OW;
    const float* __restrict__ wblk = p.w + (long)cb * 9 * CIN * 16;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = p.bias[cb * 16 + j];
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * p.stride - 1 + ky;
        const bool vy = iy >= 0 && iy < p.IH;
        const int cy = vy ? iy : 0;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * p.stride - 1 + kx;
            const bool ok = vy && ix >= 0 && ix < p.IW;
            const int cx = (ix >= 0 && ix < p.IW) ? ix : 0;
            const float z = ok ? 1.f : 0.f;
            const float* __restrict__ wk = wblk + (ky * 3 + kx) * CIN * 16;
            if (NCHW) {
                const long plane = (long)p.IH * p.IW;
                const half_t* xp = p.x + (long)n * CIN * plane + (long)cy * p.IW + cx;
#pragma unroll
                for (int c = 0; c < CIN; ++c) {
                    const float v = z * (float)xp[c * plane];
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[j] = __builtin_fmaf(v, wk[c * 16 + j], acc[j]);
                }
            } else {
                const half_t* xp = p.x + (((long)n * p.IH + cy) * p.IW + cx) * CIN;
#pragma unroll 2
                for (int c8 = 0; c8 < CIN / 8; ++c8) {
                    const h8 v8 = *reinterpret_cast<const h8*>(xp + c8 * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = z * (float)v8[e];
                        const float* we = wk + (c8 * 8 + e) * 16;
#pragma unroll
                        for (int j = 0; j < 16; ++j) acc[j] = __builtin_fmaf(v, we[j], acc[j]);
                    }
                }
            }
        }
    }
    h8 o[2];
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j >> 3][j & 7] = (half_t)(p.silu ? silu_f(acc[j]) : acc[j]);
    half_t* yp = p.y + pix * p.Cout + cb * 16;
    *reinterpret_cast<h8*>(yp) = o[0];
    *reinterpret_cast<h8*>(yp + 8) = o[1];
}

// OIHW fp16 -> [O / 16][kh][kw][I][16] fp32
__global__ void cn_pack_cond_kernel(const half_t* w, float* out, int O, int I) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)O * I * 9;
    if (idx >= n) return;
    const int j = (int)(idx & 15);
    long r = idx >> 4;
    const int ci = (int)(r % I); r /= I;
    const int tap = (int)(r % 9); r /= 9;
    const int cb = (int)r;
    const int co = cb * 16 + j;
    out[idx] = (float)w[((long)co * I + ci) * 9 + tap];
}

}  // namespace

bool cn_residual_supported(const CnResParams& p) {
    if (p.count < 1 || p.count > kCnMaxProblems) return false;
    int next = 0;
    for (int i = 0; i < p.count; ++i) {
        const CnResProblem& q = p.p[i];
        if (q.C <= 0 || q.C % 64 != 0 || q.M <= 0 || q.first != next) return false;
        if (!q.x || !q.w || !q.bias || !q.y || q.ldx < q.C || q.ldy < q.C || q.ldx % 8 != 0 || q.ldy % 4 != 0) return false;
        if ((reinterpret_cast<uintptr_t>(q.x) & 15) || (reinterpret_cast<uintptr_t>(q.y) & 7) ||
            (reinterpret_cast<uintptr_t>(q.w) & 15) || (reinterpret_cast<uintptr_t>(q.bias) & 15)) return false;
        next += cdiv(q.M, kResBM) * (q.C / kResBN);
    }
    return next == p.total;
}

int cn_residual_tiles(int M, int C) { return cdiv(M, kResBM) * (C / kResBN); }

int launch_cn_residual(const CnResParams& p, hipStream_t s) {
    if (!cn_residual_supported(p)) { set_error("cn_residual: unsupported problem table"); return 4; }
    if (p.scale == 0.f) return 0;          // y + 0 (x W^T + b) == y
    hipLaunchKernelGGL(cn_residual_kernel, dim3((unsigned)p.total), dim3(256), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return 3; }
    return 0;
}

int cn_fold_blocks(int rows, int C, int n) { return (int)cdiv((long)rows * n * (C / 8) + rows / 4, 256); }

bool cn_fold_supported(const CnFoldParams& p) {
    if (p.count < 1 || p.count > kCnMaxProblems || p.n < 1 || p.n > kCnMaxNets) return false;
    int next = 0;
    for (int i = 0; i < p.count; ++i) {
        const CnFoldSite& q = p.s[i];
        if (q.C <= 0 || q.C % 8 != 0 || q.rows <= 0 || q.rows % 4 != 0 || q.first != next) return false;
        if (!q.w_cat || !q.b_cat || (reinterpret_cast<uintptr_t>(q.w_cat) & 15) || (reinterpret_cast<uintptr_t>(q.b_cat) & 15)) return false;
        for (int j = 0; j < p.n; ++j)
            if (!q.w[j] || !q.bias[j] || (reinterpret_cast<uintptr_t>(q.w[j]) & 15) || (reinterpret_cast<uintptr_t>(q.bias[j]) & 15)) return false;
        next += cn_fold_blocks(q.rows, q.C, p.n);
    }
    return next == p.total;
}

int launch_cn_fold_scales(const CnFoldParams& p, hipStream_t s) {
    if (!cn_fold_supported(p)) { set_error("cn_fold_scales: unsupported site table"); return 4; }
    hipLaunchKernelGGL(cn_fold_scales_kernel, dim3((unsigned)p.total), dim3(256), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return 3; }
    return 0;
}

namespace {
std::atomic<int> g_cn_kcat_mode{-1};
// The default for two or more running nets (profiles/multi_controlnet.txt).
constexpr bool kCnKcatDefault = true;
}  // namespace
void cn_kcat_force(int mode) { g_cn_kcat_mode = mode < -1 || mode > 1 ? -1 : mode; }
bool cn_kcat_on() {
    const int m = g_cn_kcat_mode;
    if (m >= 0) return m == 1;
    static const bool off = getenv("SD_NO_CN_KCAT") != nullptr && getenv("SD_NO_CN_KCAT")[0] == '1';
    return kCnKcatDefault && !off;
}

bool cn_cond_conv_supported(const CnCondConvParams& p) {
    const bool cin_ok = p.nchw ? p.Cin == 3 : (p.Cin == 16 || p.Cin == 32 || p.Cin == 96);
    if (!cin_ok || p.Cout <= 0 || p.Cout % 16 != 0 || (p.stride != 1 && p.stride != 2)) return false;
    if (p.N <= 0 || p.IH <= 0 || p.IW <= 0) return false;
    return p.OH == (p.IH - 1) / p.stride + 1 && p.OW == (p.IW - 1) / p.stride + 1;
}

int launch_cn_cond_conv(const CnCondConvParams& p, hipStream_t s) {
    if (!cn_cond_conv_supported(p)) { set_error("cn_cond_conv: unsupported layer"); return 4; }
    const long total = (long)p.N * p.OH * p.OW;
    const dim3 grid((unsigned)cdiv(total, 256), (unsigned)(p.Cout / 16));
    if (p.nchw) hipLaunchKernelGGL((cn_cond_conv_kernel<3, true>), grid, dim3(256), 0, s, p);
    else if (p.Cin == 16) hipLaunchKernelGGL((cn_cond_conv_kernel<16, false>), grid, dim3(256), 0, s, p);
    else if (p.Cin == 32) hipLaunchKernelGGL((cn_cond_conv_kernel<32, false>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((cn_cond_conv_kernel<96, false>), grid, dim3(256), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return 3; }
    return 0;
}

int launch_cn_pack_cond(const half_t* w_oihw, float* out, int O, int I, hipStream_t s) {
    if (O % 16 != 0) { set_error("cn_pack_cond: output channels must be a multiple of 16"); return 4; }
    const long n = (long)O * I * 9;
    hipLaunchKernelGGL(cn_pack_cond_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, w_oihw, out, O, I);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return 3; }
    return 0;
}

}  // namespace sd
