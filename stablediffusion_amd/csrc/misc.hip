// Small / HBM-bound helper kernels for the gfx950 denoise engine: timestep sinusoid, batch-sized
// linear layers (time-embedding MLPs), layout changes at the NCHW boundary, weight packing and the
// CFG + DDIM elementwise update.  wave64 throughout.
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "kernels.h"

namespace sd {
namespace {

// diffusers get_timestep_embedding (Timesteps): restated for UNet2DConditionModel.time_proj /
// add_time_proj under /root/reference/pipelines/sd_unified_pipeline.py:475-482.
// One (sin, cos) pair of the embedding: every kernel that writes a sinusoid calls this, so their bits agree.
__device__ __forceinline__ void sinusoid_pair(float t, int f, int half, float shift, float* sn, float* cs) {
    const float freq = __expf(-9.210340371976184f * (float)f / ((float)half - shift));
    const float ang = t * freq;
    sincosf(ang, sn, cs);
}

__global__ void sinusoid_kernel(const float* __restrict__ t, int t_stride, float* __restrict__ out, int count,
                                int dim, int flip, float shift, long out_ld) {
    const int half = dim >> 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * half) return;
    const int b = i / half, f = i - b * half;
    float sn, cs;
    sinusoid_pair(t[(long)b * t_stride], f, half, shift, &sn, &cs);
    float* o = out + (long)b * out_ld;
    if (flip) { o[f] = cs; o[half + f] = sn; } else { o[f] = sn; o[half + f] = cs; }
}

// The input of add_embedding.linear_1 (text_time conditioning), one launch for B rows of P + n * ad floats, out_ld apart:
//   out[b, :P] = f32(text[b, :]),   out[b, P + j*ad + (f | half + f)] = sinusoid(ids[b, j]) pair f,   j < n
// and zeros in the columns [P + n * ad, out_ld) (the row padded to the packed weight's K).  One thread per output unit
// of a row: the first P units convert one pooled value each (exact), the next n * ad / 2 each own one (sin, cos) pair
// as a thread of sinusoid_kernel does, the last out_ld - (P + n * ad) write one zero each.
__global__ __launch_bounds__(256) void text_time_input_kernel(const half_t* __restrict__ text, const float* __restrict__ ids,
                                                              float* __restrict__ out, int B, int P, int ad, int n,
                                                              int flip, float shift, int out_ld) {
    const int half = ad >> 1;
    const int width = P + n * ad;
    const int per_row = P + n * half + (out_ld - width);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * per_row) return;
    const int b = (int)(i / per_row), u = (int)(i - (long)b * per_row);
    float* o = out + (long)b * out_ld;
    if (u < P) { o[u] = (float)text[(long)b * P + u]; return; }
    if (u >= P + n * half) { o[width + (u - P - n * half)] = 0.f; return; }
    const int j = (u - P) / half, f = (u - P) - j * half;
    float sn, cs;
    sinusoid_pair(ids[(long)b * n + j], f, half, shift, &sn, &cs);
    o += P + j * ad;
    if (flip) { o[f] = cs; o[half + f] = sn; } else { o[f] = sn; o[half + f] = cs; }
}

// The input of a guidance-embedded UNet's time embedding (diffusers TimestepEmbedding with cond_proj_dim, LCM):
//   out[b, j] = sinusoid(t_b)[j] + sum_k W[j, k] cond[b, k]
// in the place of sinusoid_kernel's launch.  One wave per (b, f): it owns the output pair (f, half + f) like a thread of
// sinusoid_kernel does, so the sinusoid is that kernel's expression instruction for instruction, and the two dot
// products (fp16 weights, fp32 accumulation, lanes over k, butterfly reduction) are added to it last: cond = 0 leaves the
// sinusoid's bits.  w rows are ldw halves apart (the packed K of WeightStore::pack_conv, zero padded; cond_dim itself for
// a raw matrix); VEC: ldw % 8 == 0 and a 16-byte aligned base, 16-byte weight loads.  A few hundred KB of weights: the
// launch costs what the sinusoid's did.
template <bool VEC>
__global__ __launch_bounds__(256) void temb_cond_kernel(const float* __restrict__ t, const float* __restrict__ cond,
                                                        const half_t* __restrict__ w, long ldw, float* __restrict__ out,
                                                        int count, int dim, int cond_dim, int flip, float shift) {
    const int half = dim >> 1;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // wave-uniform
    if (i >= count * half) return;
    const int b = i / half, f = i - b * half;
    const int r0 = flip ? half + f : f, r1 = flip ? f : half + f;            // rows of the sin and of the cos output
    const half_t* w0 = w + (long)r0 * ldw;
    const half_t* w1 = w + (long)r1 * ldw;
    const float* c = cond + (long)b * cond_dim;
    float a0 = 0.f, a1 = 0.f;
    if (VEC) {
        for (int k = lane * 8; k < cond_dim; k += 64 * 8) {
            const h8 v0 = *reinterpret_cast<const h8*>(w0 + k);
            const h8 v1 = *reinterpret_cast<const h8*>(w1 + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ce = k + e < cond_dim ? c[k + e] : 0.f;
                a0 = __builtin_fmaf((float)v0[e], ce, a0);
                a1 = __builtin_fmaf((float)v1[e], ce, a1);
            }
        }
    } else {
        for (int k = lane; k < cond_dim; k += 64) {
            const float ce = c[k];
            a0 = __builtin_fmaf((float)w0[k], ce, a0);
            a1 = __builtin_fmaf((float)w1[k], ce, a1);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_xor(a0, off);
        a1 += __shfl_xor(a1, off);
    }
    if (lane != 0) return;
    float sn, cs;
    sinusoid_pair(t[b], f, half, shift, &sn, &cs);
    float* o = out + (long)b * dim;
    o[r0] = sn + a0;
    o[r1] = cs + a1;
}

// y[b, n] = bias[n] + sum_k act(x[b,k]) W[n,k] for a handful of rows b (time-embedding MLPs).
// Weight-bandwidth bound (the stacked time_emb_proj matrix is 67 MB): one wave owns SL_COLS output
// columns so it keeps SL_COLS independent 16-byte weight loads in flight per lane; the activation
// rows (a few KB) are re-read from L1/L2.  Batch chunked by 8.
constexpr int SL_MAXB = 8;
constexpr int SL_COLS = 4;
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ x, long ldx,
                                                           const half_t* __restrict__ w,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ y, long ldy, int B,
                                                           int K, int Nout, int silu_in, int silu_out) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SL_COLS;
    if (n0 >= Nout) return;
    for (int b0 = 0; b0 < B; b0 += SL_MAXB) {
        float acc[SL_COLS][SL_MAXB];
#pragma unroll
        for (int c = 0; c < SL_COLS; ++c)
#pragma unroll
            for (int b = 0; b < SL_MAXB; ++b) acc[c][b] = 0.f;
        for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
            h8 wv[SL_COLS];
#pragma unroll
            for (int c = 0; c < SL_COLS; ++c) {
                const int n = n0 + c < Nout ? n0 + c : Nout - 1;
                wv[c] = *reinterpret_cast<const h8*>(w + (long)n * K + k0);
            }
#pragma unroll
            for (int b = 0; b < SL_MAXB; ++b) {
                if (b0 + b < B) {
                    const float* xr = x + (long)(b0 + b) * ldx + k0;
                    const f4 x0 = *reinterpret_cast<const f4*>(xr);
                    const f4 x1 = *reinterpret_cast<const f4*>(xr + 4);
                    float a[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = silu_in ? silu_f(x0[e]) : x0[e];
                        a[e + 4] = silu_in ? silu_f(x1[e]) : x1[e];
                    }
#pragma unroll
                    for (int c = 0; c < SL_COLS; ++c)
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[c][b] += a[e] * (float)wv[c][e];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < SL_COLS; ++c)
#pragma unroll
            for (int b = 0; b < SL_MAXB; ++b) {
                float a = acc[c][b];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
                if (lane == 0 && b0 + b < B && n0 + c < Nout) {
                    a += bias ? bias[n0 + c] : 0.f;
                    if (silu_out) a = silu_f(a);
                    y[(long)(b0 + b) * ldy + n0 + c] = a;
                }
            }
    }
}

// y = act(y + x): the SDXL `emb + aug_emb`, and (x == nullptr) a plain in-place SiLU.
__global__ void add_f32_kernel(float* y, const float* x, long n, int silu) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        float v = y[i] + (x ? x[i] : 0.f);
        y[i] = silu ? silu_f(v) : v;
    }
}
__global__ void f16_to_f32_kernel(const half_t* x, float* y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (float)x[i];
}
__global__ void f32_to_f16_kernel(const float* x, half_t* y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (half_t)x[i];
}

// x NCHW [N,C,H,W] (tiny C) -> col [N*H*W, Kpad], k = (kh*3+kw)*C + c, zero padded.
__global__ void im2col_nchw3x3_kernel(const half_t* __restrict__ x, half_t* __restrict__ col, int N,
                                      int C, int H, int W, int Kpad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)N * H * W * Kpad;
    if (i >= total) return;
    const int kq = (int)(i % Kpad);
    const long m = i / Kpad;
    half_t val = (half_t)0.f;
    if (kq < 9 * C) {
        const int tap = kq / C, c = kq - tap * C;
        const int kh = tap / 3, kw = tap - kh * 3;
        const int w_ = (int)(m % W);
        const int h_ = (int)((m / W) % H);
        const int n = (int)(m / ((long)W * H));
        const int ih = h_ + kh - 1, iw = w_ + kw - 1;
        if (ih >= 0 && ih < H && iw >= 0 && iw < W) val = x[(((long)n * C + c) * H + ih) * W + iw];
    }
    col[i] = val;
}

__global__ void nhwc_to_nchw_kernel(const half_t* __restrict__ x, long ldx, half_t* __restrict__ y,
                                    int N, long HW, int C) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over N*C*HW (output order)
    if (i >= (long)N * C * HW) return;
    const long pix = i % HW;
    const int c = (int)((i / HW) % C);
    const long n = i / (HW * C);
    y[i] = x[(n * HW + pix) * ldx + c];
}

__global__ void nchw_to_nhwc_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long ldy,
                                    int N, long HW, int C) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over N*HW*C (output order)
    if (i >= (long)N * C * HW) return;
    const int c = (int)(i % C);
    const long pix = (i / C) % HW;
    const long n = i / (HW * C);
    y[(n * HW + pix) * ldy + c] = x[(n * C + c) * HW + pix];
}

__global__ void pointwise_nchw_kernel(const half_t* __restrict__ x, const half_t* __restrict__ w,
                                      const float* __restrict__ bias, half_t* __restrict__ y, int N,
                                      int Cin, int Cout, long HW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * Cout * HW) return;
    const long pix = i % HW;
    const int co = (int)((i / HW) % Cout);
    const long n = i / (HW * Cout);
    float acc = bias ? bias[co] : 0.f;
    for (int ci = 0; ci < Cin; ++ci)
        acc += (float)x[(n * Cin + ci) * HW + pix] * (float)w[co * Cin + ci];
    y[i] = (half_t)acc;
}

// K order of a packed KxK conv weight row (Cin % 64 == 0): [Cin/64][KH][KW][64] -- the nine taps of
// one 64-channel slab are consecutive, so the implicit-GEMM gather re-reads the same input lines
// nine times back to back (L2 hits) instead of streaming the whole tile footprint once per tap.
// Small-Cin convs (conv_in, via im2col) keep [KH][KW][Cin].
__global__ void pack_conv_kernel(const half_t* __restrict__ w, half_t* __restrict__ wp, int O, int I,
                                 int KH, int KW, long Kpad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over O * Kpad
    if (i >= (long)O * Kpad) return;
    const long kq = i % Kpad;
    const long o = i / Kpad;
    half_t val = (half_t)0.f;
    if (kq < (long)KH * KW * I) {
        int ci, tap;
        if (I % 64 == 0) {
            const int slab = (int)(kq >> 6), cl = (int)(kq & 63);
            const int cs = slab / (KH * KW);
            tap = slab - cs * (KH * KW);
            ci = cs * 64 + cl;
        } else {
            ci = (int)(kq % I);
            tap = (int)(kq / I);
        }
        const int kh = tap / KW, kw = tap - kh * KW;
        val = w[((o * I + ci) * KH + kh) * KW + kw];
    }
    wp[i] = val;
}

// Nearest-2x upsample + 3x3 conv = four 2x2 convs on the input map (kernels.h: launch_fold_upconv).  One thread per
// folded weight: parity (dy, dx), output row o, K position [I/64][a][b][64].  Row tap a of parity dy covers kernel
// rows lo..hi (dy 0: {0}, {1, 2}; dy 1: {0, 1}, {2}), columns likewise; summed in fp32, kh-major, one rounding.
__global__ void fold_upconv_kernel(const half_t* __restrict__ w, half_t* __restrict__ wp, int O, int I, long rows) {
    const long K4 = 4L * I;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over 4 * O * K4
    if (i >= 4 * O * K4) return;
    const long kq = i % K4;
    const long o = (i / K4) % O;
    const int par = (int)(i / (K4 * O));
    const int dy = par >> 1, dx = par & 1;
    const int slab = (int)(kq >> 6), cl = (int)(kq & 63);
    const int tap = slab & 3, a = tap >> 1, b = tap & 1;
    const long ci = (long)(slab >> 2) * 64 + cl;
    const int h_lo = a == 0 ? 0 : 2 - (1 - dy), h_hi = a == 0 ? dy : 2;
    const int w_lo = b == 0 ? 0 : 2 - (1 - dx), w_hi = b == 0 ? dx : 2;
    float s = 0.f;
    for (int kh = h_lo; kh <= h_hi; ++kh)
        for (int kw = w_lo; kw <= w_hi; ++kw) s += (float)w[((o * I + ci) * 3 + kh) * 3 + kw];
    wp[((long)par * rows + o) * K4 + kq] = (half_t)s;
}

// sd_unified_pipeline.py:467-472: latent_model_input = scale_model_input(cat([latents]*2))
__global__ void cfg_duplicate_kernel(const half_t* __restrict__ lat, half_t* __restrict__ out, long n,
                                     float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const half_t v = (half_t)((float)lat[i] * scale);
    out[i] = v;
    out[n + i] = v;
}
// Shared CFG prefix (UNet::run): the first B rows of a tensor that the 2B-row remainder of the forward reads are copied
// onto its second B rows.  One launch for every such tensor: segment i is `rows` rows of w16 16-byte units, row stride
// ld16 units, copied from src to dst; its blocks are [first, next segment's first), RD_UNITS units each.
constexpr int RD_PER_THREAD = 4;
constexpr int RD_UNITS = 256 * RD_PER_THREAD;
struct RowDupDev {
    const uint4* src[kRowDupMax];
    uint4* dst[kRowDupMax];
    long ld16[kRowDupMax], w16[kRowDupMax], units[kRowDupMax];
    int first[kRowDupMax + 1];
    int count;
};
__global__ __launch_bounds__(256) void row_dup_kernel(RowDupDev p) {
    int sg = 0;
    while (sg + 1 < p.count && (int)blockIdx.x >= p.first[sg + 1]) ++sg;
    const uint4* __restrict__ src = p.src[sg];
    uint4* __restrict__ dst = p.dst[sg];
    const long ld = p.ld16[sg], w = p.w16[sg], n = p.units[sg];
    const long base = (long)((int)blockIdx.x - p.first[sg]) * RD_UNITS + threadIdx.x;
    uint4 v[RD_PER_THREAD];
    long off[RD_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RD_PER_THREAD; ++j) {
        const long i = base + j * 256;
        off[j] = -1;
        if (i < n) {
            const long r = i / w;
            off[j] = r * ld + (i - r * w);
            v[j] = src[off[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < RD_PER_THREAD; ++j)
        if (off[j] >= 0) dst[off[j]] = v[j];
}
// out[i] = fp16(lat[i] * scale): cfg_duplicate_kernel's rounding, one copy
__global__ void scale_copy_f16_kernel(const half_t* __restrict__ lat, half_t* __restrict__ out, long n, float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (half_t)((float)lat[i] * scale);
}
// out[n][c][px] = c < Ca ? fp16(a[n % Na][c][px] * scale) : n < zero_from ? b[n % Nb][c - Ca][px] : 0
__global__ void concat_sample_kernel(const half_t* __restrict__ a, int Na, int Ca, float scale, const half_t* __restrict__ b,
                                     int Nb, int Cb, int zero_from, half_t* __restrict__ out, long total, long HW) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long px = i % HW, nc = i / HW;
    const int C = Ca + Cb, c = (int)(nc % C), n = (int)(nc / C);
    half_t v = (half_t)0.f;
    if (c < Ca) v = (half_t)((float)a[((long)(n % Na) * Ca + c) * HW + px] * scale);
    else if (n < zero_from) v = b[((long)(n % Nb) * Cb + (c - Ca)) * HW + px];
    out[i] = v;
}
__global__ void dup_f32_kernel(const float* __restrict__ x, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    out[i] = v;
    out[n + i] = v;
}

// sd_unified_pipeline.py:484-489 for any scheduler whose update is linear in (x, eps, previous x0 prediction): DDIM, Euler, DPM-Solver++(2M).
//   eps = u + g (t - u);  x0 = hx x + he eps;  x <- cx x + ce eps + ch hist;  hist <- x0
// (hist fp32, like the host schedulers keep their history; null when the scheduler has none)
__global__ void cfg_linear_kernel(const half_t* __restrict__ eps2b, half_t* __restrict__ lat,
                                  float* __restrict__ hist, long n, float g, float cx, float ce, float ch,
                                  float hx, float he) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float eu = (float)eps2b[i], et = (float)eps2b[n + i];
    const float e = (float)(half_t)(g * (et - eu) + eu);
    const float x = (float)lat[i];
    float out = cx * x + ce * e;
    if (hist) {
        out += ch * hist[i];
        hist[i] = hx * x + he * e;
    }
    lat[i] = (half_t)out;
}

// One step of a scheduler that adds noise (LCMScheduler.step), the guidance combine included:
//   m = model_out (ROWS == 1) or fp16(u + g (t - u)) (ROWS == 2, cfg_linear_kernel's rounding: one fma, then fp16)
//   den = dx x + dout m;  denoised <- fp16(den);  x <- fp16(pden den + pnoise noise)
// den and the update are evaluated in fp64: dx x and dout m cancel (|dx|, |dout| ~ 15 on the first of four steps, the
// result O(1) and often near 0) and fp16 resolves 2^-24 around zero, so the 4e-7 an fp32 evaluation of the two products
// is off by there would be several fp16 ulps.  A dozen fp64 FMAs per element next to four or five fp16 streams; the
// kernel's time next to the fp32 step kernel of the same traffic is in DESIGN.md section 4.
// VEC: n % 8 == 0 and 16-byte aligned bases.
template <int ROWS>
__device__ __forceinline__ void lcm_element(float eu, float et, float xf, float nz, float g, double dx, double dout,
                                            double pden, double pnoise, half_t* den16, half_t* x16) {
    const float m = ROWS == 2 ? (float)(half_t)__builtin_fmaf(g, et - eu, eu) : eu;
    const double den = __builtin_fma(dx, (double)xf, dout * (double)m);
    *den16 = (half_t)den;
    *x16 = (half_t)__builtin_fma(pden, den, pnoise * (double)nz);
}
template <int ROWS, bool VEC>
__global__ __launch_bounds__(256) void lcm_step_kernel(const half_t* __restrict__ mo, half_t* __restrict__ lat,
                                                       const half_t* __restrict__ noise, half_t* __restrict__ denoised,
                                                       long n, float g, float dx, float dout, float pden, float pnoise) {
    if (VEC) {
        const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
        if (i >= n) return;
        const h8 vu = *reinterpret_cast<const h8*>(mo + i);
        h8 vt = vu, vn = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ROWS == 2) vt = *reinterpret_cast<const h8*>(mo + n + i);
        const h8 vx = *reinterpret_cast<const h8*>(lat + i);
        if (noise) vn = *reinterpret_cast<const h8*>(noise + i);
        h8 od, ox;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            half_t d, x;
            lcm_element<ROWS>((float)vu[j], (float)vt[j], (float)vx[j], (float)vn[j], g, dx, dout, pden, pnoise, &d, &x);
            od[j] = d;
            ox[j] = x;
        }
        *reinterpret_cast<h8*>(lat + i) = ox;
        if (denoised) *reinterpret_cast<h8*>(denoised + i) = od;
    } else {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        half_t d, x;
        lcm_element<ROWS>((float)mo[i], ROWS == 2 ? (float)mo[n + i] : 0.f, (float)lat[i], noise ? (float)noise[i] : 0.f, g,
                          dx, dout, pden, pnoise, &d, &x);
        lat[i] = x;
        if (denoised) denoised[i] = d;
    }
}

// One step of a scheduler that is affine in (x, m, z) and up to four fp32 history tensors (EulerAncestral, DPM++ 2M SDE,
// PNDM, UniPC: schedulers.py `affine_plan`), the guidance combine included:
//   v = (x, m, z, h_0 .. h_3), m as in lcm_element;  x <- fp16(out . v);  h[write_slot[j]] <- fp32(write[j] . v)
// Every row is a chain of fp64 FMAs over the columns whose coefficient is not 0 (the plan is a kernel argument: the
// branches are uniform), rounded once: UniPC's collected predictor / corrector rows and the sigma-space x and m terms of
// the first steps cancel, as lcm_element's do.  `use` has bit k set when column k is non-zero in some used row; the
// other operands are never loaded, so an unwritten slot or an absent noise tensor may hold anything.  A thread loads all
// its operands before it stores anything and no other thread touches its elements, so a slot may be read and written.
// VEC: n % 8 == 0, stride % 4 == 0 and 16-byte aligned bases.
template <int W>
__device__ __forceinline__ void step_load(const half_t* __restrict__ p, float* o) {
    if constexpr (W == 8) {
        const h8 v = *reinterpret_cast<const h8*>(p);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = (float)v[j];
    } else {
        o[0] = (float)p[0];
    }
}
__device__ __forceinline__ double step_row(const double* c, const double* v) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < STEP_COLS; ++k)
        if (c[k] != 0.0) acc = __builtin_fma(c[k], v[k], acc);
    return acc;
}
template <int ROWS, bool VEC>
__global__ __launch_bounds__(256) void sched_affine_kernel(const half_t* __restrict__ mo, half_t* __restrict__ lat,
                                                           const half_t* __restrict__ noise, float* __restrict__ bank,
                                                           long stride, long n, float g, StepRows p, unsigned use) {
    constexpr int W = VEC ? 8 : 1;
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= n) return;
    float x[W] = {}, u[W] = {}, t[W] = {}, z[W] = {}, h[STEP_SLOTS][W] = {};
    if (use & 1u) step_load<W>(lat + i, x);
    if (use & 2u) {
        step_load<W>(mo + i, u);
        if (ROWS == 2) step_load<W>(mo + n + i, t);
    }
    if (use & 4u) step_load<W>(noise + i, z);
#pragma unroll
    for (int k = 0; k < STEP_SLOTS; ++k) {
        if (!(use & (8u << k))) continue;
        const float* src = bank + k * stride + i;
        if constexpr (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
            h[k][0] = a.x; h[k][1] = a.y; h[k][2] = a.z; h[k][3] = a.w;
            h[k][4] = b.x; h[k][5] = b.y; h[k][6] = b.z; h[k][7] = b.w;
        } else {
            h[k][0] = src[0];
        }
    }
    half_t ox[W];
    float ow[STEP_WRITES][W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const float m = ROWS == 2 ? (float)(half_t)__builtin_fmaf(g, t[j] - u[j], u[j]) : u[j];
        double v[STEP_COLS] = {(double)x[j], (double)m, (double)z[j]};
#pragma unroll
        for (int k = 0; k < STEP_SLOTS; ++k) v[3 + k] = (double)h[k][j];
        ox[j] = (half_t)step_row(p.out, v);
#pragma unroll
        for (int w = 0; w < STEP_WRITES; ++w) ow[w][j] = (float)step_row(p.write[w], v);
    }
    if constexpr (VEC) {
        h8 o;
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = ox[j];
        *reinterpret_cast<h8*>(lat + i) = o;
    } else {
        lat[i] = ox[0];
    }
#pragma unroll
    for (int w = 0; w < STEP_WRITES; ++w) {
        if (w >= p.n_writes) break;
        float* dst = bank + p.write_slot[w] * stride + i;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(dst) = make_float4(ow[w][0], ow[w][1], ow[w][2], ow[w][3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(ow[w][4], ow[w][5], ow[w][6], ow[w][7]);
        } else {
            dst[0] = ow[w][0];
        }
    }
}

// ---- guidance rescale (Lin et al. 2023, section 3.4; diffusers rescale_noise_cfg) in front of the same linear update ----
//   e = fp16(u + g (t - u));  k_b = 1 + phi (std(t_b) / std(e_b) - 1);  the update of cfg_linear_kernel on k_b e
// std is per sample over all n elements; std(t) / std(e) = sqrt(M2(t) / M2(e)) (the ddof cancels), M2 = sum (x - mean)^2.
// Two launches: rs_stats_kernel leaves one centred (count, mean, M2) triple per tensor and chunk of a sample, every wave of
// rs_apply_kernel merges its sample's triples (Chan et al.) in the same order, so all blocks of a sample agree on k_b bit
// for bit, and applies the update.  M2 is never formed as E[x^2] - E[x]^2: at a mean of 100 and a deviation of 0.5 that
// difference has lost every digit in fp32 (commit 4edffab's lesson for the GroupNorm summaries).
constexpr int RS_MAX_PARTS = 64;          // chunks per sample: one per lane of the wave that merges them
constexpr int RS_MIN_CHUNK = 2048;        // elements: one 16-byte load per thread and tensor

struct RsStat { float n, mean, m2; };

__device__ __forceinline__ RsStat rs_merge(const RsStat a, const RsStat b) {
    RsStat r;
    r.n = a.n + b.n;
    const float d = b.mean - a.mean;
    const float w = r.n > 0.f ? b.n / r.n : 0.f;
    r.mean = a.mean + d * w;
    r.m2 = a.m2 + b.m2 + d * d * a.n * w;
    return r;
}
__device__ __forceinline__ RsStat rs_wave_merge(RsStat s) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        RsStat o;
        o.n = __shfl_xor(s.n, off);
        o.mean = __shfl_xor(s.mean, off);
        o.m2 = __shfl_xor(s.m2, off);
        // the lower lane of a pair is always the left operand, so both lanes compute the same value
        s = (threadIdx.x & off) ? rs_merge(o, s) : rs_merge(s, o);
    }
    return s;
}
__device__ __forceinline__ float rs_cfg(float eu, float et, float g) { return (float)(half_t)(g * (et - eu) + eu); }
// a x + b e with the roundings cfg_linear_kernel's `a * x + b * e` compiles to under -ffp-contract=fast: the product b e is
// rounded, a x is fused into the add.  Written out because the contraction the compiler picks depends on the code around
// the expression, and k_b = 1 has to reproduce that kernel bit for bit.
__device__ __forceinline__ float rs_axpby(float a, float x, float b, float e) { return __builtin_fmaf(a, x, b * e); }

// part [B][parts][2] triples: (t, e) of chunk p of sample b.  VEC: n % 8 == 0 and 16-byte aligned bases.
template <bool VEC>
__global__ __launch_bounds__(256) void rs_stats_kernel(const half_t* __restrict__ eps2b, RsStat* __restrict__ part, long n,
                                                       long chunk, long total, float g) {
    const int b = blockIdx.y, p = blockIdx.x;
    const half_t* u = eps2b + (long)b * n;
    const half_t* t = u + total;
    const long lo = (long)p * chunk, hi = lo + chunk < n ? lo + chunk : n;
    RsStat st = {0.f, 0.f, 0.f}, se = {0.f, 0.f, 0.f};
    if (VEC) {
        for (long i = lo + (long)threadIdx.x * 8; i < hi; i += 256 * 8) {
            const h8 vu = *reinterpret_cast<const h8*>(u + i);
            const h8 vt = *reinterpret_cast<const h8*>(t + i);
            float ft[8], fe[8], sumt = 0.f, sume = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ft[k] = (float)vt[k];
                fe[k] = rs_cfg((float)vu[k], ft[k], g);
                sumt += ft[k];
                sume += fe[k];
            }
            RsStat vt8 = {8.f, sumt * 0.125f, 0.f}, ve8 = {8.f, sume * 0.125f, 0.f};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float dt = ft[k] - vt8.mean, de = fe[k] - ve8.mean;
                vt8.m2 += dt * dt;
                ve8.m2 += de * de;
            }
            st = rs_merge(st, vt8);
            se = rs_merge(se, ve8);
        }
    } else {
        for (long i = lo + threadIdx.x; i < hi; i += 256) {
            const float ft = (float)t[i];
            const RsStat a = {1.f, ft, 0.f}, c = {1.f, rs_cfg((float)u[i], ft, g), 0.f};
            st = rs_merge(st, a);
            se = rs_merge(se, c);
        }
    }
    st = rs_wave_merge(st);
    se = rs_wave_merge(se);
    __shared__ RsStat sh[4][2];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave][0] = st; sh[wave][1] = se; }
    __syncthreads();
    if (threadIdx.x == 0) {
        RsStat* o = part + ((long)b * gridDim.x + p) * 2;
        o[0] = rs_merge(rs_merge(sh[0][0], sh[1][0]), rs_merge(sh[2][0], sh[3][0]));
        o[1] = rs_merge(rs_merge(sh[0][1], sh[1][1]), rs_merge(sh[2][1], sh[3][1]));
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void rs_apply_kernel(const half_t* __restrict__ eps2b, half_t* __restrict__ lat,
                                                       float* __restrict__ hist, const RsStat* __restrict__ part, int parts,
                                                       long n, long total, float g, float phi, float cx, float ce, float ch,
                                                       float hx, float he, float* __restrict__ factors) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    RsStat st = {0.f, 0.f, 0.f}, se = {0.f, 0.f, 0.f};
    if (lane < parts) {
        const RsStat* q = part + ((long)b * parts + lane) * 2;
        st = q[0];
        se = q[1];
    }
    st = rs_wave_merge(st);
    se = rs_wave_merge(se);
    // std(e) = 0 gives inf or nan, as the reference function does: no epsilon
    const float k = 1.f + phi * (sqrtf(st.m2 / se.m2) - 1.f);
    if (factors && blockIdx.x == 0 && threadIdx.x == 0) factors[b] = k;
    const long base = (long)b * n;
    const half_t* u = eps2b + base;
    const half_t* t = u + total;
    half_t* x = lat + base;
    float* h = hist ? hist + base : nullptr;
    if (VEC) {
        const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
        if (i >= n) return;
        const h8 vu = *reinterpret_cast<const h8*>(u + i);
        const h8 vt = *reinterpret_cast<const h8*>(t + i);
        const h8 vx = *reinterpret_cast<const h8*>(x + i);
        float hv[8], x0[8];
        if (h) {
            const f4 h0 = *reinterpret_cast<const f4*>(h + i), h1 = *reinterpret_cast<const f4*>(h + i + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { hv[j] = h0[j]; hv[j + 4] = h1[j]; }
        }
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = k * rs_cfg((float)vu[j], (float)vt[j], g);
            const float xf = (float)vx[j];
            float out = rs_axpby(cx, xf, ce, e);
            if (h) {
                out = __builtin_fmaf(ch, hv[j], out);
                x0[j] = rs_axpby(hx, xf, he, e);
            }
            o[j] = (half_t)out;
        }
        *reinterpret_cast<h8*>(x + i) = o;
        if (h) {
            f4 h0, h1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h0[j] = x0[j]; h1[j] = x0[j + 4]; }
            *reinterpret_cast<f4*>(h + i) = h0;
            *reinterpret_cast<f4*>(h + i + 4) = h1;
        }
    } else {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        const float e = k * rs_cfg((float)u[i], (float)t[i], g);
        const float xf = (float)x[i];
        float out = rs_axpby(cx, xf, ce, e);
        if (h) {
            out = __builtin_fmaf(ch, h[i], out);
            h[i] = rs_axpby(hx, xf, he, e);
        }
        x[i] = (half_t)out;
    }
}

// ---- perturbed-attention guidance (Ahn et al. 2024) in front of the same linear update ----
//   rows [u ; t ; p]: e = fp16(fma(s, t - p, fma(g, t - u, u)));  rows [t ; p]: e = fp16(fma(s, t - p, t))
// (fp32, one rounding to fp16; s == 0 skips the outer fma, so three rows at s = 0 give cfg_linear_kernel's e bit for bit
// whatever the signs of its zeros), then cfg_linear_kernel's update with its roundings (rs_axpby).  STEP = false writes e
// itself: the one-row model output the LCM / affine step entries then take.  VEC: n % 8 == 0 and 16-byte aligned bases.
// Guide::Ip2p is InstructPix2Pix's dual guidance (Brooks et al., eq. 3) through the same kernel: three rows [t ; i ; u]
// (text+image, image only, neither), e = fp16(fma(gi, i - u, fma(gt, t - i, u))) with (g, sp) = (gt, gi).  An element
// with i == u skips the outer fma (it would add an exact zero, of the wrong sign when the inner one gives -0), so rows
// [t ; u ; u] give cfg_linear_kernel's e on [u ; t] bit for bit.
enum class Guide { Pag2, Pag3, Ip2p };      // which formula, and with it how many rows of model_out are read
constexpr int guide_rows(Guide f) { return f == Guide::Pag2 ? 2 : 3; }
template <Guide F>
__device__ __forceinline__ float pag_eps(float a, float b, float c, float g, float sp) {
    if (F == Guide::Ip2p) {
        float e = __builtin_fmaf(g, a - b, c);
        if (b != c) e = __builtin_fmaf(sp, b - c, e);
        return (float)(half_t)e;
    }
    // Pag3: (a, b, c) = (u, t, p);  Pag2: (a, b) = (t, p)
    const float t = F == Guide::Pag3 ? b : a, p = F == Guide::Pag3 ? c : b;
    float e = F == Guide::Pag3 ? __builtin_fmaf(g, b - a, a) : a;
    if (sp != 0.f) e = __builtin_fmaf(sp, t - p, e);
    return (float)(half_t)e;
}
template <Guide F, bool VEC, bool STEP>
__global__ __launch_bounds__(256) void pag_step_kernel(const half_t* __restrict__ mo, half_t* __restrict__ x,
                                                       float* __restrict__ h, long n, float g, float sp, float cx, float ce,
                                                       float ch, float hx, float he) {
    if (VEC) {
        const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
        if (i >= n) return;
        const h8 va = *reinterpret_cast<const h8*>(mo + i);
        const h8 vb = *reinterpret_cast<const h8*>(mo + n + i);
        h8 vc = vb, vx = vb;
        if (guide_rows(F) == 3) vc = *reinterpret_cast<const h8*>(mo + 2 * n + i);
        if (STEP) vx = *reinterpret_cast<const h8*>(x + i);
        float hv[8], x0[8];
        if (STEP && h) {
            const f4 h0 = *reinterpret_cast<const f4*>(h + i), h1 = *reinterpret_cast<const f4*>(h + i + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { hv[j] = h0[j]; hv[j + 4] = h1[j]; }
        }
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = pag_eps<F>((float)va[j], (float)vb[j], (float)vc[j], g, sp);
            if (!STEP) { o[j] = (half_t)e; continue; }
            const float xf = (float)vx[j];
            float out = rs_axpby(cx, xf, ce, e);
            if (h) {
                out = __builtin_fmaf(ch, hv[j], out);
                x0[j] = rs_axpby(hx, xf, he, e);
            }
            o[j] = (half_t)out;
        }
        *reinterpret_cast<h8*>(x + i) = o;
        if (STEP && h) {
            f4 h0, h1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { h0[j] = x0[j]; h1[j] = x0[j + 4]; }
            *reinterpret_cast<f4*>(h + i) = h0;
            *reinterpret_cast<f4*>(h + i + 4) = h1;
        }
    } else {
        const long i = (long)blockIdx.x * 256 + threadIdx.x;
        if (i >= n) return;
        const float e = pag_eps<F>((float)mo[i], (float)mo[n + i], guide_rows(F) == 3 ? (float)mo[2 * n + i] : 0.f, g, sp);
        if (!STEP) { x[i] = (half_t)e; return; }
        const float xf = (float)x[i];
        float out = rs_axpby(cx, xf, ce, e);
        if (h) {
            out = __builtin_fmaf(ch, h[i], out);
            h[i] = rs_axpby(hx, xf, he, e);
        }
        x[i] = (half_t)out;
    }
}

// convert_pt_to_numpy (runpod-worker/handler_logic.py:21-29) on the device: the reference runs
// (x / 2 + 0.5).clamp(0, 1), permute to HWC, * 255, .to(uint8) on the fp16 image tensor, i.e. every
// step rounds to fp16 and the final cast truncates.  Same op order and roundings here, so the bytes
// match the reference's bit for bit.  One thread per output pixel (C <= 4 channels).
__global__ void image_to_uint8_kernel(const half_t* __restrict__ img, unsigned char* __restrict__ out, int C, long HW,
                                      long total_px) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_px) return;
    const long b = i / HW, px = i - b * HW;
    const half_t* src = img + b * C * HW + px;
    unsigned char* dst = out + i * C;
    for (int c = 0; c < C; ++c) {
        half_t v = src[(long)c * HW] * (half_t)0.5f;   // x / 2 (exact)
        v = v + (half_t)0.5f;
        v = v < (half_t)0.f ? (half_t)0.f : (v > (half_t)1.f ? (half_t)1.f : v);
        v = v * (half_t)255.f;
        dst[c] = (unsigned char)(int)(float)v;
    }
}

// CLIPTextEmbeddings (transformers modeling_clip.py): token + learned position embedding.
__global__ void clip_embed_kernel(const int* __restrict__ ids, const half_t* __restrict__ tok,
                                  const half_t* __restrict__ pos, half_t* __restrict__ out, long rows, int T, int H8,
                                  int vocab) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * H8) return;
    const long r = i / H8;
    const int c = (int)(i - r * H8) * 8;
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const int t = (int)(r % T);
    const h8 a = *reinterpret_cast<const h8*>(tok + (long)id * H8 * 8 + c);
    const h8 b = *reinterpret_cast<const h8*>(pos + (long)t * H8 * 8 + c);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)a[e] + (float)b[e]);
    *reinterpret_cast<h8*>(out + r * H8 * 8 + c) = o;
}
__global__ void gather_rows_kernel(const half_t* __restrict__ x, long ldx, const int* __restrict__ idx,
                                   half_t* __restrict__ out16, float* __restrict__ out32, int B, int T, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * H) return;
    const int b = (int)(i / H), c = (int)(i - (long)b * H);
    int t = idx[b];
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    const half_t v = x[((long)b * T + t) * ldx + c];
    if (out16) out16[i] = v;
    if (out32) out32[i] = (float)v;
}

// Inpainting with a 4-channel UNet (sd_unified_pipeline.py:492-506): outside the mask the latents are
// reset to the (re-noised) original image latents after every step.
//   x <- m x + (1 - m) (a img + b noise),  m = mask[b, 0, h, w] broadcast over channels
__global__ void inpaint_blend_kernel(half_t* __restrict__ lat, const half_t* __restrict__ img,
                                     const half_t* __restrict__ noise, const half_t* __restrict__ mask, float a,
                                     float b, int C, long HW, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long bc = i / HW, px = i - bc * HW;
    const float m = (float)mask[(bc / C) * HW + px];
    float keep = a * (float)img[i];
    if (noise) keep += b * (float)noise[i];
    lat[i] = (half_t)(m * (float)lat[i] + (1.f - m) * keep);
}

__global__ void scale_f16_kernel(half_t* __restrict__ x, long n, float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = (half_t)((float)x[i] * scale);
}

// Pack-time LayerNorm fold (launch_ln_fold): one wave per weight row.
__global__ __launch_bounds__(256) void ln_fold_kernel(half_t* __restrict__ w, long K, int rows,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ bias_in, float* __restrict__ bias,
                                                      float* __restrict__ wsum, int rows_scaled, float row_scale) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= rows) return;
    const float sc = n < rows_scaled ? row_scale : 1.0f;
    half_t* row = w + (long)n * K;
    float ws = 0.f, wb = 0.f;
    for (long k = lane; k < K; k += 64) {
        const float old = (float)row[k];
        const half_t nw = (half_t)(old * gamma[k] * sc);
        row[k] = nw;
        ws += (float)nw;
        wb += old * beta[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ws += __shfl_xor(ws, off); wb += __shfl_xor(wb, off); }
    if (lane == 0) {
        wsum[n] = ws;
        bias[n] = sc * ((bias_in ? bias_in[n] : 0.f) + wb);
    }
}


// Pack-time fold of an outer linear over an inner one (launch_fold_linear), one thread per output element:
// wp[n][k] = fp16(sum_j wo[n][j] wi[j][k]) for k < K, wo[n][k - K] for K <= k < K + J.  A product of two fp16 values is
// exact in fp32 and the sum is compensated (Kahan), so the one rounding to fp16 is the only error of note.
__global__ __launch_bounds__(256) void fold_linear_kernel(const half_t* __restrict__ wo, const half_t* __restrict__ wi,
                                                          half_t* __restrict__ wp, int J, int K, long Kp) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = blockIdx.y;
    if (k >= (long)K + J) return;
    if (k >= K) { wp[n * Kp + k] = wo[n * J + (k - K)]; return; }
    float s = 0.f, c = 0.f;
    for (int j = 0; j < J; ++j) {
        const float y = fmaf((float)wo[n * J + j], (float)wi[(long)j * K + k], -c);
        const float t = s + y;
        c = (t - s) - y;
        s = t;
    }
    wp[n * Kp + k] = (half_t)s;
}

// ---------------------------------------------------------------------------------------------------
// conv_out: 3x3 / stride 1 / pad 1 convolution to a handful of output channels (UNet 320 -> 4, VAE decoder
// 128 -> 3; diffusers `conv_out` under sd_unified_pipeline.py:475-482 / :523), NHWC f16 in, NCHW f16 out.
// HBM-bound (the input is read once: 268 MB for the 512 px VAE batch), not a matrix-core shape: a 16-column
// MFMA tile would still waste 4-5x and the generic 64-column tile ran it at 21 TF/s / 0.79 TB/s (0.33 ms).
// One thread = two neighbouring output pixels, all COUT channels; a block's 8 x 64 pixels share a
// (10 x 66)-pixel halo tile of 32 input channels in LDS (pixel stride 80 B: conflict-free ds_read_b128 across
// consecutive pixels); the slab's weights sit in LDS too and are read as broadcasts (a first version fed
// them as scalar loads / SGPR operands: 140 exposed scalar-cache waits per slab made it slower than the
// tile it replaced); v_dot2_f32_f16 with fp32 accumulation; the result goes straight out channel-major
// (coalesced along W), so no NHWC -> NCHW pass follows.
// Weights: the packed layout of pack_conv_kernel, K order [Cin/64][kh][kw][64].
// ---------------------------------------------------------------------------------------------------
constexpr int CO_TH = 8, CO_TW = 64;                      // output tile (rows x cols) per 256-thread block: 2 pixels per thread
constexpr int CO_CS = 32;                                 // input channels per LDS slab
constexpr int CO_PSTR = CO_CS + 8;                        // halo pixel stride in halves (80 B: conflict-free b128 reads)
template <int COUT>
__global__ __launch_bounds__(256) void conv3x3_small_cout_kernel(const half_t* __restrict__ x, long ldx,
                                                                 const half_t* __restrict__ w, long K,
                                                                 const float* __restrict__ bias,
                                                                 half_t* __restrict__ y, int N, int H, int W, int Cin,
                                                                 int cout_real) {
    constexpr int HP = (CO_TH + 2) * (CO_TW + 2);
    __shared__ __attribute__((aligned(16))) half_t halo[HP * CO_PSTR];
    __shared__ __attribute__((aligned(16))) half_t wl[9 * (CO_CS / 8) * COUT * 8];      // [tap][chunk][co][8]
    const int tid = threadIdx.x;
    const int tiles_w = (W + CO_TW - 1) / CO_TW, tiles_h = (H + CO_TH - 1) / CO_TH;
    int b = blockIdx.x;
    const int tw = b % tiles_w; b /= tiles_w;
    const int th = b % tiles_h;
    const int n = b / tiles_h;
    const int oh0 = th * CO_TH, ow0 = tw * CO_TW;
    const int lr = tid / (CO_TW / 2), lc = (tid % (CO_TW / 2)) * 2;     // this thread's two pixels: (lr, lc), (lr, lc + 1)
    float acc[2][COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) { acc[0][co] = 0.f; acc[1][co] = 0.f; }
    const half_t* xn = x + (long)n * H * W * ldx;
    for (int c0 = 0; c0 < Cin; c0 += CO_CS) {
        __syncthreads();                                  // previous slab fully consumed
        for (int i = tid; i < HP * (CO_CS / 8); i += 256) {       // halo pixel, 16-byte chunk
            const int hp = i / (CO_CS / 8), ch = i % (CO_CS / 8);
            const int hr = hp / (CO_TW + 2), hc = hp - hr * (CO_TW + 2);
            const int ih = oh0 - 1 + hr, iw = ow0 - 1 + hc;
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                v = *reinterpret_cast<const h8*>(xn + ((long)ih * W + iw) * ldx + c0 + ch * 8);
            *reinterpret_cast<h8*>(halo + hp * CO_PSTR + ch * 8) = v;
        }
        // the slab's weights, packed K order [Cin / 64][tap][64]: this slab is the (c0 % 64)-th half of a 64-group
        for (int i = tid; i < 9 * (CO_CS / 8) * COUT; i += 256) {
            const int co = i % COUT, ch = (i / COUT) % (CO_CS / 8), tap = i / (COUT * (CO_CS / 8));
            *reinterpret_cast<h8*>(wl + i * 8) =
                *reinterpret_cast<const h8*>(w + (long)co * K + ((long)(c0 / 64) * 9 + tap) * 64 + (c0 % 64) + ch * 8);
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const half_t* px = halo + ((lr + tap / 3) * (CO_TW + 2) + lc + tap % 3) * CO_PSTR;
#pragma unroll
            for (int ch = 0; ch < CO_CS / 8; ++ch) {
                const h8 x0 = *reinterpret_cast<const h8*>(px + ch * 8);
                const h8 x1 = *reinterpret_cast<const h8*>(px + CO_PSTR + ch * 8);
#pragma unroll
                for (int co = 0; co < COUT; ++co) {
                    const h8 wv = *reinterpret_cast<const h8*>(wl + ((tap * (CO_CS / 8) + ch) * COUT + co) * 8);   // LDS broadcast
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const h2 wp = {wv[2 * e], wv[2 * e + 1]};
                        acc[0][co] = __builtin_amdgcn_fdot2(h2{x0[2 * e], x0[2 * e + 1]}, wp, acc[0][co], false);
                        acc[1][co] = __builtin_amdgcn_fdot2(h2{x1[2 * e], x1[2 * e + 1]}, wp, acc[1][co], false);
                    }
                }
            }
        }
    }
    const int oh = oh0 + lr;
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
        const int ow = ow0 + lc + p2;
        if (oh < H && ow < W) {
#pragma unroll
            for (int co = 0; co < COUT; ++co)
                if (co < cout_real)
                    y[(((long)n * cout_real + co) * H + oh) * W + ow] = (half_t)(acc[p2][co] + (bias ? bias[co] : 0.f));
        }
    }
}

inline dim3 grid1d(long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

}  // namespace

int launch_timestep_sinusoid(const float* t, int t_stride, float* out, int count, int dim, int flip, float shift,
                             long out_ld, hipStream_t s) {
    hipLaunchKernelGGL(sinusoid_kernel, grid1d((long)count * (dim / 2)), dim3(256), 0, s, t, t_stride, out, count,
                       dim, flip, shift, out_ld);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_text_time_input(const half_t* text, const float* ids, float* out, int B, int P, int ad, int n, int flip,
                           float shift, int out_ld, hipStream_t s) {
    if (out_ld < P + n * ad) { set_error("text_time_input: out_ld < P + n * ad"); return 1; }
    const long units = (long)B * (P + n * (ad / 2) + (out_ld - (P + n * ad)));
    if (units <= 0) return 0;
    hipLaunchKernelGGL(text_time_input_kernel, grid1d(units), dim3(256), 0, s, text, ids, out, B, P, ad, n, flip, shift,
                       out_ld);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_timestep_cond(const float* t, const float* cond, const half_t* w, long ldw, float* out, int count, int dim,
                         int cond_dim, int flip, float shift, hipStream_t s) {
    const long waves = (long)count * (dim / 2);
    if (waves <= 0) return 0;
    const bool vec = ldw % 8 == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (vec)
        hipLaunchKernelGGL(temb_cond_kernel<true>, grid, dim3(256), 0, s, t, cond, w, ldw, out, count, dim, cond_dim, flip, shift);
    else
        hipLaunchKernelGGL(temb_cond_kernel<false>, grid, dim3(256), 0, s, t, cond, w, ldw, out, count, dim, cond_dim, flip, shift);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

// The same operator on the matrix cores, for the shapes of the time-embedding path (B <= 16 rows, K <= 1280):
// small_linear_kernel re-reads the activation rows through L1 once per wave and column group -- four times the bytes
// of the weights it streams -- and reduces every output over the 64 lanes with shuffles: 26 us per launch on average,
// 66 us for the stacked time_emb_proj matrix (51.6 MB: 0.8 TB/s).  Here
//   * a 16-column tile of W is the MFMA's first operand, fetched straight from global memory as fragments (lane = one
//     row, 16 bytes of it), the activations are the second operand and stay in REGISTERS for the whole launch: the four
//     waves of a block split K (32-wide steps dealt round-robin), each keeps its <= 10 steps of x;
//   * x is fp32 and must stay so (it is the fp32 path of the reference's fp16 Linear only in the products' rounding):
//     it is split as hi + lo, two fp16 fragments and two MFMAs per weight fragment -- the matrix pipe is idle anyway;
//   * the reduction over K is the MFMA's, the reduction over the four waves goes through 4 KB of LDS (double-buffered,
//     one barrier per tile), where bias and SiLU are applied; the next tile's weight fragments are in flight meanwhile.
constexpr int SK_MAXKS = 10;          // 32-wide K steps per wave: K <= 4 * 10 * 32 = 1280
__global__ __launch_bounds__(256) void skinny_linear_kernel(const float* __restrict__ x, long ldx, const half_t* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, long ldy,
                                                            int B, int K, int Nout, int silu_in, int silu_out) {
    __shared__ float red[2][4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int KS = K / 32;
    const int tiles = Nout / 16;
    // ---- this wave's K steps of x as (hi, lo) fp16 fragments: lane = (row fr, 8 values at fq) ----
    h8 xh[SK_MAXKS], xl[SK_MAXKS];
#pragma unroll
    for (int j = 0; j < SK_MAXKS; ++j) {
        const int ks = wave + 4 * j;
        h8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ks < KS && fr < B) {
            const float* xr = x + (long)fr * ldx + ks * 32 + fq * 8;
            const f4 a = *reinterpret_cast<const f4*>(xr), b = *reinterpret_cast<const f4*>(xr + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = e < 4 ? a[e] : b[e - 4];
                if (silu_in) v = silu_f(v);
                hi[e] = (half_t)v;
                lo[e] = (half_t)(v - (float)hi[e]);
            }
        }
        xh[j] = hi; xl[j] = lo;
    }
    auto fetch = [&](int t, h8* wf) {
        // (unconditional loads on a clamped tile / step: see gn_apply2_kernel)
        const int tt = t < tiles ? t : tiles - 1;
        const half_t* wr = w + ((long)tt * 16 + fr) * K + fq * 8;
#pragma unroll
        for (int j = 0; j < SK_MAXKS; ++j) {
            const int ks = wave + 4 * j;
            wf[j] = *reinterpret_cast<const h8*>(wr + (ks < KS ? ks : KS - 1) * 32);
        }
    };
    h8 wcur[SK_MAXKS], wnext[SK_MAXKS];
    int t = blockIdx.x;
    fetch(t, wcur);
    int par = 0;
    for (; t < tiles; t += gridDim.x, par ^= 1) {
        fetch(t + gridDim.x, wnext);
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < SK_MAXKS; ++j) {
            if (wave + 4 * j < KS) {                          // wave-uniform
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wcur[j], xh[j], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wcur[j], xl[j], acc, 0, 0, 0);
            }
        }
        // acc: batch row fr, columns fq * 4 + e of the tile
#pragma unroll
        for (int e = 0; e < 4; ++e) red[par][wave][(fq * 4 + e) * 16 + fr] = acc[e];
        __syncthreads();
        {
            const int col = tid >> 4, row = tid & 15;
            if (row < B) {
                float v = red[par][0][tid] + red[par][1][tid] + red[par][2][tid] + red[par][3][tid];
                v += bias ? bias[t * 16 + col] : 0.f;
                if (silu_out) v = silu_f(v);
                y[(long)row * ldy + t * 16 + col] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < SK_MAXKS; ++j) wcur[j] = wnext[j];
    }
}

int small_linear_plan(int B, int K, int Nout) {
    static const bool no_skinny = getenv("SD_NO_SKINNY_LINEAR") != nullptr;
    if (K % 8 != 0) return -1;
    return !no_skinny && B <= 16 && K % 32 == 0 && K <= 4 * SK_MAXKS * 32 && Nout % 16 == 0 ? 1 : 0;
}

int launch_small_linear(const float* x, long ldx, const half_t* w, const float* bias, float* y, long ldy,
                        int B, int K, int Nout, int silu_in, int silu_out, hipStream_t s) {
    const int plan = small_linear_plan(B, K, Nout);
    if (plan < 0 || ldx % 4 != 0) { set_error("small_linear: K%8, ldx%4"); return 1; }
    if (plan == 1) {
        const int tiles = Nout / 16;
        hipLaunchKernelGGL(skinny_linear_kernel, dim3(tiles < 512 ? tiles : 512), dim3(256), 0, s, x, ldx, w, bias, y, ldy, B, K, Nout,
                           silu_in, silu_out);
        SD_HIP_CHECK(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(small_linear_kernel, dim3(cdiv(Nout, 4 * SL_COLS)), dim3(256), 0, s, x, ldx, w, bias, y, ldy, B, K,
                       Nout, silu_in, silu_out);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_add_f32(float* y, const float* x, long n, int silu, hipStream_t s) {
    hipLaunchKernelGGL(add_f32_kernel, grid1d(n), dim3(256), 0, s, y, x, n, silu);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_f16_to_f32(const half_t* x, float* y, long n, hipStream_t s) {
    hipLaunchKernelGGL(f16_to_f32_kernel, grid1d(n), dim3(256), 0, s, x, y, n);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_f32_to_f16(const float* x, half_t* y, long n, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_f16_kernel, grid1d(n), dim3(256), 0, s, x, y, n);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_im2col_nchw3x3(const half_t* x, half_t* col, int N, int C, int H, int W, int Kpad, hipStream_t s) {
    hipLaunchKernelGGL(im2col_nchw3x3_kernel, grid1d((long)N * H * W * Kpad), dim3(256), 0, s, x, col, N, C, H,
                       W, Kpad);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_nhwc_to_nchw(const half_t* x, long ldx, half_t* y, int N, long HW, int C, hipStream_t s) {
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid1d((long)N * C * HW), dim3(256), 0, s, x, ldx, y, N, HW, C);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_nchw_to_nhwc(const half_t* x, half_t* y, long ldy, int N, long HW, int C, hipStream_t s) {
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid1d((long)N * C * HW), dim3(256), 0, s, x, y, ldy, N, HW, C);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_pointwise_nchw(const half_t* x, const half_t* w, const float* bias, half_t* y, int N, int Cin,
                          int Cout, long HW, hipStream_t s) {
    hipLaunchKernelGGL(pointwise_nchw_kernel, grid1d((long)N * Cout * HW), dim3(256), 0, s, x, w, bias, y, N,
                       Cin, Cout, HW);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_conv3x3_small_cout(const half_t* x, long ldx, const half_t* w, long K, const float* bias, half_t* y_nchw,
                              int N, int H, int W, int Cin, int Cout, hipStream_t s) {
    if (Cout < 1 || Cout > 4 || Cin % 64 != 0 || K != 9L * Cin) { set_error("conv3x3_small_cout: Cout in 1..4, Cin % 64 == 0"); return 1; }
    const long tiles = (long)N * ((H + CO_TH - 1) / CO_TH) * ((W + CO_TW - 1) / CO_TW);
    if (tiles == 0) return 0;
    hipLaunchKernelGGL(conv3x3_small_cout_kernel<4>, dim3((unsigned)tiles), dim3(256), 0, s, x, ldx, w, K, bias, y_nchw, N, H, W,
                       Cin, Cout);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_pack_conv(const half_t* w, half_t* wp, int O, int I, int KH, int KW, long Kpad, hipStream_t s) {
    hipLaunchKernelGGL(pack_conv_kernel, grid1d((long)O * Kpad), dim3(256), 0, s, w, wp, O, I, KH, KW, Kpad);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_fold_upconv(const half_t* w, half_t* wp, int O, int I, hipStream_t s) {
    if (O < 1 || I < 64 || I % 64 != 0) { set_error("fold_upconv: Cin must be a multiple of 64"); return 1; }
    const long rows = ((long)O + kWeightRowPad - 1) / kWeightRowPad * kWeightRowPad;
    hipLaunchKernelGGL(fold_upconv_kernel, grid1d(16L * O * I), dim3(256), 0, s, w, wp, O, I, rows);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_cfg_duplicate(const half_t* lat, half_t* out, long n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(cfg_duplicate_kernel, grid1d(n), dim3(256), 0, s, lat, out, n, scale);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_row_dup(const RowDupSeg* segs, int count, hipStream_t s) {
    if (count < 0 || count > kRowDupMax) { set_error("row_dup: too many segments"); return 1; }
    RowDupDev p;
    int blocks = 0, k = 0;
    for (int i = 0; i < count; ++i) {
        const RowDupSeg& g = segs[i];
        if (g.rows <= 0 || g.row_bytes <= 0) continue;
        if (((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst) | (uintptr_t)g.ld_bytes |
              (uintptr_t)g.row_bytes) & 15) != 0 || g.row_bytes > g.ld_bytes) {
            set_error("row_dup: segments must be 16-byte aligned with row_bytes <= ld_bytes");
            return 1;
        }
        p.src[k] = static_cast<const uint4*>(g.src);
        p.dst[k] = static_cast<uint4*>(g.dst);
        p.ld16[k] = g.ld_bytes / 16;
        p.w16[k] = g.row_bytes / 16;
        p.units[k] = g.rows * p.w16[k];
        p.first[k] = blocks;
        const long nb = (p.units[k] + RD_UNITS - 1) / RD_UNITS;
        if (nb + blocks > 0x7fffffffL) { set_error("row_dup: too large"); return 1; }
        blocks += (int)nb;
        ++k;
    }
    if (k == 0) return 0;
    p.first[k] = blocks;
    p.count = k;
    hipLaunchKernelGGL(row_dup_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_scale_copy_f16(const half_t* x, half_t* out, long n, float scale, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(scale_copy_f16_kernel, grid1d(n), dim3(256), 0, s, x, out, n, scale);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_concat_sample(const half_t* a, int Na, int Ca, float in_scale, const half_t* b, int Nb, int Cb, int zero_from,
                         half_t* out, int N, long HW, hipStream_t s) {
    const long total = (long)N * (Ca + Cb) * HW;
    if (total <= 0) return 0;
    if (Na < 1 || Nb < 1 || Ca < 0 || Cb < 0) { set_error("concat_sample: bad arguments"); return 1; }
    hipLaunchKernelGGL(concat_sample_kernel, grid1d(total), dim3(256), 0, s, a, Na, Ca, in_scale, b, Nb, Cb, zero_from, out, total, HW);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_dup_f32(const float* x, float* out, long n, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(dup_f32_kernel, grid1d(n), dim3(256), 0, s, x, out, n);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
// What the VEC kernels ask of a launch: n % 8 == 0 and every base (a null one passes) 16-byte aligned.
static bool vec8_ok(long n, const void* a, const void* b, const void* c, const void* d = nullptr) {
    return n % 8 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}
int launch_cfg_linear(const half_t* eps2b, half_t* lat, float* hist, long n, float g, float cx, float ce, float ch,
                      float hx, float he, hipStream_t s) {
    hipLaunchKernelGGL(cfg_linear_kernel, grid1d(n), dim3(256), 0, s, eps2b, lat, hist, n, g, cx, ce, ch, hx, he);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_lcm_step(const half_t* model_out, int rows, half_t* lat, const half_t* noise, half_t* denoised, long n, float g,
                    float dx, float dout, float pden, float pnoise, hipStream_t s) {
    const bool vec = vec8_ok(n, model_out, lat, noise, denoised);
    const dim3 grid = grid1d(vec ? n / 8 : n);
#define SD_LCM_LAUNCH(R, V) \
    hipLaunchKernelGGL((lcm_step_kernel<R, V>), grid, dim3(256), 0, s, model_out, lat, noise, denoised, n, g, dx, dout, pden, pnoise)
    if (rows == 2) { if (vec) SD_LCM_LAUNCH(2, true); else SD_LCM_LAUNCH(2, false); }
    else { if (vec) SD_LCM_LAUNCH(1, true); else SD_LCM_LAUNCH(1, false); }
#undef SD_LCM_LAUNCH
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
template <bool STEP>
static int launch_pag_step(const half_t* mo, Guide form, half_t* x, float* hist, long n, float g, float sp, float cx, float ce,
                           float ch, float hx, float he, hipStream_t s) {
    const bool vec = vec8_ok(n, mo, x, hist);
    const dim3 grid = grid1d(vec ? n / 8 : n);
#define SD_PAG_LAUNCH(R, V) \
    hipLaunchKernelGGL((pag_step_kernel<R, V, STEP>), grid, dim3(256), 0, s, mo, x, hist, n, g, sp, cx, ce, ch, hx, he)
    if (form == Guide::Ip2p) { if (vec) SD_PAG_LAUNCH(Guide::Ip2p, true); else SD_PAG_LAUNCH(Guide::Ip2p, false); }
    else if (form == Guide::Pag3) { if (vec) SD_PAG_LAUNCH(Guide::Pag3, true); else SD_PAG_LAUNCH(Guide::Pag3, false); }
    else { if (vec) SD_PAG_LAUNCH(Guide::Pag2, true); else SD_PAG_LAUNCH(Guide::Pag2, false); }
#undef SD_PAG_LAUNCH
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_pag_linear(const half_t* model_out, int rows, half_t* lat, float* hist, long n, float g, float sp, float cx,
                      float ce, float ch, float hx, float he, hipStream_t s) {
    if (rows != 2 && rows != 3) { set_error("pag_linear: rows must be 2 or 3"); return 1; }
    return launch_pag_step<true>(model_out, rows == 3 ? Guide::Pag3 : Guide::Pag2, lat, hist, n, g, sp, cx, ce, ch, hx, he, s);
}
int launch_pag_combine(const half_t* model_out, int rows, half_t* out, long n, float g, float sp, hipStream_t s) {
    if (rows != 2 && rows != 3) { set_error("pag_combine: rows must be 2 or 3"); return 1; }
    return launch_pag_step<false>(model_out, rows == 3 ? Guide::Pag3 : Guide::Pag2, out, nullptr, n, g, sp, 0.f, 0.f, 0.f, 0.f, 0.f, s);
}
int launch_ip2p_linear(const half_t* model_out, half_t* lat, float* hist, long n, float gt, float gi, float cx, float ce,
                       float ch, float hx, float he, hipStream_t s) {
    return launch_pag_step<true>(model_out, Guide::Ip2p, lat, hist, n, gt, gi, cx, ce, ch, hx, he, s);
}
int launch_ip2p_combine(const half_t* model_out, half_t* out, long n, float gt, float gi, hipStream_t s) {
    return launch_pag_step<false>(model_out, Guide::Ip2p, out, nullptr, n, gt, gi, 0.f, 0.f, 0.f, 0.f, 0.f, s);
}
int launch_sched_affine_step(const half_t* model_out, int rows, half_t* lat, const half_t* noise, float* bank, long stride,
                             long n, float g, const StepRows& p, hipStream_t s) {
    unsigned use = 0;                                       // columns that some row reads
    for (int k = 0; k < STEP_COLS; ++k) {
        bool any = p.out[k] != 0.0;
        for (int w = 0; w < p.n_writes; ++w) any = any || p.write[w][k] != 0.0;
        if (any) use |= 1u << k;
    }
    const bool vec = stride % 4 == 0 && vec8_ok(n, model_out, lat, noise, bank);
    const dim3 grid = grid1d(vec ? n / 8 : n);
#define SD_STEP_LAUNCH(R, V) \
    hipLaunchKernelGGL((sched_affine_kernel<R, V>), grid, dim3(256), 0, s, model_out, lat, noise, bank, stride, n, g, p, use)
    if (rows == 2) { if (vec) SD_STEP_LAUNCH(2, true); else SD_STEP_LAUNCH(2, false); }
    else { if (vec) SD_STEP_LAUNCH(1, true); else SD_STEP_LAUNCH(1, false); }
#undef SD_STEP_LAUNCH
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
// Chunk summaries of launch_cfg_rescale_linear: one grow-only buffer per (device, stream), so that calls on different
// streams never share one and calls on one stream are ordered by it.  Allocated on the first call for a stream (or when
// B grows); a steady loop allocates nothing and never synchronises.
static RsStat* rs_workspace(int B, hipStream_t s) {
    struct Buf { RsStat* p = nullptr; int B = 0; };
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Buf> bufs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    Buf& b = bufs[{dev, s}];
    if (b.B < B) {
        if (b.p) (void)hipFree(b.p);          // waits for the device: nothing queued still reads it
        b.p = nullptr;
        b.B = 0;
        if (hipMalloc(reinterpret_cast<void**>(&b.p), (size_t)B * RS_MAX_PARTS * 2 * sizeof(RsStat)) != hipSuccess) {
            b.p = nullptr;
            return nullptr;
        }
        b.B = B;
    }
    return b.p;
}
int launch_cfg_rescale_linear(const half_t* eps2b, half_t* lat, float* hist, int B, long n, float g, float phi, float cx,
                              float ce, float ch, float hx, float he, float* factors, hipStream_t s) {
    RsStat* part = rs_workspace(B, s);
    if (!part) { set_error("cfg_rescale_linear: no device memory for the chunk summaries"); return 1; }
    const long total = (long)B * n;
    const bool vec = vec8_ok(n, eps2b, lat, hist);
    long parts = (n + RS_MIN_CHUNK - 1) / RS_MIN_CHUNK;
    if (parts > RS_MAX_PARTS) parts = RS_MAX_PARTS;
    long chunk = (n + parts - 1) / parts;
    chunk = (chunk + 7) / 8 * 8;
    parts = (n + chunk - 1) / chunk;
    const long per_block = vec ? 256 * 8 : 256;
    const long blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffL) { set_error("cfg_rescale_linear: sample too large"); return 1; }
    const dim3 gs((unsigned)parts, (unsigned)B), ga((unsigned)blocks, (unsigned)B);
    if (vec) {
        hipLaunchKernelGGL(rs_stats_kernel<true>, gs, dim3(256), 0, s, eps2b, part, n, chunk, total, g);
        hipLaunchKernelGGL(rs_apply_kernel<true>, ga, dim3(256), 0, s, eps2b, lat, hist, part, (int)parts, n, total, g, phi, cx,
                           ce, ch, hx, he, factors);
    } else {
        hipLaunchKernelGGL(rs_stats_kernel<false>, gs, dim3(256), 0, s, eps2b, part, n, chunk, total, g);
        hipLaunchKernelGGL(rs_apply_kernel<false>, ga, dim3(256), 0, s, eps2b, lat, hist, part, (int)parts, n, total, g, phi, cx,
                           ce, ch, hx, he, factors);
    }
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_clip_embed(const int* ids, const half_t* tok, const half_t* pos, half_t* out, int B, int T, int H, int vocab,
                      hipStream_t s) {
    if (H % 8 != 0) { set_error("clip_embed: hidden size must be a multiple of 8"); return 1; }
    const long n = (long)B * T * (H / 8);
    hipLaunchKernelGGL(clip_embed_kernel, grid1d(n), dim3(256), 0, s, ids, tok, pos, out, (long)B * T, T, H / 8, vocab);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_gather_rows(const half_t* x, long ldx, const int* idx, half_t* out16, float* out32, int B, int T, int H,
                       hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, grid1d((long)B * H), dim3(256), 0, s, x, ldx, idx, out16, out32, B, T, H);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_inpaint_blend(half_t* lat, const half_t* img, const half_t* noise, const half_t* mask, float a, float b, int B,
                         int C, long HW, hipStream_t s) {
    const long n = (long)B * C * HW;
    if (n == 0) return 0;
    hipLaunchKernelGGL(inpaint_blend_kernel, grid1d(n), dim3(256), 0, s, lat, img, noise, mask, a, b, C, HW, n);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_ln_fold(half_t* w, long K, int rows, const float* gamma, const float* beta, const float* bias_in,
                   float* bias, float* wsum, int rows_scaled, float row_scale, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(ln_fold_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w, K, rows, gamma, beta, bias_in, bias, wsum,
                       rows_scaled, row_scale);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_fold_linear(const half_t* wo, const half_t* wi, half_t* wp, int O, int J, int K, long Kp, hipStream_t s) {
    if (O <= 0 || J <= 0 || K <= 0 || O > 65535 || Kp < (long)K + J) { set_error("fold_linear: bad shape"); return 1; }
    hipLaunchKernelGGL(fold_linear_kernel, dim3((unsigned)((K + J + 255) / 256), (unsigned)O), dim3(256), 0, s, wo, wi, wp, J, K, Kp);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_scale_f16(half_t* x, long n, float scale, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(scale_f16_kernel, grid1d(n), dim3(256), 0, s, x, n, scale);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}
int launch_image_to_uint8(const half_t* img, unsigned char* out, int B, int C, long HW, hipStream_t s) {
    const long total = (long)B * HW;
    if (total == 0) return 0;
    hipLaunchKernelGGL(image_to_uint8_kernel, grid1d(total), dim3(256), 0, s, img, out, C, HW, total);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
