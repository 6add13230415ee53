// FreeU (diffusers 0.27.2 apply_freeu / fourier_filter) as one in-place launch on a concatenation view [hidden | skip].
//
//   hidden[:, :C1 / 2] *= b                                   (backbone)
//   skip = ifftn(ifftshift(mask * fftshift(fftn(skip)))).real (mask = s on the 2 x 2 centre box, 1 elsewhere)
//
// The box holds the frequencies {-1, 0} of each axis, so the filter is x plus a rank-limited correction:
//   y[h,w] = x[h,w] + (s-1)/(H W) sum_{h',w'} x[h',w'] [(1 + cos t)(1 + cos f) - sin t sin f],  t = 2 pi (h-h')/H, f = 2 pi (w-w')/W
// With a = 2 pi h / H, b = 2 pi w / W and d = cos a cos b - sin a sin b, e = cos a sin b + sin a cos b the bracket
// separates into seven products of a factor of (h,w) and a factor of (h',w'):
//   1 + cos a cos a' + sin a sin a' + cos b cos b' + sin b sin b' + d d' + e e'
// so every (image, channel) plane needs seven fp32 moments sum x' {1, cos a', sin a', cos b', sin b', d', e'} and the
// apply is x + k (m0 + cos a m1 + sin a m2 + cos b m3 + sin b m4 + d m5 + e m6): a reduction and an apply, no transform.
// An axis of length 1 has its only frequency inside the box: its factor is 1, which cos = sin = 0 for that axis gives.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace sd {
namespace {

constexpr int kFreeuThreads = 256;
constexpr int kFreeuMoments = 7;
constexpr size_t kFreeuLdsMax = 72 * 1024;      // two blocks per CU; a 64 x 64 plane of 8 channels (64 KB) still fits
constexpr int kFreeuTargetBlocks = 512;         // two per CU before the channel group narrows

struct FreeuParams {
    half_t* x;          // [N, H W, ld]: hidden = columns [0, C1), skip = [C1, C1 + C2)
    long ld;
    int N, H, W, HW, C1, C2;
    float b, k;         // backbone factor, (s - 1) / (H W)
    int gvec;           // channel vectors per block (power of two, divides 64)
    int groups;         // channel groups per image = ceil(C2 / VEC / gvec)
    int skip_blocks;    // N * groups; the blocks after them scale the backbone channels
    int in_lds;         // 1: the block's plane stays in LDS between the reduction and the apply
    int plane_off;      // byte offset of that plane in dynamic LDS
};

template <int VEC>
__device__ __forceinline__ void freeu_load(const half_t* p, float (&v)[VEC]) {
    if constexpr (VEC == 8) {
        const h8 r = *reinterpret_cast<const h8*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)r[e];
    } else {
        v[0] = (float)p[0];
    }
}
template <int VEC>
__device__ __forceinline__ void freeu_store(half_t* p, const float (&v)[VEC]) {
    if constexpr (VEC == 8) {
        h8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)v[e];
        *reinterpret_cast<h8*>(p) = r;
    } else {
        p[0] = (half_t)v[0];
    }
}

// VEC = 8: 16-byte accesses (base, ld, C1 / 2 and C2 all multiples of 8 halves); VEC = 1: any even C1, any C2.
template <int VEC>
__global__ __launch_bounds__(kFreeuThreads) void freeu_kernel(FreeuParams p) {
    extern __shared__ __align__(16) unsigned char freeu_smem[];
    const int tid = threadIdx.x;

    if ((int)blockIdx.x >= p.skip_blocks) {
        // ---- backbone: hidden[:, :C1 / 2] *= b, grid-stride over [N H W][C1 / 2 / VEC] ----
        const int nv = (p.C1 / 2) / VEC;
        const long total = (long)p.N * p.HW * nv;
        const long stride = (long)((int)gridDim.x - p.skip_blocks) * kFreeuThreads;
        for (long i = (long)((int)blockIdx.x - p.skip_blocks) * kFreeuThreads + tid; i < total; i += stride) {
            const long row = i / nv;
            const int v = (int)(i - row * nv);
            half_t* q = p.x + row * p.ld + v * VEC;
            float x[VEC];
            freeu_load<VEC>(q, x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) x[e] *= p.b;
            freeu_store<VEC>(q, x);
        }
        return;
    }

    // ---- skip: one (image, channel group) per block ----
    float* cosH = reinterpret_cast<float*>(freeu_smem);
    float* sinH = cosH + p.H;
    float* cosW = sinH + p.H;
    float* sinW = cosW + p.W;
    float* red = sinW + p.W;                                   // [4 waves][gvec][7][VEC]
    half_t* plane = reinterpret_cast<half_t*>(freeu_smem + p.plane_off);   // [HW][gvec][VEC]

    // twiddles of exact rational angles, once per block (an axis of length 1 contributes the factor 1: cos = sin = 0)
    for (int i = tid; i < p.H + p.W; i += kFreeuThreads) {
        const int len = i < p.H ? p.H : p.W, idx = i < p.H ? i : i - p.H;
        float sv = 0.f, cv = 0.f;
        if (len > 1) sincospif(2.0f * (float)idx / (float)len, &sv, &cv);
        if (i < p.H) { cosH[idx] = cv; sinH[idx] = sv; }
        else { cosW[idx] = cv; sinW[idx] = sv; }
    }
    __syncthreads();

    const int n = (int)blockIdx.x / p.groups, g = (int)blockIdx.x - n * p.groups;
    const int vec = tid & (p.gvec - 1), lane = tid / p.gvec, step = kFreeuThreads / p.gvec;
    const int cvec = g * p.gvec + vec;
    const bool act = cvec < p.C2 / VEC;
    half_t* base = p.x + (long)n * p.HW * p.ld + p.C1 + (long)cvec * VEC;

    float m[kFreeuMoments][VEC];
#pragma unroll
    for (int j = 0; j < kFreeuMoments; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) m[j][e] = 0.f;

    if (act) {
        for (int px = lane; px < p.HW; px += step) {
            const int h = px / p.W, w = px - h * p.W;
            const float ca = cosH[h], sa = sinH[h], cb = cosW[w], sb = sinW[w];
            const float d = ca * cb - sa * sb, e2 = ca * sb + sa * cb;
            float x[VEC];
            if constexpr (VEC == 8) {
                const h8 r = *reinterpret_cast<const h8*>(base + (long)px * p.ld);
                if (p.in_lds) *reinterpret_cast<h8*>(plane + ((long)px * p.gvec + vec) * 8) = r;
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = (float)r[e];
            } else {
                const half_t r = base[(long)px * p.ld];
                if (p.in_lds) plane[(long)px * p.gvec + vec] = r;
                x[0] = (float)r;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                m[0][e] += x[e];
                m[1][e] = __builtin_fmaf(x[e], ca, m[1][e]);
                m[2][e] = __builtin_fmaf(x[e], sa, m[2][e]);
                m[3][e] = __builtin_fmaf(x[e], cb, m[3][e]);
                m[4][e] = __builtin_fmaf(x[e], sb, m[4][e]);
                m[5][e] = __builtin_fmaf(x[e], d, m[5][e]);
                m[6][e] = __builtin_fmaf(x[e], e2, m[6][e]);
            }
        }
    }

    // lanes of one wave that hold the same channel vector differ in the bits >= gvec; then the four waves through LDS
#pragma unroll
    for (int j = 0; j < kFreeuMoments; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float v = m[j][e];
            for (int off = SD_WAVE / 2; off >= p.gvec; off >>= 1) v += __shfl_xor(v, off, SD_WAVE);
            m[j][e] = v;
        }
    const int wave = tid / SD_WAVE, wl = tid & (SD_WAVE - 1);
    constexpr int kWaves = kFreeuThreads / SD_WAVE;
    if (wl < p.gvec) {
        float* r = red + (long)(wave * p.gvec + wl) * kFreeuMoments * VEC;
#pragma unroll
        for (int j = 0; j < kFreeuMoments; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[j * VEC + e] = m[j][e];
    }
    __syncthreads();
    if (!act) return;
#pragma unroll
    for (int j = 0; j < kFreeuMoments; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float v = 0.f;
#pragma unroll
            for (int wv = 0; wv < kWaves; ++wv) v += red[(long)(wv * p.gvec + vec) * kFreeuMoments * VEC + j * VEC + e];
            m[j][e] = v * p.k;
        }

    // ---- apply: y = x + k (m0 + cos a m1 + sin a m2 + cos b m3 + sin b m4 + d m5 + e m6), rounded to fp16 once ----
    for (int px = lane; px < p.HW; px += step) {
        const int h = px / p.W, w = px - h * p.W;
        const float ca = cosH[h], sa = sinH[h], cb = cosW[w], sb = sinW[w];
        const float d = ca * cb - sa * sb, e2 = ca * sb + sa * cb;
        half_t* q = base + (long)px * p.ld;
        float x[VEC];
        if (p.in_lds) freeu_load<VEC>(plane + ((long)px * p.gvec + vec) * VEC, x);
        else freeu_load<VEC>(q, x);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float corr = m[0][e];
            corr = __builtin_fmaf(ca, m[1][e], corr);
            corr = __builtin_fmaf(sa, m[2][e], corr);
            corr = __builtin_fmaf(cb, m[3][e], corr);
            corr = __builtin_fmaf(sb, m[4][e], corr);
            corr = __builtin_fmaf(d, m[5][e], corr);
            corr = __builtin_fmaf(e2, m[6][e], corr);
            x[e] += corr;
        }
        freeu_store<VEC>(q, x);
    }
}

template <int VEC>
int freeu_launch(FreeuParams p, size_t lds, unsigned grid, hipStream_t s) {
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&freeu_kernel<VEC>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFreeuLdsMax));
    }
    hipLaunchKernelGGL(freeu_kernel<VEC>, dim3(grid), dim3(kFreeuThreads), lds, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return 3; }
    return 0;
}

}  // namespace

// Forms.  Vector form (16-byte accesses) when the view's base is 16-byte aligned and ld, C1 / 2 and C2 are multiples
// of 8; the scalar form otherwise (any even C1, any C2 >= 1).  A block owns one image and gvec channel vectors of the
// skip half: gvec starts at 4 vectors (64 contiguous bytes per pixel; 32 channels in the scalar form) and halves while
// the launch has fewer than 512 skip blocks, then while the block's plane [H W][gvec][VEC] fp16 plus its twiddles does
// not fit 72 KB of LDS.  A plane that fits is read from memory once (LDS-resident: every map of SD1.5 at 512 px and of
// SDXL at 1024 px, the 64 x 64 one with gvec = 1); a larger one (H W > about 4500 in the vector form) is read a
// second time by the apply pass, through L2, with no moment buffer in between: the block that reduced it applies it.
int launch_freeu(half_t* x, long ld, int N, int H, int W, int C1, int C2, float b, float s, hipStream_t st) {
    if (!x || N < 1 || H < 1 || W < 1 || C1 < 0 || C1 % 2 != 0 || C2 < 1 || ld < (long)C1 + C2) {
        set_error("freeu: needs N, H, W >= 1, an even C1 >= 0, C2 >= 1 and ld >= C1 + C2");
        return 1;
    }
    if (!std::isfinite(b) || !std::isfinite(s)) { set_error("freeu: factors must be finite"); return 1; }
    if ((long)H + W > 4096 || (long)H * W > (1L << 24) || (long)N * C2 > (1L << 28)) {
        set_error("freeu: beyond the kernel's twiddle table and grid (H + W <= 4096, H W <= 2^24, N C2 <= 2^28)");
        return 4;
    }
    const bool vec8 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ld % 8 == 0 && C1 % 16 == 0 && C2 % 8 == 0;
    const int VEC = vec8 ? 8 : 1;
    const int nvec = C2 / VEC;
    FreeuParams p;
    p.x = x; p.ld = ld; p.N = N; p.H = H; p.W = W; p.HW = H * W; p.C1 = C1; p.C2 = C2;
    p.b = b; p.k = (s - 1.f) / (float)((long)H * W);
    const size_t tw = (size_t)2 * (H + W) * sizeof(float);
    auto head = [&](int gvec) { return (tw + (size_t)4 * gvec * kFreeuMoments * VEC * sizeof(float) + 15) & ~size_t(15); };
    auto plane = [&](int gvec) { return (size_t)p.HW * gvec * VEC * sizeof(half_t); };
    int gvec = vec8 ? 4 : 32;
    while (gvec > 1 && (long)N * cdiv(nvec, gvec) < kFreeuTargetBlocks) gvec >>= 1;
    while (gvec > 1 && head(gvec) + plane(gvec) > kFreeuLdsMax) gvec >>= 1;
    p.gvec = gvec;
    p.groups = cdiv(nvec, gvec);
    p.skip_blocks = N * p.groups;
    p.in_lds = head(gvec) + plane(gvec) <= kFreeuLdsMax ? 1 : 0;
    p.plane_off = (int)head(gvec);
    const size_t lds = head(gvec) + (p.in_lds ? plane(gvec) : 0);
    const long hid_vecs = (long)N * p.HW * ((C1 / 2) / VEC);
    // (b == 1 leaves every fp16 value as it is: no backbone blocks)
    const int hid_blocks = (b == 1.f) ? 0 : (int)(hid_vecs > 2048L * kFreeuThreads ? 2048 : cdiv(hid_vecs, kFreeuThreads));
    const unsigned grid = (unsigned)(p.skip_blocks + hid_blocks);
    return vec8 ? freeu_launch<8>(p, lds, grid, st) : freeu_launch<1>(p, lds, grid, st);
}

}  // namespace sd
