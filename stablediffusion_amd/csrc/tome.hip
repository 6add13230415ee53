// Token merging for self-attention (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion"; tomesd's
// bipartite_soft_matching_random2d, restated in DESIGN.md and tests/tome_oracle.py).
//
// The H x W map is cut into sy x sx cells; one token of every whole cell is a destination (the first, or one drawn by a
// counter-based hash of (seed, step, site, cell)), every other token is a source.  Each source finds the destination of
// largest cosine similarity; the r sources with the largest such similarity are merged into their destinations (mean), the
// rest stay.  The merged sequence is [unmerged sources in raster order | destinations in raster order].
//
// Launches per merged block, all on one opaque plan buffer (tome_plan_bytes):
//   tome_prep_kernel     one wave per (image, token): fp32 reciprocal norm of the row; the waves of image 0 also place the
//                        token in the rank -> token table (sources first, then destinations) and one thread writes the header
//   tome_match_kernel    x_src x_dst^T on 16x16x32 fp16 MFMAs, fp32 accumulation over all of C, scaled by the two reciprocal
//                        norms afterwards; running (max, lowest argmax) per source row: the Ns x Nd scores are never stored
//   tome_select_kernel   one block per image: radix select of the r largest keys (ties to the lower source rank), prefix
//                        sum compaction of the unmerged ranks, member lists per merged row in ascending token index
//   tome_merge_kernel    rows of a [B T, ld] buffer -> [B T', ld'] (fp32 sum over the member list, one divide, one rounding)
//   tome_unmerge_kernel  the gather back through map
// No global atomics; LDS counters only order a scratch list that is ranked afterwards, so every result is reproducible.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace sd {

// ---- plan buffer (ints): [header 16][tok_of T][per image: map T | off T + 1 | members T | tmp T | rnorm T | nmax T | nidx T]
namespace {
constexpr int kTomeHdr = 16;
constexpr int kTomeMagic = 0x746f6d65;
enum { kHdrMagic = 0, kHdrT, kHdrTm, kHdrNd, kHdrNs, kHdrR, kHdrB };
__host__ __device__ inline long tome_img_ints(int T) { return 7L * T + 1; }
__host__ __device__ inline long tome_img_off(int b, int T) { return kTomeHdr + (long)T + (long)b * tome_img_ints(T); }
// offsets inside an image's part
__host__ __device__ inline long tome_o_map(int T) { (void)T; return 0; }
__host__ __device__ inline long tome_o_off(int T) { return T; }
__host__ __device__ inline long tome_o_mem(int T) { return 2L * T + 1; }
__host__ __device__ inline long tome_o_tmp(int T) { return 3L * T + 1; }
__host__ __device__ inline long tome_o_rn(int T) { return 4L * T + 1; }
__host__ __device__ inline long tome_o_nmax(int T) { return 5L * T + 1; }
__host__ __device__ inline long tome_o_nidx(int T) { return 6L * T + 1; }

// the destination token of cell (cy, cx)
__host__ __device__ inline int tome_dst_token(const TomeGeom& g, int cy, int cx) {
    const int k = g.use_rand ? (int)(mix32(g.seed, g.step, g.site, (uint32_t)(cy * g.wsx + cx)) % (uint32_t)(g.sx * g.sy)) : 0;
    return (cy * g.sy + k / g.sx) * g.W + cx * g.sx + k % g.sx;
}
}  // namespace

long tome_plan_bytes(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return (long)sizeof(int) * (kTomeHdr + (long)T + (long)B * tome_img_ints(T));
}

int tome_geom(int H, int W, int sx, int sy, double ratio, int use_rand, uint32_t seed, uint32_t step, uint32_t site, TomeGeom* g) {
    if (H < 1 || W < 1 || sx < 1 || sx > 8 || sy < 1 || sy > 8 || !(ratio >= 0.0 && ratio <= 0.75) || (long)H * W > (1L << 24)) {
        set_error("tome: needs H, W >= 1 (H W <= 2^24), sx and sy in 1..8, ratio in [0, 0.75]");
        return 1;
    }
    g->H = H; g->W = W; g->sx = sx; g->sy = sy;
    g->hsy = H / sy; g->wsx = W / sx;
    g->use_rand = use_rand ? 1 : 0; g->seed = seed; g->step = step; g->site = site;
    g->T = H * W;
    g->Nd = g->hsy * g->wsx;
    g->Ns = g->T - g->Nd;
    const int want = (int)((double)g->T * ratio);
    g->r = want < g->Ns ? want : g->Ns;
    g->Tm = g->T - g->r;
    return 0;
}

void tome_dst_tokens(const TomeGeom& g, int* dst_tok) {
    for (int cy = 0; cy < g.hsy; ++cy)
        for (int cx = 0; cx < g.wsx; ++cx) dst_tok[cy * g.wsx + cx] = tome_dst_token(g, cy, cx);
    std::sort(dst_tok, dst_tok + g.Nd);     // ranks are raster order
}

namespace {

// ------------------------------------------------------------------------------------------------ prep
// One wave per (image, token).  rnorm = 1 / sqrt(sum x^2) in fp32 (0 for a zero row: its scores are then 0).
__global__ __launch_bounds__(256) void tome_prep_kernel(const half_t* __restrict__ x, long ldx, int B, int C, TomeGeom g,
                                                        int* __restrict__ plan) {
    const int lane = threadIdx.x & 63;
    const long wv = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int T = g.T;
    if (wv >= (long)B * T) return;
    const int b = (int)(wv / T), t = (int)(wv - (long)b * T);
    const half_t* row = x + ((long)b * T + t) * ldx;
    float ss = 0.f;
    for (int v = lane; v < C / 8; v += 64) {
        const h8 r = *reinterpret_cast<const h8*>(row + v * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss = __builtin_fmaf((float)r[e], (float)r[e], ss);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, SD_WAVE);
    if (lane == 0) {
        float* rn = reinterpret_cast<float*>(plan + tome_img_off(b, T) + tome_o_rn(T));
        rn[t] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
    }
    if (b != 0) return;
    // rank -> token: a source's rank is its raster index minus the destinations in front of it
    const int y = t / g.W, xx = t - y * g.W;
    const int cy = y / g.sy;
    int before = 0, self = 0;
    if (cy < g.hsy) {
        for (int c = lane; c < g.wsx; c += 64) {
            const int d = tome_dst_token(g, cy, c);
            before += d < t ? 1 : 0;
            self += d == t ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            before += __shfl_xor(before, off, SD_WAVE);
            self += __shfl_xor(self, off, SD_WAVE);
        }
        before += cy * g.wsx;
    } else {
        before = g.Nd;
    }
    if (lane == 0) {
        int* tok_of = plan + kTomeHdr;
        // (`before` counts the destinations in front of t in raster order: a destination's own rank, too)
        if (self) tok_of[g.Ns + before] = t;
        else tok_of[t - before] = t;
        if (t == 0) {
            plan[kHdrMagic] = kTomeMagic; plan[kHdrT] = T; plan[kHdrTm] = g.Tm; plan[kHdrNd] = g.Nd; plan[kHdrNs] = g.Ns;
            plan[kHdrR] = g.r; plan[kHdrB] = B;
        }
    }
}

// ------------------------------------------------------------------------------------------------ match
// Block = 4 waves = 128 source rows of one image; a wave owns 32 of them (two 16-row MFMA tiles) and sweeps the
// destinations in tiles of 64 (four 16-column MFMA tiles).  Fragments come straight from global memory: lane (fr, fq) of
// an operand tile holds row fr, 8 halves at k0 + 8 fq; the result lane holds rows 4 fq + e, column fr.
__global__ __launch_bounds__(256) void tome_match_kernel(const half_t* __restrict__ x, long ldx, int C, int T, int Ns, int Nd,
                                                         int* __restrict__ plan) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.y;
    const int* tok_of = plan + kTomeHdr;
    int* img = plan + tome_img_off(b, T);
    const float* rn = reinterpret_cast<const float*>(img + tome_o_rn(T));
    const half_t* xb = x + (long)b * T * ldx;
    const int base = blockIdx.x * 128 + wave * 32;
    if (base >= Ns) return;

    const half_t* pa[2];
    float rna[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int ra = min(base + a * 16 + fr, Ns - 1);
        pa[a] = xb + (long)tok_of[ra] * ldx + fq * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) rna[a][e] = rn[tok_of[min(base + a * 16 + fq * 4 + e, Ns - 1)]];
    }
    float best[2][4];
    int bidx[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) { best[a][e] = -INFINITY; bidx[a][e] = 0x7fffffff; }

    for (int j0 = 0; j0 < Nd; j0 += 64) {
        const half_t* pb[4];
        float rnb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int tk = tok_of[Ns + min(j0 + s * 16 + fr, Nd - 1)];
            pb[s] = xb + (long)tk * ldx + fq * 8;
            rnb[s] = rn[tk];
        }
        f4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[a][s] = f4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < C; k0 += 32) {
            h8 fa[2], fb[4];
#pragma unroll
            for (int a = 0; a < 2; ++a) fa[a] = *reinterpret_cast<const h8*>(pa[a] + k0);
#pragma unroll
            for (int s = 0; s < 4; ++s) fb[s] = *reinterpret_cast<const h8*>(pb[s] + k0);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[a][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a], fb[s], acc[a][s], 0, 0, 0);
        }
        // ascending destination rank per lane: a strict > keeps the lowest rank that attains the maximum
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = j0 + s * 16 + fr;
            if (j < Nd) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sc = acc[a][s][e] * rna[a][e] * rnb[s];
                        if (sc > best[a][e]) { best[a][e] = sc; bidx[a][e] = j; }
                    }
            }
        }
    }
    float* nmax = reinterpret_cast<float*>(img + tome_o_nmax(T));
    int* nidx = img + tome_o_nidx(T);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = best[a][e];
            int i = bidx[a][e];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const float v2 = __shfl_xor(v, off, SD_WAVE);
                const int i2 = __shfl_xor(i, off, SD_WAVE);
                if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
            }
            const int row = base + a * 16 + fq * 4 + e;
            if (fr == 0 && row < Ns) {
                // (scores that are not numbers never win: such a row reports destination 0 at score 0)
                const bool ok = i < Nd;
                nmax[row] = ok ? v : 0.f;
                nidx[row] = ok ? i : 0;
            }
        }
}

// The same tile for C = 32 KS with KS in {2, 4, 10, 20} (C = 64, 128, 320, 640: every level of SD1.5 / SDXL that
// merges at max_downsample <= 2): the wave's two source tiles stay in registers for the whole sweep (2 KS fragments), and
// a destination tile of 64 rows is staged once per block in LDS, rows C + 8 halves apart (the 16 rows a fragment load
// touches then start 4 banks apart: no conflicts), instead of once per wave from global memory.  The next tile's rows
// are fetched into registers while the current one is multiplied.  Results are the direct kernel's bit for bit: the
// same MFMAs in the same order.
template <int KS>
__global__ __launch_bounds__(256) void tome_match_lds_kernel(const half_t* __restrict__ x, long ldx, int T, int Ns, int Nd,
                                                             int* __restrict__ plan) {
    extern __shared__ __align__(16) unsigned char tome_match_smem[];
    half_t* tile = reinterpret_cast<half_t*>(tome_match_smem);     // [64][C + 8]
    constexpr int C = KS * 32, LD = C + 8, VPR = C / 8;             // vectors per row; 64 VPR / 256 = KS per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int b = blockIdx.y;
    const int* tok_of = plan + kTomeHdr;
    int* img = plan + tome_img_off(b, T);
    const float* rn = reinterpret_cast<const float*>(img + tome_o_rn(T));
    const half_t* xb = x + (long)b * T * ldx;
    const int base = blockIdx.x * 128 + wave * 32;

    h8 fa[2][KS];
    float rna[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const half_t* pa = xb + (long)tok_of[min(base + a * 16 + fr, Ns - 1)] * ldx + fq * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) fa[a][ks] = *reinterpret_cast<const h8*>(pa + ks * 32);
#pragma unroll
        for (int e = 0; e < 4; ++e) rna[a][e] = rn[tok_of[min(base + a * 16 + fq * 4 + e, Ns - 1)]];
    }
    float best[2][4];
    int bidx[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) { best[a][e] = -INFINITY; bidx[a][e] = 0x7fffffff; }

    h8 nxt[KS];
    auto fetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int v = tid + 256 * i, row = v / VPR, col = v - row * VPR;
            nxt[i] = *reinterpret_cast<const h8*>(xb + (long)tok_of[Ns + min(j0 + row, Nd - 1)] * ldx + col * 8);
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < Nd; j0 += 64) {
        __syncthreads();                    // (the previous tile has been read)
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const int v = tid + 256 * i, row = v / VPR, col = v - row * VPR;
            *reinterpret_cast<h8*>(tile + row * LD + col * 8) = nxt[i];
        }
        __syncthreads();
        if (j0 + 64 < Nd) fetch(j0 + 64);
        float rnb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) rnb[s] = rn[tok_of[Ns + min(j0 + s * 16 + fr, Nd - 1)]];
        f4 acc[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[a][s] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            h8 fb[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) fb[s] = *reinterpret_cast<const h8*>(tile + (s * 16 + fr) * LD + ks * 32 + fq * 8);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[a][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[a][ks], fb[s], acc[a][s], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = j0 + s * 16 + fr;
            if (j < Nd) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sc = acc[a][s][e] * rna[a][e] * rnb[s];
                        if (sc > best[a][e]) { best[a][e] = sc; bidx[a][e] = j; }
                    }
            }
        }
    }
    float* nmax = reinterpret_cast<float*>(img + tome_o_nmax(T));
    int* nidx = img + tome_o_nidx(T);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = best[a][e];
            int i = bidx[a][e];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const float v2 = __shfl_xor(v, off, SD_WAVE);
                const int i2 = __shfl_xor(i, off, SD_WAVE);
                if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
            }
            const int row = base + a * 16 + fq * 4 + e;
            if (fr == 0 && row < Ns) {
                const bool ok = i < Nd;
                nmax[row] = ok ? v : 0.f;
                nidx[row] = ok ? i : 0;
            }
        }
}

template <int KS>
int tome_match_lds_launch(const half_t* x, long ldx, int B, const TomeGeom& g, int* p, hipStream_t s) {
    constexpr size_t lds = (size_t)64 * (KS * 32 + 8) * sizeof(half_t);
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tome_match_lds_kernel<KS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(tome_match_lds_kernel<KS>, dim3((unsigned)cdiv(g.Ns, 128), (unsigned)B), dim3(256), lds, s, x, ldx, g.T,
                       g.Ns, g.Nd, p);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ select
constexpr int kSelThreads = 1024;
constexpr size_t kSelLdsMax = 160 * 1024;

// exclusive prefix sum of one int per thread over the block; *total = the sum.  scratch: kSelThreads / 64 + 1 ints.
__device__ __forceinline__ int block_excl_scan(int v, int* scratch, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, SD_WAVE);
        if (lane >= off) inc += o;
    }
    __syncthreads();                        // (scratch may still be read from the previous scan)
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < kSelThreads / 64; ++w) { const int c = scratch[w]; scratch[w] = run; run += c; }
        scratch[kSelThreads / 64] = run;
    }
    __syncthreads();
    *total = scratch[kSelThreads / 64];
    return scratch[wave] + inc - v;
}

__device__ __forceinline__ uint32_t tome_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// LDS: keys [Ns] | cnt [Nd] | doff [Nd + 1] | hist [256] | scratch [kSelThreads / 64 + 1] | sel [2]
__global__ __launch_bounds__(kSelThreads) void tome_select_kernel(int* __restrict__ plan, int T, int Ns, int Nd, int r) {
    extern __shared__ __align__(16) unsigned char tome_smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(tome_smem);
    int* cnt = reinterpret_cast<int*>(keys + Ns);
    int* doff = cnt + Nd;
    int* hist = doff + Nd + 1;
    int* scratch = hist + 256;
    int* sel = scratch + kSelThreads / 64 + 1;
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int* tok_of = plan + kTomeHdr;
    int* img = plan + tome_img_off(b, T);
    int* map = img + tome_o_map(T);
    int* off = img + tome_o_off(T);
    int* members = img + tome_o_mem(T);
    int* tmp = img + tome_o_tmp(T);
    const float* nmax = reinterpret_cast<const float*>(img + tome_o_nmax(T));
    const int* nidx = img + tome_o_nidx(T);
    const int U = Ns - r;                    // unmerged sources = first row of the destinations

    for (int i = tid; i < Ns; i += kSelThreads) keys[i] = tome_key(nmax[i]);
    for (int j = tid; j < Nd; j += kSelThreads) cnt[j] = 1;

    // ---- the r-th largest key, eight bits at a time; `need` of the keys equal to it are merged (the lowest ranks) ----
    uint32_t prefix = 0, mask = 0;
    int remaining = r;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += kSelThreads) hist[i] = 0;
        __syncthreads();
        for (int i = tid; i < Ns; i += kSelThreads) {
            const uint32_t k = keys[i];
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {
            // wave 0: lane l owns bins 4 l .. 4 l + 3; `above` = the keys in the bins of the lanes above it.  The one
            // lane with above < remaining <= above + own holds the digit.
            int h[4], own = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { h[k] = hist[4 * tid + k]; own += h[k]; }
            int suf = own;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_down(suf, off, SD_WAVE);
                if (tid + off < 64) suf += o;
            }
            int acc = suf - own;
            if (acc < remaining && remaining <= acc + own) {
#pragma unroll
                for (int k = 3; k >= 0; --k) {
                    if (acc + h[k] >= remaining) { sel[0] = 4 * tid + k; sel[1] = remaining - acc; break; }
                    acc += h[k];
                }
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sel[0] << shift;
        mask |= 255u << shift;
        remaining = sel[1];
        __syncthreads();
    }
    const uint32_t kstar = prefix;
    const int need = remaining;

    // ---- every thread owns a run of consecutive source ranks ----
    const int per = (Ns + kSelThreads - 1) / kSelThreads;
    const int i0 = min(tid * per, Ns), i1 = min(i0 + per, Ns);
    int eq = 0;
    for (int i = i0; i < i1; ++i) eq += keys[i] == kstar ? 1 : 0;
    int total;
    int eq_at = block_excl_scan(eq, scratch, &total);
    int um = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t k = keys[i];
        bool merged = k > kstar;
        if (k == kstar) { merged = eq_at < need; ++eq_at; }
        keys[i] = merged ? 1u : 0u;
        um += merged ? 0 : 1;
    }
    int um_at = block_excl_scan(um, scratch, &total);
    for (int i = i0; i < i1; ++i) {
        const int tk = tok_of[i];
        if (keys[i]) {
            const int j = min(max(nidx[i], 0), Nd - 1);
            map[tk] = U + j;
            atomicAdd(&cnt[j], 1);
        } else {
            map[tk] = um_at; off[um_at] = um_at; members[um_at] = tk;
            ++um_at;
        }
    }
    __syncthreads();

    // ---- offsets of the destinations' member lists ----
    const int perd = (Nd + kSelThreads - 1) / kSelThreads;
    const int j0 = min(tid * perd, Nd), j1 = min(j0 + perd, Nd);
    int sum = 0;
    for (int j = j0; j < j1; ++j) sum += cnt[j];
    int at = block_excl_scan(sum, scratch, &total);
    for (int j = j0; j < j1; ++j) {
        doff[j] = at; off[U + j] = U + at;
        at += cnt[j];
    }
    if (tid == 0) { doff[Nd] = total; off[U + Nd] = U + total; }
    __syncthreads();
    for (int j = tid; j < Nd; j += kSelThreads) cnt[j] = 0;
    __syncthreads();

    // ---- members in any order, then each at its rank by token index (the lists are short: 1 + r / Nd on average) ----
    for (int j = tid; j < Nd; j += kSelThreads) {
        const int tk = tok_of[Ns + j];
        map[tk] = U + j;
        tmp[doff[j] + atomicAdd(&cnt[j], 1)] = tk;
    }
    for (int i = i0; i < i1; ++i)
        if (keys[i]) {
            const int j = min(max(nidx[i], 0), Nd - 1);
            tmp[doff[j] + atomicAdd(&cnt[j], 1)] = tok_of[i];
        }
    __threadfence_block();
    __syncthreads();
    for (int o = tid; o < Nd + r; o += kSelThreads) {
        const int tk = tmp[o];
        const int j = map[tk] - U;
        int pos = 0;
        for (int q = doff[j]; q < doff[j + 1]; ++q) pos += tmp[q] < tk ? 1 : 0;
        members[U + doff[j] + pos] = tk;
    }
    // (the scratch list ends as a copy of the ranked one: the whole plan is the same bytes from run to run)
    __threadfence_block();
    __syncthreads();
    for (int o = tid; o < Nd + r; o += kSelThreads) tmp[o] = members[U + o];
}

// ------------------------------------------------------------------------------------------------ merge / unmerge
template <int VEC>
__global__ __launch_bounds__(256) void tome_merge_kernel(const half_t* __restrict__ src, long lds, int cols,
                                                         const int* __restrict__ plan, int B, int T, int rows_bound,
                                                         half_t* __restrict__ dst, long ldd) {
    if (plan[kHdrMagic] != kTomeMagic || plan[kHdrT] != T || plan[kHdrB] < B) return;
    const int Tm = plan[kHdrTm];
    const int nv = cols / VEC;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * rows_bound * nv) return;
    const long row = i / nv;
    const int v = (int)(i - row * nv);
    const int b = (int)(row / rows_bound), m = (int)(row - (long)b * rows_bound);
    if (m >= Tm) return;
    const int* img = plan + tome_img_off(b, T);
    const int* off = img + tome_o_off(T);
    const int* members = img + tome_o_mem(T);
    const int o0 = off[m], o1 = off[m + 1];
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int o = o0; o < o1; ++o) {
        const half_t* p = src + ((long)b * T + members[o]) * lds + v * VEC;
        if constexpr (VEC == 8) {
            const h8 r = *reinterpret_cast<const h8*>(p);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)r[e];
        } else {
            acc[0] += (float)p[0];
        }
    }
    const float n = (float)(o1 - o0);
    half_t* q = dst + ((long)b * Tm + m) * ldd + v * VEC;
    if constexpr (VEC == 8) {
        h8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)(acc[e] / n);
        *reinterpret_cast<h8*>(q) = r;
    } else {
        q[0] = (half_t)(acc[0] / n);
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void tome_unmerge_kernel(const half_t* __restrict__ src, long lds, int cols,
                                                           const int* __restrict__ plan, int B, int T,
                                                           half_t* __restrict__ dst, long ldd) {
    if (plan[kHdrMagic] != kTomeMagic || plan[kHdrT] != T || plan[kHdrB] < B) return;
    const int Tm = plan[kHdrTm];
    const int nv = cols / VEC;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * T * nv) return;
    const long row = i / nv;
    const int v = (int)(i - row * nv);
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const int m = plan[tome_img_off(b, T) + tome_o_map(T) + t];
    if ((unsigned)m >= (unsigned)Tm) return;
    const half_t* p = src + ((long)b * Tm + m) * lds + v * VEC;
    half_t* q = dst + row * ldd + v * VEC;
    if constexpr (VEC == 8) *reinterpret_cast<h8*>(q) = *reinterpret_cast<const h8*>(p);
    else q[0] = p[0];
}

inline bool tome_vec8(const void* a, long lda, const void* b, long ldb, int cols) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && lda % 8 == 0 && ldb % 8 == 0 &&
           cols % 8 == 0;
}

size_t tome_select_lds(int Ns, int Nd) {
    return sizeof(int) * ((size_t)Ns + 2 * (size_t)Nd + 1 + 256 + kSelThreads / 64 + 1 + 2);
}

}  // namespace

bool tome_supported(const TomeGeom& g) {
    return g.T <= 16384 && g.Nd >= 1 && tome_select_lds(g.Ns, g.Nd) <= kSelLdsMax;
}

int launch_tome_match(const half_t* x, long ldx, int B, int C, const TomeGeom& g, void* plan, hipStream_t s, int stage) {
    if (!x || !plan || B < 1 || B > 65535 || C < 32 || C % 32 != 0 || ldx < C || ldx % 8 != 0 ||
        (reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(plan) & 3) != 0) {
        set_error("tome_match: needs 1 <= B <= 65535, C a multiple of 32, ldx >= C and a multiple of 8, a 16-byte aligned x");
        return 1;
    }
    if (!tome_supported(g)) { set_error("tome_match: T above 16384 or a map without a whole cell is not supported"); return 4; }
    if (g.r < 1) { set_error("tome_match: nothing to merge (r = 0)"); return 1; }
    if (stage < 0 || stage > 3) { set_error("tome_match: unknown stage"); return 1; }
    int* p = static_cast<int*>(plan);
    if (stage == 0 || stage == 1) {
        const long waves = (long)B * g.T;
        hipLaunchKernelGGL(tome_prep_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, x, ldx, B, C, g, p);
        SD_HIP_CHECK(hipGetLastError());
    }
    static const bool no_lds = getenv("SD_NO_TOME_LDS") != nullptr;     // (read once, like the other A/B switches)
    const int ks = no_lds ? 0 : C / 32;
    if ((stage == 0 || stage == 2) && (ks == 2 || ks == 4 || ks == 10 || ks == 20)) {
        int rc = ks == 2 ? tome_match_lds_launch<2>(x, ldx, B, g, p, s) : ks == 4 ? tome_match_lds_launch<4>(x, ldx, B, g, p, s)
               : ks == 10 ? tome_match_lds_launch<10>(x, ldx, B, g, p, s) : tome_match_lds_launch<20>(x, ldx, B, g, p, s);
        if (rc) return rc;
    } else if (stage == 0 || stage == 2) {
        hipLaunchKernelGGL(tome_match_kernel, dim3((unsigned)cdiv(g.Ns, 128), (unsigned)B), dim3(256), 0, s, x, ldx, C, g.T,
                           g.Ns, g.Nd, p);
        SD_HIP_CHECK(hipGetLastError());
    }
    if (stage == 1 || stage == 2) return 0;
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tome_select_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSelLdsMax));
    }
    hipLaunchKernelGGL(tome_select_kernel, dim3((unsigned)B), dim3(kSelThreads), tome_select_lds(g.Ns, g.Nd), s, p, g.T, g.Ns,
                       g.Nd, g.r);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int tome_plan_fetch(const void* plan, int B, int T, int Ns, int* map_out, float* node_max, int* node_idx, hipStream_t s) {
    const int* p = static_cast<const int*>(plan);
    for (int b = 0; b < B; ++b) {
        const int* img = p + tome_img_off(b, T);
        if (map_out) SD_HIP_CHECK(hipMemcpyAsync(map_out + (long)b * T, img + tome_o_map(T), (size_t)T * 4, hipMemcpyDeviceToDevice, s));
        if (node_max && Ns > 0) SD_HIP_CHECK(hipMemcpyAsync(node_max + (long)b * Ns, img + tome_o_nmax(T), (size_t)Ns * 4, hipMemcpyDeviceToDevice, s));
        if (node_idx && Ns > 0) SD_HIP_CHECK(hipMemcpyAsync(node_idx + (long)b * Ns, img + tome_o_nidx(T), (size_t)Ns * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

int tome_plan_read_map(const void* plan, int b, int T, int* map_host) {
    const int* p = static_cast<const int*>(plan);
    SD_HIP_CHECK(hipMemcpy(map_host, p + tome_img_off(b, T) + tome_o_map(T), (size_t)T * 4, hipMemcpyDeviceToHost));
    return 0;
}

int tome_plan_from_map(const int* map_host, int B, int T, int Tm, void* plan, hipStream_t s) {
    if (!map_host || !plan || B < 1 || T < 1 || Tm < 1 || Tm > T) { set_error("tome_plan_from_map: bad arguments"); return 1; }
    std::vector<int> h((size_t)(tome_plan_bytes(B, T) / sizeof(int)), 0);
    h[kHdrMagic] = kTomeMagic; h[kHdrT] = T; h[kHdrTm] = Tm; h[kHdrNd] = 0; h[kHdrNs] = 0; h[kHdrR] = T - Tm; h[kHdrB] = B;
    for (int b = 0; b < B; ++b) {
        const int* mp = map_host + (long)b * T;
        int* img = h.data() + tome_img_off(b, T);
        int* off = img + tome_o_off(T);
        int* members = img + tome_o_mem(T);
        std::vector<int> cnt((size_t)Tm, 0);
        for (int t = 0; t < T; ++t) {
            if (mp[t] < 0 || mp[t] >= Tm) { set_error("tome_plan_from_map: a map entry outside [0, T')"); return 1; }
            img[tome_o_map(T) + t] = mp[t];
            ++cnt[(size_t)mp[t]];
        }
        int run = 0;
        for (int m = 0; m < Tm; ++m) {
            if (cnt[(size_t)m] == 0) { set_error("tome_plan_from_map: a merged row without a member"); return 1; }
            off[m] = run; run += cnt[(size_t)m]; cnt[(size_t)m] = 0;
        }
        off[Tm] = run;
        for (int t = 0; t < T; ++t) members[off[mp[t]] + cnt[(size_t)mp[t]]++] = t;      // ascending token index
    }
    SD_HIP_CHECK(hipMemcpyAsync(plan, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s));
    SD_HIP_CHECK(hipStreamSynchronize(s));      // (h leaves scope)
    return 0;
}

int launch_tome_merge(const half_t* src, long lds, int cols, const void* plan, int B, int T, int Tm_host, half_t* dst, long ldd,
                      hipStream_t s) {
    if (!src || !dst || !plan || B < 1 || T < 1 || cols < 1 || lds < cols || ldd < cols || Tm_host < 0 || Tm_host > T) {
        set_error("tome_merge: bad arguments (cols >= 1, both row strides at least cols)");
        return 1;
    }
    const bool vec = tome_vec8(src, lds, dst, ldd, cols);
    const int rows = Tm_host > 0 ? Tm_host : T;         // (unknown on the host: the kernel reads T' from the plan)
    const long total = (long)B * rows * (vec ? cols / 8 : cols);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("tome_merge: too many elements for one launch"); return 1; }
    const int* p = static_cast<const int*>(plan);
    if (vec) hipLaunchKernelGGL(tome_merge_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, cols, p, B, T, rows, dst, ldd);
    else hipLaunchKernelGGL(tome_merge_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, cols, p, B, T, rows, dst, ldd);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_tome_unmerge(const half_t* src, long lds, int cols, const void* plan, int B, int T, half_t* dst, long ldd,
                        hipStream_t s) {
    if (!src || !dst || !plan || B < 1 || T < 1 || cols < 1 || lds < cols || ldd < cols) {
        set_error("tome_unmerge: bad arguments (cols >= 1, both row strides at least cols)");
        return 1;
    }
    const bool vec = tome_vec8(src, lds, dst, ldd, cols);
    const long total = (long)B * T * (vec ? cols / 8 : cols);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("tome_unmerge: too many elements for one launch"); return 1; }
    const int* p = static_cast<const int*>(plan);
    if (vec) hipLaunchKernelGGL(tome_unmerge_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, cols, p, B, T, dst, ldd);
    else hipLaunchKernelGGL(tome_unmerge_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, cols, p, B, T, dst, ldd);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
