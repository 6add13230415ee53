// Regional prompts ("attention couple") for gfx950 (CDNA4, wave64), one launch per attn2 site:
//   out[n, t] = sum_r W[n % Bw, t, r] * softmax(s q[n, t] K[n, rL:(r+1)L]^T) V[n, rL:(r+1)L]
// fp16 in/out, fp32 scores, weights and accumulators.  The R prompts ride in one encoder_hidden_states of R * L
// tokens, so K / V of all regions come out of the forward's one text-K/V GEMM; this kernel is ip_xattn_kernel
// (ip_attention.hip) generalised from two fixed segments to R of them with a coefficient per query.  It shares that
// kernel's building blocks (ip_attention_blocks.h): swapped products, ds_read_b64_tr_b16 V reads, odd-multiple-of-32-byte
// LDS row strides, an exact softmax per segment, and the coefficient W / l folded into P before the fp16 rounding, so
// all segments accumulate into one set of fp32 output registers.
//
// LDS.  One segment is 32 ceil(L / 32) rows of K and of V: 24.6 KB at d = 40, 30.7 KB at d = 64, 67.6 KB at d = 160
// for 77 keys.  region_plan splits the R segments into the fewest groups that fit 160 KiB and evens them out:
//   * one group (all resident): the block stages every segment once and walks its share of the query tiles, as
//     ip_xattn_kernel does;
//   * several groups: one query tile per block (eight waves, 128 queries).  The block works through the groups,
//     restaging K / V behind a barrier, while each wave's output tile stays in registers.  Only the segments some
//     query of the block's tile weighs are staged, and a group none of them weighs costs neither a barrier nor a byte.
// Skipping.  A wave skips a segment whose weight is zero for all 16 QT queries of its tile (a wave-uniform branch on a
// ballot): with disjoint masks almost every tile has one live region, and the launch costs about what the plain
// cross-attention does.  A segment that is zero for only some queries of a tile runs; those queries' P is exactly zero.
#include "ip_attention_blocks.h"

namespace sd {
namespace {

constexpr int kRegionMax = 8;
constexpr int kRegionLds = 160 * 1024;
constexpr int kRegionTailBytes = 16;          // the block's live-segment mask behind the K / V slots

constexpr int region_seg_bytes(int D, int L) { return 32 * ((L + 31) / 32) * (ip_kstr(D) + ip_vstr(D)) * 2; }

template <int D, int QT, int NWV>
__global__ __launch_bounds__(64 * NWV) void region_xattn_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k,
                                                            const half_t* __restrict__ v, const float* __restrict__ w,
                                                            half_t* __restrict__ out, int Tq, int L, int R, int heads,
                                                            long ldq, long ldk, long ldv, long ldo, int Bw,
                                                            float scale_log2e, int qblocks, int SG, int NG) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KS = (D + 31) / 32;
    constexpr int DT = (D + 15) / 16;
    constexpr int KSTR = ip_kstr(D), VSTR = ip_vstr(D);
    constexpr int QB = 16 * QT * NWV;
    constexpr int NTH = 64 * NWV;
    const int nkt = (L + 31) / 32, rows = nkt * 32;
    const int slot = rows * (KSTR + VSTR);            // halves per staged segment: K rows, then V rows

    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sKV = reinterpret_cast<half_t*>(smem);
    unsigned* s_need = reinterpret_cast<unsigned*>(smem + (size_t)SG * slot * 2);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = bid / qblocks, qblk = bid - bh * qblocks;
    const int b = bh / heads, h = bh - b * heads;
    const bool grouped = NG > 1;

    const half_t* kb = k + (long)b * R * L * ldk + h * D;
    const half_t* vb = v + (long)b * R * L * ldv + h * D;
    const float* wb = w + (long)(b % Bw) * Tq * R;
    const half_t* qb = q + (long)b * Tq * ldq + h * D;
    half_t* ob = out + (long)b * Tq * ldo + h * D;

    if (!grouped) {
        for (int r = 0; r < R; ++r) {
            stage_rows<D>(sKV + r * slot, KSTR, kb + (long)r * L * ldk, ldk, L, rows, tid, NTH);
            stage_rows<D>(sKV + r * slot + rows * KSTR, VSTR, vb + (long)r * L * ldv, ldv, L, rows, tid, NTH);
        }
        __syncthreads();
    }

    const int qtiles = (Tq + QB - 1) / QB;
    for (int qt = qblk; qt < qtiles; qt += qblocks) {      // block-uniform trip count: the barriers below are safe
        const int q0 = qt * QB + wave * 16 * QT;           // (a wave past Tq has no live segment and stores nothing)
        h8 qf[QT][KS];
        float wq[QT][kRegionMax];
        unsigned live = 0;                                 // wave-uniform: segments some query of this wave's tile weighs
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int qi = q0 + t * 16 + fr;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int c = ks * 32 + fq * 8;
                h8 val = {0, 0, 0, 0, 0, 0, 0, 0};
                if (qi < Tq && c < D) val = *reinterpret_cast<const h8*>(qb + (long)qi * ldq + c);
                qf[t][ks] = val;
            }
#pragma unroll
            for (int r = 0; r < kRegionMax; ++r) {
                float val = 0.f;
                if (r < R && qi < Tq) val = wb[(long)qi * R + r];
                wq[t][r] = val;
                if (__ballot(val != 0.f) != 0) live |= 1u << r;
            }
        }
        unsigned need = live;
        if (grouped) {
            // what the whole block's tile weighs: the segments worth staging
            __syncthreads();
            if (tid == 0) *s_need = 0u;
            __syncthreads();
            if (lane == 0 && live) atomicOr(s_need, live);
            __syncthreads();
            need = *s_need;
        }
        f4 o[DT][QT];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int t = 0; t < QT; ++t) o[i][t] = f4{0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < NG; ++g) {
            const int r0 = g * SG;
            const int nseg = R - r0 < SG ? R - r0 : SG;
            if (grouped) {
                const unsigned gmask = ((1u << nseg) - 1u) << r0;
                if (!(need & gmask)) continue;             // block-uniform
                __syncthreads();                           // every wave is done with the slots' previous contents
                for (int sg = 0; sg < nseg; ++sg) {
                    const int r = r0 + sg;
                    if (!((need >> r) & 1u)) continue;
                    stage_rows<D>(sKV + sg * slot, KSTR, kb + (long)r * L * ldk, ldk, L, rows, tid, NTH);
                    stage_rows<D>(sKV + sg * slot + rows * KSTR, VSTR, vb + (long)r * L * ldv, ldv, L, rows, tid, NTH);
                }
                __syncthreads();
            }
            for (int sg = 0; sg < nseg; ++sg) {
                const int r = r0 + sg;
                if (!((live >> r) & 1u)) continue;         // wave-uniform: nobody in this tile weighs region r
                float coef[QT];
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    float c = wq[t][0];
#pragma unroll
                    for (int j = 1; j < kRegionMax; ++j) c = r == j ? wq[t][j] : c;
                    coef[t] = c;
                }
                const half_t* cK = sKV + sg * slot;
                ip_segment<D, QT, kMaxTextSteps>(cK, cK + rows * KSTR, L, nkt, coef, scale_log2e, qf, o, fr, fq);
            }
        }
        // lane holds 4 consecutive d of one query
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int qi = q0 + t * 16 + fr;
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const int dd = i * 16 + fq * 4;
                if (qi < Tq && dd < D) {
                    const f4 val = o[i][t];
                    h4 wv = {(half_t)val[0], (half_t)val[1], (half_t)val[2], (half_t)val[3]};
                    *reinterpret_cast<h4*>(ob + (long)qi * ldo + dd) = wv;
                }
            }
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D, int QT, int NWV>
int launch_region(const half_t* q, const half_t* k, const half_t* v, const float* w, half_t* out, int B, int Tq, int L,
                  int R, int heads, long ldq, long ldk, long ldv, long ldo, int Bw, bool prescaled, const RegionPlan& pl,
                  hipStream_t s) {
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&region_xattn_kernel<D, QT, NWV>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kRegionLds));
    }
    const float scale_log2e = prescaled ? 1.0f : 1.4426950408889634f / sqrtf((float)D);
    constexpr int QB = 16 * QT * NWV;
    const int qtiles = cdiv(Tq, QB);
    const long bh = (long)B * heads;
    // all resident: as many blocks as the 256 CUs hold at once -- up to four per CU, fewer when the staged segments fill
    // the LDS -- each walking its share of the query tiles against the K / V it staged once (every block stages all R
    // segments, so more blocks than that only stage more); grouped: one query tile per block
    int qblocks = qtiles;
    if (pl.groups == 1) {
        int per_cu = kRegionLds / pl.lds_bytes;
        per_cu = per_cu > 4 ? 4 : per_cu < 1 ? 1 : per_cu;
        qblocks = (int)((256L * per_cu + bh - 1) / bh);
        if (qblocks > qtiles) qblocks = qtiles;
        if (qblocks < 1) qblocks = 1;
    }
    if (bh * qblocks > 0x7fffffffL) { set_error("region attention: too many blocks"); return 4; }
    hipLaunchKernelGGL((region_xattn_kernel<D, QT, NWV>), dim3((unsigned)(bh * qblocks)), dim3(64 * NWV),
                       (size_t)pl.lds_bytes, s, q, k, v, w, out, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, scale_log2e, qblocks,
                       pl.seg_per_group, pl.groups);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int S>
__device__ __forceinline__ float region_block_mean(const float* p, int W) {
    if constexpr (S == 1) {
        return p[0];
    } else {
        constexpr int Hh = S / 2;
        const float a = region_block_mean<Hh>(p, W), b = region_block_mean<Hh>(p + Hh, W);
        const float c = region_block_mean<Hh>(p + (long)Hh * W, W), d = region_block_mean<Hh>(p + (long)Hh * W + Hh, W);
        return (((a + b) + c) + d) * 0.25f;
    }
}

// Every level's weights in one launch: level l of `out` is [Bw, (H >> l) (W >> l), R], the 2x2 mean of level l - 1 (level
// 0: the input transposed), levels back to back.  One thread per output element.
__global__ void region_pyramid_kernel(const float* __restrict__ w, float* __restrict__ out, int Bw, int R, int H, int W,
                                      int levels, long total) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    int l = 0;
    for (; l < levels - 1; ++l) {
        const long n = (long)Bw * (H >> l) * (W >> l) * R;
        if (idx < n) break;
        idx -= n;
        out += n;
    }
    const int Wl = W >> l;
    const long Tl = (long)(H >> l) * Wl;
    const int r = (int)(idx % R);
    const long t = (idx / R) % Tl;
    const long b = idx / (R * Tl);
    const int y = (int)(t / Wl), x = (int)(t - (long)y * Wl);
    const float* p = w + ((b * R + r) * H + ((long)y << l)) * W + ((long)x << l);
    float m;
    switch (l) {
        case 0: m = region_block_mean<1>(p, W); break;
        case 1: m = region_block_mean<2>(p, W); break;
        case 2: m = region_block_mean<4>(p, W); break;
        default: m = region_block_mean<8>(p, W); break;
    }
    out[idx] = m;
}

}  // namespace

int region_plan(int R, int L, int d, RegionPlan* pl) {
    if (!ip_attention_supported(d)) { set_error("region attention: unsupported head dim " + std::to_string(d)); return 4; }
    if (R < 1 || R > kRegionMax) { set_error("region attention: regions must be in [1, 8]"); return 4; }
    if (L < 1 || L > 32 * kMaxTextSteps) { set_error("region attention: tokens per region must be in [1, 160]"); return 4; }
    int seg = 0;
    switch (d) {
        case 32: seg = region_seg_bytes(32, 32); break;
        case 40: seg = region_seg_bytes(40, 32); break;
        case 64: seg = region_seg_bytes(64, 32); break;
        case 80: seg = region_seg_bytes(80, 32); break;
        default: seg = region_seg_bytes(160, 32); break;
    }
    seg *= (L + 31) / 32;
    const int fit = (kRegionLds - kRegionTailBytes) / seg;        // >= 1: one 160-key segment at d = 160 is 112.6 KB
    const int groups = (R + fit - 1) / fit;
    const int per = (R + groups - 1) / groups;
    if (pl) {
        pl->seg_per_group = per;
        pl->groups = groups;
        pl->lds_bytes = per * seg + kRegionTailBytes;
        pl->seg_bytes = seg;
    }
    return 0;
}

long region_level_offset(int Bw, int R, int H, int W, int level) {
    long off = 0;
    for (int l = 0; l < level; ++l) off += (long)Bw * (H >> l) * (W >> l) * R;
    return off;
}

int launch_region_pyramid(const float* w, float* out, int Bw, int R, int H, int W, int levels, hipStream_t s) {
    if (!w || !out) { set_error("region pyramid: null argument"); return 1; }
    if (Bw < 1 || R < 1 || R > kRegionMax || H < 1 || W < 1 || levels < 1 || levels > 4) {
        set_error("region pyramid: Bw, H, W >= 1, R in [1, 8] and levels in [1, 4] required");
        return 1;
    }
    const int div = 1 << (levels - 1);
    if (H % div != 0 || W % div != 0) { set_error("region pyramid: H and W must be divisible by 2^(levels-1)"); return 1; }
    const long total = region_level_offset(Bw, R, H, W, levels);
    hipLaunchKernelGGL(region_pyramid_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, w, out, Bw, R, H, W, levels,
                       total);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_region_attention(const half_t* q, const half_t* k, const half_t* v, const float* w, half_t* out, int B, int Tq,
                            int L, int R, int heads, int d, long ldq, long ldk, long ldv, long ldo, int Bw, int prescaled,
                            hipStream_t s) {
    if (!q || !k || !v || !w || !out) { set_error("region attention: null argument"); return 1; }
    if ((ldq | ldk | ldv | ldo) % 8 != 0) { set_error("region attention: row strides must be multiples of 8"); return 1; }
    if (Bw < 1 || (B > 0 && B % Bw != 0)) { set_error("region attention: the weights' batch must divide the batch"); return 1; }
    RegionPlan pl;
    if (int rc = region_plan(R, L, d, &pl)) return rc;
    if (B <= 0 || Tq <= 0 || heads <= 0) return 0;
    const bool ps = prescaled != 0;
    // grouped launches restage K / V for every query tile: eight waves (128 queries) per block halve that traffic
    if (pl.groups > 1) {
        switch (d) {
            case 32: return launch_region<32, 1, 8>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
            case 40: return launch_region<40, 1, 8>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
            case 64: return launch_region<64, 1, 8>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
            case 80: return launch_region<80, 1, 8>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
            default: return launch_region<160, 1, 8>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
        }
    }
    switch (d) {
        case 32: return launch_region<32, 1, 4>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
        case 40: return launch_region<40, 1, 4>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
        case 64: return launch_region<64, 1, 4>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
        case 80: return launch_region<80, 1, 4>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
        default: return launch_region<160, 1, 4>(q, k, v, w, out, B, Tq, L, R, heads, ldq, ldk, ldv, ldo, Bw, ps, pl, s);
    }
}

}  // namespace sd
