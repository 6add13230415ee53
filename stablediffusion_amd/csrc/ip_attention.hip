// Decoupled cross-attention of IP-Adapter for gfx950 (CDNA4, wave64), one launch per attn2 site:
//   out = softmax(s q K_t^T) V_t + lambda * softmax(s q K_ip^T) V_ip
// fp16 in/out, fp32 scores and accumulators.  diffusers 0.27.2 IPAdapterAttnProcessor2_0 computes the same
// thing as two scaled_dot_product_attention calls and an add; here the IP branch costs a few more MFMAs on
// queries that are already in registers, and the output is written once.
//
// Both key sets are short (text L <= 154 -- 77 in practice --, image tokens T_ip <= 64), so unlike the streaming
// attn_kernel (attention.hip) this kernel:
//   * stages ALL keys and values of one (batch, head) -- text and image -- into LDS once per block, zero-padded to
//     multiples of 32 keys, and runs several query tiles against them (the block loops over its share of tiles);
//   * computes each softmax exactly: max over the whole segment, exp, row sum, no running max and no rescale.  The
//     probabilities are normalised (times lambda for the image segment) BEFORE they are rounded to fp16 and fed to
//     the PV product, so both segments accumulate into one set of fp32 output registers and nothing is left to
//     divide at the end.
// Shared with attention.hip: the swapped products S^T = K Q^T (a query's scores sit in one lane column, so the
// softmax needs two cross-lane reductions and nothing else), P^T taken straight from the S^T accumulators as the B
// operand of O^T = V^T P^T, V^T read with ds_read_b64_tr_b16 from row-major V, odd-multiple-of-32-byte LDS row
// strides (conflict-free fragment and transposed reads), 16x16x32 MFMAs.  The ones-column denominator is not used:
// the exact softmax has its sum before the PV product.
// lambda == 0 skips the image segment (wave-uniform branch): the result is the text attention alone.
#include "ip_attention_blocks.h"

namespace sd {
namespace {

// Grid: B * heads * qblocks blocks, (batch, head) slow, pushed through the XCD remap so that the blocks of one
// (batch, head) share one L2.  Block: NWV waves x 16 QT queries per tile; the block walks the query tiles
// qblk, qblk + qblocks, ... against the K / V it staged once.
template <int D, int QT, int NWV>
__global__ __launch_bounds__(64 * NWV) void ip_xattn_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k,
                                                        const half_t* __restrict__ v, const half_t* __restrict__ kip,
                                                        const half_t* __restrict__ vip, half_t* __restrict__ out,
                                                        int Tq, int L, int Tip, int heads, long ldq, long ldk, long ldv,
                                                        long ldki, long ldvi, long ldo, float scale_log2e, float lam,
                                                        int qblocks) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KS = (D + 31) / 32;
    constexpr int DT = (D + 15) / 16;
    constexpr int KSTR = ip_kstr(D), VSTR = ip_vstr(D);
    constexpr int QB = 16 * QT * NWV;
    constexpr int NTH = 64 * NWV;
    const int nkt = (L + 31) / 32, nki = (Tip + 31) / 32;
    const int rows_t = nkt * 32, rows_i = nki * 32;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sKt = reinterpret_cast<half_t*>(smem);
    half_t* sVt = sKt + rows_t * KSTR;
    half_t* sKi = sVt + rows_t * VSTR;
    half_t* sVi = sKi + rows_i * KSTR;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int bh = bid / qblocks, qblk = bid - bh * qblocks;
    const int b = bh / heads, h = bh - b * heads;
    const bool with_ip = lam != 0.f;

    stage_rows<D>(sKt, KSTR, k + (long)b * L * ldk + h * D, ldk, L, rows_t, tid, NTH);
    stage_rows<D>(sVt, VSTR, v + (long)b * L * ldv + h * D, ldv, L, rows_t, tid, NTH);
    if (with_ip) {
        stage_rows<D>(sKi, KSTR, kip + (long)b * Tip * ldki + h * D, ldki, Tip, rows_i, tid, NTH);
        stage_rows<D>(sVi, VSTR, vip + (long)b * Tip * ldvi + h * D, ldvi, Tip, rows_i, tid, NTH);
    }
    __syncthreads();

    const half_t* qb = q + (long)b * Tq * ldq + h * D;
    half_t* ob = out + (long)b * Tq * ldo + h * D;
    const int qtiles = (Tq + QB - 1) / QB;
    for (int qt = qblk; qt < qtiles; qt += qblocks) {
        const int q0 = qt * QB + wave * 16 * QT;
        if (q0 >= Tq) break;                 // wave-uniform; no barrier below
        h8 qf[QT][KS];
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
        }
        f4 o[DT][QT];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int t = 0; t < QT; ++t) o[i][t] = f4{0.f, 0.f, 0.f, 0.f};
        ip_segment<D, QT, kMaxTextSteps>(sKt, sVt, L, nkt, 1.f, scale_log2e, qf, o, fr, fq);
        if (with_ip) ip_segment<D, QT, kMaxIpSteps>(sKi, sVi, Tip, nki, lam, scale_log2e, qf, o, fr, fq);
        // lane holds 4 consecutive d of one query
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int qi = q0 + t * 16 + fr;
#pragma unroll
            for (int i = 0; i < DT; ++i) {
                const int dd = i * 16 + fq * 4;
                if (qi < Tq && dd < D) {
                    const f4 val = o[i][t];
                    h4 w = {(half_t)val[0], (half_t)val[1], (half_t)val[2], (half_t)val[3]};
                    *reinterpret_cast<h4*>(ob + (long)qi * ldo + dd) = w;
                }
            }
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}

// Every instantiation below runs 16 * kIpQT * kIpNWV = 64 queries per block tile.
constexpr int kIpQT = 1, kIpNWV = 4;

template <int D>
int launch_ip(const IpPlan& pl, const half_t* q, const half_t* k, const half_t* v, const half_t* kip, const half_t* vip,
              half_t* out, int B, int Tq, int L, int Tip, int heads, long ldq, long ldk, long ldv, long ldki, long ldvi,
              long ldo, float lam, bool prescaled, hipStream_t s) {
    constexpr int STR = ip_kstr(D) + ip_vstr(D);
    constexpr size_t lds_max = (size_t)32 * (kMaxTextSteps + kMaxIpSteps) * STR * 2;
    static_assert(lds_max <= 160 * 1024, "LDS");
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        SD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ip_xattn_kernel<D, kIpQT, kIpNWV>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    }
    const float scale_log2e = prescaled ? 1.0f : 1.4426950408889634f / sqrtf((float)D);
    hipLaunchKernelGGL((ip_xattn_kernel<D, kIpQT, kIpNWV>), dim3((unsigned)((long)B * heads * pl.qblocks)), dim3(64 * kIpNWV),
                       (size_t)pl.lds_bytes, s, q, k, v, kip, vip, out, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo,
                       scale_log2e, lam, pl.qblocks);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

// y += a x on [rows, cols] fp16 slices (cols % 8 == 0): the add of the unfused composition that
// tools/run_ip_attn.py times against the fused kernel
__global__ void axpy_f16_kernel(half_t* __restrict__ y, long ldy, const half_t* __restrict__ x, long ldx, long rows,
                                int cols, float a) {
    const int cpr = cols / 8;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cpr) return;
    const long r = idx / cpr;
    const int c = (int)(idx - r * cpr) * 8;
    const h8 xv = *reinterpret_cast<const h8*>(x + r * ldx + c);
    h8 yv = *reinterpret_cast<const h8*>(y + r * ldy + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) yv[e] = (half_t)((float)yv[e] + a * (float)xv[e]);
    *reinterpret_cast<h8*>(y + r * ldy + c) = yv;
}

}  // namespace

int launch_axpy_f16(half_t* y, long ldy, const half_t* x, long ldx, long rows, int cols, float a, hipStream_t s) {
    if (cols % 8 != 0 || (ldx | ldy) % 8 != 0) { set_error("axpy_f16: cols and strides must be multiples of 8"); return 1; }
    const long n = rows * (cols / 8);
    if (n <= 0) return 0;
    hipLaunchKernelGGL(axpy_f16_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, y, ldy, x, ldx, rows, cols, a);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

bool ip_attention_supported(int d) { return d == 32 || d == 40 || d == 64 || d == 80 || d == 160; }

int ip_attention_plan(int B, int Tq, int L, int Tip, int heads, int d, float ip_scale, IpPlan* pl) {
    *pl = IpPlan();
    if (L < 1 || L > 32 * kMaxTextSteps) { set_error("ip attention: text length must be in [1, 160]"); return 4; }
    if (Tip < 1 || Tip > 32 * kMaxIpSteps) { set_error("ip attention: image tokens must be in [1, 64]"); return 4; }
    if (!(ip_scale == ip_scale)) { set_error("ip attention: scale is NaN"); return 1; }
    if (!ip_attention_supported(d)) { set_error("ip attention: unsupported head dim " + std::to_string(d)); return 4; }
    pl->tile_rows = 16 * kIpQT * kIpNWV;
    if (B <= 0 || Tq <= 0 || heads <= 0) return 0;      // nothing to launch
    // all text keys and values, and the image ones unless ip_scale == 0, in rows padded to 32-key steps
    const int rows = 32 * ((L + 31) / 32) + (ip_scale != 0.f ? 32 * ((Tip + 31) / 32) : 0);
    pl->lds_bytes = rows * (ip_kstr(d) + ip_vstr(d)) * 2;
    // enough blocks for about four per CU, each walking several query tiles against the K / V it staged
    pl->qtiles = cdiv(Tq, pl->tile_rows);
    const long bh = (long)B * heads;
    long qblocks = (1024 + bh - 1) / bh;
    if (qblocks > pl->qtiles) qblocks = pl->qtiles;
    if (qblocks < 1) qblocks = 1;
    pl->qblocks = (int)qblocks;
    return 0;
}

int launch_ip_attention(const half_t* q, const half_t* k, const half_t* v, const half_t* kip, const half_t* vip,
                        half_t* out, int B, int Tq, int L, int Tip, int heads, int d, long ldq, long ldk, long ldv,
                        long ldki, long ldvi, long ldo, float ip_scale, int prescaled, hipStream_t s) {
    if ((ldq | ldk | ldv | ldki | ldvi | ldo) % 8 != 0) { set_error("ip attention: row strides must be multiples of 8"); return 1; }
    if (B <= 0 || Tq <= 0 || heads <= 0) return 0;
    IpPlan pl;
    if (int rc = ip_attention_plan(B, Tq, L, Tip, heads, d, ip_scale, &pl)) return rc;
    const bool ps = prescaled != 0;
    switch (d) {
        case 32: return launch_ip<32>(pl, q, k, v, kip, vip, out, B, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo, ip_scale, ps, s);
        case 40: return launch_ip<40>(pl, q, k, v, kip, vip, out, B, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo, ip_scale, ps, s);
        case 64: return launch_ip<64>(pl, q, k, v, kip, vip, out, B, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo, ip_scale, ps, s);
        case 80: return launch_ip<80>(pl, q, k, v, kip, vip, out, B, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo, ip_scale, ps, s);
        default: return launch_ip<160>(pl, q, k, v, kip, vip, out, B, Tq, L, Tip, heads, ldq, ldk, ldv, ldki, ldvi, ldo, ip_scale, ps, s);
    }
}

}  // namespace sd
