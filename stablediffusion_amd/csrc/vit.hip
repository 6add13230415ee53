// CLIPVisionEmbeddings (transformers modeling_clip.py) in one launch: the stride-P, P x P patch convolution read straight
// from the NCHW pixels, the class row and the learned position embedding.
//   out[b, 0, :]     = class_embedding + pos[0]
//   out[b, 1 + n, :] = sum_k patch(b, n)[k] * W[:, k] + pos[1 + n],   k = (c, ph, pw), K = 3 P^2
// W is the raw conv weight [H][3][P][P] (no bias), whose flat row is already in k order, so nothing is packed and no
// im2col buffer exists.  K = 588 at P = 14 is no multiple of the 32-wide MFMA step: the last K chunk is zero-filled in
// LDS.  fp32 accumulation on v_mfma_f32_16x16x32_f16, the position row added in fp32, one fp16 rounding at the store.
#include "kernels.h"

namespace sd {

namespace {

constexpr int VBM = 64, VBN = 64, VBK = 32;
constexpr int VLD = VBK + 8;        // LDS row stride in halves: 80 bytes, keeps the 16-byte fragment reads aligned

__global__ __launch_bounds__(256) void vit_patch_embed_kernel(const half_t* __restrict__ px, const half_t* __restrict__ w,
                                                              const half_t* __restrict__ cls, const half_t* __restrict__ pos,
                                                              half_t* __restrict__ out, long ld, int B, int S, int P, int H) {
    __shared__ __attribute__((aligned(16))) half_t sA[VBM * VLD];
    __shared__ __attribute__((aligned(16))) half_t sB[VBN * VLD];

    const int G = S / P, N = G * G, PP = P * P, K = 3 * PP;
    const int M = B * N;
    const int tiles_n = (H + VBN - 1) / VBN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * VBM, n0 = tn * VBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // the class row of every image: written by the first row tile of each column tile
    if (tm == 0) {
        for (int idx = tid; idx < B * VBN; idx += 256) {
            const int b = idx / VBN, n = n0 + (idx - b * VBN);
            if (n < H) out[(long)b * (1 + N) * ld + n] = (half_t)((float)cls[n] + (float)pos[n]);
        }
    }

    // staging: thread -> (tile row, 8 consecutive k) of both operands
    const int lr = tid >> 2, lk = (tid & 3) * 8;
    const int am = m0 + lr;
    const bool a_ok = am < M;
    long a_base = 0;                 // offset of the patch's first pixel in channel 0
    if (a_ok) {
        const int b = am / N, pn = am - b * N;
        const int py = pn / G, pxn = pn - py * G;
        a_base = ((long)b * 3 * S + (long)py * P) * S + (long)pxn * P;
    }
    const int bn = n0 + lr;
    const bool b_ok = bn < H;
    const half_t* wrow = w + (long)(b_ok ? bn : 0) * K;

    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    for (int k0 = 0; k0 < K; k0 += VBK) {
        h8 va = {0, 0, 0, 0, 0, 0, 0, 0}, vb = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + lk + e;
            if (k < K) {
                if (a_ok) {
                    const int c = k / PP, r = k - c * PP;
                    const int ph = r / P, pw = r - ph * P;
                    va[e] = px[a_base + ((long)c * S + ph) * S + pw];
                }
                if (b_ok) vb[e] = wrow[k];
            }
        }
        __syncthreads();            // the previous chunk's fragment reads are done
        *reinterpret_cast<h8*>(sA + lr * VLD + lk) = va;
        *reinterpret_cast<h8*>(sB + lr * VLD + lk) = vb;
        __syncthreads();
        h8 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const h8*>(sA + (wm * 32 + i * 16 + fr) * VLD + fq * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const h8*>(sB + (wn * 32 + j * 16 + fr) * VLD + fq * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }

    // acc[i][j][e]: patch row wm*32 + i*16 + fr, hidden column wn*32 + j*16 + fq*4 + e
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 32 + i * 16 + fr;
        if (m >= M) continue;
        const int b = m / N, pn = m - b * N;
        const long orow = ((long)b * (1 + N) + 1 + pn) * ld;
        const half_t* prow = pos + (long)(1 + pn) * H;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * 32 + j * 16 + fq * 4;
            if (n >= H) continue;   // H % 8 == 0: a group of four columns is inside or outside as a whole
            const h4 pv = *reinterpret_cast<const h4*>(prow + n);
            const f4 v = acc[i][j];
            const h4 o = {(half_t)(v[0] + (float)pv[0]), (half_t)(v[1] + (float)pv[1]), (half_t)(v[2] + (float)pv[2]),
                          (half_t)(v[3] + (float)pv[3])};
            *reinterpret_cast<h4*>(out + orow + n) = o;
        }
    }
}

}  // namespace

int launch_vit_patch_embed(const half_t* pixels, const half_t* w, const half_t* cls, const half_t* pos, half_t* out, long ld,
                           int B, int S, int P, int H, hipStream_t s) {
    if (B <= 0 || S <= 0 || P <= 0 || S % P != 0 || H <= 0 || H % 8 != 0 || ld < H || ld % 8 != 0) {
        set_error("vit_patch_embed: needs B > 0, S % P == 0, H % 8 == 0 and a row stride >= H that is a multiple of 8");
        return 1;
    }
    const long M = (long)B * (S / P) * (S / P);
    const long tiles = (long)cdiv(M, VBM) * cdiv(H, VBN);
    if (tiles >= (1L << 31)) { set_error("vit_patch_embed: problem too large"); return 1; }
    hipLaunchKernelGGL(vit_patch_embed_kernel, dim3((unsigned)tiles), dim3(256), 0, s, pixels, w, cls, pos, out, ld, B, S, P, H);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
