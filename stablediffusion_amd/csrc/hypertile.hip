// HyperTile (sd_unet_set_hypertile): self-attention restricted to the tokens of one spatial tile.  The attention kernel
// wants the tokens of one sequence in consecutive rows, so the q|k|v rows of an Hs x Ws map are brought into tile order
// in front of it and its output back into raster order behind it:
//
//   hypertile_gather_kernel   dst row ((b nh + ty) nw + tx) th tw + y tw + x  <-  src row (b Hs + ty th + y) Ws + tx tw + x
//   hypertile_scatter_kernel  the inverse map
//
// Both are pure fp16 copies of `cols` columns with 16 bytes per lane; src and dst have their own row strides, and
// nothing outside the `cols` columns or beyond the last row is touched.  A group of `lpr` lanes (a power of two, picked
// on the host so that few lanes idle on the row's last pass) owns one row: the row index is taken apart once, then the
// group walks the row's 16-byte pieces, four of them in flight per lane.
//
// The division itself (hypertile_counts / hypertile_plan) is host arithmetic on the counter hash of the token-merging
// plan (kernels.h: mix32).
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace sd {

int hypertile_counts(int n, int tile_size, int swap_size, int* counts) {
    if (n < 1 || tile_size < 1 || swap_size < 1 || swap_size > kHyperTileMaxSwap) return 0;
    const int m = tile_size < n ? tile_size : n;
    int k = 0;
    for (int e = m; e <= n && k < swap_size; ++e)
        if (n % e == 0) counts[k++] = n / e;
    return k;                                                   // >= 1: e = n always divides
}

int hypertile_plan(int Hs, int Ws, int tile_size, int swap_size, uint32_t seed, uint32_t step, uint32_t site, HyperTileGeom* g) {
    int ch[kHyperTileMaxSwap], cw[kHyperTileMaxSwap];
    const int kh = hypertile_counts(Hs, tile_size, swap_size, ch), kw = hypertile_counts(Ws, tile_size, swap_size, cw);
    if (kh < 1 || kw < 1 || (long)Hs * Ws > (1L << 24)) {
        set_error("hypertile: needs Hs, Ws >= 1 (Hs Ws <= 2^24), tile_size >= 1 and swap_size in 1..8");
        return 1;
    }
    g->Hs = Hs; g->Ws = Ws;
    g->nh = ch[mix32(seed, step, site, 0u) % (uint32_t)kh];
    g->nw = cw[mix32(seed, step, site, 1u) % (uint32_t)kw];
    g->th = Hs / g->nh; g->tw = Ws / g->nw;
    return 0;
}

namespace {

// tile-order row r of the B Hs Ws rows -> its raster-order row
__device__ inline unsigned hypertile_raster_row(unsigned r, const HyperTileGeom& g) {
    const unsigned tt = (unsigned)(g.th * g.tw);
    const unsigned tile = r / tt, i = r - tile * tt;
    const unsigned y = i / (unsigned)g.tw, x = i - y * (unsigned)g.tw;
    const unsigned q = tile / (unsigned)g.nw, tx = tile - q * (unsigned)g.nw;
    const unsigned b = q / (unsigned)g.nh, ty = q - b * (unsigned)g.nh;
    return (b * (unsigned)g.Hs + ty * (unsigned)g.th + y) * (unsigned)g.Ws + tx * (unsigned)g.tw + x;
}

template <bool SCATTER>
__device__ inline void hypertile_copy(const half_t* __restrict__ src, long lds, half_t* __restrict__ dst, long ldd, int nv,
                                      int lpr_log2, unsigned rows, const HyperTileGeom& g) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = gi >> lpr_log2;
    if (row >= (long)rows) return;
    const int lpr = 1 << lpr_log2;
    const int lane = (int)(gi & (lpr - 1));
    const unsigned r = (unsigned)row, p = hypertile_raster_row(r, g);
    const h8* s = reinterpret_cast<const h8*>(src + (long)(SCATTER ? r : p) * lds);
    h8* d = reinterpret_cast<h8*>(dst + (long)(SCATTER ? p : r) * ldd);
    for (int v = lane; v < nv; v += 4 * lpr) {
        const int v1 = v + lpr, v2 = v + 2 * lpr, v3 = v + 3 * lpr;
        h8 a0 = s[v], a1 = a0, a2 = a0, a3 = a0;
        if (v1 < nv) a1 = s[v1];
        if (v2 < nv) a2 = s[v2];
        if (v3 < nv) a3 = s[v3];
        d[v] = a0;
        if (v1 < nv) d[v1] = a1;
        if (v2 < nv) d[v2] = a2;
        if (v3 < nv) d[v3] = a3;
    }
}

__global__ __launch_bounds__(256) void hypertile_gather_kernel(const half_t* __restrict__ src, long lds, half_t* __restrict__ dst,
                                                               long ldd, int nv, int lpr_log2, unsigned rows, HyperTileGeom g) {
    hypertile_copy<false>(src, lds, dst, ldd, nv, lpr_log2, rows, g);
}
__global__ __launch_bounds__(256) void hypertile_scatter_kernel(const half_t* __restrict__ src, long lds, half_t* __restrict__ dst,
                                                                long ldd, int nv, int lpr_log2, unsigned rows, HyperTileGeom g) {
    hypertile_copy<true>(src, lds, dst, ldd, nv, lpr_log2, rows, g);
}

// lanes per row: the widest of 64 / 32 / 16 / 8 that keeps at least 90 % of its lanes busy over the row's passes, else the
// one that keeps the most
int hypertile_lpr_log2(int nv) {
    int best = 6;
    double best_eff = 0.0;
    for (int l = 6; l >= 3; --l) {
        const int lpr = 1 << l;
        const double eff = (double)nv / (double)(((nv + lpr - 1) / lpr) * lpr);
        if (eff >= 0.9) return l;
        if (eff > best_eff) { best_eff = eff; best = l; }
    }
    return best;
}

int hypertile_launch(bool scatter, const half_t* src, long lds, int cols, int B, int Hs, int Ws, int nh, int nw, half_t* dst,
                     long ldd, hipStream_t s) {
    const char* const who = scatter ? "hypertile_scatter" : "hypertile_gather";
    if (!src || !dst || B < 1 || Hs < 1 || Ws < 1 || nh < 1 || nw < 1 || cols < 8 || cols % 8 != 0 || lds < cols || ldd < cols ||
        lds % 8 != 0 || ldd % 8 != 0 || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) != 0) {
        set_error(std::string(who) + ": needs B, nh, nw >= 1, cols a multiple of 8, both row strides at least cols and "
                  "multiples of 8, 16-byte aligned pointers");
        return 1;
    }
    if (Hs % nh != 0 || Ws % nw != 0) { set_error(std::string(who) + ": nh must divide Hs and nw must divide Ws"); return 1; }
    const long rows = (long)B * Hs * Ws;
    const int nv = cols / 8, l = hypertile_lpr_log2(nv);
    const long blocks = ((rows << l) + 255) / 256;
    if (rows >= (1L << 31) || blocks > 0x7fffffffL) { set_error(std::string(who) + ": too many rows for one launch"); return 1; }
    HyperTileGeom g;
    g.Hs = Hs; g.Ws = Ws; g.nh = nh; g.nw = nw; g.th = Hs / nh; g.tw = Ws / nw;
    if (scatter) hipLaunchKernelGGL(hypertile_scatter_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, dst, ldd, nv, l, (unsigned)rows, g);
    else hipLaunchKernelGGL(hypertile_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, lds, dst, ldd, nv, l, (unsigned)rows, g);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int launch_hypertile_gather(const half_t* src, long lds, int cols, int B, int Hs, int Ws, int nh, int nw, half_t* dst, long ldd,
                            hipStream_t s) {
    return hypertile_launch(false, src, lds, cols, B, Hs, Ws, nh, nw, dst, ldd, s);
}

int launch_hypertile_scatter(const half_t* src, long lds, int cols, int B, int Hs, int Ws, int nh, int nw, half_t* dst, long ldd,
                             hipStream_t s) {
    return hypertile_launch(true, src, lds, cols, B, Hs, Ws, nh, nw, dst, ldd, s);
}

}  // namespace sd
