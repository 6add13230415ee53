// Tiled VAE (diffusers 0.27.2 AutoencoderKL.tiled_decode / tiled_encode / blend_v / blend_h): a canvas too large for one
// decode or encode is cut into overlapping tiles, every tile goes through the unchanged decoder / encoder at its own size,
// and the outputs are cross-faded over `blend` rows / columns and cropped to `limit`.  Three pieces live here: the plan
// (host only), the gather that stacks tiles of one shape for a chunk, and the merge.
//
// The merge is one launch per output canvas and writes every pixel once, from the raw tiles.  diffusers blends in place
// in raster order: tile (iy, ix) first takes its top `ev` rows from the tile above (as that one stands after its own
// blends), then its left `eh` columns from the tile to its left (likewise).  With blend <= tile / 2 the rows and columns a
// neighbour lends (its bottom-most ev rows, its right-most eh columns) lie outside that neighbour's own blended strips
// but for one case each -- the lent rows of the tile above inside ITS left strip, the lent columns of the left tile inside
// ITS top strip -- and both of those resolve to the raw above-left tile.  So, with b the tile whose crop holds the pixel,
// A / L / AL the raw tiles above / left / above-left, ty = y / ev and tx = x / eh inside the strips:
//     out = lerp_x( lerp_y(AL, L), lerp_y( lerp_x(AL, A), b ) ),     lerp(p, q, t) = p (1 - t) + q t
// where a lerp whose strip the pixel is not in passes its second operand through unread (DESIGN.md section 4 derives it).
//
// Geometry in closed form (nothing to upload): tile k of an axis of output length L starts at k limit, has size
// min(T, L - k limit); every tile is full-size but at most the last two, so an axis has at most three sizes and the
// canvas at most nine shape classes.  The stack holds the classes one after the other, a class's tiles in raster order,
// each tile's B images together: [class][tile][b][C][th][tw].
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "model.h"

namespace sd {
namespace {

struct AxisPos { int k, p, size, e, prev; };
// where output coordinate P falls: tile k, offset p in it, that tile's size, the blend extent with the tile in front of it
// (0 for the first) and that tile's size
__device__ __forceinline__ AxisPos axis_pos(int P, int L, int T, int blend, int limit) {
    AxisPos a;
    a.k = P / limit;
    a.p = P - a.k * limit;
    const int rest = L - a.k * limit;
    a.size = rest < T ? rest : T;
    a.e = a.k > 0 ? (a.size < blend ? a.size : blend) : 0;       // (the tile in front is always larger than blend)
    a.prev = rest + limit < T ? rest + limit : T;
    return a;
}
// element offset of image b of tile (iy, ix), of shape [C, th, tw], in the stack
__device__ __forceinline__ long tile_base(const VaeMergeGeom& g, int iy, int ix, int th, int tw, int b) {
    const int cy = iy < g.nfy ? 0 : 1 + iy - g.nfy, ry = iy < g.nfy ? iy : 0;
    const int cx = ix < g.nfx ? 0 : 1 + ix - g.nfx, rx = ix < g.nfx ? ix : 0;
    const int cols = cx == 0 ? g.nfx : 1;
    return g.cls_off[cy * 3 + cx] + (((long)ry * cols + rx) * g.B + b) * ((long)g.C * th * tw);
}

template <int E>
__device__ __forceinline__ void load_e(const half_t* p, float* v) {
    if (E == 8) {
        const h8 t = *reinterpret_cast<const h8*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
    } else {
        v[0] = (float)*p;
    }
}
__device__ __forceinline__ float lerp1(float p, float q, float t) { return p * (1.0f - t) + q * t; }

// One thread owns E consecutive X of one (b, c, Y) of the canvas (row stride ld).  fp32 lerps, one rounding to fp16.
template <bool VEC>
__global__ __launch_bounds__(256) void vae_tile_merge_kernel(const half_t* __restrict__ tiles, half_t* __restrict__ canvas,
                                                             const VaeMergeGeom g, long ld, long total) {
    constexpr int E = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Wq = g.Wo / E;
    long r = i / Wq;
    const int X = (int)(i - r * Wq) * E;
    const int Y = (int)(r % g.Ho); r /= g.Ho;
    const int c = (int)(r % g.C);
    const int b = (int)(r / g.C);
    const AxisPos ay = axis_pos(Y, g.Ho, g.T, g.blend, g.limit);
    const AxisPos ax = axis_pos(X, g.Wo, g.T, g.blend, g.limit);
    const int th = ay.size, tw = ax.size, ah = ay.prev, lw = ax.prev;
    const bool inY = ay.p < ay.e, inX = ax.p < ax.e;            // (VEC: eh and x are multiples of 8, so the 8 agree)
    const int ar = ah - ay.e + ay.p;                            // the lending row of the tiles above
    const int lc = lw - ax.e + ax.p;                            // the lending column of the tiles to the left

    float o[E];
    load_e<E>(tiles + tile_base(g, ay.k, ax.k, th, tw, b) + ((long)c * th + ay.p) * tw + ax.p, o);
    const float ty = inY ? (float)ay.p / (float)ay.e : 0.f;
    float tx[E];
#pragma unroll
    for (int j = 0; j < E; ++j) tx[j] = inX ? (float)(ax.p + j) / (float)ax.e : 0.f;
    float al[E];
    if (inY && inX) load_e<E>(tiles + tile_base(g, ay.k - 1, ax.k - 1, ah, lw, b) + ((long)c * ah + ar) * lw + lc, al);
    if (inY) {
        float top[E];
        load_e<E>(tiles + tile_base(g, ay.k - 1, ax.k, ah, tw, b) + ((long)c * ah + ar) * tw + ax.p, top);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (inX) top[j] = lerp1(al[j], top[j], tx[j]);
            o[j] = lerp1(top[j], o[j], ty);
        }
    }
    if (inX) {
        float left[E];
        load_e<E>(tiles + tile_base(g, ay.k, ax.k - 1, th, lw, b) + ((long)c * th + ay.p) * lw + lc, left);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (inY) left[j] = lerp1(al[j], left[j], ty);
            o[j] = lerp1(left[j], o[j], tx[j]);
        }
    }
    half_t* dst = canvas + (((long)b * g.C + c) * g.Ho + Y) * ld + X;
    if (VEC) {
        h8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (half_t)o[j];
        *reinterpret_cast<h8*>(dst) = v;
    } else {
        *dst = (half_t)o[0];
    }
}

// stack[i, c, y, x] = canvas[b_i, c, ys_i + y, xs_i + x]: image i of the chunk is one tile of one canvas image; a pure copy.
template <bool VEC>
__global__ __launch_bounds__(256) void vae_tile_gather_kernel(const half_t* __restrict__ canvas, half_t* __restrict__ stack,
                                                              const VaeGatherList l, int C, int Hc, long ld, int th, int tw,
                                                              long total) {
    constexpr int E = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int wq = tw / E;
    long r = i / wq;
    const int x = (int)(i - r * wq) * E;
    const int y = (int)(r % th); r /= th;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const half_t* src = canvas + (((long)l.b[n] * C + c) * Hc + l.ys[n] + y) * ld + l.xs[n] + x;
    if (VEC) *reinterpret_cast<h8*>(stack + i * 8) = *reinterpret_cast<const h8*>(src);
    else stack[i] = *src;
}

inline bool aligned16(const void* a, const void* b) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// sizes of one axis: tile k of `n`, input space
inline int axis_size(int k, int L, int tile, int stride) { return L - k * stride < tile ? L - k * stride : tile; }

}  // namespace

namespace {
// The plan from diffusers' integers; every relation the kernels rest on is checked here, so that a plan handed back in
// through the operator entries can be verified by rebuilding it (vae_tile_plan_valid).
int plan_from_ints(bool encode, int h, int w, int tin, int stride, int tout, int blend, int scale, sd_vae_tiles* out) {
    if (h < 1 || w < 1 || tin < 1 || tout < 1 || scale < 1 || (encode ? (long)tout * scale != tin : (long)tin * scale != tout)) {
        set_error("sd_vae_tile_plan: non-positive size"); return 1;
    }
    if (stride < 1 || stride > tin) { set_error("sd_vae_tile_plan: the tiles' starts do not advance"); return 1; }
    if (blend < 0 || 2 * blend > tout) { set_error("sd_vae_tile_plan: blend extent above half a tile"); return 1; }
    const int limit = tout - blend;
    // the crops must tile the output canvas: a start `stride` further in is a crop `limit` further out
    const bool fits = encode ? (stride % scale == 0 && stride / scale == limit && h % scale == 0 && w % scale == 0)
                             : (long)stride * scale == limit;
    if (!fits) {
        set_error("sd_vae_tile_plan: the cropped tiles do not tile the canvas (int(tile (1 - f)) and tile - int(tile f) "
                  "disagree between latent and sample space, or an image size is no multiple of the VAE's scale)");
        return 1;
    }
    const long ny = ((long)h + stride - 1) / stride, nx = ((long)w + stride - 1) / stride;
    if (ny > SD_VAE_TILE_MAX_AXIS || nx > SD_VAE_TILE_MAX_AXIS) {
        set_error("sd_vae_tile_plan: more than 64 tiles on one axis"); return 1;
    }
    sd_vae_tiles p = {};
    p.ny = (int)ny; p.nx = (int)nx;
    p.tile_in = tin; p.stride_in = stride; p.tile_out = tout; p.blend = blend; p.limit = limit; p.scale = scale;
    p.in_h = h; p.in_w = w;
    p.out_h = encode ? h / scale : h * scale;
    p.out_w = encode ? w / scale : w * scale;
    for (int k = 0; k < p.ny; ++k) p.size_y[k] = axis_size(k, h, tin, stride);
    for (int k = 0; k < p.nx; ++k) p.size_x[k] = axis_size(k, w, tin, stride);
    // runs of equal size along each axis: sizes never grow, and since 2 stride >= tile_in (blend <= tile_out / 2) only
    // the last two tiles can be truncated, so there are at most three runs
    int y0[4], x0[4], nry = 0, nrx = 0;
    for (int k = 0; k < p.ny; ++k) if (k == 0 || p.size_y[k] != p.size_y[k - 1]) y0[nry++] = k;
    for (int k = 0; k < p.nx; ++k) if (k == 0 || p.size_x[k] != p.size_x[k - 1]) x0[nrx++] = k;
    y0[nry] = p.ny; x0[nrx] = p.nx;
    for (int a = 0; a < nry; ++a)
        for (int b = 0; b < nrx; ++b) {
            const int c = p.n_classes++;
            p.class_iy0[c] = y0[a]; p.class_ny[c] = y0[a + 1] - y0[a];
            p.class_ix0[c] = x0[b]; p.class_nx[c] = x0[b + 1] - x0[b];
            p.class_h[c] = p.size_y[y0[a]]; p.class_w[c] = p.size_x[x0[b]];
            p.class_count[c] = p.class_ny[c] * p.class_nx[c];
        }
    *out = p;
    return 0;
}
}  // namespace

int vae_tile_plan(int encode, int h, int w, int tile_sample, int tile_latent, double f, sd_vae_tiles* out) {
    if (!out) { set_error("sd_vae_tile_plan: null plan"); return 1; }
    if (tile_sample < 1 || tile_latent < 1) { set_error("sd_vae_tile_plan: non-positive size"); return 1; }
    if (!(f >= 0.0 && f <= 0.5)) { set_error("sd_vae_tile_plan: tile_overlap_factor outside [0, 0.5]"); return 1; }
    if (tile_sample % tile_latent != 0) {
        set_error("sd_vae_tile_plan: tile_sample_min_size must be a multiple of tile_latent_min_size"); return 1;
    }
    const int tin = encode ? tile_sample : tile_latent, tout = encode ? tile_latent : tile_sample;
    // diffusers' integers: overlap_size = int(tile_in (1 - f)), blend_extent = int(tile_out f), row_limit = tile_out - blend
    return plan_from_ints(encode != 0, h, w, tin, (int)((double)tin * (1.0 - f)), tout, (int)((double)tout * f),
                          tile_sample / tile_latent, out);
}

bool vae_tile_plan_valid(const sd_vae_tiles& p) {
    sd_vae_tiles q;
    if (plan_from_ints(p.tile_out < p.tile_in, p.in_h, p.in_w, p.tile_in, p.stride_in, p.tile_out, p.blend, p.scale, &q)) return false;
    return memcmp(&p, &q, sizeof(q)) == 0;
}

long vae_tile_stack(const sd_vae_tiles& p, int B, int C, VaeMergeGeom* g, long* class_off) {
    VaeMergeGeom m = {};
    m.Ho = p.out_h; m.Wo = p.out_w; m.T = p.tile_out; m.blend = p.blend; m.limit = p.limit; m.B = B; m.C = C;
    // full-size tiles in front on each axis
    for (int k = 0; k < p.ny && p.size_y[k] == p.tile_in; ++k) m.nfy = k + 1;
    for (int k = 0; k < p.nx && p.size_x[k] == p.tile_in; ++k) m.nfx = k + 1;
    const bool enc = p.tile_out < p.tile_in;
    long off = 0;
    for (int c = 0; c < p.n_classes; ++c) {
        const int oh = enc ? p.class_h[c] / p.scale : p.class_h[c] * p.scale;
        const int ow = enc ? p.class_w[c] / p.scale : p.class_w[c] * p.scale;
        const int cy = p.class_iy0[c] < m.nfy ? 0 : 1 + p.class_iy0[c] - m.nfy;
        const int cx = p.class_ix0[c] < m.nfx ? 0 : 1 + p.class_ix0[c] - m.nfx;
        m.cls_off[cy * 3 + cx] = off;
        if (class_off) class_off[c] = off;
        off += (long)p.class_count[c] * B * C * oh * ow;
    }
    if (g) *g = m;
    return off;
}

int launch_vae_tile_gather(const half_t* canvas, long ld, half_t* stack, const VaeGatherList& l, int n, int C, int Hc,
                           int th, int tw, hipStream_t s) {
    bool vec = tw % 8 == 0 && ld % 8 == 0 && aligned16(canvas, stack);
    for (int i = 0; i < n && vec; ++i) vec = l.xs[i] % 8 == 0;
    const long total = (long)n * C * th * (vec ? tw / 8 : tw);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("vae_tile_gather: too many elements for one launch"); return 1; }
    const dim3 grid((unsigned)blocks);
    if (vec) hipLaunchKernelGGL(vae_tile_gather_kernel<true>, grid, dim3(256), 0, s, canvas, stack, l, C, Hc, ld, th, tw, total);
    else hipLaunchKernelGGL(vae_tile_gather_kernel<false>, grid, dim3(256), 0, s, canvas, stack, l, C, Hc, ld, th, tw, total);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_vae_tile_merge(const half_t* tiles, half_t* canvas, long ld, const VaeMergeGeom& g, hipStream_t s) {
    // 8 columns share a tile and a side of every strip, and every row they touch starts 16-byte aligned
    const bool vec = g.T % 8 == 0 && g.blend % 8 == 0 && g.limit % 8 == 0 && g.Wo % 8 == 0 && ld % 8 == 0 &&
                     aligned16(tiles, canvas);
    const long total = (long)g.B * g.C * g.Ho * (vec ? g.Wo / 8 : g.Wo);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("vae_tile_merge: too many elements for one launch"); return 1; }
    const dim3 grid((unsigned)blocks);
    if (vec) hipLaunchKernelGGL(vae_tile_merge_kernel<true>, grid, dim3(256), 0, s, tiles, canvas, g, ld, total);
    else hipLaunchKernelGGL(vae_tile_merge_kernel<false>, grid, dim3(256), 0, s, tiles, canvas, g, ld, total);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
