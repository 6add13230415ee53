// MultiDiffusion (Bar-Tal et al. 2023): the denoising loop runs the UNet on overlapping fixed-size windows ("views") of a
// large latent canvas and averages what the windows say where they overlap.  Two memory-bound kernels around the UNet
// forwards: the gather cuts the windows out of the canvas, the merge turns the windows' model outputs into one
// canvas-shaped model output, which every device step of the engine then reads as it reads a plain forward's.
//
// Both kernels come as a vector / scalar pair like pag_step_kernel: one thread per 8 consecutive halves (one 16-byte load
// or store per operand) when the window width, the canvas width and every x start are multiples of 8 and the bases are
// 16-byte aligned -- then a group of 8 columns lies inside or outside a view as a whole, wrapped or not -- and one thread
// per element otherwise.  The starts are launch parameters (ViewStarts, 2 x 64 int): no device table, nothing to upload.
#include <cstdint>

#include "kernels.h"

namespace sd {
namespace {

// windows[(v * B + b), c, y, x] = canvas[b, c, ys[iy] + y, (xs[ix] + x) mod Wc],  v = iy * nx + ix.  E halves per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void view_gather_kernel(const half_t* __restrict__ canvas, half_t* __restrict__ windows,
                                                          const ViewStarts st, int nx, int B, int C, int Hc, int Wc, int h,
                                                          int w, long total) {
    constexpr int E = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int wq = w / E;
    long r = i / wq;
    const int x = (int)(i - r * wq) * E;
    const int y = (int)(r % h); r /= h;
    const int c = (int)(r % C); r /= C;
    const int b = (int)(r % B);
    const int v = (int)(r / B);
    const int iy = v / nx, ix = v - iy * nx;
    int sx = st.xs[ix] + x;
    if (sx >= Wc) sx -= Wc;                          // (wrapped views only: the others end inside the canvas)
    const half_t* src = canvas + (((long)b * C + c) * Hc + st.ys[iy] + y) * Wc + sx;
    if (VEC) *reinterpret_cast<h8*>(windows + i * 8) = *reinterpret_cast<const h8*>(src);
    else windows[i] = *src;
}

// One thread owns E consecutive X of one (g * B + b, c, Y) of the canvas and walks the views that cover them in ascending
// v: a gather over the canvas, no atomics, so the result does not depend on the launch.  fp32 sums of w * e and of w, one
// reciprocal per pixel, one rounding to fp16.
template <bool VEC, bool WT>
__global__ __launch_bounds__(256) void view_merge_kernel(const half_t* __restrict__ mo, half_t* __restrict__ eps,
                                                         const float* __restrict__ wt, const ViewStarts st, int ny, int nx,
                                                         int wrap, int G, int B, int C, int Hc, int Wc, int h, int w, int vpc,
                                                         long total) {
    constexpr int E = VEC ? 8 : 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Wq = Wc / E;
    long r = i / Wq;
    const int X = (int)(i - r * Wq) * E;
    const int Y = (int)(r % Hc); r /= Hc;
    const int c = (int)(r % C); r /= C;
    const int b = (int)(r % B);
    const int g = (int)(r / B);
    const int V = ny * nx;
    float acc[E], ws[E];
#pragma unroll
    for (int j = 0; j < E; ++j) { acc[j] = 0.f; ws[j] = 0.f; }
    for (int iy = 0; iy < ny; ++iy) {
        const int dy = Y - st.ys[iy];
        if ((unsigned)dy >= (unsigned)h) continue;
        for (int ix = 0; ix < nx; ++ix) {
            int dx = X - st.xs[ix];
            if (wrap && dx < 0) dx += Wc;
            if ((unsigned)dx >= (unsigned)w) continue;
            // the row of (g, v, b) inside the chunked buffer: every chunk in front of v's is full
            const int v = iy * nx + ix;
            const int ch = v / vpc, k = v - ch * vpc;
            const int size = V - ch * vpc < vpc ? V - ch * vpc : vpc;
            const long row = (long)ch * vpc * G * B + ((long)g * size + k) * B + b;
            const long off = ((row * C + c) * h + dy) * w + dx;
            if (VEC) {
                const h8 e = *reinterpret_cast<const h8*>(mo + off);
                if (WT) {
                    const f4 w0 = *reinterpret_cast<const f4*>(wt + (long)dy * w + dx);
                    const f4 w1 = *reinterpret_cast<const f4*>(wt + (long)dy * w + dx + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[j] += w0[j] * (float)e[j];
                        acc[j + 4] += w1[j] * (float)e[j + 4];
                        ws[j] += w0[j];
                        ws[j + 4] += w1[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { acc[j] += (float)e[j]; ws[j] += 1.f; }
                }
            } else {
                const float wv = WT ? wt[(long)dy * w + dx] : 1.f;
                acc[0] += wv * (float)mo[off];
                ws[0] += wv;
            }
        }
    }
    if (VEC) {
        h8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(acc[j] * (1.0f / ws[j]));
        *reinterpret_cast<h8*>(eps + i * 8) = o;
    } else {
        eps[i] = (half_t)(acc[0] * (1.0f / ws[0]));
    }
}

inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
// Whether 8 consecutive columns starting at a multiple of 8 are inside or outside every view together.
inline bool vec8_views(int Wc, int w, const ViewStarts& st, int nx) {
    if (w % 8 != 0 || Wc % 8 != 0) return false;
    for (int i = 0; i < nx; ++i)
        if (st.xs[i] % 8 != 0) return false;
    return true;
}

}  // namespace

int launch_views_gather(const half_t* canvas, half_t* windows, int B, int C, int Hc, int Wc, int h, int w,
                        const ViewStarts& st, int ny, int nx, int wrap_x, hipStream_t s) {
    (void)wrap_x;                                    // (a wrapped view differs only in where its columns end)
    const bool vec = vec8_views(Wc, w, st, nx) && aligned16(canvas, windows);
    const long total = (long)ny * nx * B * C * h * (vec ? w / 8 : w);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("views_gather: too many elements for one launch"); return 1; }
    const dim3 grid((unsigned)blocks);
    if (vec) hipLaunchKernelGGL(view_gather_kernel<true>, grid, dim3(256), 0, s, canvas, windows, st, nx, B, C, Hc, Wc, h, w, total);
    else hipLaunchKernelGGL(view_gather_kernel<false>, grid, dim3(256), 0, s, canvas, windows, st, nx, B, C, Hc, Wc, h, w, total);
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_views_merge(const half_t* model_out, half_t* eps, const float* wt, int G, int B, int C, int Hc, int Wc, int h,
                       int w, const ViewStarts& st, int ny, int nx, int wrap_x, int vpc, hipStream_t s) {
    const bool vec = vec8_views(Wc, w, st, nx) && aligned16(model_out, eps, wt);
    const long total = (long)G * B * C * Hc * (vec ? Wc / 8 : Wc);
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) { set_error("views_merge: too many elements for one launch"); return 1; }
    const dim3 grid((unsigned)blocks);
#define SD_VIEW_MERGE(V, W) \
    hipLaunchKernelGGL((view_merge_kernel<V, W>), grid, dim3(256), 0, s, model_out, eps, wt, st, ny, nx, wrap_x, G, B, C, Hc, Wc, h, w, vpc, total)
    if (wt) { if (vec) SD_VIEW_MERGE(true, true); else SD_VIEW_MERGE(false, true); }
    else { if (vec) SD_VIEW_MERGE(true, false); else SD_VIEW_MERGE(false, false); }
#undef SD_VIEW_MERGE
    SD_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sd
