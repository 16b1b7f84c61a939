// ssim.hip -- SSIM on the device: the evaluation metric (the reference's SSIMMeter, nerf/utils.py:259-293: torchmetrics'
// structural_similarity_index_measure with its defaults) and the D-SSIM term of a patch batch.  The definition is written out in
// include/laenerf.h above lae_ssim; laenerf_amd/metrics.py restates it in float64 (ssim_numpy, ssim_grad_numpy).
//
//   k_ssim_minmax   the data rule's first launch: per-block min / max of both images into scratch (min and max do not depend on
//                   the order, so every block of the main kernel can fold the partials itself: no host read, capturable)
//   k_ssim_tile     one workgroup per tile of SS_TH x SS_TW window positions: the halo tile of both images (all three channels,
//                   fp32) into LDS with bounds checks, then per channel a horizontal pass (five fp64 sums per halo row and
//                   column into LDS) and a vertical pass (the five window sums, S); per-thread sums in a fixed order, an LDS
//                   tree, one fp64 partial per workgroup
//   k_ssim_finish   one block: the partials in a fixed order, divided by the number of values
//   k_ssim_patch_forward    one workgroup per patch: the same tile body over the patch's tiles, one fixed-order sum
//   k_ssim_patch_backward   one workgroup per (16 x 16 pixels, channel, patch): recomputes the five sums of the 26 x 26 window
//                   positions that touch its pixels from a 36 x 36 input tile, forms Dm, Dxx, Dxy in LDS and spreads them back
//                   with the transposed separable pass; fp64 throughout, one rounding at the store, one owner per element
// Every window sum, S and the gradient are fp64: with fp32 sums exx - mx^2 cancels (a near-flat image, 0.7 +- 1e-3, moved the
// mean by 1.1e-6).  The inputs stay fp32 in LDS.
#include "lae_common.h"
#include "raymarch_common.h"                 // STREAM
#include <algorithm>
#include <cmath>

namespace {

constexpr int SS_K = 11, SS_THREADS = 256;
constexpr int SS_TW = LAE_SSIM_TILE_W, SS_TH = LAE_SSIM_TILE_H;      // window positions per workgroup
constexpr int SS_HW = SS_TW + SS_K - 1, SS_HH = SS_TH + SS_K - 1;    // its halo tile: 42 x 26 pixels
constexpr uint32_t SS_MM_BLOCKS = LAE_SSIM_MINMAX_BLOCKS;
static_assert(SS_MM_BLOCKS <= SS_THREADS, "a block of the main kernel folds one min/max partial per thread");
static_assert((SS_TW * SS_TH) % SS_THREADS == 0, "whole passes over a tile");

struct SsimWin { double g[SS_K]; };          // exp(-((k - 5) / 1.5)^2 / 2) / sum, computed once on the host in double

struct SsimLds {
    float in[2][SS_HH][SS_HW * 3];           // 26208 B: both images' halo tile, pixel-interleaved channels as in memory
    double mid[5][SS_HH][SS_TW];             // 33280 B: the horizontal pass of one channel (x, y, xx, yy, xy)
    double red[SS_THREADS];                  //  2048 B
};
static_assert(sizeof(SsimLds) <= 64 * 1024, "static LDS");

__device__ __forceinline__ double ssim_value(double mx, double my, double exx, double eyy, double exy, double C1, double C2) {
    const double mxy = mx * my, mxx = mx * mx, myy = my * my;
    const double A1 = 2.0 * mxy + C1, A2 = 2.0 * (exy - mxy) + C2;
    const double B1 = (mxx + myy) + C1, B2 = ((exx - mxx) + (eyy - myy)) + C2;
    return (A1 * A2) / (B1 * B2);
}

// the tile of window positions (oy.., ox..) of an H x W x 3 image pair -> this thread's sum of S over its valid positions and the
// three channels, in a fixed order.  Ends behind a barrier: the caller may run the next tile at once.
__device__ double ssim_tile(const float* __restrict__ x, const float* __restrict__ y, uint32_t H, uint32_t W, uint32_t oy, uint32_t ox,
                            double C1, double C2, bool all_nan, const SsimWin& win, float* __restrict__ map, SsimLds& s) {
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < (uint32_t)(SS_HH * SS_HW * 3); i += SS_THREADS) {
        const uint32_t r = i / (SS_HW * 3), j = i % (SS_HW * 3);
        const bool in = oy + r < H && ox + j / 3 < W;                            // bounds: rows and columns past the image read as 0
        const size_t at = ((size_t)(oy + r) * W + ox) * 3 + j;
        s.in[0][r][j] = in ? x[at] : 0.0f;
        s.in[1][r][j] = in ? y[at] : 0.0f;
    }
    __syncthreads();
    const uint32_t nh = H - (SS_K - 1), nw = W - (SS_K - 1);
    double sum = 0.0;
    for (int c = 0; c < 3; c++) {
        for (uint32_t i = t; i < (uint32_t)(SS_HH * SS_TW); i += SS_THREADS) {    // horizontal: 26 rows x 32 columns
            const uint32_t r = i / SS_TW, col = i % SS_TW;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
            for (int k = 0; k < SS_K; k++) {
                const double g = win.g[k], a = s.in[0][r][(col + k) * 3 + c], b = s.in[1][r][(col + k) * 3 + c];
                a0 = fma(g, a, a0); a1 = fma(g, b, a1); a2 = fma(g, a * a, a2); a3 = fma(g, b * b, a3); a4 = fma(g, a * b, a4);
            }
            s.mid[0][r][col] = a0; s.mid[1][r][col] = a1; s.mid[2][r][col] = a2; s.mid[3][r][col] = a3; s.mid[4][r][col] = a4;
        }
        __syncthreads();
        for (uint32_t i = t; i < (uint32_t)(SS_TH * SS_TW); i += SS_THREADS) {    // vertical: 16 x 32 window positions
            const uint32_t r = i / SS_TW, col = i % SS_TW;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
            for (int k = 0; k < SS_K; k++) {
                const double g = win.g[k];
                a0 = fma(g, s.mid[0][r + k][col], a0); a1 = fma(g, s.mid[1][r + k][col], a1); a2 = fma(g, s.mid[2][r + k][col], a2);
                a3 = fma(g, s.mid[3][r + k][col], a3); a4 = fma(g, s.mid[4][r + k][col], a4);
            }
            if (oy + r < nh && ox + col < nw) {
                const double S = all_nan ? __builtin_nan("") : ssim_value(a0, a1, a2, a3, a4, C1, C2);
                sum += S;
                if (map) map[((size_t)(oy + r) * nw + (ox + col)) * 3 + c] = (float)S;
            }
        }
        __syncthreads();
    }
    return sum;
}

// the sum of one value per thread over the block, thread 0 receiving it: a fixed tree
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void mm_fold(float v, float& lo, float& hi) { lo = fminf(lo, v); hi = fmaxf(hi, v); }

// per-block min x, max x, min y, max y -> mm[4 * block ..]
__global__ __launch_bounds__(SS_THREADS) void k_ssim_minmax(const float* __restrict__ x, const float* __restrict__ y, uint64_t n,
                                                           bool vec, double* __restrict__ mm) {
    __shared__ float s_mm[4][SS_THREADS];
    const float inf = __builtin_inff();
    float lx = inf, hx = -inf, ly = inf, hy = -inf;
    const uint64_t stride = (uint64_t)gridDim.x * SS_THREADS, gt = (uint64_t)blockIdx.x * SS_THREADS + threadIdx.x;
    const uint64_t n4 = vec ? n / 4 : 0;
    for (uint64_t i = gt; i < n4; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(x)[i], b = reinterpret_cast<const float4*>(y)[i];
        mm_fold(a.x, lx, hx); mm_fold(a.y, lx, hx); mm_fold(a.z, lx, hx); mm_fold(a.w, lx, hx);
        mm_fold(b.x, ly, hy); mm_fold(b.y, ly, hy); mm_fold(b.z, ly, hy); mm_fold(b.w, ly, hy);
    }
    for (uint64_t i = 4 * n4 + gt; i < n; i += stride) { mm_fold(x[i], lx, hx); mm_fold(y[i], ly, hy); }
    s_mm[0][threadIdx.x] = lx; s_mm[1][threadIdx.x] = hx; s_mm[2][threadIdx.x] = ly; s_mm[3][threadIdx.x] = hy;
    __syncthreads();
    for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const int o = threadIdx.x + h;
            s_mm[0][threadIdx.x] = fminf(s_mm[0][threadIdx.x], s_mm[0][o]); s_mm[1][threadIdx.x] = fmaxf(s_mm[1][threadIdx.x], s_mm[1][o]);
            s_mm[2][threadIdx.x] = fminf(s_mm[2][threadIdx.x], s_mm[2][o]); s_mm[3][threadIdx.x] = fmaxf(s_mm[3][threadIdx.x], s_mm[3][o]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) mm[4 * blockIdx.x + threadIdx.x] = (double)s_mm[threadIdx.x][0];
}

__global__ __launch_bounds__(SS_THREADS) void k_ssim_tile(const float* __restrict__ x, const float* __restrict__ y, uint32_t H, uint32_t W,
                                                         double data_range, const double* __restrict__ mm, uint32_t n_mm, SsimWin win,
                                                         double* __restrict__ partials, float* __restrict__ map) {
    __shared__ SsimLds s;
    double L = data_range;
    if (!(data_range > 0.0)) {               // the data rule: max(max x - min x, max y - min y) from the first launch's partials
        const double inf = __builtin_inf();
        double v[4] = {inf, -inf, inf, -inf};
        if (threadIdx.x < n_mm) {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = mm[4 * threadIdx.x + k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            s.red[threadIdx.x] = v[k];
            __syncthreads();
            for (int h = SS_THREADS / 2; h > 0; h >>= 1) {
                if ((int)threadIdx.x < h) s.red[threadIdx.x] = (k & 1) ? fmax(s.red[threadIdx.x], s.red[threadIdx.x + h]) : fmin(s.red[threadIdx.x], s.red[threadIdx.x + h]);
                __syncthreads();
            }
            v[k] = s.red[0];
            __syncthreads();
        }
        L = fmax(v[1] - v[0], v[3] - v[2]);
    }
    const double c1 = 0.01 * L, c2 = 0.03 * L;
    const double sum = ssim_tile(x, y, H, W, blockIdx.y * SS_TH, blockIdx.x * SS_TW, c1 * c1, c2 * c2, L == 0.0, win, map, s);
    const double total = block_sum(sum, s.red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(SS_THREADS) void k_ssim_finish(const double* __restrict__ partials, uint32_t n, double count, double* out) {
    __shared__ double s_red[SS_THREADS];
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += SS_THREADS) v += partials[i];
    const double total = block_sum(v, s_red);
    if (threadIdx.x == 0) *out = total / count;
}

__global__ __launch_bounds__(SS_THREADS) void k_ssim_patch_forward(const float* __restrict__ pred, const float* __restrict__ gt, uint32_t P,
                                                                  double data_range, SsimWin win, double* __restrict__ per_patch) {
    __shared__ SsimLds s;
    const size_t base = (size_t)blockIdx.x * P * P * 3;
    const uint32_t n = P - (SS_K - 1);
    const double c1 = 0.01 * data_range, c2 = 0.03 * data_range;
    double sum = 0.0;
    for (uint32_t oy = 0; oy < n; oy += SS_TH)
        for (uint32_t ox = 0; ox < n; ox += SS_TW)
            sum += ssim_tile(pred + base, gt + base, P, P, oy, ox, c1 * c1, c2 * c2, false, win, nullptr, s);
    const double total = block_sum(sum, s.red);
    if (threadIdx.x == 0) per_patch[blockIdx.x] = total / (3.0 * (double)n * (double)n);
}

// ---------------------------------------------------------------- the gradient of a patch's SSIM with respect to the prediction
constexpr int SB_T = 16;                              // pixels per side of a workgroup's tile
constexpr int SB_D = SB_T + SS_K - 1;                 // 26: the window positions that touch them
constexpr int SB_I = SB_D + SS_K - 1;                 // 36: the pixels those windows read
struct SsimBwdLds {
    float in[2][SB_I][SB_I];                          // 10368 B
    union {
        double mid[5][SB_I][SB_D];                    // 37440 B: the horizontal pass
        double tr[3][SB_T][SB_D];                     //  9984 B: the transposed vertical pass (after mid's last read)
    };
    double D[3][SB_D][SB_D];                          // 16224 B: Dm, Dxx, Dxy; 0 at positions outside the patch
};
static_assert(sizeof(SsimBwdLds) <= 64 * 1024, "static LDS");
static_assert(SB_T * SB_T == SS_THREADS, "one pixel per thread in the last pass");

__global__ __launch_bounds__(SS_THREADS) void k_ssim_patch_backward(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   uint32_t n_patch, uint32_t P, uint32_t tiles, double data_range,
                                                                   const float* __restrict__ gout, SsimWin win,
                                                                   float* __restrict__ grad_pred) {
    __shared__ SsimBwdLds s;
    const uint32_t t = threadIdx.x, c = blockIdx.y;
    const size_t base = (size_t)blockIdx.z * P * P * 3;
    const int u0 = (int)(blockIdx.x / tiles) * SB_T, v0 = (int)(blockIdx.x % tiles) * SB_T;     // the tile's first pixel
    const int i0 = u0 - (SS_K - 1), j0 = v0 - (SS_K - 1);                                       // its first window position = first input pixel
    const int n = (int)P - (SS_K - 1);
    const double c1 = 0.01 * data_range, c2 = 0.03 * data_range, C1 = c1 * c1, C2 = c2 * c2;
    for (uint32_t i = t; i < (uint32_t)(SB_I * SB_I); i += SS_THREADS) {
        const int r = i / SB_I, q = i % SB_I, pi = i0 + r, pj = j0 + q;
        const bool in = pi >= 0 && pi < (int)P && pj >= 0 && pj < (int)P;
        const size_t at = base + ((size_t)(in ? pi : 0) * P + (in ? pj : 0)) * 3 + c;
        s.in[0][r][q] = in ? pred[at] : 0.0f;
        s.in[1][r][q] = in ? gt[at] : 0.0f;
    }
    __syncthreads();
    for (uint32_t i = t; i < (uint32_t)(SB_I * SB_D); i += SS_THREADS) {          // horizontal: 36 rows x 26 columns
        const uint32_t r = i / SB_D, col = i % SB_D;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const double g = win.g[k], a = s.in[0][r][col + k], b = s.in[1][r][col + k];
            a0 = fma(g, a, a0); a1 = fma(g, b, a1); a2 = fma(g, a * a, a2); a3 = fma(g, b * b, a3); a4 = fma(g, a * b, a4);
        }
        s.mid[0][r][col] = a0; s.mid[1][r][col] = a1; s.mid[2][r][col] = a2; s.mid[3][r][col] = a3; s.mid[4][r][col] = a4;
    }
    __syncthreads();
    for (uint32_t i = t; i < (uint32_t)(SB_D * SB_D); i += SS_THREADS) {          // vertical: the 26 x 26 window positions -> Dm, Dxx, Dxy
        const uint32_t r = i / SB_D, col = i % SB_D;
        double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const double g = win.g[k];
            mx = fma(g, s.mid[0][r + k][col], mx); my = fma(g, s.mid[1][r + k][col], my); exx = fma(g, s.mid[2][r + k][col], exx);
            eyy = fma(g, s.mid[3][r + k][col], eyy); exy = fma(g, s.mid[4][r + k][col], exy);
        }
        const int pi = i0 + (int)r, pj = j0 + (int)col;
        double dm = 0.0, dxx = 0.0, dxy = 0.0;
        if (pi >= 0 && pi < n && pj >= 0 && pj < n) {
            const double mxy = mx * my, mxx = mx * mx, myy = my * my;
            const double A1 = 2.0 * mxy + C1, A2 = 2.0 * (exy - mxy) + C2;
            const double B1 = (mxx + myy) + C1, B2 = ((exx - mxx) + (eyy - myy)) + C2;
            const double B12 = B1 * B2, S = (A1 * A2) / B12;
            dm = (2.0 * my * A2 - 2.0 * my * A1) / B12 - S * (2.0 * mx / B1 - 2.0 * mx / B2);
            dxx = -S / B2;
            dxy = 2.0 * A1 / B12;
        }
        s.D[0][r][col] = dm; s.D[1][r][col] = dxx; s.D[2][r][col] = dxy;
    }
    __syncthreads();                                                              // mid is dead from here: tr takes its place
    for (uint32_t i = t; i < (uint32_t)(3 * SB_T * SB_D); i += SS_THREADS) {      // transposed vertical: pixel row u collects positions u - a
        const uint32_t p = i / (SB_T * SB_D), r = (i / SB_D) % SB_T, col = i % SB_D;
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < SS_K; k++) a = fma(win.g[k], s.D[p][r + (SS_K - 1) - k][col], a);
        s.tr[p][r][col] = a;
    }
    __syncthreads();
    const uint32_t r = t / SB_T, col = t % SB_T;                                  // transposed horizontal: one pixel per thread
    const int pu = u0 + (int)r, pv = v0 + (int)col;
    if (pu < (int)P && pv < (int)P) {
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
        for (int k = 0; k < SS_K; k++) {
            const double g = win.g[k];
            g0 = fma(g, s.tr[0][r][col + (SS_K - 1) - k], g0); g1 = fma(g, s.tr[1][r][col + (SS_K - 1) - k], g1);
            g2 = fma(g, s.tr[2][r][col + (SS_K - 1) - k], g2);
        }
        const double xv = s.in[0][r + (SS_K - 1)][col + (SS_K - 1)], yv = s.in[1][r + (SS_K - 1)][col + (SS_K - 1)];
        const double scale = (double)gout[0] / ((double)n_patch * 3.0 * (double)n * (double)n);
        grad_pred[base + ((size_t)pu * P + pv) * 3 + c] = (float)(((g0 + 2.0 * xv * g1) + yv * g2) * scale);
    }
}

SsimWin make_window() {
    SsimWin w;
    double sum = 0.0;
    for (int k = 0; k < SS_K; k++) { const double d = (k - 5) / 1.5; w.g[k] = std::exp(-(d * d) / 2.0); sum += w.g[k]; }
    for (int k = 0; k < SS_K; k++) w.g[k] /= sum;
    return w;
}

bool patch_args_ok(uint32_t n_patch, uint32_t P, double data_range) {
    return P >= (uint32_t)SS_K && P <= 4096u && (uint64_t)n_patch * P * P <= 0x7fffffffull / 3 && n_patch <= 65535u &&
           data_range > 0.0 && data_range <= 1.0e300;
}

}  // namespace

extern "C" {

uint64_t lae_ssim_scratch_doubles(uint32_t H, uint32_t W) {
    if (H < (uint32_t)SS_K || W < (uint32_t)SS_K) return 4ull * SS_MM_BLOCKS;
    return 4ull * SS_MM_BLOCKS + (uint64_t)lae::cdiv(H - (SS_K - 1), SS_TH) * lae::cdiv(W - (SS_K - 1), SS_TW);
}

int lae_ssim(const float* x, const float* y, uint32_t H, uint32_t W, double data_range, double* scratch, double* out, float* map,
             void* stream) {
    if (H < (uint32_t)SS_K || W < (uint32_t)SS_K || H > 32768u || W > 32768u || (uint64_t)H * W > 0x7fffffffull / 3) return LAE_EINVAL;
    if (!(data_range <= 1.0e300)) return LAE_EINVAL;                              // NaN, infinity
    if (!x || !y || !scratch || !out) return LAE_ENULL;
    const uint32_t nh = H - (SS_K - 1), nw = W - (SS_K - 1);
    const dim3 grid(lae::cdiv(nw, SS_TW), lae::cdiv(nh, SS_TH));
    hipStream_t s = STREAM(stream);
    uint32_t n_mm = 0;
    if (!(data_range > 0.0)) {
        const uint64_t n = (uint64_t)H * W * 3;
        n_mm = std::max<uint32_t>(1, std::min<uint32_t>(lae::cdiv(n, 4 * SS_THREADS), SS_MM_BLOCKS));
        const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
        k_ssim_minmax<<<n_mm, SS_THREADS, 0, s>>>(x, y, n, vec, scratch);
        int rc = lae::check_launch("ssim_minmax");
        if (rc != LAE_OK) return rc;
    }
    double* partials = scratch + 4 * SS_MM_BLOCKS;
    k_ssim_tile<<<grid, SS_THREADS, 0, s>>>(x, y, H, W, data_range, scratch, n_mm, make_window(), partials, map);
    int rc = lae::check_launch("ssim");
    if (rc != LAE_OK) return rc;
    k_ssim_finish<<<1, SS_THREADS, 0, s>>>(partials, grid.x * grid.y, 3.0 * (double)nh * (double)nw, out);
    return lae::check_launch("ssim_finish");
}

int lae_ssim_patch_forward(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, double data_range,
                           double* per_patch, void* stream) {
    if (!patch_args_ok(n_patch, patch_size, data_range)) return LAE_EINVAL;
    if (n_patch == 0) return LAE_OK;
    if (!pred || !gt || !per_patch) return LAE_ENULL;
    k_ssim_patch_forward<<<n_patch, SS_THREADS, 0, STREAM(stream)>>>(pred, gt, patch_size, data_range, make_window(), per_patch);
    return lae::check_launch("ssim_patch_forward");
}

int lae_ssim_patch_backward(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, double data_range,
                            const float* gout, float* grad_pred, void* stream) {
    if (!patch_args_ok(n_patch, patch_size, data_range)) return LAE_EINVAL;
    if (n_patch == 0) return LAE_OK;
    if (!pred || !gt || !gout || !grad_pred) return LAE_ENULL;
    const uint32_t tiles = lae::cdiv(patch_size, SB_T);
    k_ssim_patch_backward<<<dim3(tiles * tiles, 3, n_patch), SS_THREADS, 0, STREAM(stream)>>>(pred, gt, n_patch, patch_size, tiles,
                                                                                              data_range, gout, make_window(), grad_pred);
    return lae::check_launch("ssim_patch_backward");
}

}  // extern "C"
