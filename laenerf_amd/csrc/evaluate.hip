// evaluate.hip -- scoring a rendered view (the reference's evaluate_one_epoch / test, nerf/utils.py:1526-1624, :777-827, with
// PSNRMeter and LPIPSMeter(net='alex'), main_nerf.py:203, 242; LAENeRF's eval_masked, nerf/gui.py:853-947).
//
//   k_eval_view     ONE pass over a view: reads the render (fp32 rgb [HW,3] + depth [HW]) and the ground truth in its storage
//                   dtype (uint8 / fp16 / fp32, C = 3 or 4) once, four pixels per thread with vector loads; per pixel the blended
//                   ground truth, the squared error and the masked squared error (fp64), the uint8 rgb / depth and the LPIPS input.
//                   Per-block fp64 partials, summed in a fixed order by k_eval_finish (one block): two runs give the same bits.
//   k_lpips_head    LPIPS v0.1's distance head (normalize_tensor, NetLinLayer, spatial_average, the sum over layers) for all
//                   five layers and a batch of pairs in one launch: one lane per pixel of one layer, a loop over the channels
//                   (NCHW: every load coalesced across the wave), fp64 sums; per-block partials / (h w), k_lpips_finish sums a
//                   pair's partials in a fixed order.
//   k_lpips_head_grad   the head's gradient with respect to the features, again one launch for all layers and pairs: one wave per
//                   pixel, lanes over the channels; k_patch_pack / k_patch_unpack_grad move a patch batch's rows into the trunk's
//                   input layout and its gradient back (LPIPS as a training term, losses.lpips_patch_loss).
//   k_consistency_pair  multi-view consistency of two rendered views (the metric is written down above the kernel): ONE gather pass
//                   per pair, one lane per pixel of the target view, both flows recomputed in registers from the views' depth
//                   and the two poses; per-block fp64 partials of the squared error and the valid count, summed by k_sum_partials.
#include "lae_common.h"
#include "raymarch_common.h"                 // pinhole_ray, STREAM
#include <algorithm>

namespace {

constexpr int EV_THREADS = 256;
constexpr uint32_t EV_MAX_BLOCKS = LAE_EVAL_VIEW_SCRATCH_DOUBLES / 2;
constexpr uint32_t CONS_MAX_BLOCKS = LAE_CONSISTENCY_SCRATCH_DOUBLES / 2;   // one lane per pixel up to 2 M pixels: no second trip through the gather chain at 1920 x 1080

// `img.float() / 255` on the device: torch divides by a CPU scalar as a multiplication by its fp32 reciprocal
// (div_true_kernel_cuda), which is what Trainer.evaluate's ground truth went through
__device__ __forceinline__ float to_f(uint8_t v) { return __fmul_rn((float)v, 1.0f / 255.0f); }
__device__ __forceinline__ float to_f(_Float16 v) { return (float)v; }
__device__ __forceinline__ float to_f(float v) { return v; }

__device__ __forceinline__ uint8_t to_u8(float x) { return (uint8_t)(int)__fmul_rn(lae::clampf(x, 0.0f, 1.0f), 255.0f); }

struct EvalOut {
    double* scratch;             // [2 * EV_MAX_BLOCKS]: per-block sse | masked sse
    float* gt_out;               // [HW,3] or NULL
    uint8_t* rgb_u8;             // [HW,3] or NULL
    uint8_t* depth_u8;           // [HW] or NULL
    float* lpips_in;             // [2,3,H,W] or NULL
};

// the four pixels 4q .. 4q+3 of a thread's quad are loaded in one piece: B bytes of ground truth in W-byte vector loads
template <typename T, int C> struct Quad {
    static constexpr int B = 4 * C * (int)sizeof(T);
    static constexpr int W = B % 16 == 0 ? 16 : (B % 8 == 0 ? 8 : 4);
};

template <typename T, int C, bool VEC>
__device__ __forceinline__ void load_gt(const T* __restrict__ gt, uint32_t p0, int n, T (&v)[4 * C]) {
    if constexpr (VEC) {
        constexpr int B = Quad<T, C>::B, W = Quad<T, C>::W;
        const uint8_t* src = reinterpret_cast<const uint8_t*>(gt + (size_t)p0 * C);
        uint32_t raw[B / 4];
#pragma unroll
        for (int k = 0; k < B / W; k++) {
            if constexpr (W == 16) {
                const uint4 x = reinterpret_cast<const uint4*>(src)[k];
                raw[4 * k] = x.x; raw[4 * k + 1] = x.y; raw[4 * k + 2] = x.z; raw[4 * k + 3] = x.w;
            } else if constexpr (W == 8) {
                const uint2 x = reinterpret_cast<const uint2*>(src)[k];
                raw[2 * k] = x.x; raw[2 * k + 1] = x.y;
            } else {
                raw[k] = reinterpret_cast<const uint32_t*>(src)[k];
            }
        }
        __builtin_memcpy(v, raw, B);
    } else {
#pragma unroll
        for (int k = 0; k < 4 * C; k++) v[k] = k < n * C ? gt[(size_t)p0 * C + k] : T(0);
    }
}

template <typename T, int C, bool VEC>
__global__ __launch_bounds__(EV_THREADS) void k_eval_view(const float* __restrict__ pred, const float* __restrict__ depth,
                                                          const T* __restrict__ gt, uint32_t HW, float bg,
                                                          const uint8_t* __restrict__ mask, EvalOut o) {
    __shared__ double s_red[2][EV_THREADS];
    const float shift[3] = {-0.030f, -0.088f, -0.188f};          // lpips ScalingLayer (lpips/pretrained_networks.py)
    const float scale[3] = {0.458f, 0.448f, 0.450f};
    double sse = 0.0, msse = 0.0;
    const uint32_t quads = (HW + 3) / 4;
    for (uint32_t q = blockIdx.x * EV_THREADS + threadIdx.x; q < quads; q += gridDim.x * EV_THREADS) {
        const uint32_t p0 = 4 * q;
        const int n = (int)min(4u, HW - p0);
        float pr[12], de[4];
        T g[4 * C];
        if (n == 4) {                                            // 48 + 16 bytes of render in four 16-byte loads
            const float4* pp = reinterpret_cast<const float4*>(pred + (size_t)p0 * 3);
#pragma unroll
            for (int k = 0; k < 3; k++) { const float4 x = pp[k]; pr[4 * k] = x.x; pr[4 * k + 1] = x.y; pr[4 * k + 2] = x.z; pr[4 * k + 3] = x.w; }
            if (depth) { const float4 x = *reinterpret_cast<const float4*>(depth + p0); de[0] = x.x; de[1] = x.y; de[2] = x.z; de[3] = x.w; }
            else { de[0] = de[1] = de[2] = de[3] = 0.0f; }
            if (gt) load_gt<T, C, VEC>(gt, p0, 4, g);
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) pr[k] = k < 3 * n ? pred[(size_t)p0 * 3 + k] : 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) de[k] = (depth && k < n) ? depth[p0 + k] : 0.0f;
            if (gt) load_gt<T, C, false>(gt, p0, n, g);
        }
        uint32_t mw = 0;                                         // the mask bytes of the quad
        if (mask) {
            if (n == 4 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0) mw = *reinterpret_cast<const uint32_t*>(mask + p0);
            else for (int k = 0; k < n; k++) mw |= (uint32_t)mask[p0 + k] << (8 * k);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k >= n) break;
            const uint32_t p = p0 + k;
            float x[3];
            if (gt) {
                float raw[3];
#pragma unroll
                for (int c = 0; c < 3; c++) raw[c] = to_f(g[k * C + c]);
                if constexpr (C == 4) {                          // img[:, :3] * a + bg * (1 - a), each op rounded as torch's
                    const float a = to_f(g[k * C + 3]);
                    const float b = __fmul_rn(bg, __fsub_rn(1.0f, a));
#pragma unroll
                    for (int c = 0; c < 3; c++) x[c] = __fadd_rn(__fmul_rn(raw[c], a), b);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; c++) x[c] = raw[c];
                }
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double d = (double)pr[3 * k + c] - (double)x[c];
                    sse = fma(d, d, sse);
                }
                if (mask && ((mw >> (8 * k)) & 255u) == 0u) {    // eval_masked: m = 1 - clip(mask, 0, 1), no blend
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const double d = (double)pr[3 * k + c] - (double)raw[c];
                        msse = fma(d, d, msse);
                    }
                }
                if (o.gt_out) {
#pragma unroll
                    for (int c = 0; c < 3; c++) o.gt_out[(size_t)p * 3 + c] = x[c];
                }
            }
            if (o.rgb_u8) {
#pragma unroll
                for (int c = 0; c < 3; c++) o.rgb_u8[(size_t)p * 3 + c] = to_u8(pr[3 * k + c]);
            }
            if (o.depth_u8) o.depth_u8[p] = to_u8(de[k]);
            if (o.lpips_in && gt) {                              // lpips(truths, preds, normalize=True): [0] = gt, [1] = pred
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float u = __fsub_rn(__fmul_rn(2.0f, x[c]), 1.0f);
                    const float v = __fsub_rn(__fmul_rn(2.0f, pr[3 * k + c]), 1.0f);
                    o.lpips_in[(size_t)c * HW + p] = __fdiv_rn(__fsub_rn(u, shift[c]), scale[c]);
                    o.lpips_in[(size_t)(3 + c) * HW + p] = __fdiv_rn(__fsub_rn(v, shift[c]), scale[c]);
                }
            }
        }
    }
    s_red[0][threadIdx.x] = sse;
    s_red[1][threadIdx.x] = msse;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {               // fixed-order tree
        if ((int)threadIdx.x < s) {
            s_red[0][threadIdx.x] += s_red[0][threadIdx.x + s];
            s_red[1][threadIdx.x] += s_red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        o.scratch[blockIdx.x] = s_red[0][0];
        o.scratch[EV_MAX_BLOCKS + blockIdx.x] = s_red[1][0];
    }
}

// one block per row of n partials (rows `stride` apart), summed in a fixed order: thread t takes t, t + 256, ..., then a tree.
// The sum of row r goes to out1 when r == 1 and out1 is given (the view's masked sum), else to out0[r].
__global__ __launch_bounds__(EV_THREADS) void k_sum_partials(const double* __restrict__ part, uint32_t n, uint32_t stride,
                                                             double* out0, double* out1) {
    __shared__ double s_red[EV_THREADS];
    const double* p = part + (size_t)blockIdx.x * stride;
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += EV_THREADS) s += p[i];
    s_red[threadIdx.x] = s;
    __syncthreads();
    for (int h = EV_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_red[threadIdx.x] += s_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (out1 && blockIdx.x == 1) *out1 = s_red[0];
        else out0[blockIdx.x] = s_red[0];
    }
}

constexpr int LP_MAX_LAYERS = 5;
struct LpipsArgs {
    const float* f[LP_MAX_LAYERS];          // [2 * n_pairs, C, h, w]: pair p = rows 2p (x0) and 2p + 1 (x1)
    const float* w[LP_MAX_LAYERS];          // [C]
    uint32_t C[LP_MAX_LAYERS], hw[LP_MAX_LAYERS];
    uint32_t blk0[LP_MAX_LAYERS + 1];       // first block of each layer; blk0[n_layers] = blocks per pair
    uint32_t n_layers;
};

__global__ __launch_bounds__(EV_THREADS) void k_lpips_head(LpipsArgs a, uint32_t blocks_per_pair, double* __restrict__ partials) {
    __shared__ double s_red[EV_THREADS];
    const uint32_t pair = blockIdx.y, b = blockIdx.x;
    uint32_t l = 0;
    while (l + 1 < a.n_layers && b >= a.blk0[l + 1]) l++;
    const uint32_t hw = a.hw[l], C = a.C[l];
    const uint32_t px = (b - a.blk0[l]) * EV_THREADS + threadIdx.x;
    double d = 0.0;
    if (px < hw) {
        const float* __restrict__ f0 = a.f[l] + (size_t)(2 * pair) * C * hw + px;
        const float* __restrict__ f1 = f0 + (size_t)C * hw;
        const float* __restrict__ w = a.w[l];
        // one pass: |f0|^2, |f1|^2 and the weighted sums of f0 f0, f0 f1, f1 f1; then
        // sum_c w_c (f0 / n0 - f1 / n1)^2 = w00 / n0^2 - 2 w01 / (n0 n1) + w11 / n1^2 with n = sqrt(|f|^2) + 1e-10 (fp64 throughout)
        double s00 = 0.0, s11 = 0.0, w00 = 0.0, w01 = 0.0, w11 = 0.0;
        uint32_t c = 0;
        for (; c + 4 <= C; c += 4) {
            float x[4], y[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { x[k] = f0[(size_t)(c + k) * hw]; y[k] = f1[(size_t)(c + k) * hw]; }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double xd = x[k], yd = y[k], wc = w[c + k];
                s00 = fma(xd, xd, s00); s11 = fma(yd, yd, s11);
                w00 = fma(wc * xd, xd, w00); w01 = fma(wc * xd, yd, w01); w11 = fma(wc * yd, yd, w11);
            }
        }
        for (; c < C; c++) {
            const double xd = f0[(size_t)c * hw], yd = f1[(size_t)c * hw], wc = w[c];
            s00 = fma(xd, xd, s00); s11 = fma(yd, yd, s11);
            w00 = fma(wc * xd, xd, w00); w01 = fma(wc * xd, yd, w01); w11 = fma(wc * yd, yd, w11);
        }
        const double n0 = sqrt(s00) + 1e-10, n1 = sqrt(s11) + 1e-10;
        const double t0 = w00 / (n0 * n0), t1 = w01 / (n0 * n1), t2 = w11 / (n1 * n1);
        d = (t0 - 2.0 * t1) + t2;                                // identical features: t0 = t1 = t2, exactly 0
    }
    s_red[threadIdx.x] = d;
    __syncthreads();
    for (int h = EV_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_red[threadIdx.x] += s_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[(size_t)pair * blocks_per_pair + b] = s_red[0] / (double)hw;
}

// ---------------------------------------------------------------- LPIPS as a training term (losses.lpips_patch_loss)
// the sum of one fp64 value per lane over the wave, every lane receiving it; a fixed butterfly: two calls give the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int LG_WAVES = EV_THREADS / 64;    // pixels per block
constexpr int LG_PER_LANE = 8;               // channels a lane keeps in registers: C <= 512
struct LpipsGradArgs {
    const float* f[LP_MAX_LAYERS];
    const float* w[LP_MAX_LAYERS];
    float* g[LP_MAX_LAYERS];                // [2 * n_pairs, C, hw], every element written
    uint32_t C[LP_MAX_LAYERS], hw[LP_MAX_LAYERS];
    uint32_t blk0[LP_MAX_LAYERS + 1];
    uint32_t n_layers;
};

// the gradient of k_lpips_head with respect to the features, all layers and pairs in one launch: one wave per (pair, layer, pixel),
// lanes over the channels (the features of both sides stay in registers), two wave reductions (the norms, then a_0 and a_1).  The
// sizes it sees -- hw from 1 to a few hundred, C from 64 to 384 -- are latency-bound; with hw = 1 the loads and stores are
// coalesced.  fp64 throughout, gout multiplied in before the single rounding to fp32; one owner per output element.
__global__ __launch_bounds__(EV_THREADS) void k_lpips_head_grad(LpipsGradArgs a, const double* __restrict__ gout, int both) {
    const uint32_t pair = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t l = 0;
    while (l + 1 < a.n_layers && b >= a.blk0[l + 1]) l++;
    const uint32_t hw = a.hw[l], C = a.C[l];
    const uint32_t px = (b - a.blk0[l]) * LG_WAVES + wave;
    if (px >= hw) return;                                        // the whole wave: no lane of it reaches a shuffle
    const size_t row = (size_t)C * hw;
    const float* __restrict__ f0 = a.f[l] + (size_t)(2 * pair) * row + px;
    const float* __restrict__ f1 = f0 + row;
    const float* __restrict__ w = a.w[l];
    double x0[LG_PER_LANE], x1[LG_PER_LANE], wc[LG_PER_LANE];
    double s00 = 0.0, s11 = 0.0;
#pragma unroll
    for (int j = 0; j < LG_PER_LANE; j++) {
        const uint32_t c = lane + 64u * j;
        const bool in = c < C;
        x0[j] = in ? (double)f0[(size_t)c * hw] : 0.0;
        x1[j] = in ? (double)f1[(size_t)c * hw] : 0.0;
        wc[j] = in ? (double)w[c] : 0.0;
        s00 += x0[j] * x0[j];
        s11 += x1[j] * x1[j];
    }
    const double n0 = sqrt(wave_sum(s00)), n1 = sqrt(wave_sum(s11));
    const double e0 = n0 + 1e-10, e1 = n1 + 1e-10;
    double a0 = 0.0, a1 = 0.0, wd[LG_PER_LANE];
#pragma unroll
    for (int j = 0; j < LG_PER_LANE; j++) {
        wd[j] = wc[j] * (x0[j] / e0 - x1[j] / e1);
        a0 += wd[j] * x0[j];
        a1 += wd[j] * x1[j];
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    const double k = 2.0 * gout[pair] / (double)hw;
    // a side whose norm is exactly 0 gets a zero gradient: the slope there is 1 / eps, an artefact of eps (include/laenerf.h)
    const bool on0 = both && n0 != 0.0, on1 = n1 != 0.0;
    const double q0 = on0 ? a0 / (n0 * e0 * e0) : 0.0, q1 = on1 ? a1 / (n1 * e1 * e1) : 0.0;
    float* __restrict__ g0 = a.g[l] + (size_t)(2 * pair) * row + px;
    float* __restrict__ g1 = g0 + row;
#pragma unroll
    for (int j = 0; j < LG_PER_LANE; j++) {
        const uint32_t c = lane + 64u * j;
        if (c < C) {
            g0[(size_t)c * hw] = on0 ? (float)(k * (wd[j] / e0 - x0[j] * q0)) : 0.0f;
            g1[(size_t)c * hw] = on1 ? (float)(-k * (wd[j] / e1 - x1[j] * q1)) : 0.0f;
        }
    }
}

// pred / gt rows [n_patch * P^2, 3] -> the trunk's input [2 * n_patch, 3, P, P] (row 2p the ground truth, 2p + 1 the prediction) with
// k_eval_view's statements; normalize = 0 leaves out the 2v - 1
__global__ __launch_bounds__(EV_THREADS) void k_patch_pack(const float* __restrict__ pred, const float* __restrict__ gt, uint32_t n_rows,
                                                           uint32_t PP, int normalize, float* __restrict__ x) {
    const float shift[3] = {-0.030f, -0.088f, -0.188f};          // lpips ScalingLayer, as in k_eval_view
    const float scale[3] = {0.458f, 0.448f, 0.450f};
    const uint32_t r = blockIdx.x * EV_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t p = r / PP, px = r % PP;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float u = gt[(size_t)r * 3 + c], v = pred[(size_t)r * 3 + c];
        if (normalize) { u = __fsub_rn(__fmul_rn(2.0f, u), 1.0f); v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f); }
        x[((size_t)(2 * p) * 3 + c) * PP + px] = __fdiv_rn(__fsub_rn(u, shift[c]), scale[c]);
        x[((size_t)(2 * p + 1) * 3 + c) * PP + px] = __fdiv_rn(__fsub_rn(v, shift[c]), scale[c]);
    }
}

// k_patch_pack's transpose onto the prediction: every row of grad_pred is written
__global__ __launch_bounds__(EV_THREADS) void k_patch_unpack_grad(const float* __restrict__ grad_x, uint32_t n_rows, uint32_t PP,
                                                                  int normalize, float* __restrict__ grad_pred) {
    const float scale[3] = {0.458f, 0.448f, 0.450f};
    const uint32_t r = blockIdx.x * EV_THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t p = r / PP, px = r % PP;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float g = grad_x[((size_t)(2 * p + 1) * 3 + c) * PP + px];
        if (normalize) g = __fmul_rn(g, 2.0f);
        grad_pred[(size_t)r * 3 + c] = __fdiv_rn(g, scale[c]);
    }
}

// ---------------------------------------------------------------- multi-view consistency of a pair of rendered views
// LAENeRF, ARF and Ref-NPR score a result without ground truth by its short- and long-range view consistency (the reference's
// scripts/eval/consistency_metrics.py: frame i warped onto frame i + step by an optical flow, occlusions masked, the masked
// squared error and the LPIPS of the warped frame against the target).  The script takes the flow from a RAFT network; here
// the model that rendered the frames also rendered their depth and the cameras are known, so the flow is a reprojection.
//
// a is the source view and b the target view.  Each view v has a cam2world pose P_v = [R_v | T_v]; all views share the
// intrinsics (fx, fy, cx, cy).  Each view has a frame F_v [H, W, 3], a depth D_v (the raw sum w t of
// render_eval(scale_depth=False)) and an opacity A_v (weights_sum).
//   Geometry     defined at pixel p = (x, y) of view v iff A_v[p] >= min_opacity (default 0.5, a choice: below one half the
//                expected termination is not a surface).  Then t = D_v[p] / A_v[p] and X_v(p) = o + t d with (o, d) from
//                pinhole_ray (pixel centre = index + 0.5, unit direction).
//   Projection   proj_v(X): q = R_v^T (X - T_v), defined iff q.z > 0; (fx q.x / q.z + cx - 0.5, fy q.y / q.z + cy - 0.5), in
//                pixel-index coordinates.
//   Flows        fw(p) = proj_a(X_b(p)) - p for pixels p of b;  bw(r) = proj_b(X_a(r)) - r for pixels r of a.
//   Landing      l = p + fw(p) must satisfy 0 <= l.x <= W-1 and 0 <= l.y <= H-1.  The taps are x0 = min(floor(l.x), W-2),
//                y0 = min(floor(l.y), H-2) and the three neighbours; bw must be defined at all four.  bw~ and the warped colour
//                Fw are the bilinear means of bw and F_a over those taps (cv2.INTER_LINEAR away from the border; the border
//                case is invalid, not zero-filled).
//   Occlusion    (detect_occlusion's constants) occluded iff |fw + bw~|^2 > 0.01 (|fw|^2 + |bw~|^2) + 0.5.
//   Boundary     (compute_flow_gradients' constants) du = fw(x,y) - fw(x+1,y), 0 in the last column; dv = fw(x,y) - fw(x,y+1),
//                0 in the last row; a neighbour whose fw is undefined makes the pixel invalid; on a motion boundary iff
//                |du|^2 + |dv|^2 > 0.01 |fw|^2 + 0.002.
//   Validity     valid(p) = everything above is defined and neither rule fires.
//   Error        err(p) = sum_c (Fw_c - F_b(p)_c)^2;  sse = sum over valid of err, count = sum of valid;
//                warp_mse = sse / count (the number the script prints as "RSME": it takes no root), formed by the caller.
//   LPIPS input  [2, 3, H, W] with k_eval_view's scaling: index 0 is valid ? Fw : F_b(p), index 1 is F_b(p); invalid pixels
//                contribute nothing.
// Two deliberate departures from the script: it multiplies the error by the occlusion mask itself where the metric it follows
// (Lai et al.) uses the complement, as here; and it feeds LPIPS the warped frame with remap's zero border where invalid pixels
// are filled from the target here.
// The flows are never stored: a lane recomputes fw at its pixel and the right and lower neighbours and bw at the four taps --
// seven ray / projection evaluations against about 60 bytes of traffic per pixel.
struct ConsIn {
    const float *Da, *Aa, *Db, *Ab, *Pa, *Pb;
    float fx, fy, cx, cy, min_opacity;
    uint32_t H, W;
};
struct ConsOut {
    double* scratch;             // [2 * CONS_MAX_BLOCKS]: per-block sse | count
    uint8_t* valid;              // [HW] or NULL
    float* warped;               // [HW,3] or NULL (0 where invalid)
    float* lpips_in;             // [2,3,H,W] or NULL
};

// X_v(pix); false where the geometry is undefined
__device__ __forceinline__ bool cons_point(const float* __restrict__ P, const float* __restrict__ D, const float* __restrict__ A,
                                           const ConsIn& g, uint32_t pix, float X[3]) {
    const float a = A[pix];
    if (!(a >= g.min_opacity)) return false;
    const float t = D[pix] / a;
    float o[3], d[3];
    pinhole_ray(P, g.fx, g.fy, g.cx, g.cy, g.W, (int64_t)pix, 0, 0.0f, 0.0f, o, d);
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = fmaf(t, d[k], o[k]);
    return true;
}

// proj_v(X) in pixel-index coordinates; false where q.z <= 0 (or not a number)
__device__ __forceinline__ bool cons_project(const float* __restrict__ P, const ConsIn& g, const float X[3], float& u, float& v) {
    const float v0 = X[0] - P[3], v1 = X[1] - P[7], v2 = X[2] - P[11];
    const float qx = fmaf(P[8], v2, fmaf(P[4], v1, P[0] * v0));
    const float qy = fmaf(P[9], v2, fmaf(P[5], v1, P[1] * v0));
    const float qz = fmaf(P[10], v2, fmaf(P[6], v1, P[2] * v0));
    if (!(qz > 0.0f)) return false;
    u = g.fx * qx / qz + g.cx - 0.5f;
    v = g.fy * qy / qz + g.cy - 0.5f;
    return true;
}

// where pixel `pix` of b lands in a: l = p + fw(p)
__device__ __forceinline__ bool cons_land(const ConsIn& g, uint32_t pix, float& lx, float& ly) {
    float X[3];
    return cons_point(g.Pb, g.Db, g.Ab, g, pix, X) && cons_project(g.Pa, g, X, lx, ly);
}

template <typename T>
__global__ __launch_bounds__(EV_THREADS) void k_consistency_pair(const T* __restrict__ Fa, const T* __restrict__ Fb, ConsIn g, ConsOut o) {
    __shared__ double s_red[2][EV_THREADS];
    const float shift[3] = {-0.030f, -0.088f, -0.188f};          // lpips ScalingLayer, as in k_eval_view
    const float scale[3] = {0.458f, 0.448f, 0.450f};
    const uint32_t HW = g.H * g.W;
    double sse = 0.0, cnt = 0.0;
    for (uint32_t p = blockIdx.x * EV_THREADS + threadIdx.x; p < HW; p += gridDim.x * EV_THREADS) {
        const uint32_t x = p % g.W, y = p / g.W;
        const float xf = (float)x, yf = (float)y;
        float fb[3], fw_c[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 3; c++) fb[c] = to_f(Fb[(size_t)p * 3 + c]);
        float lx = 0.0f, ly = 0.0f;
        bool ok = cons_land(g, p, lx, ly);
        ok = ok && lx >= 0.0f && lx <= (float)(g.W - 1) && ly >= 0.0f && ly <= (float)(g.H - 1);     // a NaN fails here
        const float fwx = lx - xf, fwy = ly - yf;
        float dux = 0.0f, duy = 0.0f, dvx = 0.0f, dvy = 0.0f;
        if (ok && x + 1 < g.W) {                                 // motion boundary: the right and the lower neighbour's fw
            float nx, ny;
            ok = cons_land(g, p + 1, nx, ny);
            if (ok) { dux = fwx - (nx - (xf + 1.0f)); duy = fwy - (ny - yf); }
        }
        if (ok && y + 1 < g.H) {
            float nx, ny;
            ok = cons_land(g, p + g.W, nx, ny);
            if (ok) { dvx = fwx - (nx - xf); dvy = fwy - (ny - (yf + 1.0f)); }
        }
        if (ok) {
            const float grad = (dux * dux + dvx * dvx) + (duy * duy + dvy * dvy);
            const float mag = fwx * fwx + fwy * fwy;
            ok = !(grad > 0.01f * mag + 0.002f);
            if (ok) {
                // 0 <= l <= W-1 / H-1 was checked above: x0 in [0, W-2], y0 in [0, H-2], all four taps inside the frame
                const uint32_t x0 = min((uint32_t)floorf(lx), g.W - 2u), y0 = min((uint32_t)floorf(ly), g.H - 2u);
                const float wx = lx - (float)x0, wy = ly - (float)y0;
                float tap[4][5];                                 // per tap: bw.x, bw.y, F_a
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t rx = x0 + (k & 1), ry = y0 + (k >> 1);
                    const uint32_t r = ry * g.W + rx;
                    float X[3], u = 0.0f, v = 0.0f;
                    ok = ok && cons_point(g.Pa, g.Da, g.Aa, g, r, X) && cons_project(g.Pb, g, X, u, v);
                    if (!ok) break;
                    tap[k][0] = u - (float)rx;
                    tap[k][1] = v - (float)ry;
#pragma unroll
                    for (int c = 0; c < 3; c++) tap[k][2 + c] = to_f(Fa[(size_t)r * 3 + c]);
                }
                if (ok) {
                    // the bilinear mean as two lerps along x and one along y: a constant over the taps comes back as it is
                    float m[5];
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        const float top = fmaf(wx, tap[1][c] - tap[0][c], tap[0][c]);
                        const float bot = fmaf(wx, tap[3][c] - tap[2][c], tap[2][c]);
                        m[c] = fmaf(wy, bot - top, top);
                    }
                    const float bwx = m[0], bwy = m[1];
#pragma unroll
                    for (int c = 0; c < 3; c++) fw_c[c] = m[2 + c];
                    const float sx = fwx + bwx, sy = fwy + bwy;
                    ok = !(sx * sx + sy * sy > 0.01f * (mag + (bwx * bwx + bwy * bwy)) + 0.5f);
                }
            }
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double d = (double)fw_c[c] - (double)fb[c];
                sse = fma(d, d, sse);
            }
            cnt += 1.0;
        }
        if (o.valid) o.valid[p] = ok ? 1 : 0;
        if (o.warped) {
#pragma unroll
            for (int c = 0; c < 3; c++) o.warped[(size_t)p * 3 + c] = ok ? fw_c[c] : 0.0f;
        }
        if (o.lpips_in) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float u = __fsub_rn(__fmul_rn(2.0f, ok ? fw_c[c] : fb[c]), 1.0f);
                const float v = __fsub_rn(__fmul_rn(2.0f, fb[c]), 1.0f);
                o.lpips_in[(size_t)c * HW + p] = __fdiv_rn(__fsub_rn(u, shift[c]), scale[c]);
                o.lpips_in[(size_t)(3 + c) * HW + p] = __fdiv_rn(__fsub_rn(v, shift[c]), scale[c]);
            }
        }
    }
    s_red[0][threadIdx.x] = sse;
    s_red[1][threadIdx.x] = cnt;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {               // fixed-order tree
        if ((int)threadIdx.x < s) {
            s_red[0][threadIdx.x] += s_red[0][threadIdx.x + s];
            s_red[1][threadIdx.x] += s_red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        o.scratch[blockIdx.x] = s_red[0][0];
        o.scratch[CONS_MAX_BLOCKS + blockIdx.x] = s_red[1][0];
    }
}

template <typename T, int C>
void launch_eval(bool vec, uint32_t blocks, const float* pred, const float* depth, const void* gt, uint32_t HW, float bg,
                 const uint8_t* mask, const EvalOut& o, hipStream_t s) {
    if (vec) k_eval_view<T, C, true><<<blocks, EV_THREADS, 0, s>>>(pred, depth, (const T*)gt, HW, bg, mask, o);
    else k_eval_view<T, C, false><<<blocks, EV_THREADS, 0, s>>>(pred, depth, (const T*)gt, HW, bg, mask, o);
}

}  // namespace

extern "C" {

int lae_eval_view(const float* pred, const float* depth, const void* gt, int gt_dtype, uint32_t gt_channels, uint32_t n_pixels, float bg,
                  const uint8_t* mask, double* scratch, double* sse_out, double* masked_sse_out, float* gt_out, uint8_t* rgb_u8,
                  uint8_t* depth_u8, float* lpips_in, void* stream) {
    if (n_pixels == 0) return LAE_OK;
    if (!pred || !scratch) return LAE_ENULL;
    if (gt_dtype < 0 || gt_dtype > 2 || (gt_channels != 3 && gt_channels != 4)) return LAE_EINVAL;
    if (!gt && (sse_out || masked_sse_out || gt_out || lpips_in || mask)) return LAE_ENULL;     // these need the ground truth
    if (masked_sse_out && (!mask || !sse_out)) return LAE_ENULL;
    if (depth_u8 && !depth) return LAE_ENULL;
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(depth)) & 15) return LAE_EINVAL;   // float4 loads
    const size_t esize = gt_dtype == 0 ? 1 : (gt_dtype == 1 ? 2 : 4);
    const size_t quad_bytes = 4 * gt_channels * esize;
    const size_t w = quad_bytes % 16 == 0 ? 16 : (quad_bytes % 8 == 0 ? 8 : 4);
    const bool vec = gt && (reinterpret_cast<uintptr_t>(gt) % w) == 0;
    const uint32_t quads = (n_pixels + 3) / 4;
    const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>(lae::cdiv(quads, EV_THREADS), EV_MAX_BLOCKS));
    hipStream_t s = STREAM(stream);
    EvalOut o{scratch, gt_out, rgb_u8, depth_u8, lpips_in};
    const bool c4 = gt_channels == 4;
    if (gt_dtype == 0) { if (c4) launch_eval<uint8_t, 4>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); else launch_eval<uint8_t, 3>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); }
    else if (gt_dtype == 1) { if (c4) launch_eval<_Float16, 4>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); else launch_eval<_Float16, 3>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); }
    else { if (c4) launch_eval<float, 4>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); else launch_eval<float, 3>(vec, blocks, pred, depth, gt, n_pixels, bg, mask, o, s); }
    int rc = lae::check_launch("eval_view");
    if (rc != LAE_OK || !sse_out) return rc;
    // row 0 of the partials -> sse_out, row 1 -> masked_sse_out
    k_sum_partials<<<masked_sse_out ? 2 : 1, EV_THREADS, 0, s>>>(scratch, blocks, EV_MAX_BLOCKS, sse_out, masked_sse_out);
    return lae::check_launch("eval_view_sum");
}

int lae_lpips_head(uint32_t n_layers, const float* const* feats, const float* const* weights, const uint32_t* channels, const uint32_t* hw,
                   uint32_t n_pairs, double* scratch, double* out, void* stream) {
    if (n_pairs == 0) return LAE_OK;
    if (!feats || !weights || !channels || !hw || !scratch || !out) return LAE_ENULL;
    if (n_layers == 0 || n_layers > (uint32_t)LP_MAX_LAYERS || n_pairs > 65535u) return LAE_EINVAL;
    LpipsArgs a{};
    uint32_t nb = 0;
    for (uint32_t l = 0; l < n_layers; l++) {
        if (!feats[l] || !weights[l]) return LAE_ENULL;
        if (channels[l] == 0 || hw[l] == 0) return LAE_EINVAL;
        a.f[l] = feats[l]; a.w[l] = weights[l]; a.C[l] = channels[l]; a.hw[l] = hw[l];
        a.blk0[l] = nb;
        nb += lae::cdiv(hw[l], EV_THREADS);
    }
    a.blk0[n_layers] = nb;
    a.n_layers = n_layers;
    hipStream_t s = STREAM(stream);
    k_lpips_head<<<dim3(nb, n_pairs), EV_THREADS, 0, s>>>(a, nb, scratch);
    int rc = lae::check_launch("lpips_head");
    if (rc != LAE_OK) return rc;
    k_sum_partials<<<n_pairs, EV_THREADS, 0, s>>>(scratch, nb, nb, out, nullptr);     // one block per pair
    return lae::check_launch("lpips_head_sum");
}

int lae_lpips_head_grad(uint32_t n_layers, const float* const* feats, const float* const* weights, const uint32_t* channels,
                        const uint32_t* hw, uint32_t n_pairs, const double* gout, float* const* grad_feats, int both, void* stream) {
    if (n_pairs == 0) return LAE_OK;
    if (!feats || !weights || !channels || !hw || !gout || !grad_feats) return LAE_ENULL;
    if (n_layers == 0 || n_layers > (uint32_t)LP_MAX_LAYERS || n_pairs > 65535u) return LAE_EINVAL;
    LpipsGradArgs a{};
    uint32_t nb = 0;
    for (uint32_t l = 0; l < n_layers; l++) {
        if (!feats[l] || !weights[l] || !grad_feats[l]) return LAE_ENULL;
        if (channels[l] == 0 || channels[l] > 64u * LG_PER_LANE || hw[l] == 0) return LAE_EINVAL;
        a.f[l] = feats[l]; a.w[l] = weights[l]; a.g[l] = grad_feats[l]; a.C[l] = channels[l]; a.hw[l] = hw[l];
        a.blk0[l] = nb;
        nb += lae::cdiv(hw[l], LG_WAVES);
    }
    a.blk0[n_layers] = nb;
    a.n_layers = n_layers;
    k_lpips_head_grad<<<dim3(nb, n_pairs), EV_THREADS, 0, STREAM(stream)>>>(a, gout, both != 0);
    return lae::check_launch("lpips_head_grad");
}

int lae_patch_pack(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, int normalize, float* x, void* stream) {
    if (n_patch == 0) return LAE_OK;
    if (!pred || !gt || !x) return LAE_ENULL;
    if (patch_size == 0 || patch_size > 4096u || (uint64_t)n_patch * patch_size * patch_size > 0x7fffffffull) return LAE_EINVAL;
    const uint32_t PP = patch_size * patch_size, n_rows = n_patch * PP;
    k_patch_pack<<<lae::cdiv(n_rows, EV_THREADS), EV_THREADS, 0, STREAM(stream)>>>(pred, gt, n_rows, PP, normalize != 0, x);
    return lae::check_launch("patch_pack");
}

int lae_patch_unpack_grad(const float* grad_x, uint32_t n_patch, uint32_t patch_size, int normalize, float* grad_pred, void* stream) {
    if (n_patch == 0) return LAE_OK;
    if (!grad_x || !grad_pred) return LAE_ENULL;
    if (patch_size == 0 || patch_size > 4096u || (uint64_t)n_patch * patch_size * patch_size > 0x7fffffffull) return LAE_EINVAL;
    const uint32_t PP = patch_size * patch_size, n_rows = n_patch * PP;
    k_patch_unpack_grad<<<lae::cdiv(n_rows, EV_THREADS), EV_THREADS, 0, STREAM(stream)>>>(grad_x, n_rows, PP, normalize != 0, grad_pred);
    return lae::check_launch("patch_unpack_grad");
}

int lae_consistency_pair(const void* frame_a, const void* frame_b, int frame_dtype, const float* depth_a, const float* opacity_a,
                         const float* depth_b, const float* opacity_b, const float* pose_a, const float* pose_b, float fx, float fy,
                         float cx, float cy, uint32_t H, uint32_t W, float min_opacity, double* scratch, double* sse_out,
                         double* count_out, uint8_t* valid, float* warped, float* lpips_in, void* stream) {
    if (!frame_a || !frame_b || !depth_a || !opacity_a || !depth_b || !opacity_b || !pose_a || !pose_b || !scratch || !sse_out ||
        !count_out) return LAE_ENULL;
    if (frame_dtype != 0 && frame_dtype != 2) return LAE_EINVAL;                 // uint8 or fp32, lae_eval_view's codes
    if (H < 2 || W < 2 || (uint64_t)H * W > 0x7fffffffull) return LAE_EINVAL;      // four taps need a 2 x 2 frame; 32-bit pixel index
    if (!(fx > 0.0f) || !(fy > 0.0f) || !(min_opacity > 0.0f)) return LAE_EINVAL;  // t = D / A needs A > 0
    const uint32_t HW = H * W;
    const uint32_t blocks = std::min<uint32_t>(lae::cdiv(HW, EV_THREADS), CONS_MAX_BLOCKS);
    hipStream_t s = STREAM(stream);
    ConsIn g{depth_a, opacity_a, depth_b, opacity_b, pose_a, pose_b, fx, fy, cx, cy, min_opacity, H, W};
    ConsOut o{scratch, valid, warped, lpips_in};
    if (frame_dtype == 0) k_consistency_pair<uint8_t><<<blocks, EV_THREADS, 0, s>>>((const uint8_t*)frame_a, (const uint8_t*)frame_b, g, o);
    else k_consistency_pair<float><<<blocks, EV_THREADS, 0, s>>>((const float*)frame_a, (const float*)frame_b, g, o);
    int rc = lae::check_launch("consistency_pair");
    if (rc != LAE_OK) return rc;
    // row 0 of the partials -> sse_out, row 1 -> count_out; no pixel valid: both 0, the division is the caller's
    k_sum_partials<<<2, EV_THREADS, 0, s>>>(scratch, blocks, CONS_MAX_BLOCKS, sse_out, count_out);
    return lae::check_launch("consistency_pair_sum");
}

}  // extern "C"
