// exposure.hip -- per-image exposure and white balance learned inside the training step (lae_exposure_step, lae_exposure_publish,
// include/laenerf.h).
//
// The reference takes every training image as shot with one exposure and one white balance; Instant-NGP learns a per-image exposure
// beside its extrinsics.  Here image i carries a log2 gain e[i][c] per colour channel.  The sampler (batch.hip, the *_gain entry points)
// multiplies the TARGET colour by gains[i][c] = 2^(e[i][c] - mean_i e[.][c]) before the background blend and leaves fg, the part of the
// target that scales with the gain.  Every colour criterion of the fused step is a function of pred - gt (MAPE's denominator is
// detached), so d loss / d gt = -d loss / d pred, and with d gt / d e = ln 2 * fg
//     G[i][c] = d loss / d e[i][c] = -(ln 2 / (3 N)) sum over the rays n of image i of  w_n^2 * dv(pred_nc - gt_nc) * fg_nc
// is recomputed from the two [N,3] arrays the step leaves (its image and the batch's gt): the compositing kernels are not touched.  The
// gradient is analytic and unscaled: the loss scale does not enter.
//
// k_exposure_step: one workgroup per image -- the sum above in fp64 and in a fixed order (thread t adds its rays t, t + 1024, ... in
// order, then the 1024 partial sums are added as a fixed tree), a sparse Adam step with the image's own count, e <- e + delta on the fp64
// master.  Every thread loads its rays' values whether or not they are the image's and selects afterwards: the loads of the unrolled
// iterations are in flight together (with a branch around them the kernel's time was one memory latency per ray and thread).
// k_exposure_publish: one workgroup -- the per-channel mean of the master over the images, then the fp32 gains.
//
// The mean is subtracted only where the gains are published.  A common gain cannot be told from a brighter scene, so without the
// centring the common mode drifts; the master itself is not re-centred, which keeps the Adam moments consistent with it.  The gradient
// above ignores the -1/n coupling of every gain to every other image's e through that mean, deliberately: the centring is a projection
// applied after the step, not a part of the model the step differentiates.
#include <math.h>
#include "lae_common.h"

namespace {

constexpr int EX_THREADS = 1024;

__device__ __forceinline__ void block_tree_sum(double (*red)[EX_THREADS], int rows, uint32_t t) {      // row sums end in red[.][0]
    __syncthreads();
    for (uint32_t s = EX_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s)
            for (int c = 0; c < rows; c++) red[c][t] += red[c][t + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(EX_THREADS) void k_exposure_step(
    const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ fg, const int64_t* __restrict__ inds,
    uint32_t N, uint64_t hw, uint32_t n_img, const void* __restrict__ weights, int w_dtype, int kind, float delta, int gray,
    double* __restrict__ master, double* __restrict__ m, double* __restrict__ v, int32_t* __restrict__ counts,
    const int32_t* __restrict__ opt_state, const float* __restrict__ lr, double beta1, double beta2, double eps) {
    __shared__ double red[4][EX_THREADS];
    const uint32_t img = blockIdx.x, t = threadIdx.x;
    if (img >= n_img) return;
    double a[3] = {0.0, 0.0, 0.0}, cnt = 0.0;
    const uint64_t lo = (uint64_t)img * hw, hi = lo + hw;                  // inds[n] / hw == img, without the division
#pragma unroll 4
    for (uint32_t n = t; n < N; n += EX_THREADS) {
        const uint64_t pi = (uint64_t)inds[n];
        const bool mine = pi >= lo && pi < hi;                             // hence pi < n_img * hw, the weight plane's size
        double w2 = 1.0;
        if (weights && mine) {
            const double w = w_dtype == LAE_IMG_F16 ? (double)(float)reinterpret_cast<const _Float16*>(weights)[pi]
                                                    : (double)reinterpret_cast<const float*>(weights)[pi];
            w2 = w * w;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float g = gt[3 * (size_t)n + c];
            const float e = __fsub_rn(pred[3 * (size_t)n + c], g);         // the step's own residual
            float dv = lae::colour_elem_loss(kind, delta, e, g).dv;
            if (e != e) dv = e;                                            // sign(NaN) is 0 there; here a NaN residual must reach G
            const double term = (w2 * (double)dv) * (double)fg[3 * (size_t)n + c];
            if (mine) a[c] += term;
        }
        if (mine) cnt += 1.0;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) red[c][t] = a[c];
    red[3][t] = cnt;
    block_tree_sum(red, 4, t);
    if (t >= 3) return;                                                    // thread c updates channel c (one wave: in step)
    if (red[3][0] == 0.0 || opt_state[3] != 0) return;                     // no ray of this image in the batch; a skipped step
    const double k = -(0.69314718055994530942 / (3.0 * (double)N));
    double G[3];
#pragma unroll
    for (int c = 0; c < 3; c++) G[c] = k * red[c][0];
    if (gray) { const double s = (G[0] + G[1]) + G[2]; G[0] = G[1] = G[2] = s; }
    if (!(isfinite(G[0]) && isfinite(G[1]) && isfinite(G[2]))) return;
    const int32_t step = counts[img] + 1;                                  // read by the three threads before thread 0 writes it
    __builtin_amdgcn_wave_barrier();
    if (t == 0) counts[img] = step;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    const double step_size = (double)lr[0] / bc1;
    const double Gc = t == 0 ? G[0] : (t == 1 ? G[1] : G[2]);
    const size_t i = 3 * (size_t)img + t;
    const double mm = beta1 * m[i] + (1.0 - beta1) * Gc;
    const double vv = beta2 * v[i] + (1.0 - beta2) * (Gc * Gc);
    m[i] = mm; v[i] = vv;
    const double d = -(step_size * (mm / (sqrt(vv) / bc2_sqrt + eps)));
    if (d != 0.0) master[i] += d;                                          // a zero step keeps the operand's bits
}

__global__ __launch_bounds__(EX_THREADS) void k_exposure_publish(const double* __restrict__ master, uint32_t n_img, int center,
                                                                 float* __restrict__ gains) {
    __shared__ double red[3][EX_THREADS];
    const uint32_t t = threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    if (center)
        for (uint32_t i = t; i < n_img; i += EX_THREADS)
#pragma unroll
            for (int c = 0; c < 3; c++) a[c] += master[3 * (size_t)i + c];
#pragma unroll
    for (int c = 0; c < 3; c++) red[c][t] = a[c];
    block_tree_sum(red, 3, t);
    const double mean[3] = {red[0][0] / (double)n_img, red[1][0] / (double)n_img, red[2][0] / (double)n_img};
    for (uint32_t i = t; i < n_img; i += EX_THREADS)
#pragma unroll
        for (int c = 0; c < 3; c++) gains[3 * (size_t)i + c] = (float)exp2(master[3 * (size_t)i + c] - mean[c]);
}

}  // namespace

extern "C" {

int lae_exposure_step(const float* pred, const float* gt, const float* fg, const int64_t* inds, uint32_t N, uint64_t hw, uint32_t n_img,
                      const void* weights, int weights_dtype, int loss_kind, float loss_param, int gray, double* master, double* m,
                      double* v, int32_t* counts, const int32_t* opt_state, const float* lr, double beta1, double beta2, double eps,
                      void* stream) {
    if (n_img == 0) return LAE_OK;
    if (!master || !m || !v || !counts || !opt_state || !lr || (N > 0 && (!pred || !gt || !fg || !inds))) return LAE_ENULL;
    if (hw == 0 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return LAE_EINVAL;
    if (!lae::colour_loss_kind_ok(loss_kind, loss_param)) return LAE_EINVAL;
    if (weights && weights_dtype != LAE_IMG_F16 && weights_dtype != LAE_IMG_F32) return LAE_EINVAL;
    hipLaunchKernelGGL(k_exposure_step, dim3(n_img), dim3(EX_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pred, gt, fg, inds, N,
                       hw, n_img, weights, weights_dtype, loss_kind, loss_param, gray != 0, master, m, v, counts, opt_state, lr, beta1,
                       beta2, eps);
    return lae::check_launch("exposure_step");
}

int lae_exposure_publish(const double* master, uint32_t n_img, int center, float* gains, void* stream) {
    if (n_img == 0) return LAE_OK;
    if (!master || !gains) return LAE_ENULL;
    hipLaunchKernelGGL(k_exposure_publish, dim3(1), dim3(EX_THREADS), 0, reinterpret_cast<hipStream_t>(stream), master, n_img,
                       center != 0, gains);
    return lae::check_launch("exposure_publish");
}

}  // extern "C"
