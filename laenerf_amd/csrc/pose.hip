// pose.hip -- refinement of the training cameras inside the training step (lae_pose_ray_grad, lae_pose_step, include/laenerf.h).
//
// The reference takes its poses as exact; Instant-NGP optimises the extrinsics beside the field.  The gradient of the sample
// positions comes from lae_grid_input_grad (gridencoder.hip).  Moving camera (R, T) to (Exp(w) R, T + t) moves every sample x of
// its rays to T + t + Exp(w)(x - T), so at w = t = 0
//     d loss / d t = sum_k g_k,        d loss / d w = sum_k (x_k - T) x g_k.
// k_pose_ray_grad forms the two sums per ray, k_pose_step adds them per image, takes a sparse Adam step in that tangent space and
// composes it onto an fp64 master of the poses, from which the fp32 matrices the sampler reads are rewritten.  Everything is fp64
// and added in a fixed order: two runs give the same bits.
#include <math.h>
#include "lae_common.h"

namespace {

constexpr int PR_WAVES = 4;                                // rays per workgroup of k_pose_ray_grad: one wave each
constexpr int PS_THREADS = 256;

__device__ __forceinline__ double wave_tree_sum(double v) {               // lane 0 (every lane) holds the sum; a fixed butterfly
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(64 * PR_WAVES) void k_pose_ray_grad(
    const int32_t* __restrict__ rays, const float* __restrict__ xyzs, const float* __restrict__ grad_x, const float* __restrict__ rays_o,
    uint32_t N, uint32_t M, double* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = blockIdx.x * PR_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint32_t index = (uint32_t)rays[3 * (size_t)n], offset = (uint32_t)rays[3 * (size_t)n + 1], count = (uint32_t)rays[3 * (size_t)n + 2];
    if (index >= N) return;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool has = !(count == 0 || (uint64_t)offset + count > M);       // the compositing kernels' rule (load_ray_head, raymarching.hip)
    if (has) {
        const double o0 = rays_o[3 * (size_t)index], o1 = rays_o[3 * (size_t)index + 1], o2 = rays_o[3 * (size_t)index + 2];
        for (uint32_t k = lane; k < count; k += 64u) {
            const size_t i = 3 * ((size_t)offset + k);
            const double g0 = grad_x[i], g1 = grad_x[i + 1], g2 = grad_x[i + 2];
            const double r0 = (double)xyzs[i] - o0, r1 = (double)xyzs[i + 1] - o1, r2 = (double)xyzs[i + 2] - o2;
            a[0] += g0; a[1] += g1; a[2] += g2;
            a[3] += r1 * g2 - r2 * g1;
            a[4] += r2 * g0 - r0 * g2;
            a[5] += r0 * g1 - r1 * g0;
        }
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] = wave_tree_sum(a[c]);
    }
    if (lane < 6u) {
        double r = a[0];
#pragma unroll
        for (int c = 1; c < 6; c++) r = lane == (uint32_t)c ? a[c] : r;
        out[6 * (size_t)index + lane] = r;
    }
}

// Exp(w) as a row-major 3 x 3 matrix (Rodrigues): I + A K + B K^2, A = sin t / t, B = (1 - cos t) / t^2, t = |w|
__device__ __forceinline__ void exp_so3(const double w[3], double E[9]) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B;
    if (t2 < 1e-12) { A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0; }
    else { const double t = sqrt(t2); A = sin(t) / t; B = (1.0 - cos(t)) / t2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double k2 = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
            E[3 * i + j] = (i == j ? 1.0 : 0.0) + (A * K[3 * i + j] + B * k2);
        }
}

__global__ __launch_bounds__(PS_THREADS) void k_pose_step(
    const double* __restrict__ ray_grads, const int64_t* __restrict__ inds, uint32_t N, uint64_t hw, uint32_t n_img,
    double* __restrict__ master, double* __restrict__ m, double* __restrict__ v, int32_t* __restrict__ counts,
    float* __restrict__ train_poses, const int32_t* __restrict__ opt_state, const float* __restrict__ lr, double beta1, double beta2,
    double eps) {
    __shared__ double red[7][PS_THREADS];
    const uint32_t img = blockIdx.x, t = threadIdx.x;
    if (img >= n_img) return;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, cnt = 0.0;
    for (uint32_t n = t; n < N; n += PS_THREADS) {
        if ((uint64_t)inds[n] / hw != (uint64_t)img) continue;
#pragma unroll
        for (int c = 0; c < 6; c++) a[c] += ray_grads[6 * (size_t)n + c];
        cnt += 1.0;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) red[c][t] = a[c];
    red[6][t] = cnt;
    __syncthreads();
    for (uint32_t s = PS_THREADS / 2; s >= 1; s >>= 1) {                  // a fixed tree
        if (t < s) {
#pragma unroll
            for (int c = 0; c < 7; c++) red[c][t] += red[c][t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    if (red[6][0] == 0.0 || opt_state[3] != 0) return;                    // no ray of this image in the batch; a skipped step
    const double inv_scale = (double)__int_as_float(opt_state[7]);
    double g[6];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 6; c++) { g[c] = red[c][0] * inv_scale; finite &= isfinite(g[c]); }
    if (!finite) return;
    const int32_t step = counts[img] + 1;
    counts[img] = step;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    const double step_size = (double)lr[0] / bc1;
    double d[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double mm = beta1 * m[6 * (size_t)img + c] + (1.0 - beta1) * g[c];
        const double vv = beta2 * v[6 * (size_t)img + c] + (1.0 - beta2) * (g[c] * g[c]);
        m[6 * (size_t)img + c] = mm; v[6 * (size_t)img + c] = vv;
        d[c] = -(step_size * (mm / (sqrt(vv) / bc2_sqrt + eps)));
    }
    double* P = master + 12 * (size_t)img;                                // rows of [R | tau]
    if (d[3] != 0.0 || d[4] != 0.0 || d[5] != 0.0) {
        double E[9], R[9];
        exp_so3(d + 3, E);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[3 * i + j] = P[4 * i + j];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) P[4 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (d[i] != 0.0) P[4 * i + 3] += d[i];
    float* out = train_poses + 16 * (size_t)img;
#pragma unroll
    for (int i = 0; i < 12; i++) out[i] = (float)P[i];
}

}  // namespace

extern "C" {

int lae_pose_ray_grad(const int32_t* rays, const float* xyzs, const float* grad_x, const float* rays_o, uint32_t N, uint32_t M,
                      double* out, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays || !rays_o || !out || (M > 0 && (!xyzs || !grad_x))) return LAE_ENULL;
    hipLaunchKernelGGL(k_pose_ray_grad, dim3(lae::cdiv(N, PR_WAVES)), dim3(64 * PR_WAVES), 0, reinterpret_cast<hipStream_t>(stream),
                       rays, xyzs, grad_x, rays_o, N, M, out);
    return lae::check_launch("pose_ray_grad");
}

int lae_pose_step(const double* ray_grads, const int64_t* inds, uint32_t N, uint64_t hw, uint32_t n_img, double* master, double* m,
                  double* v, int32_t* counts, float* train_poses, const int32_t* opt_state, const float* lr, double beta1, double beta2,
                  double eps, void* stream) {
    if (n_img == 0) return LAE_OK;
    if (!master || !m || !v || !counts || !train_poses || !opt_state || !lr || (N > 0 && (!ray_grads || !inds))) return LAE_ENULL;
    if (hw == 0 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return LAE_EINVAL;
    hipLaunchKernelGGL(k_pose_step, dim3(n_img), dim3(PS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ray_grads, inds, N, hw,
                       n_img, master, m, v, counts, train_poses, opt_state, lr, beta1, beta2, eps);
    return lae::check_launch("pose_step");
}

}  // extern "C"
