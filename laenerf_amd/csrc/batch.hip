// batch.hip -- one training batch from a device-resident image stack (lae_sample_train_batch, include/laenerf.h).
//
// The reference draws a batch per step on the host side of its loader and in ~15 torch launches: NeRFDataset.collate ->
// get_rays (nerf/provider.py:294-343, nerf/utils.py:62-153) -> Trainer.train_step's gather, sRGB conversion and random
// background blend (nerf/utils.py:560-580).  Here one thread per ray draws its image / pixel / background with a
// counter-based generator keyed by (seed, step), gathers the pixel, builds the ray with the arithmetic of lae_get_rays
// and blends; the step is read from device memory and advanced by a second one-thread launch, so a captured graph
// draws a fresh batch on every replay.
//
// Compiled with -ffp-contract=off like every file of the library: the blend is rgb * a + bg * (1 - a) with three
// roundings, in the reference's order.
#include "lae_common.h"
#include "raymarch_common.h"

namespace {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011): returns word 0 of the block
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

struct BatchRng {
    uint32_t step, k0, k1;
    __device__ __forceinline__ uint32_t u(uint32_t ray, uint32_t word) const { return philox4x32_10_w0(step, ray, word, 0u, k0, k1); }
};

__device__ __forceinline__ uint32_t scale_u32(uint32_t u, uint64_t n) { return (uint32_t)(((uint64_t)u * n) >> 32); }

// 0..255 / 255 as numpy's astype(float32) / 255 computes it (a table filled at compile time with correctly rounded fp32
// divisions: no question of the device's division mode or a reciprocal)
struct U8Table { float v[256]; };
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int i = 0; i < 256; i++) t.v[i] = (float)i / 255.0f;
    return t;
}
__constant__ U8Table c_u8 = make_u8_table();

__device__ __forceinline__ float srgb_to_linear(float x) {            // nerf/utils.py srgb_to_linear
    return x < 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f);
}

template <int DT>
__device__ __forceinline__ float texel(const void* __restrict__ images, size_t e) {
    if (DT == LAE_IMG_U8) return c_u8.v[reinterpret_cast<const uint8_t*>(images)[e]];
    if (DT == LAE_IMG_F16) return (float)reinterpret_cast<const _Float16*>(images)[e];      // exact widening
    return reinterpret_cast<const float*>(images)[e];
}

template <int DT>
__global__ __launch_bounds__(256) void k_sample_train_batch(
    const void* __restrict__ images, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
    const float* __restrict__ poses, float fx, float fy, float cx, float cy, uint32_t N, const float* __restrict__ aabb,
    float min_near, uint32_t k0, uint32_t k1, const int64_t* __restrict__ step_counter, int mode, int bg_mode, int linear,
    float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears, float* __restrict__ fars,
    float* __restrict__ gt, float* __restrict__ bg_out, int64_t* __restrict__ inds) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const BatchRng rng{(uint32_t)(uint64_t)step_counter[0], k0, k1};
    const uint64_t HW = (uint64_t)H * W;
    const uint32_t pix = scale_u32(rng.u(n, 0), HW);                                 // < H * W
    const uint32_t img = scale_u32(rng.u(mode == LAE_BATCH_IMAGE ? 0xFFFFFFFFu : n, 1), n_img);   // < n_img
    inds[n] = (int64_t)img * (int64_t)HW + pix;

    float o[3], d[3];
    pinhole_ray(poses + 16 * (size_t)img, fx, fy, cx, cy, W, (int64_t)pix, 0, 0.f, 0.f, o, d);
#pragma unroll
    for (int k = 0; k < 3; k++) { rays_o[3 * (size_t)n + k] = o[k]; rays_d[3 * (size_t)n + k] = d[k]; }
    ray_box(o, d, aabb, min_near, nears + n, fars + n);

    const size_t e = ((size_t)img * HW + pix) * C;
    float rgb[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        rgb[c] = texel<DT>(images, e + c);
        if (linear) rgb[c] = srgb_to_linear(rgb[c]);
    }
    float bg[3] = {1.f, 1.f, 1.f};
    if (bg_mode == LAE_BG_RANDOM) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            bg[c] = (float)(rng.u(n, 2 + c) >> 8) * 0x1p-24f;                       // exact: 24-bit integer times 2^-24
            bg_out[3 * (size_t)n + c] = bg[c];
        }
    }
    if (C == 4) {
        const float a = texel<DT>(images, e + 3);
        const float one_minus_a = __fsub_rn(1.0f, a);
#pragma unroll
        for (int c = 0; c < 3; c++) rgb[c] = __fadd_rn(__fmul_rn(rgb[c], a), __fmul_rn(bg[c], one_minus_a));
    }
#pragma unroll
    for (int c = 0; c < 3; c++) gt[3 * (size_t)n + c] = rgb[c];
}

__global__ void k_advance_step(int64_t* __restrict__ step_counter) { step_counter[0] += 1; }

}  // namespace

extern "C" {

int lae_sample_train_batch(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                           const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                           const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                           int srgb_to_linear, float* rays_o, float* rays_d, float* nears, float* fars, float* gt,
                           float* bg_out, int64_t* inds, void* stream) {
    if (N == 0) return LAE_OK;
    if (!images || !poses || !aabb || !step_counter || !rays_o || !rays_d || !nears || !fars || !gt || !inds) return LAE_ENULL;
    if (bg_mode == LAE_BG_RANDOM && !bg_out) return LAE_ENULL;
    if (n_img == 0 || H == 0 || W == 0 || (C != 3 && C != 4) || (uint64_t)H * W > 0xFFFFFFFFull) return LAE_EINVAL;
    if (dtype != LAE_IMG_U8 && dtype != LAE_IMG_F16 && dtype != LAE_IMG_F32) return LAE_EINVAL;
    if (mode != LAE_BATCH_IMAGE && mode != LAE_BATCH_ALL) return LAE_EINVAL;
    if (bg_mode != LAE_BG_WHITE && bg_mode != LAE_BG_RANDOM) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const dim3 grid(lae::cdiv(N, 256)), block(256);
#define LAE_BATCH_ARGS images, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, k0, k1, step_counter, mode, bg_mode, \
                       srgb_to_linear, rays_o, rays_d, nears, fars, gt, bg_out, inds
    if (dtype == LAE_IMG_U8) k_sample_train_batch<LAE_IMG_U8><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else if (dtype == LAE_IMG_F16) k_sample_train_batch<LAE_IMG_F16><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else k_sample_train_batch<LAE_IMG_F32><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
#undef LAE_BATCH_ARGS
    k_advance_step<<<1, 1, 0, s>>>(step_counter);
    return lae::check_launch("sample_train_batch");
}

}  // extern "C"
