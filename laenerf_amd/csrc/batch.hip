// batch.hip -- one training batch from a device-resident image stack (lae_sample_train_batch, include/laenerf.h).
//
// The reference draws a batch per step on the host side of its loader and in ~15 torch launches: NeRFDataset.collate ->
// get_rays (nerf/provider.py:294-343, nerf/utils.py:62-153) -> Trainer.train_step's gather, sRGB conversion and random
// background blend (nerf/utils.py:560-580).  Here one thread per ray draws its image / pixel / background with a
// counter-based generator keyed by (seed, step), gathers the pixel, builds the ray with the arithmetic of lae_get_rays
// and blends; the step is read from device memory and advanced by a second one-thread launch, so a captured graph
// draws a fresh batch on every replay.
//
// lae_sample_train_batch_patch draws square pixel patches instead of independent pixels (the reference's --patch_size,
// nerf/utils.py:88-105): the same per-ray body, another pixel rule.
//
// The *_gain entry points (lae_sample_train_batch_gain, lae_sample_train_batch_weighted_gain) multiply the colour by a per-image,
// per-channel gain before the blend and also write fg, the part of the target that scales with it: the exposure refinement of
// exposure.hip.  They are the same kernels instantiated with GAIN = true; the entry points without a gain compile without the multiply.
//
// Compiled with -ffp-contract=off like every file of the library: the blend is rgb * a + bg * (1 - a) with three
// roundings, in the reference's order.
#include "lae_common.h"
#include "raymarch_common.h"
#include "philox.h"

namespace {

using lae::philox4x32_10_w0;

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

// the per-ray body shared by both samplers: ray and near / far of pixel `pix` of image `img`, the texel gather, the
// background draw (words 2..4 of ray n) and the blend.  GAIN (the *_gain entry points): the colour is multiplied by the image's
// gain before the blend, one rounding, and fg receives the part of the target that scales with it (the background does not); a
// gain of 1.0f gives the bits of GAIN = false, whose instantiations hold no multiply
template <int DT, bool GAIN>
__device__ __forceinline__ void batch_ray(
    const void* __restrict__ images, uint64_t HW, uint32_t W, uint32_t C, const float* __restrict__ poses, float fx, float fy,
    float cx, float cy, const float* __restrict__ aabb, float min_near, const BatchRng& rng, uint32_t n, uint32_t img, uint32_t pix,
    int bg_mode, int linear, float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears,
    float* __restrict__ fars, float* __restrict__ gt, float* __restrict__ bg_out, int64_t* __restrict__ inds,
    const float* __restrict__ gains, float* __restrict__ fg) {
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
        if constexpr (GAIN) rgb[c] = __fmul_rn(rgb[c], gains[3 * (size_t)img + c]);
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
        for (int c = 0; c < 3; c++) {
            const float f = __fmul_rn(rgb[c], a);
            if constexpr (GAIN) fg[3 * (size_t)n + c] = f;
            rgb[c] = __fadd_rn(f, __fmul_rn(bg[c], one_minus_a));
        }
    } else if constexpr (GAIN) {
#pragma unroll
        for (int c = 0; c < 3; c++) fg[3 * (size_t)n + c] = rgb[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) gt[3 * (size_t)n + c] = rgb[c];
}

template <int DT, bool GAIN>
__global__ __launch_bounds__(256) void k_sample_train_batch(
    const void* __restrict__ images, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
    const float* __restrict__ poses, float fx, float fy, float cx, float cy, uint32_t N, const float* __restrict__ aabb,
    float min_near, uint32_t k0, uint32_t k1, const int64_t* __restrict__ step_counter, int mode, int bg_mode, int linear,
    float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears, float* __restrict__ fars,
    float* __restrict__ gt, float* __restrict__ bg_out, int64_t* __restrict__ inds, const float* __restrict__ gains,
    float* __restrict__ fg) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const BatchRng rng{(uint32_t)(uint64_t)step_counter[0], k0, k1};
    const uint64_t HW = (uint64_t)H * W;
    const uint32_t pix = scale_u32(rng.u(n, 0), HW);                                 // < H * W
    const uint32_t img = scale_u32(rng.u(mode == LAE_BATCH_IMAGE ? 0xFFFFFFFFu : n, 1), n_img);   // < n_img
    batch_ray<DT, GAIN>(images, HW, W, C, poses, fx, fy, cx, cy, aabb, min_near, rng, n, img, pix, bg_mode, linear, rays_o, rays_d,
                        nears, fars, gt, bg_out, inds, gains, fg);
}

// ---------------------------------------------------------------- the weighted draw (lae_sample_train_batch_weighted)
constexpr uint32_t EM_SIDE = 128, EM_CELLS = EM_SIDE * EM_SIDE;      // the reference's 128 x 128 error map
constexpr uint32_t SEL_THREADS = 1024, SEL_PER = EM_CELLS / SEL_THREADS;   // 16 consecutive cells per thread

// -ln(u) for u = j * 2^-25, j odd in [1, 2^25) (u = ((v >> 8) + 0.5) * 2^-24): the rule of include/laenerf.h.  The reduction
// u = m * 2^e, m = 1 + f in [sqrt(1/2), sqrt(2)) is done on the integer j, so f = (j - 2^p) * 2^-p is exact in fp32 (|j - 2^p| <
// 2^24) even where u itself is not; then log1p(f) = f - f^2/2 + f^3 P(f) (a degree-8 minimax P, Cephes logf) and e * ln 2
// in two parts, every operation one fp32 rounding in the stated order.
__device__ __forceinline__ float neg_log_u(uint32_t j) {
    int p = 32 - __clz(j);                                             // j in [2^(p-1), 2^p)
    if (2ull * j * j < (1ull << (2 * p))) p -= 1;                      // j / 2^p < sqrt(1/2): one octave down
    const float f = __fmul_rn((float)((int32_t)j - (int32_t)(1u << p)), __int_as_float((127 - p) << 23));
    const float e = (float)(p - 25);
    const float z = __fmul_rn(f, f);
    float P = 7.0376836292e-2f;
    P = __fadd_rn(__fmul_rn(P, f), -1.1514610310e-1f);
    P = __fadd_rn(__fmul_rn(P, f), 1.1676998740e-1f);
    P = __fadd_rn(__fmul_rn(P, f), -1.2420140846e-1f);
    P = __fadd_rn(__fmul_rn(P, f), 1.4249322787e-1f);
    P = __fadd_rn(__fmul_rn(P, f), -1.6668057665e-1f);
    P = __fadd_rn(__fmul_rn(P, f), 2.0000714765e-1f);
    P = __fadd_rn(__fmul_rn(P, f), -2.4999993993e-1f);
    P = __fadd_rn(__fmul_rn(P, f), 3.3333331174e-1f);
    float y = __fmul_rn(f, __fmul_rn(z, P));
    y = __fadd_rn(y, __fmul_rn(e, -2.12194440e-4f));
    y = __fadd_rn(y, __fmul_rn(-0.5f, z));
    float r = __fadd_rn(f, y);
    r = __fadd_rn(r, __fmul_rn(e, 0.693359375f));
    return -r;
}

// the bit pattern of key = w / E (>= +0: a weight that is negative, NaN or infinite counts as 0)
__device__ __forceinline__ uint32_t cell_key(float w, uint32_t step, uint32_t c, uint32_t k0, uint32_t k1) {
    if (!(w > 0.0f) || !(w < INFINITY)) return 0u;
    const uint32_t v = philox4x32_10_w0(step, c, 0u, 1u, k0, k1);
    return __float_as_uint(__fdiv_rn(w, neg_log_u(((v >> 8) << 1) | 1u)));
}

// exclusive prefix sum over the 1024 threads of the block (wave64 shuffles, then the 16 wave totals through LDS)
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* __restrict__ s_wave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SEL_THREADS / 64; w++) {
        const uint32_t t = s_wave[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();                                                   // s_wave is reused by the next scan
    total = all;
    return before + x - v;
}

// the N largest keys of one image's map (4 passes of an 8-bit radix select for the N-th largest key T, then the keys > T
// and the lowest-index keys == T), written in increasing cell order
__global__ __launch_bounds__(SEL_THREADS) void k_select_cells(
    const float* __restrict__ error_map, uint32_t n_img, uint32_t N, uint32_t k0, uint32_t k1,
    const int64_t* __restrict__ step_counter, int32_t* __restrict__ cells_out) {
    __shared__ uint32_t s_hist[256], s_wave[SEL_THREADS / 64], s_digit, s_rank;
    const BatchRng rng{(uint32_t)(uint64_t)step_counter[0], k0, k1};
    const uint32_t img = scale_u32(rng.u(0xFFFFFFFFu, 1), n_img);    // the uniform sampler's image rule
    const float* __restrict__ row = error_map + (size_t)img * EM_CELLS;
    const uint32_t t = threadIdx.x, c0 = t * SEL_PER;
    uint32_t key[SEL_PER];
#pragma unroll
    for (uint32_t i = 0; i < SEL_PER; i++) key[i] = cell_key(row[c0 + i], rng.step, c0 + i, k0, k1);

    uint32_t prefix = 0, rank = N;                                     // rank: the wanted key's 1-based rank among the matching keys
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        const uint32_t hi_mask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
        if (t < 256) s_hist[t] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < SEL_PER; i++)
            if ((key[i] & hi_mask) == prefix) atomicAdd(&s_hist[(key[i] >> shift) & 255u], 1u);
        __syncthreads();
        // the digit d with (count of digits > d) < rank <= (count of digits >= d): thread t < 256 holds bin 255 - t, so its
        // exclusive prefix sum is the count above that bin
        const uint32_t h = t < 256 ? s_hist[255 - t] : 0u;
        uint32_t total;
        const uint32_t above = block_exclusive_scan(h, s_wave, total);
        if (t < 256 && above < rank && rank <= above + h) { s_digit = 255 - t; s_rank = rank - above; }
        __syncthreads();
        prefix |= s_digit << shift;
        rank = s_rank;
        __syncthreads();
    }
    const uint32_t T = prefix;                                        // the N-th largest key; `rank` of the keys == T are taken
    uint32_t gt = 0, eq = 0;
#pragma unroll
    for (uint32_t i = 0; i < SEL_PER; i++) { gt += key[i] > T; eq += key[i] == T; }
    uint32_t total;
    const uint32_t eq_before = block_exclusive_scan(eq, s_wave, total);
    const uint32_t take_eq = eq_before >= rank ? 0u : min(eq, rank - eq_before);
    const uint32_t pos0 = block_exclusive_scan(gt + take_eq, s_wave, total);
    uint32_t pos = pos0, ties = 0;
#pragma unroll
    for (uint32_t i = 0; i < SEL_PER; i++) {
        bool take = key[i] > T;
        if (key[i] == T) { take = ties < take_eq; ties++; }
        if (take && pos < N) cells_out[pos++] = (int32_t)(c0 + i);
    }
}

// one thread per ray: the pixel drawn inside its cell, then the uniform sampler's per-ray body
template <int DT, bool GAIN>
__global__ __launch_bounds__(256) void k_sample_train_batch_weighted(
    const void* __restrict__ images, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
    const float* __restrict__ poses, float fx, float fy, float cx, float cy, uint32_t N, const float* __restrict__ aabb,
    float min_near, uint32_t k0, uint32_t k1, const int64_t* __restrict__ step_counter, int bg_mode, int linear,
    float sx, float sy, const int32_t* __restrict__ cells, float* __restrict__ rays_o, float* __restrict__ rays_d,
    float* __restrict__ nears, float* __restrict__ fars, float* __restrict__ gt, float* __restrict__ bg_out,
    int64_t* __restrict__ inds, const float* __restrict__ gains, float* __restrict__ fg) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const BatchRng rng{(uint32_t)(uint64_t)step_counter[0], k0, k1};
    const uint64_t HW = (uint64_t)H * W;
    const uint32_t img = scale_u32(rng.u(0xFFFFFFFFu, 1), n_img);
    const uint32_t c = (uint32_t)cells[n];
    const float rx = (float)(rng.u(n, 0) >> 8) * 0x1p-24f, ry = (float)(rng.u(n, 5) >> 8) * 0x1p-24f;
    const float fr = __fadd_rn(__fmul_rn((float)(c / EM_SIDE), sx), __fmul_rn(rx, sx));
    const float fc = __fadd_rn(__fmul_rn((float)(c % EM_SIDE), sy), __fmul_rn(ry, sy));
    const uint32_t r = min((uint32_t)fr, H - 1), col = min((uint32_t)fc, W - 1);    // trunc of a value >= 0
    batch_ray<DT, GAIN>(images, HW, W, C, poses, fx, fy, cx, cy, aabb, min_near, rng, n, img, r * W + col, bg_mode, linear, rays_o,
                        rays_d, nears, fars, gt, bg_out, inds, gains, fg);
}

// ---------------------------------------------------------------- the patch draw (lae_sample_train_batch_patch)
// one thread per ray: ray n is pixel (n % P^2) of patch q = n / P^2, row-major inside the patch; the patch's top-left corner comes from
// words 5 and 6 of "ray" q with the reference's exclusive bounds H - P and W - P (nerf/utils.py:93-94), its image from word 1 of
// 0xFFFFFFFF (LAE_BATCH_IMAGE) or of q (LAE_BATCH_ALL: an image per patch); then the uniform sampler's per-ray body
template <int DT>
__global__ __launch_bounds__(256) void k_sample_train_batch_patch(
    const void* __restrict__ images, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
    const float* __restrict__ poses, float fx, float fy, float cx, float cy, uint32_t N, uint32_t P, const float* __restrict__ aabb,
    float min_near, uint32_t k0, uint32_t k1, const int64_t* __restrict__ step_counter, int mode, int bg_mode, int linear,
    float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears, float* __restrict__ fars,
    float* __restrict__ gt, float* __restrict__ bg_out, int64_t* __restrict__ inds) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const BatchRng rng{(uint32_t)(uint64_t)step_counter[0], k0, k1};
    const uint64_t HW = (uint64_t)H * W;
    const uint32_t PP = P * P, q = n / PP, rem = n % PP;
    const uint32_t row = scale_u32(rng.u(q, 5), H - P), col = scale_u32(rng.u(q, 6), W - P);      // < H - P, < W - P
    const uint32_t pix = (row + rem / P) * W + (col + rem % P);                                   // row + P - 1 < H - 1: inside the image
    const uint32_t img = scale_u32(rng.u(mode == LAE_BATCH_IMAGE ? 0xFFFFFFFFu : q, 1), n_img);
    batch_ray<DT, false>(images, HW, W, C, poses, fx, fy, cx, cy, aabb, min_near, rng, n, img, pix, bg_mode, linear, rays_o, rays_d,
                         nears, fars, gt, bg_out, inds, nullptr, nullptr);
}

// one thread per ray: map[image][cell] = 0.1 * map + 0.9 * mean over RGB of (pred - gt)^2
__global__ __launch_bounds__(256) void k_error_map_update(
    float* __restrict__ error_map, uint32_t n_img, uint64_t HW, const int64_t* __restrict__ inds, const int32_t* __restrict__ cells,
    const float* __restrict__ pred, const float* __restrict__ gt, uint32_t N) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float d = __fsub_rn(pred[3 * (size_t)n + k], gt[3 * (size_t)n + k]);
        s = k == 0 ? __fmul_rn(d, d) : __fadd_rn(s, __fmul_rn(d, d));
    }
    const float err = __fdiv_rn(s, 3.0f);
    const uint64_t img = (uint64_t)inds[n] / HW;
    const uint32_t c = (uint32_t)cells[n];
    if (img >= n_img || c >= EM_CELLS) return;                        // not a batch of this stack: nothing to update
    float* m = error_map + (size_t)img * EM_CELLS + c;
    *m = __fadd_rn(__fmul_rn(0.1f, *m), __fmul_rn(0.9f, err));
}

// k_error_map_update with the element loss of another colour criterion in the squared error's place (lae::colour_elem_loss)
__global__ __launch_bounds__(256) void k_error_map_update_crit(
    float* __restrict__ error_map, uint32_t n_img, uint64_t HW, const int64_t* __restrict__ inds, const int32_t* __restrict__ cells,
    const float* __restrict__ pred, const float* __restrict__ gt, uint32_t N, int kind, float delta) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float g = gt[3 * (size_t)n + k];
        const float v = lae::colour_elem_loss(kind, delta, __fsub_rn(pred[3 * (size_t)n + k], g), g).v;
        s = k == 0 ? v : __fadd_rn(s, v);
    }
    const float err = __fdiv_rn(s, 3.0f);
    const uint64_t img = (uint64_t)inds[n] / HW;
    const uint32_t c = (uint32_t)cells[n];
    if (img >= n_img || c >= EM_CELLS) return;
    float* m = error_map + (size_t)img * EM_CELLS + c;
    *m = __fadd_rn(__fmul_rn(0.1f, *m), __fmul_rn(0.9f, err));
}

__global__ void k_advance_step(int64_t* __restrict__ step_counter) { step_counter[0] += 1; }

// the bodies of the sampler entry points; GAIN: the *_gain siblings (gains [n_img,3] read, fg [N,3] written)
template <bool GAIN>
int sample_uniform(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C, const float* poses, float fx,
                   float fy, float cx, float cy, uint32_t N, const float* aabb, float min_near, uint64_t seed, int64_t* step_counter,
                   int mode, int bg_mode, int srgb_to_linear, const float* gains, float* rays_o, float* rays_d, float* nears,
                   float* fars, float* gt, float* fg, float* bg_out, int64_t* inds, void* stream) {
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
                       srgb_to_linear, rays_o, rays_d, nears, fars, gt, bg_out, inds, gains, fg
    if (dtype == LAE_IMG_U8) k_sample_train_batch<LAE_IMG_U8, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else if (dtype == LAE_IMG_F16) k_sample_train_batch<LAE_IMG_F16, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else k_sample_train_batch<LAE_IMG_F32, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
#undef LAE_BATCH_ARGS
    k_advance_step<<<1, 1, 0, s>>>(step_counter);
    return lae::check_launch("sample_train_batch");
}

template <bool GAIN>
int sample_weighted(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C, const float* poses, float fx,
                    float fy, float cx, float cy, uint32_t N, const float* aabb, float min_near, uint64_t seed, int64_t* step_counter,
                    int bg_mode, int srgb_to_linear, const float* error_map, int32_t* cells_out, const float* gains, float* rays_o,
                    float* rays_d, float* nears, float* fars, float* gt, float* fg, float* bg_out, int64_t* inds, void* stream) {
    if (N == 0) return LAE_OK;
    if (!images || !poses || !aabb || !step_counter || !error_map || !cells_out || !rays_o || !rays_d || !nears || !fars || !gt ||
        !inds) return LAE_ENULL;
    if (bg_mode == LAE_BG_RANDOM && !bg_out) return LAE_ENULL;
    if (N > EM_CELLS) return LAE_EINVAL;
    if (n_img == 0 || H == 0 || W == 0 || (C != 3 && C != 4) || (uint64_t)H * W > 0xFFFFFFFFull) return LAE_EINVAL;
    if (dtype != LAE_IMG_U8 && dtype != LAE_IMG_F16 && dtype != LAE_IMG_F32) return LAE_EINVAL;
    if (bg_mode != LAE_BG_WHITE && bg_mode != LAE_BG_RANDOM) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float sx = (float)((double)H / EM_SIDE), sy = (float)((double)W / EM_SIDE);
    k_select_cells<<<1, SEL_THREADS, 0, s>>>(error_map, n_img, N, k0, k1, step_counter, cells_out);
    const dim3 grid(lae::cdiv(N, 256)), block(256);
#define LAE_BATCH_ARGS images, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, k0, k1, step_counter, bg_mode, \
                       srgb_to_linear, sx, sy, cells_out, rays_o, rays_d, nears, fars, gt, bg_out, inds, gains, fg
    if (dtype == LAE_IMG_U8) k_sample_train_batch_weighted<LAE_IMG_U8, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else if (dtype == LAE_IMG_F16) k_sample_train_batch_weighted<LAE_IMG_F16, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else k_sample_train_batch_weighted<LAE_IMG_F32, GAIN><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
#undef LAE_BATCH_ARGS
    k_advance_step<<<1, 1, 0, s>>>(step_counter);
    return lae::check_launch("sample_train_batch_weighted");
}

}  // namespace

extern "C" {

int lae_sample_train_batch(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                           const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                           const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                           int srgb_to_linear, float* rays_o, float* rays_d, float* nears, float* fars, float* gt,
                           float* bg_out, int64_t* inds, void* stream) {
    return sample_uniform<false>(images, dtype, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, seed, step_counter, mode, bg_mode,
                                 srgb_to_linear, nullptr, rays_o, rays_d, nears, fars, gt, nullptr, bg_out, inds, stream);
}

int lae_sample_train_batch_gain(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                                int srgb_to_linear, const float* gains, float* rays_o, float* rays_d, float* nears, float* fars,
                                float* gt, float* fg, float* bg_out, int64_t* inds, void* stream) {
    if (N > 0 && (!gains || !fg)) return LAE_ENULL;
    return sample_uniform<true>(images, dtype, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, seed, step_counter, mode, bg_mode,
                                srgb_to_linear, gains, rays_o, rays_d, nears, fars, gt, fg, bg_out, inds, stream);
}

int lae_sample_train_batch_weighted(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                    const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                    const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int bg_mode,
                                    int srgb_to_linear, const float* error_map, int32_t* cells_out, float* rays_o, float* rays_d,
                                    float* nears, float* fars, float* gt, float* bg_out, int64_t* inds, void* stream) {
    return sample_weighted<false>(images, dtype, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, seed, step_counter, bg_mode,
                                  srgb_to_linear, error_map, cells_out, nullptr, rays_o, rays_d, nears, fars, gt, nullptr, bg_out, inds,
                                  stream);
}

int lae_sample_train_batch_weighted_gain(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                         const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                         const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int bg_mode,
                                         int srgb_to_linear, const float* error_map, int32_t* cells_out, const float* gains,
                                         float* rays_o, float* rays_d, float* nears, float* fars, float* gt, float* fg, float* bg_out,
                                         int64_t* inds, void* stream) {
    if (N > 0 && (!gains || !fg)) return LAE_ENULL;
    return sample_weighted<true>(images, dtype, n_img, H, W, C, poses, fx, fy, cx, cy, N, aabb, min_near, seed, step_counter, bg_mode,
                                 srgb_to_linear, error_map, cells_out, gains, rays_o, rays_d, nears, fars, gt, fg, bg_out, inds, stream);
}

int lae_sample_train_batch_patch(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                 const float* poses, float fx, float fy, float cx, float cy, uint32_t N, uint32_t patch_size,
                                 const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                                 int srgb_to_linear, float* rays_o, float* rays_d, float* nears, float* fars, float* gt,
                                 float* bg_out, int64_t* inds, void* stream) {
    const uint32_t P = patch_size;
    if (P < 2 || P >= H || P >= W || P > 0xFFFFu) return LAE_EINVAL;
    if (N == 0 || N % (P * P) != 0) return LAE_EINVAL;                     // whole patches only
    if (!images || !poses || !aabb || !step_counter || !rays_o || !rays_d || !nears || !fars || !gt || !inds) return LAE_ENULL;
    if (bg_mode == LAE_BG_RANDOM && !bg_out) return LAE_ENULL;
    if (n_img == 0 || (C != 3 && C != 4) || (uint64_t)H * W > 0xFFFFFFFFull) return LAE_EINVAL;
    if (dtype != LAE_IMG_U8 && dtype != LAE_IMG_F16 && dtype != LAE_IMG_F32) return LAE_EINVAL;
    if (mode != LAE_BATCH_IMAGE && mode != LAE_BATCH_ALL) return LAE_EINVAL;
    if (bg_mode != LAE_BG_WHITE && bg_mode != LAE_BG_RANDOM) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const dim3 grid(lae::cdiv(N, 256)), block(256);
#define LAE_BATCH_ARGS images, n_img, H, W, C, poses, fx, fy, cx, cy, N, P, aabb, min_near, k0, k1, step_counter, mode, bg_mode, \
                       srgb_to_linear, rays_o, rays_d, nears, fars, gt, bg_out, inds
    if (dtype == LAE_IMG_U8) k_sample_train_batch_patch<LAE_IMG_U8><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else if (dtype == LAE_IMG_F16) k_sample_train_batch_patch<LAE_IMG_F16><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
    else k_sample_train_batch_patch<LAE_IMG_F32><<<grid, block, 0, s>>>(LAE_BATCH_ARGS);
#undef LAE_BATCH_ARGS
    k_advance_step<<<1, 1, 0, s>>>(step_counter);
    return lae::check_launch("sample_train_batch_patch");
}

int lae_error_map_update(float* error_map, uint32_t n_img, uint32_t H, uint32_t W, const int64_t* inds, const int32_t* cells,
                         const float* pred, const float* gt, uint32_t N, void* stream) {
    if (N == 0) return LAE_OK;
    if (!error_map || !inds || !cells || !pred || !gt) return LAE_ENULL;
    if (n_img == 0 || H == 0 || W == 0 || N > EM_CELLS) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    k_error_map_update<<<lae::cdiv(N, 256), 256, 0, s>>>(error_map, n_img, (uint64_t)H * W, inds, cells, pred, gt, N);
    return lae::check_launch("error_map_update");
}

int lae_error_map_update_crit(float* error_map, uint32_t n_img, uint32_t H, uint32_t W, const int64_t* inds, const int32_t* cells,
                              const float* pred, const float* gt, uint32_t N, int loss_kind, float loss_param, void* stream) {
    if (!lae::colour_loss_kind_ok(loss_kind, loss_param)) return LAE_EINVAL;
    if (loss_kind == LAE_LOSS_MSE) return lae_error_map_update(error_map, n_img, H, W, inds, cells, pred, gt, N, stream);
    if (N == 0) return LAE_OK;
    if (!error_map || !inds || !cells || !pred || !gt) return LAE_ENULL;
    if (n_img == 0 || H == 0 || W == 0 || N > EM_CELLS) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    k_error_map_update_crit<<<lae::cdiv(N, 256), 256, 0, s>>>(error_map, n_img, (uint64_t)H * W, inds, cells, pred, gt, N, loss_kind,
                                                              loss_param);
    return lae::check_launch("error_map_update_crit");
}

}  // extern "C"
