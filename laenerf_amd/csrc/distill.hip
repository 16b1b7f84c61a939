// distill.hip -- LAENeRF's dataset rewrite before the edit is distilled into the NeRF (nerf/gui.py:357-541 distill_dataset: a per-view
// host loop of forward_train, ~20 torch ops, a host round trip of every image and a torchvision Resize in the reference).
//
// lae_distill_compose: one thread per extracted row over all views: the palette network's colour under the user's edit (the rule of
//   palette_edit.h, shared with lae_recolor_compose), the optional smooth transition towards the original palette, the blend with the
//   distill render, written into the row's training image where the edit weight exceeds the threshold.
// lae_error_map_seed: LAENeRF's --use_error_maps seed: the dense edit-weight image of every view, bilinearly resized to 128 x 128
//   (torch's align_corners=False rule, no antialiasing), + 0.15, clamped (include/laenerf.h states the rules).
// lae_ref_distill_init / lae_ref_distill_scatter: the data set of the Ref-NPR distillation (the reference's dataloader_nerf,
//   editing/single_view_edit_dataset.py:447-519: a per-view host loop of scatters and a host copy of five planes per view) over all
//   views at once: a dense pass that writes the background rule of the four planes, then one thread per packed row.
#include "lae_common.h"
#include "palette_edit.h"

namespace {

typedef _Float16 half_t;

constexpr int DC_THREADS = 256;
constexpr uint32_t SEED_SIDE = 128;
constexpr uint32_t SEED_CELLS = SEED_SIDE * SEED_SIDE;

struct DistillArgs {
    const int32_t* img; const int32_t* pix; const float* w; const float* pred; const float* dist;
    const half_t* w_logits; uint32_t w_stride;
    const half_t* o_raw; uint32_t o_stride;
    uint32_t active_mask;
    const float* palette_mod; const float* palette_og; const float* p_weights; const float* p_bias;
    float thresh;
    void* images; uint32_t n_img, HW, C;
    uint32_t R;
};

template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ half_t from_f32<half_t>(float x) { return (half_t)x; }      // round to nearest even

template <typename T, bool SMOOTH, bool NO_BG>
__global__ void __launch_bounds__(DC_THREADS) k_distill_compose(DistillArgs a) {
    const uint32_t r = blockIdx.x * DC_THREADS + threadIdx.x;
    if (r >= a.R) return;
    const float w = a.w[r];
    if (!(w > a.thresh)) return;                               // at or below the threshold: the pixel keeps the ground truth
    const uint32_t img = (uint32_t)a.img[r], pix = (uint32_t)a.pix[r];
    if (img >= a.n_img || pix >= a.HW) return;
    const half_t* wl = a.w_logits + (uint64_t)r * a.w_stride;
    const half_t* orw = a.o_raw + (uint64_t)r * a.o_stride;
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (float)tanh((double)(float)orw[c]);
    float l[16];
    const float sum = lae::palette_softmax_exp(wl, a.active_mask, l);
    lae::palette_normalise(l, a.active_mask, sum);
    float acc[3];
    if (SMOOTH) {
        // (d w_og + (1 - d) w') @ (d pal_og + (1 - d) pal_mod): every product and sum one rounding, columns in order
        float og[16];
#pragma unroll
        for (int j = 0; j < 16; j++) og[j] = l[j];
        lae::palette_edit(l, a.active_mask, a.p_weights, a.p_bias);
        const float d = a.dist[r];
        const float e = __fsub_rn(1.0f, d);
        acc[0] = acc[1] = acc[2] = 0.0f;
        int act = 0;
#pragma unroll
        for (int j = 0; j < 16; j++)
            if ((a.active_mask >> j) & 1u) {
                const float wi = __fadd_rn(__fmul_rn(d, og[j]), __fmul_rn(e, l[j]));
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float pi = __fadd_rn(__fmul_rn(d, a.palette_og[3 * act + c]), __fmul_rn(e, a.palette_mod[3 * act + c]));
                    acc[c] = __fadd_rn(acc[c], __fmul_rn(wi, pi));
                }
                act++;
            }
    } else {
        lae::palette_edit(l, a.active_mask, a.p_weights, a.p_bias);
        lae::palette_product(l, a.active_mask, a.palette_mod, acc);
    }
    const float u = __fsub_rn(1.0f, w);
    T* out = static_cast<T*>(a.images) + ((uint64_t)img * a.HW + pix) * a.C;
    const float* p = a.pred + 3 * (uint64_t)r;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float col = lae::clampf(__fadd_rn(acc[c], o[c]), 0.0f, 1.0f);
        const float s = NO_BG ? __fmul_rn(w, col) : __fadd_rn(__fmul_rn(u, p[c]), __fmul_rn(w, col));
        out[c] = from_f32<T>(lae::clampf(s, 0.0f, 1.0f));
    }
}

template <typename T>
void launch_compose(const DistillArgs& a, bool smooth, bool no_bg, hipStream_t s) {
    const uint32_t nb = lae::cdiv(a.R, DC_THREADS);
    if (smooth && no_bg) k_distill_compose<T, true, true><<<nb, DC_THREADS, 0, s>>>(a);
    else if (smooth) k_distill_compose<T, true, false><<<nb, DC_THREADS, 0, s>>>(a);
    else if (no_bg) k_distill_compose<T, false, true><<<nb, DC_THREADS, 0, s>>>(a);
    else k_distill_compose<T, false, false><<<nb, DC_THREADS, 0, s>>>(a);
}

// dense[img][pix] = w of every row (the scratch is zeroed before)
__global__ void k_seed_scatter(uint32_t R, const int32_t* __restrict__ img, const int32_t* __restrict__ pix, const float* __restrict__ w,
                               uint32_t n_img, uint32_t HW, float* __restrict__ dense) {
    const uint32_t r = blockIdx.x * DC_THREADS + threadIdx.x;
    if (r >= R) return;
    const uint32_t i = (uint32_t)img[r], p = (uint32_t)pix[r];
    if (i < n_img && p < HW) dense[(uint64_t)i * HW + p] = w[r];
}

// torch's linear source index (align_corners=False, no antialiasing): src = max(scale * (dst + 0.5) - 0.5, 0),
// i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), lambda = clamp(src - i0, 0, 1)
__device__ __forceinline__ void linear_index(uint32_t dst, uint32_t in, float scale, uint32_t& i0, uint32_t& i1, float& lambda) {
    const float src = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f), 0.0f);
    i0 = min((uint32_t)floorf(src), in - 1);
    i1 = i0 + (i0 < in - 1 ? 1u : 0u);
    lambda = lae::clampf(__fsub_rn(src, (float)i0), 0.0f, 1.0f);
}

__global__ void k_seed_resize(const int32_t* __restrict__ view_img, uint32_t V, uint32_t n_img, uint32_t H, uint32_t W,
                              const float* __restrict__ dense, float* __restrict__ error_map) {
    const uint64_t t = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (t >= (uint64_t)V * SEED_CELLS) return;
    const uint32_t v = (uint32_t)(t / SEED_CELLS), cell = (uint32_t)(t % SEED_CELLS);
    const uint32_t img = (uint32_t)view_img[v];
    if (img >= n_img) return;
    uint32_t y0, y1, x0, x1;
    float ly, lx;
    linear_index(cell / SEED_SIDE, H, __fdiv_rn((float)H, (float)SEED_SIDE), y0, y1, ly);
    linear_index(cell % SEED_SIDE, W, __fdiv_rn((float)W, (float)SEED_SIDE), x0, x1, lx);
    const float* src = dense + (uint64_t)img * H * W;
    const float wx0 = __fsub_rn(1.0f, lx), wy0 = __fsub_rn(1.0f, ly);
    // h0 * (w0 x[y0][x0] + w1 x[y0][x1]) + h1 * (w0 x[y1][x0] + w1 x[y1][x1]): torch's CPU order
    const float top = __fadd_rn(__fmul_rn(src[(uint64_t)y0 * W + x0], wx0), __fmul_rn(src[(uint64_t)y0 * W + x1], lx));
    const float bot = __fadd_rn(__fmul_rn(src[(uint64_t)y1 * W + x0], wx0), __fmul_rn(src[(uint64_t)y1 * W + x1], lx));
    const float x = __fadd_rn(__fmul_rn(top, wy0), __fmul_rn(bot, ly));
    error_map[(uint64_t)img * SEED_CELLS + cell] = lae::clampf(__fadd_rn(x, 0.15f), 0.0f, 1.0f);
}

// ---- Ref-NPR distillation data.  a = the training image's alpha (1 for 3-channel data)
__device__ __forceinline__ float src_alpha(const void* src, int dtype, uint32_t C, uint64_t p) {
    if (C != 4) return 1.0f;
    const uint64_t i = 4 * p + 3;
    if (dtype == LAE_IMG_U8) return __fdiv_rn((float)static_cast<const uint8_t*>(src)[i], 255.0f);
    return dtype == LAE_IMG_F16 ? (float)static_cast<const half_t*>(src)[i] : static_cast<const float*>(src)[i];
}

struct RefPlanes { void* images; void* weights; void* second; float* depths; };

// every pixel: images = (0, 0, 0, a), weights = 1 - a, second = 0, depths = 0
template <typename T>
__global__ void __launch_bounds__(DC_THREADS) k_ref_distill_init(const void* __restrict__ src, int src_dtype, uint32_t C, uint64_t n_pix,
                                                                 RefPlanes o) {
    const uint64_t p = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
    if (p >= n_pix) return;
    const float a = src_alpha(src, src_dtype, C, p);
    const T z = from_f32<T>(0.0f);
    T* im = static_cast<T*>(o.images) + 4 * p;
    T* s2 = static_cast<T*>(o.second) + 4 * p;
    im[0] = z; im[1] = z; im[2] = z; im[3] = from_f32<T>(a);
    s2[0] = z; s2[1] = z; s2[2] = z; s2[3] = z;
    static_cast<T*>(o.weights)[p] = from_f32<T>(__fsub_rn(1.0f, a));
    o.depths[p] = 0.0f;
}

struct RefRows {
    uint32_t R_reg; const int32_t* reg_img; const int32_t* reg_pix; const float* reg_rgb; const float* reg_w;
    uint32_t R_ext; const int32_t* ext_img; const int32_t* ext_pix; const float* ext_rgb; const float* ext_depth;
};

// thread r < R_reg: a registered row -> images rgb = the registered colour, weights = max(w, 0) + (1 - a);
// thread R_reg + r: an extracted row -> second = (the network's colour, a), depths = the row's depth.  The two kinds write different
// planes; two rows of one kind on the same pixel are the caller's error (the last writer wins, unspecified).
template <typename T>
__global__ void __launch_bounds__(DC_THREADS) k_ref_distill_scatter(RefRows rw, const void* __restrict__ src, int src_dtype, uint32_t C,
                                                                    uint32_t n_img, uint32_t HW, RefPlanes o) {
    const uint32_t r = blockIdx.x * DC_THREADS + threadIdx.x;
    if (r >= rw.R_reg + rw.R_ext) return;
    const bool reg = r < rw.R_reg;
    const uint32_t q = reg ? r : r - rw.R_reg;
    const uint32_t img = (uint32_t)(reg ? rw.reg_img[q] : rw.ext_img[q]), pix = (uint32_t)(reg ? rw.reg_pix[q] : rw.ext_pix[q]);
    if (img >= n_img || pix >= HW) return;
    const uint64_t p = (uint64_t)img * HW + pix;
    const float a = src_alpha(src, src_dtype, C, p);
    if (reg) {
        T* im = static_cast<T*>(o.images) + 4 * p;
        for (int c = 0; c < 3; c++) im[c] = from_f32<T>(rw.reg_rgb[3 * (uint64_t)q + c]);
        static_cast<T*>(o.weights)[p] = from_f32<T>(__fadd_rn(fmaxf(rw.reg_w[q], 0.0f), __fsub_rn(1.0f, a)));
    } else {
        T* s2 = static_cast<T*>(o.second) + 4 * p;
        for (int c = 0; c < 3; c++) s2[c] = from_f32<T>(rw.ext_rgb[3 * (uint64_t)q + c]);
        s2[3] = from_f32<T>(a);
        o.depths[p] = rw.ext_depth[q];
    }
}

}  // namespace

extern "C" {

int lae_distill_compose(uint32_t R, const int32_t* img_idx, const int32_t* pix, const float* w, const float* pred, const float* dist,
                        const void* w_logits, uint32_t w_stride, const void* o_raw, uint32_t o_stride, uint32_t P, uint32_t active_mask,
                        const float* palette_mod, const float* palette_og, const float* p_weights, const float* p_bias, float blend_thresh,
                        int flags, void* images, int dtype, uint32_t n_img, uint32_t HW, uint32_t C, void* stream) {
    if (R == 0) return LAE_OK;
    if (P == 0 || P > 16 || w_stride < P || o_stride < 3 || (C != 3 && C != 4) || HW == 0 || n_img == 0) return LAE_EINVAL;
    if (dtype != 1 && dtype != 2) return LAE_EINVAL;                                  // fp16 / fp32 images (ResidentImages codes)
    if (flags & ~LAE_DISTILL_NO_BG) return LAE_EINVAL;
    active_mask &= (1u << P) - 1u;
    if (active_mask == 0) return LAE_EINVAL;
    if (!img_idx || !pix || !w || !pred || !w_logits || !o_raw || !palette_mod || !p_weights || !p_bias || !images) return LAE_ENULL;
    if (dist && !palette_og) return LAE_ENULL;
    DistillArgs a{img_idx, pix, w, pred, dist, static_cast<const half_t*>(w_logits), w_stride, static_cast<const half_t*>(o_raw), o_stride,
                  active_mask, palette_mod, palette_og, p_weights, p_bias, blend_thresh, images, n_img, HW, C, R};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool smooth = dist != nullptr, no_bg = flags & LAE_DISTILL_NO_BG;
    if (dtype == 1) launch_compose<half_t>(a, smooth, no_bg, s);
    else launch_compose<float>(a, smooth, no_bg, s);
    return lae::check_launch("distill_compose");
}

int lae_error_map_seed(uint32_t R, const int32_t* img_idx, const int32_t* pix, const float* w, const int32_t* view_img, uint32_t V,
                       uint32_t n_img, uint32_t H, uint32_t W, float* dense, float* error_map, void* stream) {
    if (V == 0) return LAE_OK;
    if (H == 0 || W == 0 || n_img == 0 || (uint64_t)H * W > 0xffffffffull) return LAE_EINVAL;
    if (!view_img || !dense || !error_map || (R && (!img_idx || !pix || !w))) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t HW = H * W;
    if (hipMemsetAsync(dense, 0, (uint64_t)n_img * HW * sizeof(float), s) != hipSuccess) return lae::check_launch("error_map_seed/clear");
    if (R) {
        k_seed_scatter<<<lae::cdiv(R, DC_THREADS), DC_THREADS, 0, s>>>(R, img_idx, pix, w, n_img, HW, dense);
        const int rc = lae::check_launch("error_map_seed/scatter");
        if (rc) return rc;
    }
    k_seed_resize<<<lae::cdiv((uint64_t)V * SEED_CELLS, DC_THREADS), DC_THREADS, 0, s>>>(view_img, V, n_img, H, W, dense, error_map);
    return lae::check_launch("error_map_seed/resize");
}

int lae_ref_distill_init(const void* src_images, int src_dtype, uint32_t n_img, uint32_t HW, uint32_t C, int dtype, void* images,
                         void* weights, void* second, float* depths, void* stream) {
    if (n_img == 0 || HW == 0) return LAE_OK;
    if ((C != 3 && C != 4) || (dtype != LAE_IMG_F16 && dtype != LAE_IMG_F32)) return LAE_EINVAL;
    if (src_dtype != LAE_IMG_U8 && src_dtype != LAE_IMG_F16 && src_dtype != LAE_IMG_F32) return LAE_EINVAL;
    if (!src_images || !images || !weights || !second || !depths) return LAE_ENULL;
    const uint64_t n_pix = (uint64_t)n_img * HW;
    if ((n_pix + DC_THREADS - 1) / DC_THREADS > 0x7fffffffull) return LAE_EINVAL;
    const uint32_t nb = lae::cdiv(n_pix, DC_THREADS);
    const RefPlanes o{images, weights, second, depths};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == LAE_IMG_F16) k_ref_distill_init<half_t><<<nb, DC_THREADS, 0, s>>>(src_images, src_dtype, C, n_pix, o);
    else k_ref_distill_init<float><<<nb, DC_THREADS, 0, s>>>(src_images, src_dtype, C, n_pix, o);
    return lae::check_launch("ref_distill_init");
}

int lae_ref_distill_scatter(uint32_t R_reg, const int32_t* reg_img, const int32_t* reg_pix, const float* reg_rgb, const float* reg_w,
                            uint32_t R_ext, const int32_t* ext_img, const int32_t* ext_pix, const float* ext_rgb, const float* ext_depth,
                            const void* src_images, int src_dtype, uint32_t n_img, uint32_t HW, uint32_t C, int dtype, void* images,
                            void* weights, void* second, float* depths, void* stream) {
    if ((uint64_t)R_reg + R_ext == 0) return LAE_OK;
    if ((uint64_t)R_reg + R_ext > 0xffffffffull) return LAE_EINVAL;
    if ((C != 3 && C != 4) || (dtype != LAE_IMG_F16 && dtype != LAE_IMG_F32) || n_img == 0 || HW == 0) return LAE_EINVAL;
    if (src_dtype != LAE_IMG_U8 && src_dtype != LAE_IMG_F16 && src_dtype != LAE_IMG_F32) return LAE_EINVAL;
    if (!src_images || !images || !weights || !second || !depths) return LAE_ENULL;
    if (R_reg && (!reg_img || !reg_pix || !reg_rgb || !reg_w)) return LAE_ENULL;
    if (R_ext && (!ext_img || !ext_pix || !ext_rgb || !ext_depth)) return LAE_ENULL;
    const RefRows rw{R_reg, reg_img, reg_pix, reg_rgb, reg_w, R_ext, ext_img, ext_pix, ext_rgb, ext_depth};
    const RefPlanes o{images, weights, second, depths};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nb = lae::cdiv(R_reg + R_ext, (uint32_t)DC_THREADS);
    if (dtype == LAE_IMG_F16) k_ref_distill_scatter<half_t><<<nb, DC_THREADS, 0, s>>>(rw, src_images, src_dtype, C, n_img, HW, o);
    else k_ref_distill_scatter<float><<<nb, DC_THREADS, 0, s>>>(rw, src_images, src_dtype, C, n_img, HW, o);
    return lae::check_launch("ref_distill_scatter");
}

}  // extern "C"
