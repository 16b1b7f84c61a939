// style_image.hip -- the image-space half of LAENeRF's stylization step (nerf/utils.py:997-1033 in train_LAENeRF_step;
// editing/style_encoder.py:207-235 for the image terms, editing/style_network.py:129-191 for the VGG input), on the step's view
// as the device step counter names it (lae_style_image_forward / _backward, include/laenerf.h).
//
// The reference scatters the palette network's fp16 colours into a zeroed H x W canvas, crops it with exclusive upper bounds,
// resizes the crop to S x S (torchvision Resize on a tensor = F.interpolate bilinear, align_corners=False, no antialias),
// normalizes it with the ImageNet statistics for VGG and sums three stencil terms over the crop.  Here the edit set carries a
// crop-sized pixel -> row map per view, so every read is a gather (no canvas, no scatter), and everything the launches need --
// the view, its crop, the live row count K -- is read from device memory: one captured graph serves every view.
//
// Reductions: every workgroup of a FIXED grid (n_blocks, chosen by the host from the largest crop of the set) strides over the
// crop's pixels in a fixed order and writes one partial row; one workgroup sums the rows in a fixed order.  The backward is a
// gather per row (the adjoint of the resize as the sum over the output pixels whose taps hit the row's crop pixel, plus the
// stencils), with no atomics: eager runs and graph replays give the same bits.
#include "lae_common.h"

namespace {

typedef _Float16 half_t;
constexpr uint32_t SI_BLOCK = 256;
constexpr int SI_COLS = 5;                        // partial sums: tv (h), tv (v), smooth, disc (h), disc (v)
__constant__ float kMean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float kStd[3] = {0.229f, 0.224f, 0.225f};

// the step's view and crop, as the sampler left them: v = schedule[(step - 1) mod n_sched] (the counter was advanced after the
// draw), K = *m_dev
struct ImgView {
    uint32_t K;
    int32_t h, w;                                 // crop rows / columns (>= 1, validated on the host)
    int64_t off;                                  // first crop pixel of the view in the per-pixel arrays
    float max_h, max_v;                           // the depth-discontinuity term's divisors
    uint32_t v;
};

struct ImgSet {
    const half_t* pred; uint32_t cap; const uint32_t* m_dev;
    const int32_t* schedule; uint32_t n_sched; const int64_t* step_counter; uint32_t V;
    const int32_t* box; const int64_t* img_off; const int32_t* pix2row;
    const float* cut_gt; const float* tv_h; const float* tv_v; const float* smooth; const float* vmax;
};

__device__ __forceinline__ ImgView load_view(const ImgSet& a) {
    ImgView iv;
    const int64_t n = (int64_t)a.n_sched;
    const int64_t s = ((a.step_counter[0] - 1) % n + n) % n;
    const int32_t sv = a.schedule[s];
    iv.v = sv < 0 ? 0u : min((uint32_t)sv, a.V - 1u);
    iv.K = min(*a.m_dev, a.cap);
    iv.h = a.box[iv.v * 4 + 1] - a.box[iv.v * 4 + 0];
    iv.w = a.box[iv.v * 4 + 3] - a.box[iv.v * 4 + 2];
    iv.off = a.img_off[iv.v];
    iv.max_h = a.vmax[iv.v * 2 + 0];
    iv.max_v = a.vmax[iv.v * 2 + 1];
    return iv;
}

// crop pixel (i, j), 0 where no live row lands
__device__ __forceinline__ void px(const ImgSet& a, const ImgView& iv, int i, int j, float out[3]) {
    const int32_t r = a.pix2row[iv.off + (int64_t)i * iv.w + j];
    if (r >= 0 && (uint32_t)r < iv.K) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = (float)a.pred[(size_t)r * 3 + c];
    } else {
        out[0] = out[1] = out[2] = 0.0f;
    }
}

// PyTorch's bilinear source index (align_corners=False): src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out.  PyTorch's
// device kernel is compiled with contraction on, so its multiply-subtract is one fma: an unfused one differs by an ulp of src
// (up to 4e-6 in the normalized output of a 23-row crop at S = 40)
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap(int dst, int in, float scale) {
    float src = fmaf(scale, __fadd_rn((float)dst, 0.5f), -0.5f);
    src = src < 0.0f ? 0.0f : src;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = __fsub_rn(src, (float)t.i0);
    t.l0 = __fsub_rn(1.0f, t.l1);
    return t;
}

// weight with which input index `i` enters output `dst` (both taps may sit on i at the last row / column)
__device__ __forceinline__ float tap_weight(int dst, int in, float scale, int i) {
    const Tap t = tap(dst, in, scale);
    return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f);
}

// the output range whose taps can hit input index i (a conservative bracket; tap_weight decides)
__device__ __forceinline__ void tap_range(int i, int S, float scale, int& lo, int& hi) {
    lo = max(0, (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1);
    hi = min(S - 1, (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1);
}

// resize + normalize: vgg_in [3, S, S] fp32
__global__ __launch_bounds__(SI_BLOCK) void k_style_image_resize(ImgSet a, uint32_t S, float* __restrict__ vgg_in) {
    const uint32_t t = blockIdx.x * SI_BLOCK + threadIdx.x;
    if (t >= S * S) return;
    const ImgView iv = load_view(a);
    const int oy = (int)(t / S), ox = (int)(t % S);
    const float sy = (float)iv.h / (float)S, sx = (float)iv.w / (float)S;
    const Tap ty = tap(oy, iv.h, sy), tx = tap(ox, iv.w, sx);
    float p00[3], p01[3], p10[3], p11[3];
    px(a, iv, ty.i0, tx.i0, p00); px(a, iv, ty.i0, tx.i1, p01);
    px(a, iv, ty.i1, tx.i0, p10); px(a, iv, ty.i1, tx.i1, p11);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // upsample_bilinear2d: h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
        const float top = __fadd_rn(__fmul_rn(tx.l0, p00[c]), __fmul_rn(tx.l1, p01[c]));
        const float bot = __fadd_rn(__fmul_rn(tx.l0, p10[c]), __fmul_rn(tx.l1, p11[c]));
        const float val = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
        vgg_in[(size_t)c * S * S + t] = __fdiv_rn(__fsub_rn(val, kMean[c]), kStd[c]);
    }
}

// the stencil weights of pixel (i, j) towards (i + 1, j) ("h") and (i, j + 1) ("v")
__device__ __forceinline__ float tv_weight_h(const ImgSet& a, const ImgView& iv, int64_t p, int flags) {
    if (!(flags & LAE_STYLE_IMG_TV_DEPTH)) return 1.0f;
    float wgt = 1.0f - a.tv_h[iv.off + p];
    if (flags & LAE_STYLE_IMG_TV_SMOOTH) wgt *= 1.0f - a.smooth[iv.off + p + iv.w];
    return wgt;
}
__device__ __forceinline__ float tv_weight_v(const ImgSet& a, const ImgView& iv, int64_t p, int flags) {
    if (!(flags & LAE_STYLE_IMG_TV_DEPTH)) return 1.0f;
    float wgt = 1.0f - a.tv_v[iv.off + p];
    if (flags & LAE_STYLE_IMG_TV_SMOOTH) wgt *= 1.0f - a.smooth[iv.off + p + 1];
    return wgt;
}

__global__ __launch_bounds__(SI_BLOCK) void k_style_image_partial(ImgSet a, int flags, float* __restrict__ slab) {
    __shared__ float red[SI_BLOCK / 64][SI_COLS];
    const ImgView iv = load_view(a);
    const int64_t n = (int64_t)iv.h * iv.w;
    float acc[SI_COLS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t p = (int64_t)blockIdx.x * SI_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * SI_BLOCK) {
        const int i = (int)(p / iv.w), j = (int)(p % iv.w);
        float x[3];
        px(a, iv, i, j, x);
        if (i < iv.h - 1 && (flags & (LAE_STYLE_IMG_TV | LAE_STYLE_IMG_DISC))) {
            float y[3];
            px(a, iv, i + 1, j, y);
            float d2 = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) { const float d = x[c] - y[c]; d2 += d * d; }
            if (flags & LAE_STYLE_IMG_TV) acc[0] += d2 * tv_weight_h(a, iv, p, flags);
            if (flags & LAE_STYLE_IMG_DISC) acc[3] += d2 * (a.tv_h[iv.off + p] / iv.max_h);     // 0 / 0 = NaN like the reference
        }
        if (j < iv.w - 1 && (flags & (LAE_STYLE_IMG_TV | LAE_STYLE_IMG_DISC))) {
            float y[3];
            px(a, iv, i, j + 1, y);
            float d2 = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) { const float d = x[c] - y[c]; d2 += d * d; }
            if (flags & LAE_STYLE_IMG_TV) acc[1] += d2 * tv_weight_v(a, iv, p, flags);
            if (flags & LAE_STYLE_IMG_DISC) acc[4] += d2 * (a.tv_v[iv.off + p] / iv.max_v);
        }
        if (flags & LAE_STYLE_IMG_SMOOTH) {
            float d2 = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) { const float d = x[c] - a.cut_gt[(iv.off + p) * 3 + c]; d2 += d * d; }
            acc[2] += d2 * a.smooth[iv.off + p];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SI_COLS; k++) {
        float t = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
        if (lane == 0) red[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < SI_COLS) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < SI_BLOCK / 64; q++) t += red[q][threadIdx.x];
        slab[(size_t)blockIdx.x * SI_COLS + threadIdx.x] = t;
    }
}

// one workgroup of SI_COLS waves: wave k sums column k over the partial rows (lanes stride, then a butterfly)
__global__ __launch_bounds__(64 * SI_COLS) void k_style_image_final(const float* __restrict__ slab, uint32_t n_blocks, int flags,
                                                                    float* __restrict__ terms) {
    __shared__ float tot[SI_COLS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float t = 0.0f;
    for (uint32_t b = lane; b < n_blocks; b += 64) t += slab[(size_t)b * SI_COLS + wave];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
    if (lane == 0) tot[wave] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    terms[0] = (flags & LAE_STYLE_IMG_TV) ? tot[0] + tot[1] : 0.0f;
    terms[1] = (flags & LAE_STYLE_IMG_SMOOTH) ? tot[2] : 0.0f;
    terms[2] = (flags & LAE_STYLE_IMG_DISC) ? -tot[3] - tot[4] : 0.0f;
}

// one thread per row: dL/dpred[r] (fp32, scaled as the upstream gradients are); rows >= K and rows outside the crop get 0
__global__ __launch_bounds__(SI_BLOCK) void k_style_image_backward(ImgSet a, const int64_t* __restrict__ row_off,
                                                                   const int32_t* __restrict__ row2pix, uint32_t S,
                                                                   const float* __restrict__ g_vgg, const float* __restrict__ g_terms,
                                                                   int flags, float* __restrict__ g_pred) {
    const uint32_t r = blockIdx.x * SI_BLOCK + threadIdx.x;
    if (r >= a.cap) return;
    const ImgView iv = load_view(a);
    float g[3] = {0.0f, 0.0f, 0.0f};
    const int32_t p32 = r < iv.K ? row2pix[row_off[iv.v] + r] : -1;
    if (p32 >= 0) {
        const int64_t p = p32;
        const int i = (int)(p / iv.w), j = (int)(p % iv.w);
        if ((flags & LAE_STYLE_IMG_RESIZE) && g_vgg) {
            const float sy = (float)iv.h / (float)S, sx = (float)iv.w / (float)S;
            int y_lo, y_hi, x_lo, x_hi;
            tap_range(i, (int)S, sy, y_lo, y_hi);
            tap_range(j, (int)S, sx, x_lo, x_hi);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            for (int oy = y_lo; oy <= y_hi; oy++) {
                const float wy = tap_weight(oy, iv.h, sy, i);
                if (wy == 0.0f) continue;
                for (int ox = x_lo; ox <= x_hi; ox++) {
                    const float wx = tap_weight(ox, iv.w, sx, j);
                    if (wx == 0.0f) continue;
                    const float wgt = wy * wx;
                    const size_t o = (size_t)oy * S + ox;
#pragma unroll
                    for (int c = 0; c < 3; c++) acc[c] = fmaf(wgt, g_vgg[(size_t)c * S * S + o], acc[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) g[c] = acc[c] / kStd[c];
        }
        const int stencil = flags & (LAE_STYLE_IMG_TV | LAE_STYLE_IMG_DISC | LAE_STYLE_IMG_SMOOTH);
        if (stencil) {
            const float g_tv = (flags & LAE_STYLE_IMG_TV) ? g_terms[0] : 0.0f;
            const float g_sm = (flags & LAE_STYLE_IMG_SMOOTH) ? g_terms[1] : 0.0f;
            const float g_dc = (flags & LAE_STYLE_IMG_DISC) ? g_terms[2] : 0.0f;
            const bool tv = flags & LAE_STYLE_IMG_TV, dc = flags & LAE_STYLE_IMG_DISC;
            float x[3];
            px(a, iv, i, j, x);
            // each neighbour pair (q, q'): the term holds w * |x_q - x_q'|^2; d/dx_q = 2 w (x_q - x_q')
            const auto pair = [&](int64_t q, int qi, int qj, bool h_dir, float sign) {
                float y[3];
                px(a, iv, qi, qj, y);
                float wt = 0.0f;
                if (tv) wt += g_tv * (h_dir ? tv_weight_h(a, iv, q, flags) : tv_weight_v(a, iv, q, flags));
                if (dc) wt -= g_dc * (h_dir ? a.tv_h[iv.off + q] / iv.max_h : a.tv_v[iv.off + q] / iv.max_v);
#pragma unroll
                for (int c = 0; c < 3; c++) g[c] += sign * 2.0f * wt * (x[c] - y[c]);
            };
            if (tv || dc) {
                if (i < iv.h - 1) pair(p, i + 1, j, true, 1.0f);                         // (i, j) - (i + 1, j), weights at (i, j)
                if (i > 0) pair(p - iv.w, i - 1, j, true, 1.0f);                          // (i - 1, j) - (i, j), weights at (i - 1, j)
                if (j < iv.w - 1) pair(p, i, j + 1, false, 1.0f);
                if (j > 0) pair(p - 1, i, j - 1, false, 1.0f);
            }
            if (flags & LAE_STYLE_IMG_SMOOTH) {
                const float sm = a.smooth[iv.off + p];
#pragma unroll
                for (int c = 0; c < 3; c++) g[c] += g_sm * 2.0f * (x[c] - a.cut_gt[(iv.off + p) * 3 + c]) * sm;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) g_pred[(size_t)r * 3 + c] = g[c];
}

int check_set(const ImgSet& a, int flags) {
    if (!a.pred || !a.m_dev || !a.schedule || !a.step_counter || !a.box || !a.img_off || !a.pix2row || !a.vmax) return LAE_ENULL;
    if (a.cap == 0 || a.n_sched == 0 || a.V == 0) return LAE_EINVAL;
    if ((flags & LAE_STYLE_IMG_TV_DEPTH) && !a.tv_h) return LAE_ENULL;
    if ((flags & (LAE_STYLE_IMG_TV_DEPTH | LAE_STYLE_IMG_DISC)) && (!a.tv_h || !a.tv_v)) return LAE_ENULL;
    if ((flags & (LAE_STYLE_IMG_TV_SMOOTH | LAE_STYLE_IMG_SMOOTH)) && !a.smooth) return LAE_ENULL;
    if ((flags & LAE_STYLE_IMG_SMOOTH) && !a.cut_gt) return LAE_ENULL;
    return LAE_OK;
}

}  // namespace

extern "C" {

uint64_t lae_style_image_scratch_bytes(uint32_t n_blocks) { return (uint64_t)n_blocks * SI_COLS * sizeof(float) + 256; }

int lae_style_image_forward(const void* pred, uint32_t cap, const uint32_t* m_dev, const int32_t* schedule, uint32_t n_sched,
                            const int64_t* step_counter, uint32_t V, const int32_t* box, const int64_t* img_off, const int32_t* pix2row,
                            const float* cut_gt, const float* tv_h, const float* tv_v, const float* smooth, const float* vmax, uint32_t S,
                            float* vgg_in, int flags, uint32_t n_blocks, float* scratch, float* terms, void* stream) {
    const ImgSet a{(const half_t*)pred, cap, m_dev, schedule, n_sched, step_counter, V, box, img_off, pix2row, cut_gt, tv_h, tv_v, smooth, vmax};
    const int rc = check_set(a, flags);
    if (rc) return rc;
    if (!terms || !scratch || ((flags & LAE_STYLE_IMG_RESIZE) && !vgg_in)) return LAE_ENULL;
    if (n_blocks == 0 || n_blocks > 65536 || ((flags & LAE_STYLE_IMG_RESIZE) && (S == 0 || S > 4096))) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (flags & LAE_STYLE_IMG_RESIZE) k_style_image_resize<<<lae::cdiv(S * S, SI_BLOCK), SI_BLOCK, 0, s>>>(a, S, vgg_in);
    k_style_image_partial<<<n_blocks, SI_BLOCK, 0, s>>>(a, flags, scratch);
    k_style_image_final<<<1, 64 * SI_COLS, 0, s>>>(scratch, n_blocks, flags, terms);
    return lae::check_launch("style_image_forward");
}

int lae_style_image_backward(const void* pred, uint32_t cap, const uint32_t* m_dev, const int32_t* schedule, uint32_t n_sched,
                             const int64_t* step_counter, uint32_t V, const int32_t* box, const int64_t* img_off, const int32_t* pix2row,
                             const float* cut_gt, const float* tv_h, const float* tv_v, const float* smooth, const float* vmax,
                             const int64_t* row_off, const int32_t* row2pix, uint32_t S, const float* g_vgg, const float* g_terms, int flags,
                             float* g_pred, void* stream) {
    const ImgSet a{(const half_t*)pred, cap, m_dev, schedule, n_sched, step_counter, V, box, img_off, pix2row, cut_gt, tv_h, tv_v, smooth, vmax};
    const int rc = check_set(a, flags);
    if (rc) return rc;
    if (!row_off || !row2pix || !g_pred) return LAE_ENULL;
    if ((flags & (LAE_STYLE_IMG_TV | LAE_STYLE_IMG_DISC | LAE_STYLE_IMG_SMOOTH)) && !g_terms) return LAE_ENULL;
    if ((flags & LAE_STYLE_IMG_RESIZE) && (!g_vgg || S == 0 || S > 4096)) return g_vgg ? LAE_EINVAL : LAE_ENULL;
    k_style_image_backward<<<lae::cdiv(cap, SI_BLOCK), SI_BLOCK, 0, reinterpret_cast<hipStream_t>(stream)>>>(a, row_off, row2pix, S, g_vgg,
                                                                                                          g_terms, flags, g_pred);
    return lae::check_launch("style_image_backward");
}

}  // extern "C"
