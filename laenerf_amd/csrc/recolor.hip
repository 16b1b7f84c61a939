// recolor.hip -- recolored views of a trained LAENeRF palette network (nerf/utils.py:1230-1386 test_gui_styleenc /
// val_gui_styleenc, nerf/gui.py:659-714 eval_style_predictor; torch ops and a host nonzero() in the reference).
//
// lae_recolor_compact: the pixels an edit-grid render hit (d != 0 after NaN -> 0, ascending pixel order = d.nonzero()), as a
//   stable three-pass compaction (per-block counts, one-block scan, scatter), and the palette network's inputs for them.
// lae_recolor_compose: one thread per pixel, one pass: softmax of the cached logits, the palette edit and the recomposition of
//   the reference's display / evaluation paths (include/laenerf.h states the rules).
#include "lae_common.h"
#include "palette_edit.h"

namespace {

typedef _Float16 half_t;

constexpr int RC_THREADS = 256;
constexpr int RC_ITEMS = 4;                                   // contiguous pixels per thread
constexpr uint32_t RC_TILE = RC_THREADS * RC_ITEMS;           // pixels per block
constexpr int RC_SCAN_THREADS = 1024;

__device__ __forceinline__ float clean_depth(float d) { return __builtin_isnan(d) ? 0.0f : d; }

__global__ void k_recolor_count(const float* __restrict__ depth, uint32_t N, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t lds[RC_THREADS / LAE_WAVE + 1];
    const uint64_t base = (uint64_t)blockIdx.x * RC_TILE + (uint64_t)threadIdx.x * RC_ITEMS;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < RC_ITEMS; j++)
        if (base + j < N) c += clean_depth(depth[base + j]) != 0.0f;
    uint32_t total;
    lae::block_excl_scan<RC_THREADS / LAE_WAVE>(c, &total, lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one block: exclusive prefix of the block counts in place, *count = K
__global__ void k_recolor_scan(uint32_t* __restrict__ block_counts, uint32_t nb, int32_t* __restrict__ count) {
    __shared__ uint32_t lds[RC_SCAN_THREADS / LAE_WAVE + 1];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += RC_SCAN_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? block_counts[i] : 0u;
        uint32_t total;
        const uint32_t ex = lae::block_excl_scan<RC_SCAN_THREADS / LAE_WAVE>(v, &total, lds);
        if (i < nb) block_counts[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count = (int32_t)carry;
}

__global__ void k_recolor_scatter(const float* __restrict__ depth, const float* __restrict__ weights_sum,
                                  const float* __restrict__ rays_o, const float* __restrict__ rays_d, uint32_t N,
                                  const uint32_t* __restrict__ block_offsets, const int32_t* __restrict__ count,
                                  int32_t* __restrict__ indices, int32_t* __restrict__ slot_map, float* __restrict__ x_term,
                                  float* __restrict__ dirs, float* __restrict__ alpha) {
    __shared__ uint32_t lds[RC_THREADS / LAE_WAVE + 1];
    const uint64_t base = (uint64_t)blockIdx.x * RC_TILE + (uint64_t)threadIdx.x * RC_ITEMS;
    float d[RC_ITEMS];
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < RC_ITEMS; j++) {
        d[j] = base + j < N ? clean_depth(depth[base + j]) : 0.0f;
        c += d[j] != 0.0f;
    }
    uint32_t total;
    uint32_t slot = block_offsets[blockIdx.x] + lae::block_excl_scan<RC_THREADS / LAE_WAVE>(c, &total, lds);
#pragma unroll
    for (int j = 0; j < RC_ITEMS; j++) {
        const uint64_t i = base + j;
        if (i >= N) break;
        if (d[j] == 0.0f) { slot_map[i] = -1; continue; }
        indices[slot] = (int32_t)i;
        slot_map[i] = (int32_t)slot;
#pragma unroll
        for (int c3 = 0; c3 < 3; c3++) {
            const float r = rays_d[3 * i + c3];
            // rays_o + d * rays_d: a multiply, then an add (two roundings, as torch's two elementwise kernels)
            x_term[3 * (uint64_t)slot + c3] = __fadd_rn(rays_o[3 * i + c3], __fmul_rn(d[j], r));
            dirs[3 * (uint64_t)slot + c3] = r;
        }
        alpha[slot] = weights_sum[i];
        slot++;
    }
    // rows K .. round_up(K, 16) of x_term / dirs are zero (the MLPs run on multiples of 16 rows)
    if (blockIdx.x == 0 && threadIdx.x < 48) {
        const uint32_t K = (uint32_t)*count, Kp = (K + 15u) & ~15u;
        const uint32_t e = 3 * K + threadIdx.x;
        if (e < 3 * Kp) { x_term[e] = 0.0f; dirs[e] = 0.0f; }
    }
}

struct ComposeArgs {
    const int32_t* slot_map;
    const half_t* w_logits; uint32_t w_stride;
    const half_t* o_raw; uint32_t o_stride;
    uint32_t active_mask;
    const float* palette; const float* p_weights; const float* p_bias;
    const float* alpha; const float* base; const float* bg;
    uint32_t k;
    float* out; uint8_t* out_u8;
    uint32_t N;
};

// torch's float -> uint8: through int64, then the low byte (c10 static_cast_with_inter_type<uint8_t>); NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float x) {
    const float v = __fmul_rn(x, 255.0f);
    if (__builtin_isnan(v)) return 0;
    return (uint8_t)(int64_t)fminf(fmaxf(v, -9.0e18f), 9.0e18f);
}

template <int MODE, bool OFFSETS, bool TANH>
__global__ void __launch_bounds__(RC_THREADS) k_recolor_compose(ComposeArgs a) {
    const uint32_t i = blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= a.N) return;
    const float bg0 = a.bg[0], bg1 = a.bg[1], bg2 = a.bg[2];
    const int32_t s = a.slot_map[i];
    float r0, r1, r2;
    if (s < 0) {
        if (MODE == LAE_RECOLOR_EVAL) { r0 = bg0; r1 = bg1; r2 = bg2; }
        else { r0 = a.base[3 * (uint64_t)i]; r1 = a.base[3 * (uint64_t)i + 1]; r2 = a.base[3 * (uint64_t)i + 2]; }
    } else {
        const float t = a.alpha[s];
        const float u = 1.0f - t;
        const half_t* wl = a.w_logits + (uint64_t)s * a.w_stride;
        const half_t* orw = a.o_raw + (uint64_t)s * a.o_stride;
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = (float)orw[c];
            o[c] = TANH ? (float)tanh((double)v) : v;
        }
        if (MODE == LAE_RECOLOR_OFFSETS) {
            r0 = __fadd_rn(__fadd_rn(__fmul_rn(o[0], 0.5f), 0.5f), __fmul_rn(u, bg0));
            r1 = __fadd_rn(__fadd_rn(__fmul_rn(o[1], 0.5f), 0.5f), __fmul_rn(u, bg1));
            r2 = __fadd_rn(__fadd_rn(__fmul_rn(o[2], 0.5f), 0.5f), __fmul_rn(u, bg2));
        } else {
            // softmax over the active columns: e = exp(l - max) (fp32 difference, exp in double, one rounding), w = e / sum
            float l[16];
            const float sum = lae::palette_softmax_exp(wl, a.active_mask, l);
            if (MODE == LAE_RECOLOR_WEIGHTS) {
                int act = 0;
                float wk = 0.0f;
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if ((a.active_mask >> j) & 1u) { if ((uint32_t)act == a.k) wk = __fdiv_rn(l[j], sum); act++; }
                r0 = __fadd_rn(wk, __fmul_rn(u, bg0));
                r1 = __fadd_rn(wk, __fmul_rn(u, bg1));
                r2 = __fadd_rn(wk, __fmul_rn(u, bg2));
            } else {
                lae::palette_normalise(l, a.active_mask, sum);
                if (MODE == LAE_RECOLOR_PREVIEW && OFFSETS) lae::palette_edit(l, a.active_mask, a.p_weights, a.p_bias);
                float acc[3];
                lae::palette_product(l, a.active_mask, a.palette, acc);
                const float bgc[3] = {bg0, bg1, bg2};
                float r[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (MODE == LAE_RECOLOR_EVAL)
                        r[c] = __fadd_rn(__fmul_rn(lae::clampf(__fadd_rn(acc[c], o[c]), 0.0f, 1.0f), t), __fmul_rn(bgc[c], u));
                    else if (OFFSETS)
                        r[c] = __fadd_rn(lae::clampf(__fadd_rn(o[c], acc[c]), 0.0f, 1.0f), __fmul_rn(u, bgc[c]));
                    else
                        r[c] = __fadd_rn(lae::clampf(acc[c], 0.0f, 1.0f), __fmul_rn(u, bgc[c]));
                }
                r0 = r[0]; r1 = r[1]; r2 = r[2];
            }
        }
    }
    float* op = a.out + 3 * (uint64_t)i;
    op[0] = r0; op[1] = r1; op[2] = r2;
    if (a.out_u8) {
        uint8_t* q = a.out_u8 + 3 * (uint64_t)i;
        q[0] = to_u8(r0); q[1] = to_u8(r1); q[2] = to_u8(r2);
    }
}

template <int MODE>
void launch_compose(const ComposeArgs& a, bool offsets, bool tanh_act, hipStream_t s) {
    const uint32_t nb = lae::cdiv(a.N, RC_THREADS);
    if (offsets && tanh_act) k_recolor_compose<MODE, true, true><<<nb, RC_THREADS, 0, s>>>(a);
    else if (offsets) k_recolor_compose<MODE, true, false><<<nb, RC_THREADS, 0, s>>>(a);
    else if (tanh_act) k_recolor_compose<MODE, false, true><<<nb, RC_THREADS, 0, s>>>(a);
    else k_recolor_compose<MODE, false, false><<<nb, RC_THREADS, 0, s>>>(a);
}

}  // namespace

extern "C" {

uint64_t lae_recolor_compact_scratch_bytes(uint32_t N) {
    return (uint64_t)4 * (lae::cdiv(N, RC_TILE) + 1);
}

int lae_recolor_compact(const float* depth, const float* weights_sum, const float* rays_o, const float* rays_d, uint32_t N,
                        int32_t* indices, int32_t* slot_map, float* x_term, float* dirs, float* alpha, int32_t* count,
                        void* scratch, void* stream) {
    if (!count) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (N == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) return lae::check_launch("recolor_compact");
        return LAE_OK;
    }
    if (!depth || !weights_sum || !rays_o || !rays_d || !indices || !slot_map || !x_term || !dirs || !alpha || !scratch) return LAE_ENULL;
    if (N > 0x7fffffffu) return LAE_EINVAL;                      // int32 pixel indices / slots
    const uint32_t nb = lae::cdiv(N, RC_TILE);
    uint32_t* offs = static_cast<uint32_t*>(scratch);
    k_recolor_count<<<nb, RC_THREADS, 0, s>>>(depth, N, offs);
    int rc = lae::check_launch("recolor_compact/count");
    if (rc) return rc;
    k_recolor_scan<<<1, RC_SCAN_THREADS, 0, s>>>(offs, nb, count);
    rc = lae::check_launch("recolor_compact/scan");
    if (rc) return rc;
    k_recolor_scatter<<<nb, RC_THREADS, 0, s>>>(depth, weights_sum, rays_o, rays_d, N, offs, count, indices, slot_map, x_term, dirs,
                                                alpha);
    return lae::check_launch("recolor_compact/scatter");
}

int lae_recolor_compose(const int32_t* slot_map, uint32_t N, const void* w_logits, uint32_t w_stride, const void* o_raw,
                        uint32_t o_stride, uint32_t P, uint32_t active_mask, const float* palette, const float* p_weights,
                        const float* p_bias, const float* alpha, const float* base, const float* bg, int mode, uint32_t k,
                        int flags, float* out, uint8_t* out_u8, void* stream) {
    if (N == 0) return LAE_OK;
    if (P == 0 || P > 16 || w_stride < P || o_stride < 3) return LAE_EINVAL;
    active_mask &= (1u << P) - 1u;
    const uint32_t n_active = (uint32_t)__builtin_popcount(active_mask);
    if (n_active == 0 || mode < LAE_RECOLOR_PREVIEW || mode > LAE_RECOLOR_EVAL) return LAE_EINVAL;
    if (mode == LAE_RECOLOR_WEIGHTS && k >= n_active) return LAE_EINVAL;
    if (flags & ~(LAE_RECOLOR_NO_OFFSETS | LAE_RECOLOR_TANH)) return LAE_EINVAL;
    const bool offsets = !(flags & LAE_RECOLOR_NO_OFFSETS);
    const bool edit = mode == LAE_RECOLOR_PREVIEW && offsets;
    if (!slot_map || !w_logits || !o_raw || !alpha || !bg || !out) return LAE_ENULL;
    if ((mode == LAE_RECOLOR_PREVIEW || mode == LAE_RECOLOR_EVAL) && !palette) return LAE_ENULL;
    if (edit && (!p_weights || !p_bias)) return LAE_ENULL;
    if (mode != LAE_RECOLOR_EVAL && !base) return LAE_ENULL;
    ComposeArgs a{slot_map, static_cast<const half_t*>(w_logits), w_stride, static_cast<const half_t*>(o_raw), o_stride, active_mask,
                  palette, p_weights, p_bias, alpha, base, bg, k, out, out_u8, N};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool tanh_act = flags & LAE_RECOLOR_TANH;
    switch (mode) {
        case LAE_RECOLOR_PREVIEW: launch_compose<LAE_RECOLOR_PREVIEW>(a, offsets, tanh_act, s); break;
        case LAE_RECOLOR_WEIGHTS: launch_compose<LAE_RECOLOR_WEIGHTS>(a, false, tanh_act, s); break;
        case LAE_RECOLOR_OFFSETS: launch_compose<LAE_RECOLOR_OFFSETS>(a, false, tanh_act, s); break;
        default: launch_compose<LAE_RECOLOR_EVAL>(a, false, tanh_act, s); break;
    }
    return lae::check_launch("recolor_compose");
}

}  // extern "C"
