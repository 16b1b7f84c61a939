// ref_stage.hip -- the registered terms of the Ref-NPR second stage (the reference's train_styleenc_step_npr,
// nerf/utils.py:1096-1104 and :1120-1122) on the step's view as the device step counter names it (lae_ref_terms_forward /
// _backward, include/laenerf.h).
//
// The reference multiplies the palette network's fp16 colours by the view's opacity weights in place, takes a weighted MSE over
// the registered rows (an index_select, a pow, a broadcast multiply, a mean), scatters the colours into an H x W canvas and
// resizes the whole canvas to the VGG relu5 grid for the colour-patch MSE -- a dozen launches around a 1080p canvas per step.
// Here the edit set carries the registration dense over the view's rows (weight 0 = not registered) and the resize as at most
// four (row, weight) taps per output, so both terms are gathers over the rows; the view, its live row count K and its
// registered count R are read from device memory: one captured graph serves every view.
//
// Arithmetic: pred' = fp16(pred * w8s) is one rounding of the exact fp32 product.  Everything behind it -- residuals, squares,
// sums, the gradient -- runs in fp64 and is rounded to fp32 once at the end: the sums are those of the float64 restatement up to
// that one rounding (plus n * 2^-53), and a gradient element whose three parts cancel keeps its relative accuracy.
// Summation order (fixed; no atomics): a thread's three channels in order, a butterfly over the wave's 64 lanes (xor 32, 16, .., 1),
// the workgroup's four waves in order -> one partial per workgroup; the final launch has lane l of one wave add partials l, l + 64,
// .. in order, then the same butterfly.
#include "lae_common.h"

namespace {

typedef _Float16 half_t;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr uint32_t RS_BLOCK = 256;

struct RefSet {
    const half_t* pred; uint32_t cap; const uint32_t* m_dev; const float* target;
    const int32_t* schedule; uint32_t n_sched; const int64_t* step_counter; uint32_t V;
    const int64_t* row_off; const int32_t* counts;
    const half_t* w8s; const float* ref_target; const float* ref_weight; const int32_t* ref_count;
    const float* tap_w; uint32_t n_out; int mode;
};

struct RefView { uint32_t v, K, R; int64_t off; };

// v = schedule[(step - 1) mod n_sched] (the sampler advanced the counter after its draw), K = min(*m_dev, cap, counts[v])
__device__ __forceinline__ RefView load_view(const RefSet& a) {
    RefView rv;
    const int64_t n = (int64_t)a.n_sched;
    const int64_t s = ((a.step_counter[0] - 1) % n + n) % n;
    const int32_t sv = a.schedule[s];
    rv.v = sv < 0 ? 0u : min((uint32_t)sv, a.V - 1u);
    const int32_t cnt = a.counts[rv.v];
    rv.K = min(min(*a.m_dev, a.cap), cnt > 0 ? (uint32_t)cnt : 0u);
    const int32_t r = a.ref_count[rv.v];
    rv.R = r > 0 ? (uint32_t)r : 0u;
    rv.off = a.row_off[rv.v];
    return rv;
}

// pred'[i][c] = fp16(pred[i][c] * w8s[off + i]): the fp32 product of two fp16 values is exact, the conversion rounds once (a
// compiler that folds the two into one mixed-precision instruction rounds the same exact product)
__device__ __forceinline__ half_t weighted(const RefSet& a, const RefView& rv, uint32_t i, int c) {
    return (half_t)((float)a.pred[(size_t)i * 3 + c] * (float)a.w8s[rv.off + i]);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// workgroup total in the documented order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red /* RS_BLOCK / 64 */) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t q = 0; q < RS_BLOCK / 64; q++) t += red[q];
    }
    __syncthreads();
    return t;
}

// rows: pred' (fp16 and fp32; zeros in rows >= K) and the registered squared error's partial per workgroup
__global__ __launch_bounds__(RS_BLOCK) void k_ref_rows(RefSet a, half_t* __restrict__ predw16, float* __restrict__ predw32,
                                                       double* __restrict__ part) {
    __shared__ double red[RS_BLOCK / 64];
    const RefView rv = load_view(a);
    const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < rv.K) {
        const double w = a.mode == LAE_REF_MODE_REF ? (double)a.ref_weight[rv.off + i] : 1.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const half_t p = weighted(a, rv, i, c);
            predw16[(size_t)i * 3 + c] = p;
            predw32[(size_t)i * 3 + c] = (float)p;
            // an unregistered row's target is never read: its weight is an exact zero
            const double t = a.mode == LAE_REF_MODE_REF ? (w != 0.0 ? (double)a.ref_target[(rv.off + i) * 3 + c] : (double)p)
                                                        : (double)a.target[(size_t)i * 3 + c];
            const double d = t - (double)p;
            e += w * (d * d);
        }
    } else if (i < a.cap) {
#pragma unroll
        for (int c = 0; c < 3; c++) { predw16[(size_t)i * 3 + c] = (half_t)0.0f; predw32[(size_t)i * 3 + c] = 0.0f; }
    }
    const double t = block_sum(e, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// colour patch: resid[o][c] = sum_taps tap_w * pred'[tap_row] - color_patch[c][o] (fp64, kept for the backward) and the partials
// of its squares
__global__ __launch_bounds__(RS_BLOCK) void k_ref_patch(RefSet a, const int32_t* __restrict__ tap_row, const float* __restrict__ color_patch,
                                                        double* __restrict__ resid, double* __restrict__ part) {
    __shared__ double red[RS_BLOCK / 64];
    const RefView rv = load_view(a);
    const uint32_t o = blockIdx.x * RS_BLOCK + threadIdx.x;
    double e = 0.0;
    if (o < a.n_out) {
        double acc[3] = {0.0, 0.0, 0.0};
        const size_t t0 = ((size_t)rv.v * a.n_out + o) * 4;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int32_t r = tap_row[t0 + t];
            if (r >= 0 && (uint32_t)r < rv.K) {
                const double w = (double)a.tap_w[t0 + t];
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += w * (double)weighted(a, rv, (uint32_t)r, c);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double d = acc[c] - (double)color_patch[((size_t)rv.v * 3 + c) * a.n_out + o];
            resid[(size_t)o * 3 + c] = d;
            e += d * d;
        }
    }
    const double t = block_sum(e, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// one wave: the two totals and their means
__global__ __launch_bounds__(64) void k_ref_final(RefSet a, const double* __restrict__ part_rows, const double* __restrict__ part_patch,
                                                  uint32_t nb_patch, float* __restrict__ terms) {
    const RefView rv = load_view(a);
    const uint32_t nb_rows = (rv.K + RS_BLOCK - 1) / RS_BLOCK;          // the partials past the live rows are zeros
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < nb_rows; b += 64) s += part_rows[b];
    s = wave_sum(s);
    double q = 0.0;
    if (a.mode == LAE_REF_MODE_REF) {
        for (uint32_t b = threadIdx.x; b < nb_patch; b += 64) q += part_patch[b];
        q = wave_sum(q);
    }
    if (threadIdx.x != 0) return;
    const uint32_t n = a.mode == LAE_REF_MODE_REF ? rv.R : rv.K;
    terms[0] = n ? (float)(s / (3.0 * (double)n)) : 0.0f;
    terms[1] = a.mode == LAE_REF_MODE_REF ? (float)(q / (3.0 * (double)a.n_out)) : 0.0f;
}

// g_pred[i][c] = w8s * (g_predw + g_terms[0] * d terms[0] / d pred' + g_terms[1] * d terms[1] / d pred'), rows >= K exactly 0
__global__ __launch_bounds__(RS_BLOCK) void k_ref_bwd(RefSet a, const int32_t* __restrict__ row_tap, const double* __restrict__ resid,
                                                      const float* __restrict__ g_predw, const float* __restrict__ g_terms,
                                                      float* __restrict__ g_pred) {
    const uint32_t i = blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= a.cap) return;
    const RefView rv = load_view(a);
    if (i >= rv.K) {
        g_pred[(size_t)i * 3 + 0] = 0.0f; g_pred[(size_t)i * 3 + 1] = 0.0f; g_pred[(size_t)i * 3 + 2] = 0.0f;
        return;
    }
    const bool ref = a.mode == LAE_REF_MODE_REF;
    const uint32_t n = ref ? rv.R : rv.K;
    const double w = ref ? (double)a.ref_weight[rv.off + i] : 1.0;
    const double k0 = n ? (double)g_terms[0] * 2.0 * w / (3.0 * (double)n) : 0.0;
    double k1 = 0.0;
    uint32_t o = 0;
    if (ref) {
        const int32_t tp = row_tap[rv.off + i];
        if (tp >= 0 && (uint32_t)tp < a.n_out * 4u) {
            o = (uint32_t)tp >> 2;
            k1 = (double)g_terms[1] * 2.0 * (double)a.tap_w[(size_t)rv.v * a.n_out * 4 + (uint32_t)tp] / (3.0 * (double)a.n_out);
        }
    }
    const double ws = (double)a.w8s[rv.off + i];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double p = (double)weighted(a, rv, i, c);
        double g = g_predw ? (double)g_predw[(size_t)i * 3 + c] : 0.0;
        if (k0 != 0.0) {
            const double t = ref ? (double)a.ref_target[(rv.off + i) * 3 + c] : (double)a.target[(size_t)i * 3 + c];
            g += k0 * (p - t);
        }
        if (k1 != 0.0) g += k1 * resid[(size_t)o * 3 + c];
        g_pred[(size_t)i * 3 + c] = (float)(ws * g);
    }
}

int check_set(const RefSet& a) {
    if (!a.pred || !a.m_dev || !a.schedule || !a.step_counter || !a.row_off || !a.counts || !a.w8s) return LAE_ENULL;
    if (a.mode != LAE_REF_MODE_GT && a.mode != LAE_REF_MODE_REF) return LAE_EINVAL;
    if (a.mode == LAE_REF_MODE_GT && !a.target) return LAE_ENULL;
    if (a.mode == LAE_REF_MODE_REF && (!a.ref_target || !a.ref_weight || !a.ref_count || !a.tap_w)) return LAE_ENULL;
    if (a.cap == 0 || a.n_sched == 0 || a.V == 0 || (a.mode == LAE_REF_MODE_REF && (a.n_out == 0 || a.n_out > (1u << 28)))) return LAE_EINVAL;
    return LAE_OK;
}

}  // namespace

extern "C" {

uint64_t lae_ref_terms_scratch_bytes(uint32_t cap, uint32_t n_out) {
    return ((uint64_t)lae::cdiv(cap, RS_BLOCK) + lae::cdiv(n_out, RS_BLOCK)) * sizeof(double) + 256;
}

int lae_ref_terms_forward(const void* pred, uint32_t cap, const uint32_t* m_dev, const float* target, const int32_t* schedule,
                          uint32_t n_sched, const int64_t* step_counter, uint32_t V, const int64_t* row_off, const int32_t* counts,
                          const void* w8s, const float* ref_target, const float* ref_weight, const int32_t* ref_count,
                          const int32_t* tap_row, const float* tap_w, const float* color_patch, uint32_t n_out, int mode, void* predw16,
                          float* predw32, double* resid, void* scratch, float* terms, void* stream) {
    const RefSet a{(const half_t*)pred, cap, m_dev, target, schedule, n_sched, step_counter, V, row_off, counts, (const half_t*)w8s,
                   ref_target, ref_weight, ref_count, tap_w, n_out, mode};
    const int rc = check_set(a);
    if (rc) return rc;
    if (!predw16 || !predw32 || !scratch || !terms) return LAE_ENULL;
    if (mode == LAE_REF_MODE_REF && (!tap_row || !color_patch || !resid)) return LAE_ENULL;
    hipStream_t s = STREAM(stream);
    const uint32_t nb_rows = lae::cdiv(cap, RS_BLOCK), nb_patch = mode == LAE_REF_MODE_REF ? lae::cdiv(n_out, RS_BLOCK) : 0u;
    double* part_rows = (double*)scratch;
    double* part_patch = part_rows + nb_rows;
    k_ref_rows<<<nb_rows, RS_BLOCK, 0, s>>>(a, (half_t*)predw16, predw32, part_rows);
    if (nb_patch) k_ref_patch<<<nb_patch, RS_BLOCK, 0, s>>>(a, tap_row, color_patch, resid, part_patch);
    k_ref_final<<<1, 64, 0, s>>>(a, part_rows, part_patch, nb_patch, terms);
    return lae::check_launch("ref_terms_forward");
}

int lae_ref_terms_backward(const void* pred, uint32_t cap, const uint32_t* m_dev, const float* target, const int32_t* schedule,
                           uint32_t n_sched, const int64_t* step_counter, uint32_t V, const int64_t* row_off, const int32_t* counts,
                           const void* w8s, const float* ref_target, const float* ref_weight, const int32_t* ref_count,
                           const int32_t* row_tap, const float* tap_w, const double* resid, uint32_t n_out, int mode, const float* g_predw,
                           const float* g_terms, float* g_pred, void* stream) {
    const RefSet a{(const half_t*)pred, cap, m_dev, target, schedule, n_sched, step_counter, V, row_off, counts, (const half_t*)w8s,
                   ref_target, ref_weight, ref_count, tap_w, n_out, mode};
    const int rc = check_set(a);
    if (rc) return rc;
    if (!g_terms || !g_pred) return LAE_ENULL;
    if (mode == LAE_REF_MODE_REF && (!row_tap || !resid)) return LAE_ENULL;
    k_ref_bwd<<<lae::cdiv(cap, RS_BLOCK), RS_BLOCK, 0, STREAM(stream)>>>(a, row_tap, resid, g_predw, g_terms, g_pred);
    return lae::check_launch("ref_terms_backward");
}

}  // extern "C"
