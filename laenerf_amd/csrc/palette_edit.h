// palette_edit.h -- the palette network's per-row colour rule, shared by recolor.hip (lae_recolor_compose) and distill.hip
// (lae_distill_compose): softmax of the active logits, the user's weight / bias edit and the palette product.
// Every operation is one fp32 rounding (explicit _rn intrinsics, no contraction); exp runs in double and is rounded once.
// Column j of a row is active when bit j of `mask` is set; `a` counts the active columns (the row of the compacted palette).
#pragma once
#include "lae_common.h"

namespace lae {

// l[j] = exp(logit_j - max over the active logits) for active j (0 elsewhere); returns their sum in column order
__device__ __forceinline__ float palette_softmax_exp(const _Float16* wl, uint32_t mask, float (&l)[16]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        l[j] = (mask >> j) & 1u ? (float)wl[j] : 0.0f;
        if ((mask >> j) & 1u) m = fmaxf(m, l[j]);
    }
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) { l[j] = (float)exp((double)__fsub_rn(l[j], m)); sum = __fadd_rn(sum, l[j]); }
    return sum;
}

// w_j = l_j / sum (the softmax weights w_og)
__device__ __forceinline__ void palette_normalise(float (&l)[16], uint32_t mask, float sum) {
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) l[j] = __fdiv_rn(l[j], sum);
}

// the user's edit: w'_j = max(p_bias_a + p_weights_a * w_j, 0), then w' /= sum(w'); sum(w') == 0 (every edited weight clamped
// away): the weights count as zero (the reference divides 0 / 0)
__device__ __forceinline__ void palette_edit(float (&l)[16], uint32_t mask, const float* p_weights, const float* p_bias) {
    float wsum = 0.0f;
    int act = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) {
            l[j] = fmaxf(__fadd_rn(p_bias[act], __fmul_rn(p_weights[act], l[j])), 0.0f);
            wsum = __fadd_rn(wsum, l[j]);
            act++;
        }
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) l[j] = wsum > 0.0f ? __fdiv_rn(l[j], wsum) : 0.0f;
}

// acc = w @ pal (pal [n_active, 3]), summed in column order
__device__ __forceinline__ void palette_product(const float (&l)[16], uint32_t mask, const float* pal, float (&acc)[3]) {
    acc[0] = acc[1] = acc[2] = 0.0f;
    int act = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((mask >> j) & 1u) {
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] = __fadd_rn(acc[c], __fmul_rn(l[j], pal[3 * act + c]));
            act++;
        }
}

}  // namespace lae
