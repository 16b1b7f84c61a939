// mlp_frags.h -- MFMA fragment helpers shared by the MLP translation units: ffmlp.hip (the general FFMLP operator), nerfhead.hip
// (fused NeRF head forward, frame loop's head) and mlpbackward.hip (fused recompute backward).  Everything here is used by at
// least two of them; what one file alone needs lives in that file.  Fragment layout (v_mfma_f32_16x16x16_f16, wave64, network
// evaluated transposed, H^T = W * X^T): lane = (c, g) = (lane & 15, lane >> 4); an A / B fragment holds k-slots 4g .. 4g+3 of
// row / batch column c, a C/D fragment features 4g .. 4g+3 of batch column c -- see the head of ffmlp.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef _Float16 half_t;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma16(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }

// K = 32 form (gfx950: the same 16 cycles as the K = 16 instruction, twice the work).  Lane group g owns k-slots
// 8g..8g+7 of BOTH operands; we fill slots 8g..8g+3 from k-step `lo` and 8g+4..8g+7 from k-step `hi`, i.e. the two
// 16-wide fragments a lane already holds in the K = 16 layout are simply concatenated.  A and B use the same
// permutation of k, so the contraction is unchanged and activations still chain layer to layer in registers.
__device__ __forceinline__ f4 mfma32(h4 a_lo, h4 a_hi, h4 b_lo, h4 b_hi, f4 c) {
    const h8 a = __builtin_shufflevector(a_lo, a_hi, 0, 1, 2, 3, 4, 5, 6, 7);
    const h8 b = __builtin_shufflevector(b_lo, b_hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
// acc += sum_{kt < KT} A(kt) * b[kt]: k-steps two at a time, one K = 16 step for an odd tail
template <int KT, typename LoadA>
__device__ __forceinline__ f4 mfma_ksteps(LoadA&& a_of, const h4* b, f4 acc) {
#pragma unroll
    for (int kt = 0; kt + 1 < KT; kt += 2) acc = mfma32(a_of(kt), a_of(kt + 1), b[kt], b[kt + 1], acc);
    // The odd tail is a K = 32 step with zeros in the upper k-slots, NOT the K = 16 instruction: a v_mfma_f32_16x16x16_f16
    // whose accumulator input is the result of the v_mfma_f32_16x16x32_f16 issued just before it read a stale accumulator in
    // k_mlp_bwd_wave<48, 1> (second tile's first-layer sums wrong, correct again with this form or with unrelated code moved:
    // tests/test_gpu_ffmlp.py[*-48-64-2]) -- the compiler's wait-state padding between the two shapes is not enough on gfx950.
    // Same cycles (the K = 16 form occupies the pipe as long as the K = 32 form), same sums.
    if constexpr (KT & 1) {
        const h4 z = h4{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f};
        acc = mfma32(a_of(KT - 1), z, b[KT - 1], z, acc);
    }
    return acc;
}

// ReLU + fp16 rounding of a 64-wide layer.  round(max(x, 0)) == max(round(x), 0), so the maximum is taken on the packed
// halves (v_cvt_pk_f16_f32 + v_pk_max_f16: 2 values per instruction; fmaxf on the floats costs a canonicalising
// v_max_f32 plus the real one per value -- 160 of the head forward's ~700 VALU instructions per tile)
__device__ __forceinline__ void relu4(const f4 (&acc)[4], h4 (&out)[4]) {
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        h2 lo = {(half_t)acc[mt][0], (half_t)acc[mt][1]}, hi = {(half_t)acc[mt][2], (half_t)acc[mt][3]};
        lo = __builtin_elementwise_max(lo, h2{(half_t)0.0f, (half_t)0.0f});
        hi = __builtin_elementwise_max(hi, h2{(half_t)0.0f, (half_t)0.0f});
        out[mt] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
    }
}

// a row-major [rows, cols] weight matrix -> LDS with row stride ld (padded rows), by the whole workgroup of NTH threads
// (0: blockDim.x, read at run time)
template <int NTH = 0>
__device__ __forceinline__ void stage_rows(half_t* dst, int ld, const half_t* __restrict__ src, int rows, int cols) {
    for (uint32_t e = threadIdx.x; e < (uint32_t)rows * cols / 4; e += NTH ? NTH : blockDim.x) {
        const uint32_t r = (e * 4) / cols, k = (e * 4) % cols;
        *reinterpret_cast<h4*>(dst + r * ld + k) = *reinterpret_cast<const h4*>(src + (size_t)r * cols + k);
    }
}

// sh_eval: the head forward evaluates it per row, the head backward inside color_inputs
#include "sh_table.inc"

// in-kernel phase stamps for tools/ubench/mlp_probe.hip (compiled in only there): 100 MHz wall clock + shader clock.  One array
// per translation unit (no relocatable device code), like the grid files' (grid_levels.h).
#ifdef LAE_MLP_STAMPS
__device__ unsigned long long g_mlp_stamps[4096 * 64];
#define MLP_STAMP(slot, i) do { if ((threadIdx.x & 63) == 0 && (i) < 32) { g_mlp_stamps[(size_t)(slot) * 64 + 2 * (i)] = wall_clock64(); \
                                g_mlp_stamps[(size_t)(slot) * 64 + 2 * (i) + 1] = __builtin_readcyclecounter(); } } while (0)
#define MLP_PHASE(slot, i) do { if (stamp_i == 3) MLP_STAMP(slot, 16 + (i)); } while (0)
#else
#define MLP_STAMP(slot, i) do { } while (0)
#define MLP_PHASE(slot, i) do { } while (0)
#endif

}  // namespace
