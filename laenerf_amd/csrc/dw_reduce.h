// Weight-gradient slab reduction and deferred loss value of the fused NeRF head backward: the device bodies, shared by
// k_dw_reduce (ffmlp.hip) / k_dw_reduce2 (mlpbackward.hip) and by the tail tasks of the hash-grid accumulate pass (gridbackward.hip k_bwd_acc),
// which takes the reduction along instead of a launch of its own.  Both users run them with 1024 threads per workgroup and
// execute the same statements in the same order: the fp16 weight gradients and the loss value have the same bits either way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace lae_dw {

typedef _Float16 half_t;
constexpr int DWR_GROUPS = 16;
constexpr uint32_t DWR_THREADS = 64 * DWR_GROUPS;
constexpr uint32_t DWR_LDS_FLOATS = DWR_GROUPS * 64;          // scratch of one reduce block (the loss block needs 16 of them)

// sum the per-slice slabs in a fixed order (deterministic) and round once to fp16.
// 1024 threads = 64 weights x 16 slice groups, 8 slab loads in flight per lane (the kernel is pure load latency: 512
// slabs of 45 KB); the 16 partial sums are combined in a fixed tree.
// accumulate != 0: gw += sum (the optimizer's persistent gradient buffer) instead of gw = sum.
// part: DWR_LDS_FLOATS floats of LDS, free for this call from its first statement to its return (no barrier after the last read:
// the caller separates it from its next use of that memory).
__device__ __forceinline__ void dw_reduce_body(const float* __restrict__ slabs, uint32_t n_slices, uint32_t nW, half_t* __restrict__ gw,
                                               int accumulate, uint32_t block, int32_t* __restrict__ nf_flag, float* part) {
    const uint32_t e = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const uint32_t i = block * 64 + e;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nW) {
        uint32_t k = sg;
        for (; k + 7 * DWR_GROUPS < n_slices; k += 8 * DWR_GROUPS) {
#pragma unroll
            for (int u = 0; u < 8; u++) s[u] += slabs[(size_t)(k + u * DWR_GROUPS) * nW + i];
        }
        for (; k < n_slices; k += DWR_GROUPS) s[0] += slabs[(size_t)k * nW + i];
    }
    part[sg * 64 + e] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (sg == 0 && i < nW) {
        float t[DWR_GROUPS];
#pragma unroll
        for (int u = 0; u < DWR_GROUPS; u++) t[u] = part[u * 64 + e];
#pragma unroll
        for (int w = DWR_GROUPS / 2; w > 0; w >>= 1)
#pragma unroll
            for (int u = 0; u < w; u++) t[u] = t[u] + t[u + w];
        const half_t r = accumulate ? (half_t)((float)gw[i] + t[0]) : (half_t)t[0];
        gw[i] = r;
        // the caller's flag (the optimizer's found_inf word): a non-finite weight gradient is reported where it is stored
        if (nf_flag && (__builtin_bit_cast(uint16_t, r) & 0x7c00u) == 0x7c00u) atomicOr(nf_flag, 1);
    }
}

// the deferred loss value (lae_composite_rays_train_step with defer_loss): the fixed-order sum of the criterion's per-workgroup
// partials -> out[0] = mean * scale, out[1] = mean, the arithmetic of k_loss_finish (raymarching.hip).  One workgroup of 1024.
struct LossFinish { const float* partials; uint32_t n_part, n_elem; const float* scale; float* out; };
__device__ __forceinline__ void loss_finish_block(const LossFinish& lf, float* part) {
    static_assert(DWR_THREADS == 1024, "the loss sum is written for 16 waves, like k_loss_finish");
    float acc = 0.0f;
    for (uint32_t i = threadIdx.x; i < lf.n_part; i += 1024) acc += lf.partials[i];
    {   // the wave sum of raymarching.hip (wave_sum = last lane of the DPP inclusive scan), statement for statement: the
        // deferred value has the same bits as the one k_loss_finish writes
        auto dpp = [](float v, auto ctrl, auto mask) {
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, decltype(mask)::value, 0xf, false));
        };
        using std::integral_constant;
        acc += dpp(acc, integral_constant<int, 0x111>{}, integral_constant<int, 0xf>{});
        acc += dpp(acc, integral_constant<int, 0x112>{}, integral_constant<int, 0xf>{});
        acc += dpp(acc, integral_constant<int, 0x114>{}, integral_constant<int, 0xf>{});
        acc += dpp(acc, integral_constant<int, 0x118>{}, integral_constant<int, 0xf>{});
        acc += dpp(acc, integral_constant<int, 0x142>{}, integral_constant<int, 0xa>{});
        acc += dpp(acc, integral_constant<int, 0x143>{}, integral_constant<int, 0xc>{});
        acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, acc), 63));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; w++) t += part[w];
        const float loss = t / (float)lf.n_elem;
        lf.out[0] = loss * (lf.scale ? lf.scale[0] : 1.0f);
        lf.out[1] = loss;
    }
}

// the reduction of two networks' slabs (+ the loss block) as a list of workgroup-sized tasks: task [0, nb_a) reduces network A,
// [nb_a, nb_a + nb_b) network B, task nb_a + nb_b (only with lf.out) finishes the loss.  k_dw_reduce2 runs one per block; the
// accumulate pass of the grid backward runs them on the tickets behind its own tasks.
struct DwTailJob {
    const float* slabs_a; uint32_t n_a, nW_a; half_t* gw_a;
    const float* slabs_b; uint32_t n_b, nW_b; half_t* gw_b;
    uint32_t nb_a, nb_b;
    int accumulate;
    int32_t* nf_flag;
    LossFinish lf;
    uint32_t n_tasks;                                         // nb_a + nb_b + (lf.out ? 1 : 0); 0 = no job
};
__device__ __forceinline__ void dw_tail_task(const DwTailJob& j, uint32_t task, float* part) {
    if (task < j.nb_a) dw_reduce_body(j.slabs_a, j.n_a, j.nW_a, j.gw_a, j.accumulate, task, j.nf_flag, part);
    else if (task < j.nb_a + j.nb_b) dw_reduce_body(j.slabs_b, j.n_b, j.nW_b, j.gw_b, j.accumulate, task - j.nb_a, j.nf_flag, part);
    else loss_finish_block(j.lf, part);
}

}  // namespace lae_dw
