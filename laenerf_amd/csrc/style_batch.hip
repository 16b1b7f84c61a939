// style_batch.hip -- one training view of the LAENeRF palette network from a device-resident edit set
// (lae_sample_edit_view, include/laenerf.h).
//
// The reference hands each step one view of its EditDataset through a DataLoader: `collate` copies the view's CPU tensors to
// the device and jitters the termination points along their rays, x = x_term + ((rand(K) - 0.5) * depth_factor)[:, None] * dirs
// (editing/edit_dataset.py:289-300).  Here the views are packed once on the device; this kernel reads the step's view from a
// device schedule at the device step counter, writes the jittered points, directions and targets into capacity-sized
// buffers and the live row count K into device memory, and a second one-thread launch advances the counter, so a captured
// graph draws the next view on every replay.
//
// Rows K..cap-1 are copies of the jittered row K-1: they touch the hash-table lines the view touches already, and the losses
// ignore them (lae_style_loss_*_dev with the row count this kernel writes).
//
// Pure bandwidth (~60 B per row): one thread per FOUR rows, so that each of the three [cap,3] fp32 outputs is written with three
// 16-byte stores per thread (48 bytes = 4 rows); cap is a multiple of 4.  Compiled with -ffp-contract=off like every file of the
// library; the jitter's multiply and add are spelled __fmul_rn / __fadd_rn anyway.
#include "lae_common.h"
#include "philox.h"

namespace {

constexpr uint32_t SV_BLOCK = 256;
constexpr uint32_t SV_ROWS = 4;                  // rows per thread

__global__ __launch_bounds__(SV_BLOCK) void k_sample_edit_view(
    const float* __restrict__ x_term, const float* __restrict__ dirs, const float* __restrict__ targets,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ counts, const float* __restrict__ depth_factor, uint32_t V,
    const int32_t* __restrict__ schedule, uint32_t n_sched, uint32_t cap, uint32_t k0, uint32_t k1,
    const int64_t* __restrict__ step_counter, float* __restrict__ x, float* __restrict__ d, float* __restrict__ target,
    uint32_t* __restrict__ m_dev) {
    const uint64_t step = (uint64_t)step_counter[0];
    const int32_t sv = schedule[step % n_sched];
    const uint32_t v = sv < 0 ? 0u : min((uint32_t)sv, V - 1u);                 // the host validates; this only keeps reads in bounds
    const int32_t kc = counts[v];
    const uint32_t K = kc < 0 ? 0u : min((uint32_t)kc, cap);
    const uint32_t t = blockIdx.x * SV_BLOCK + threadIdx.x;
    if (t == 0) *m_dev = K;
    const uint32_t r0 = t * SV_ROWS;
    if (r0 >= cap) return;
    const size_t base = (size_t)offsets[v];
    const float df = depth_factor[v];
    float ox[SV_ROWS * 3], od[SV_ROWS * 3], ot[SV_ROWS * 3];
#pragma unroll
    for (uint32_t q = 0; q < SV_ROWS; q++) {
        const uint32_t r = r0 + q;
        if (K == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) { ox[3 * q + c] = 0.0f; od[3 * q + c] = 0.0f; ot[3 * q + c] = 0.0f; }
            continue;
        }
        const uint32_t src = r < K ? r : K - 1u;                               // pad rows: the jittered last row
        const size_t e = (base + src) * 3;
        const uint32_t w = lae::philox4x32_10_w0((uint32_t)step, src, 0u, 2u, k0, k1);
        const float u = (float)(w >> 8) * 0x1p-24f;                            // exact: 24-bit integer times 2^-24
        const float jt = __fmul_rn(__fsub_rn(u, 0.5f), df);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float dc = dirs[e + c];
            ox[3 * q + c] = __fadd_rn(x_term[e + c], __fmul_rn(jt, dc));
            od[3 * q + c] = dc;
            ot[3 * q + c] = targets[e + c];
        }
    }
    float4* __restrict__ x4 = reinterpret_cast<float4*>(x + (size_t)r0 * 3);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + (size_t)r0 * 3);
    float4* __restrict__ t4 = reinterpret_cast<float4*>(target + (size_t)r0 * 3);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        x4[j] = make_float4(ox[4 * j], ox[4 * j + 1], ox[4 * j + 2], ox[4 * j + 3]);
        d4[j] = make_float4(od[4 * j], od[4 * j + 1], od[4 * j + 2], od[4 * j + 3]);
        t4[j] = make_float4(ot[4 * j], ot[4 * j + 1], ot[4 * j + 2], ot[4 * j + 3]);
    }
}

__global__ void k_advance_edit_step(int64_t* __restrict__ step_counter) { step_counter[0] += 1; }

}  // namespace

extern "C" {

int lae_sample_edit_view(const float* x_term, const float* dirs, const float* targets, const int64_t* offsets, const int32_t* counts,
                         const float* depth_factor, uint32_t V, const int32_t* schedule, uint32_t n_sched, uint32_t cap, uint64_t seed,
                         int64_t* step_counter, float* x, float* d, float* target, uint32_t* m_dev, void* stream) {
    if (!x_term || !dirs || !targets || !offsets || !counts || !depth_factor || !schedule || !step_counter || !x || !d || !target || !m_dev)
        return LAE_ENULL;
    if (V == 0 || n_sched == 0 || cap == 0 || cap % SV_ROWS) return LAE_EINVAL;
    // the 16-byte stores need 16-byte aligned outputs (every torch allocation is)
    if (((uintptr_t)x | (uintptr_t)d | (uintptr_t)target) & 15u) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t threads = cap / SV_ROWS;
    k_sample_edit_view<<<lae::cdiv(threads, SV_BLOCK), SV_BLOCK, 0, s>>>(x_term, dirs, targets, offsets, counts, depth_factor, V, schedule,
                                                                       n_sched, cap, (uint32_t)seed, (uint32_t)(seed >> 32), step_counter,
                                                                       x, d, target, m_dev);
    k_advance_edit_step<<<1, 1, 0, s>>>(step_counter);
    return lae::check_launch("sample_edit_view");
}

}  // extern "C"
