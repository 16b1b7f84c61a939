// grid_levels.h -- what the forward (gridencoder.hip) and the backward (gridbackward.hip) of the hash / tiled grid encoder share:
// the per-level description of the table, the cell index, the blockIdx -> (level, chunk) map and the phase stamps of probe builds.
// Everything here has internal linkage: each translation unit is compiled on its own (-fno-gpu-rdc) and gets its own copy.
#pragma once
#include <math.h>
#include <stdint.h>
#include "lae_common.h"

namespace {

constexpr int MAX_LEVELS = 32;
// scale[l] = exp2(l*S)*H - 1 (host, :138).  in_shift / in_scale: optional affine map applied to every coordinate as it
// is read, x01 = (x + in_shift) * in_scale -- GridEncoder.forward's `(inputs + bound) / (2 * bound)` (grid.py:149; torch
// evaluates the division by a Python scalar as a multiplication by its fp32 reciprocal) without two extra kernels.
struct LevelScales { float scale[MAX_LEVELS]; float in_shift, in_scale; };

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));

__constant__ uint32_t k_primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};

constexpr int GRID_BLOCK = 256;

// in-kernel phase stamps for tools/grid_bwd_stamps.py (the binned backward) and tools/grid_fwd_spans.py / frame_grid_spans.py (the
// lean forward), compiled in only with -DLAE_GRID_STAMPS: the 100 MHz wall clock as thread 0 of a block passes each phase; slot =
// block, 32 stamps each.  One array per translation unit: lae_debug_grid_stamps reads the forward's, lae_debug_grid_bwd_stamps the
// backward's.
#ifdef LAE_GRID_STAMPS
__device__ unsigned long long g_grid_stamps[32768 * 32];     // (8 MB, probe builds only: a 1080p frame's encoder launch is 216 k blocks)
#define GRID_STAMP(slot, i) do { if (threadIdx.x == 0 && (uint32_t)(i) < 32u) g_grid_stamps[(size_t)(slot) * 32 + (i)] = wall_clock64(); } while (0)
#define GRID_NOTE(slot, i, v) do { if (threadIdx.x == 0 && (uint32_t)(i) < 32u) g_grid_stamps[(size_t)(slot) * 32 + (i)] = (v); } while (0)
#define GRID_STAMPS_READER(name)                                                                       \
    extern "C" __attribute__((visibility("default"))) int name(void* out, size_t bytes) {             \
        if (hipDeviceSynchronize() != hipSuccess) return 1;                                            \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_grid_stamps), bytes) == hipSuccess ? 0 : 1;       \
    }
#else
#define GRID_STAMP(slot, i) do { } while (0)
#define GRID_NOTE(slot, i, v) do { } while (0)
#endif

// block-uniform description of one level (all derived from scalars -> SGPRs)
template <int D>
struct LevelInfo {
    float scale;
    uint32_t resolution, hashmap_size, table_off;
    uint32_t stride[D];      // dense strides of the dims that fit (gridencoder.cu:72-75)
    uint32_t ndense;         // how many dims the dense loop consumed
    bool use_hash, pow2;
    bool nowrap;             // dense index provably < hashmap_size (all dims indexed and (res+1)^D <= size): no modulo needed
};

template <int D>
__device__ __forceinline__ LevelInfo<D> level_info(const LevelScales& sc, const int32_t* __restrict__ offsets,
                                                   uint32_t level, uint32_t gridtype, bool align_corners) {
    LevelInfo<D> li;
    li.scale = sc.scale[level];
    li.resolution = (uint32_t)ceilf(li.scale) + 1;
    li.table_off = (uint32_t)offsets[level];
    li.hashmap_size = (uint32_t)offsets[level + 1] - li.table_off;
    uint32_t stride = 1;
    li.ndense = 0;
#pragma unroll
    for (int d = 0; d < D; d++) {
        li.stride[d] = 0;
        if (li.ndense == (uint32_t)d && stride <= li.hashmap_size) {
            li.stride[d] = stride;
            stride *= align_corners ? li.resolution : (li.resolution + 1);
            li.ndense = d + 1;
        }
    }
    li.use_hash = (gridtype == 0) && (stride > li.hashmap_size);
    li.nowrap = (li.ndense == (uint32_t)D) && (stride <= li.hashmap_size);
    li.pow2 = (li.hashmap_size & (li.hashmap_size - 1)) == 0;
    return li;
}

// gridencoder.cu:66-84
template <int D>
__device__ __forceinline__ uint32_t cell_index(const LevelInfo<D>& li, const uint32_t (&pg)[D]) {
    uint32_t index = 0;
    if (li.use_hash) {
#pragma unroll
        for (int d = 0; d < D; d++) index ^= pg[d] * k_primes[d];
    } else {
#pragma unroll
        for (int d = 0; d < D; d++) index += pg[d] * li.stride[d];   // stride 0 for dims the loop skipped
    }
    return li.pow2 ? (index & (li.hashmap_size - 1)) : (index % li.hashmap_size);
}

__device__ __forceinline__ void block_to_level_chunk(uint32_t nb, bool xcd_mode, uint32_t& level, uint32_t& chunk) {
    const uint32_t bid = blockIdx.x;
    if (xcd_mode) {
        const uint32_t xcd = bid & 7u, j = bid >> 3;
        level = xcd + 8u * (j / nb);
        chunk = j % nb;
    } else {
        level = bid / nb;
        chunk = bid % nb;
    }
}

inline int fill_scales(LevelScales& sc, uint32_t L, float S, uint32_t H) {
    if (L == 0 || L > MAX_LEVELS) return LAE_EINVAL;
    for (uint32_t l = 0; l < L; l++) sc.scale[l] = fmaf(exp2f((float)l * S), (float)H, -1.0f);   // :138
    for (uint32_t l = L; l < MAX_LEVELS; l++) sc.scale[l] = 0.f;
    sc.in_shift = 0.0f; sc.in_scale = 1.0f;
    return LAE_OK;
}

}  // namespace
