// mesh.hip -- marching cubes over a dense fp32 field on the device (the reference runs PyMCubes on the host after copying the
// field there chunk by chunk, nerf/utils.py:189-219).  The output order is fixed by the specification in include/laenerf.h,
// not by the schedule: no atomics, so two runs give the same bits.
//
// One thread owns MC_ITEMS consecutive lattice points p (C order, so the threads of a wave walk along k).  Point p owns the
// lattice edges that start at it (its 3-bit edge mask) and the cube whose lower corner it is.
//   count:     per block, the vertices (owned crossed edges) and triangles (MC_TRI_COUNT of the cube's case)
//   scan:      one block: exclusive prefixes of the block counts, totals -> counts[0..1]
//   vertices:  positions; per point the packed word base | mask << 29 (base = the point's first vertex id)
//   triangles: each cube-local edge -> base[owner] + rank of its axis in the owner's mask; runs after the vertex pass, since
//              a cube reads the words of points in other blocks
#include "lae_common.h"

namespace {

#include "mc_table.inc"

constexpr int MC_THREADS = 256;
constexpr int MC_ITEMS = 4;
constexpr uint32_t MC_TILE = MC_THREADS * MC_ITEMS;      // points per block
constexpr int MC_SCAN_THREADS = 1024;
constexpr uint32_t MC_BASE_BITS = 29;                    // V <= 3 * 512^3 < 2^29
constexpr uint32_t MC_BASE_MASK = (1u << MC_BASE_BITS) - 1u;

struct Dims {
    uint32_t nx, ny, nz, nyz, P;
};

__host__ __device__ __forceinline__ uint32_t scratch_blocks(uint32_t P) { return (P + MC_TILE - 1) / MC_TILE; }
// scratch: uint32 vertex counts [nb], triangle counts [nb], then the per-point words [P] (16-byte aligned)
__host__ __device__ __forceinline__ uint64_t words_offset(uint32_t nb) { return ((uint64_t)8 * nb + 15) & ~(uint64_t)15; }

// the values of one lattice row at idx .. idx + 4 (entries at or beyond P are not read; they belong to no edge)
template <bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ u, uint32_t idx, uint32_t P, float (&r)[MC_ITEMS + 1]) {
    if (VEC) {                                           // idx % 4 == 0 and P % 4 == 0: idx < P -> idx + 3 < P
        if (idx < P) {
            const float4 q = *reinterpret_cast<const float4*>(u + idx);
            r[0] = q.x; r[1] = q.y; r[2] = q.z; r[3] = q.w;
        }
        if (idx + MC_ITEMS < P) r[MC_ITEMS] = u[idx + MC_ITEMS];
    } else {
#pragma unroll
        for (int q = 0; q <= MC_ITEMS; q++)
            if (idx + q < P) r[q] = u[idx + q];
    }
}

// the field around a thread's points: v[2 * dx + dy][q + dz] = u[i + dx, j + dy, k + dz] of the thread's point q
struct Window {
    float v[4][MC_ITEMS + 1];
    uint32_t p0, i, j, k;                                // the first point and its coordinates
};

template <bool VEC>
__device__ __forceinline__ void load_window(const float* __restrict__ u, const Dims& d, Window& w) {
    w.p0 = blockIdx.x * MC_TILE + threadIdx.x * MC_ITEMS;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int q = 0; q <= MC_ITEMS; q++) w.v[r][q] = 0.0f;
    w.i = w.p0 / d.nyz;
    const uint32_t rem = w.p0 - w.i * d.nyz;
    w.j = rem / d.nz;
    w.k = rem - w.j * d.nz;
    if (w.p0 >= d.P) return;
    load_row<VEC>(u, w.p0, d.P, w.v[0]);
    load_row<VEC>(u, w.p0 + d.nz, d.P, w.v[1]);
    load_row<VEC>(u, w.p0 + d.nyz, d.P, w.v[2]);
    load_row<VEC>(u, w.p0 + d.nyz + d.nz, d.P, w.v[3]);
}

// point q of the window (coordinates i, j, k): its owned-edge mask (bit = axis) and its cube's case (-1: no cube)
__device__ __forceinline__ void point_bits(const Window& w, int q, uint32_t i, uint32_t j, uint32_t k, const Dims& d, float thr,
                                           uint32_t& mask, int& cse) {
    const bool hx = i + 1 < d.nx, hy = j + 1 < d.ny, hz = k + 1 < d.nz;
    const bool b0 = w.v[0][q] > thr;                     // inside: strictly above (NaN is outside)
    mask = (uint32_t)(hx && b0 != (w.v[2][q] > thr)) | (uint32_t)(hy && b0 != (w.v[1][q] > thr)) << 1 |
           (uint32_t)(hz && b0 != (w.v[0][q + 1] > thr)) << 2;
    cse = -1;
    if (hx && hy && hz) {
        int c = 0;
#pragma unroll
        for (int corner = 0; corner < 8; corner++)
            c |= (int)(w.v[2 * (corner & 1) + ((corner >> 1) & 1)][q + (corner >> 2)] > thr) << corner;
        cse = c;
    }
}

__device__ __forceinline__ void next_point(uint32_t& i, uint32_t& j, uint32_t& k, const Dims& d) {
    if (++k == d.nz) { k = 0; if (++j == d.ny) { j = 0; i++; } }
}

// per point q: owned-edge mask and triangle count; returns (triangles << 16) | vertices summed over the thread's points
__device__ __forceinline__ uint32_t thread_counts(const Window& w, const Dims& d, float thr, uint32_t (&mask)[MC_ITEMS],
                                                  int (&cse)[MC_ITEMS]) {
    uint32_t nv = 0, nt = 0, i = w.i, j = w.j, k = w.k;
#pragma unroll
    for (int q = 0; q < MC_ITEMS; q++) {
        mask[q] = 0; cse[q] = -1;
        if (w.p0 + q < d.P) {
            point_bits(w, q, i, j, k, d, thr, mask[q], cse[q]);
            nv += __builtin_popcount(mask[q]);
            if (cse[q] >= 0) nt += MC_TRI_COUNT[cse[q]];
        }
        next_point(i, j, k, d);
    }
    return nt << 16 | nv;                                // a block holds <= 3 * 1024 vertices and <= 5 * 1024 triangles
}

template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_count(const float* __restrict__ u, Dims d, float thr, uint32_t* __restrict__ counts_v,
                                                         uint32_t* __restrict__ counts_t) {
    static_assert(3 * MC_TILE < 65536 && MC_MAX_TRIS * MC_TILE < 65536, "packed block counts");
    __shared__ uint32_t lds[MC_THREADS / LAE_WAVE + 1];
    Window w;
    load_window<VEC>(u, d, w);
    uint32_t mask[MC_ITEMS];
    int cse[MC_ITEMS];
    const uint32_t c = thread_counts(w, d, thr, mask, cse);
    uint32_t total;
    lae::block_excl_scan<MC_THREADS / LAE_WAVE>(c, &total, lds);
    if (threadIdx.x == 0) { counts_v[blockIdx.x] = total & 0xffffu; counts_t[blockIdx.x] = total >> 16; }
}

// one block: exclusive prefixes of both block-count arrays in place; counts[0] = V, counts[1] = T
__global__ void __launch_bounds__(MC_SCAN_THREADS) k_mc_scan(uint32_t* __restrict__ counts_v, uint32_t* __restrict__ counts_t, uint32_t nb,
                                                             int32_t* __restrict__ counts) {
    __shared__ uint32_t lds[MC_SCAN_THREADS / LAE_WAVE + 1];
    uint32_t* arr[2] = {counts_v, counts_t};
    for (int a = 0; a < 2; a++) {
        uint32_t carry = 0;
        for (uint32_t b0 = 0; b0 < nb; b0 += MC_SCAN_THREADS) {
            const uint32_t i = b0 + threadIdx.x;
            const uint32_t v = i < nb ? arr[a][i] : 0u;
            uint32_t total;
            const uint32_t ex = lae::block_excl_scan<MC_SCAN_THREADS / LAE_WAVE>(v, &total, lds);
            if (i < nb) arr[a][i] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) counts[a] = (int32_t)carry;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_vertices(const float* __restrict__ u, Dims d, float thr,
                                                            const uint32_t* __restrict__ offs_v, uint32_t* __restrict__ words,
                                                            float* __restrict__ verts) {
    __shared__ uint32_t lds[MC_THREADS / LAE_WAVE + 1];
    Window w;
    load_window<VEC>(u, d, w);
    uint32_t mask[MC_ITEMS];
    int cse[MC_ITEMS];
    const uint32_t c = thread_counts(w, d, thr, mask, cse);
    uint32_t total;
    uint32_t base = offs_v[blockIdx.x] + (lae::block_excl_scan<MC_THREADS / LAE_WAVE>(c, &total, lds) & 0xffffu);
    uint32_t i = w.i, j = w.j, k = w.k;
#pragma unroll
    for (int q = 0; q < MC_ITEMS; q++) {
        if (w.p0 + q < d.P) {
            words[w.p0 + q] = base | mask[q] << MC_BASE_BITS;
            const float a = w.v[0][q];
            const float nb3[3] = {w.v[2][q], w.v[1][q], w.v[0][q + 1]};
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                if (!((mask[q] >> ax) & 1u)) continue;
                // t = (thr - a) / (b - a) in fp32, non-finite -> 0.5, clamped to [0, 1]; position = lower corner + t along ax
                float t = __fdiv_rn(__fsub_rn(thr, a), __fsub_rn(nb3[ax], a));
                if (!__builtin_isfinite(t)) t = 0.5f;
                t = fminf(fmaxf(t, 0.0f), 1.0f);
                float pos[3] = {(float)i, (float)j, (float)k};
                pos[ax] = __fadd_rn(pos[ax], t);
                float* o = verts + 3 * (uint64_t)base;
                o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2];
                base++;
            }
        }
        next_point(i, j, k, d);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(MC_THREADS) k_mc_triangles(const float* __restrict__ u, Dims d, float thr,
                                                             const uint32_t* __restrict__ offs_t, const uint32_t* __restrict__ words,
                                                             int32_t* __restrict__ tris) {
    __shared__ uint32_t lds[MC_THREADS / LAE_WAVE + 1];
    Window w;
    load_window<VEC>(u, d, w);
    uint32_t mask[MC_ITEMS];
    int cse[MC_ITEMS];
    const uint32_t c = thread_counts(w, d, thr, mask, cse);
    uint32_t total;
    uint32_t slot = offs_t[blockIdx.x] + (lae::block_excl_scan<MC_THREADS / LAE_WAVE>(c, &total, lds) >> 16);
    for (int q = 0; q < MC_ITEMS; q++) {
        if (cse[q] < 0) continue;
        const uint32_t p = w.p0 + q;
        const int n = MC_TRI_COUNT[cse[q]];
        for (int s = 0; s < n; s++) {
            int32_t* o = tris + 3 * (uint64_t)slot;
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const int e = MC_TRI_EDGES[cse[q]][3 * s + v];
                const uint32_t cn = MC_EDGE_CORNER[e], ax = MC_EDGE_AXIS[e];
                const uint32_t wd = words[p + (cn & 1u) * d.nyz + ((cn >> 1) & 1u) * d.nz + (cn >> 2)];
                o[v] = (int32_t)((wd & MC_BASE_MASK) + __builtin_popcount((wd >> MC_BASE_BITS) & ((1u << ax) - 1u)));
            }
            slot++;
        }
    }
}

int check_dims(uint32_t nx, uint32_t ny, uint32_t nz, Dims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > 512 || ny > 512 || nz > 512) return LAE_EINVAL;
    d = Dims{nx, ny, nz, ny * nz, nx * ny * nz};
    return LAE_OK;
}

bool vec_ok(const float* u, const Dims& d) { return d.nz % 4 == 0 && (reinterpret_cast<uintptr_t>(u) & 15) == 0; }

}  // namespace

extern "C" {

uint64_t lae_marching_cubes_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    Dims d;
    if (check_dims(nx, ny, nz, d)) return 0;
    return words_offset(scratch_blocks(d.P)) + (uint64_t)4 * d.P;
}

int lae_marching_cubes_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* scratch, int32_t* counts,
                             void* stream) {
    Dims d;
    if (check_dims(nx, ny, nz, d)) return LAE_EINVAL;
    if (!u || !scratch || !counts) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nb = scratch_blocks(d.P);
    uint32_t* cv = static_cast<uint32_t*>(scratch);
    if (vec_ok(u, d)) k_mc_count<true><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv, cv + nb);
    else k_mc_count<false><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv, cv + nb);
    int rc = lae::check_launch("marching_cubes/count");
    if (rc) return rc;
    k_mc_scan<<<1, MC_SCAN_THREADS, 0, s>>>(cv, cv + nb, nb, counts);
    return lae::check_launch("marching_cubes/scan");
}

int lae_marching_cubes_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* scratch, float* verts,
                            int32_t* tris, void* stream) {
    Dims d;
    if (check_dims(nx, ny, nz, d)) return LAE_EINVAL;
    if (!u || !scratch || !verts || !tris) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nb = scratch_blocks(d.P);
    uint32_t* cv = static_cast<uint32_t*>(scratch);
    uint32_t* words = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + words_offset(nb));
    if (vec_ok(u, d)) k_mc_vertices<true><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv, words, verts);
    else k_mc_vertices<false><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv, words, verts);
    int rc = lae::check_launch("marching_cubes/vertices");
    if (rc) return rc;
    if (vec_ok(u, d)) k_mc_triangles<true><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv + nb, words, tris);
    else k_mc_triangles<false><<<nb, MC_THREADS, 0, s>>>(u, d, threshold, cv + nb, words, tris);
    return lae::check_launch("marching_cubes/triangles");
}

}  // extern "C"
