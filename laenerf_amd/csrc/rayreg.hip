// rayreg.hip -- ray registration of the single-reference-view stylization (Ref-NPR; the reference's
// editing/single_view_edit_dataset.py:317-349 get_ref_supervision and its caller :219-232).
//
// For every masked pixel of a training view: the nearest termination point of the reference view's cloud, the painted colour of that
// point when it is closer than reg_dist, a weight that falls with the distance and with opposing view directions, and the style guide.
// The reference takes th.linalg.norm(pred[z:z+1000, None] - ref).min(-1) in 1000-row chunks: n * M distances per view.  Every use of the
// distance is clamped at `radius` (0.1), and the cloud is the same for all views, so here the cloud is put into a UNIFORM CELL GRID once
// and a query is an exact TRUNCATED nearest-neighbour search over the 27 cells around it.
//
//   build     bounding box of the finite cloud points -> cell side s and cells per axis G (one thread, on the device: no host
//             round trip) -> points per cell -> exclusive scan -> scatter into a cell-sorted float4 copy (x, y, z, bits of the original
//             index).  The scatter advances the scanned table in place, which is afterwards the table of cell ENDS.
//   query     the view's queries are binned by cell the same way; a workgroup owns RR_QCH queries of ONE cell and streams that cell's
//             3 x 3 rows of neighbour cells (cells are x-fastest, so the three cells of a row are one contiguous range of the sorted
//             copy) through LDS in tiles, every lane holding RR_QPL queries in registers and every point read once per workgroup as a
//             broadcast -- the structure of k_min_dist (editgrid.hip), per cell.  The running minimum is the u64
//             (bits of the squared distance) << 32 | original index under an unsigned min: among equal distances the lowest original
//             index wins, whatever order the scatter's atomics left the points in.
//             mode LAE_RAYREG_GATHER: one lane per query walks the same nine ranges from global memory (the A/B predecessor).
//   supervise pass A: number of registered rows and the smallest / largest registered distance (integer atomics on the bits of the
//             non-negative floats); pass B: per row nn or -1, target colour, weight, guide.
//
// THE CELL COORDINATE.  Build and query use cell_t(): t = fl(fl(x - lo) * inv_s), cell = floor(t).  Every operation is monotone in
// x, so t is.  With s' = 1 / inv_s (the side the arithmetic really uses) and u = (x - lo) / s' exact, t = u (1 + e), |e| <= 2^-23
// (two roundings), i.e. |t - u| <= G 2^-23 for a grid of G cells on that axis.  Two points whose coordinates differ by at most r have
// u1 - u2 <= r / s', so t1 - t2 <= r / s' + G 2^-22, and their cells differ by at most ONE as long as that is below 1.  With exactly
// s = r it is not: one coordinate rounds up onto an integer while the other sits just under the previous one, and the cells are two
// apart.  So s >= r (1 + 2^-10) and G <= 1024 per axis: r / s' <= (1 + 2^-24) / (1 + 2^-10) < 1 - 2^-11 and G 2^-22 <= 2^-12.  (The
// fp32 distance test itself admits pairs up to r (1 + 2^-23) apart; the slack covers that too.)  The same bound says that a query whose
// t lies below -1 or at or above G + 1 has no point within r: such queries are answered without a search, all others are binned to
// the cell clamp(floor(t), 0, G - 1), whose 27 neighbours contain the 27 neighbours' points of the unclamped cell that lie in the grid.
#include <algorithm>
#include <cmath>

#include "lae_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr uint32_t RR_MAX_AXIS = 1024;           // cells per axis (the rounding bound above)
constexpr uint32_t RR_MAX_CELLS = 1u << 21;      // cells in all
constexpr uint32_t RR_MIN_CELLS = 64;
constexpr int RR_THREADS = 64, RR_QPL = 4, RR_TILE = 512;
constexpr uint32_t RR_QCH = RR_THREADS * RR_QPL; // queries per work item
constexpr int RR_SCAN_THREADS = 1024, RR_SCAN_PER = 4;
constexpr uint32_t RR_FAR = 0xffffffffu;
constexpr uint32_t RR_MAX_N = 1u << 30;

// the grid record at the head of the build's output (256 bytes reserved)
struct RayregGrid {
    float lo[3], s, inv_s;
    uint32_t G[3], ncells, cap, M;
    uint32_t box_lo[3], box_hi[3];               // ordered-integer images of the bounding box while it is being reduced
};
static_assert(sizeof(RayregGrid) <= 256, "grid record");
constexpr size_t RR_HDR = 256;

__host__ __device__ __forceinline__ uint32_t cell_cap(uint32_t M) {
    const uint64_t c = 4ull * M;
    return (uint32_t)(c < RR_MIN_CELLS ? RR_MIN_CELLS : (c > RR_MAX_CELLS ? RR_MAX_CELLS : c));
}
__host__ __device__ __forceinline__ size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// layout of the build's output: record | cell_end [cap + 1] | sorted float4 [M]
__host__ __device__ __forceinline__ size_t off_cells() { return RR_HDR; }
__host__ __device__ __forceinline__ size_t off_sorted(uint32_t M) { return RR_HDR + align256(4ull * (cell_cap(M) + 1)); }
// layout of the query workspace: qcell [n] | qsorted [n] | qend [cap + 1] | qchunk [cap + 1] | evals (u64)
__host__ __device__ __forceinline__ size_t qoff_sorted(uint32_t n) { return align256(4ull * n); }
__host__ __device__ __forceinline__ size_t qoff_end(uint32_t n) { return 2 * align256(4ull * n); }
__host__ __device__ __forceinline__ size_t qoff_chunk(uint32_t n, uint32_t M) { return qoff_end(n) + align256(4ull * (cell_cap(M) + 1)); }
__host__ __device__ __forceinline__ size_t qoff_evals(uint32_t n, uint32_t M) { return qoff_chunk(n, M) + align256(4ull * (cell_cap(M) + 1)); }

// floats as unsigned integers of the same order (negative: all bits flipped, others: sign bit set)
__device__ __forceinline__ uint32_t ord_of(float f) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_to(uint32_t o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// THE cell coordinate (see the header): build and query call this and nothing else
__device__ __forceinline__ float cell_t(float x, float lo, float inv_s) { return (x - lo) * inv_s; }
// a cloud point's cell on one axis: inside the box by construction, clamped against overflow only
__device__ __forceinline__ uint32_t cell_of_point(float x, float lo, float inv_s, uint32_t G) {
    const float t = fminf(fmaxf(floorf(cell_t(x, lo, inv_s)), 0.0f), (float)(G - 1));     // clamped in float, then converted
    return (uint32_t)t;
}
// a query's cell on one axis -> false when no cloud point can lie within the radius (also for NaN)
__device__ __forceinline__ bool cell_of_query(float x, float lo, float inv_s, uint32_t G, uint32_t* c) {
    const float t = cell_t(x, lo, inv_s);
    if (!(t >= -1.0f && t < (float)(G + 1))) return false;
    *c = (uint32_t)fminf(fmaxf(floorf(t), 0.0f), (float)(G - 1));
    return true;
}
__device__ __forceinline__ uint32_t range_start(const uint32_t* __restrict__ ends, uint32_t c) { return c ? ends[c - 1] : 0u; }

// ---------------------------------------------------------------------------------------------------------------- build
__global__ void k_rr_init(RayregGrid* g, uint32_t M) {
    if (threadIdx.x < 3) { g->box_lo[threadIdx.x] = 0xffffffffu; g->box_hi[threadIdx.x] = 0u; }
    if (threadIdx.x == 0) { g->M = M; g->cap = cell_cap(M); }
}

__global__ void __launch_bounds__(256) k_rr_bbox(const float* __restrict__ pts, uint32_t M, RayregGrid* g) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) continue;
        const uint32_t o[3] = {ord_of(x), ord_of(y), ord_of(z)};
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        for (int o = 32; o > 0; o >>= 1) { lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], o)); hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], o)); }
        if ((threadIdx.x & 63) == 0) { atomicMin(&g->box_lo[a], lo[a]); atomicMax(&g->box_hi[a], hi[a]); }
    }
}

// one thread: the cell side and the cells per axis.  G of an axis is cell_of(hi) + 1 with the shared cell coordinate, so that no
// point's cell reaches G; s grows by a quarter until every axis has at most RR_MAX_AXIS cells and the grid at most `cap`.
__global__ void k_rr_params(RayregGrid* g, float radius) {
    if (threadIdx.x || blockIdx.x) return;
    const bool any = g->box_lo[0] <= g->box_hi[0];
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = any ? ord_to(g->box_lo[a]) : 0.0f; hi[a] = any ? ord_to(g->box_hi[a]) : 0.0f; }
    float s = radius * (1.0f + 0x1p-10f);
    s = fmaxf(s, radius);                                         // never below the radius, whatever the product rounded to
    uint32_t G[3];
    float inv_s;
    for (int it = 0; it < 512; it++) {
        inv_s = 1.0f / s;
        bool ok = inv_s > 0.0f && 1.0f / inv_s >= radius * (1.0f + 0x1p-11f);        // s' = 1 / inv_s is the side the arithmetic uses
        uint64_t prod = 1;
        for (int a = 0; a < 3; a++) {
            const float t = floorf(cell_t(hi[a], lo[a], inv_s));
            if (!(t < (float)RR_MAX_AXIS)) { ok = false; G[a] = RR_MAX_AXIS; } else G[a] = (uint32_t)fmaxf(t, 0.0f) + 1u;
            prod *= G[a];
        }
        if (ok && prod <= g->cap) break;
        s *= 1.25f;
        if (!isfinite(s)) { s = 0x1p127f; inv_s = 1.0f / s; G[0] = G[1] = G[2] = 1; break; }   // a cloud as wide as fp32: one cell
    }
    for (int a = 0; a < 3; a++) { g->lo[a] = lo[a]; g->G[a] = G[a]; }
    g->s = s; g->inv_s = inv_s;
    g->ncells = G[0] * G[1] * G[2];
}

__global__ void __launch_bounds__(256) k_rr_zero(const RayregGrid* __restrict__ g, uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
    const uint32_t n = g->ncells + 1;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { a[i] = 0; if (b) b[i] = 0; }
}

__device__ __forceinline__ uint32_t point_cell(const RayregGrid* __restrict__ g, float x, float y, float z) {
    const uint32_t cx = cell_of_point(x, g->lo[0], g->inv_s, g->G[0]), cy = cell_of_point(y, g->lo[1], g->inv_s, g->G[1]),
                   cz = cell_of_point(z, g->lo[2], g->inv_s, g->G[2]);
    return (cz * g->G[1] + cy) * g->G[0] + cx;
}

// SCATTER = false: count the finite points per cell; true: place them (cursor = the scanned counts, left as the cells' ends)
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_rr_points(const float* __restrict__ pts, uint32_t M, const RayregGrid* __restrict__ g,
                                                   uint32_t* __restrict__ cells, float4* __restrict__ sorted) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (!finite3(x, y, z)) continue;
        const uint32_t c = point_cell(g, x, y, z);
        const uint32_t at = atomicAdd(cells + c, 1u);
        if (SCATTER) { if (at < M) sorted[at] = make_float4(x, y, z, __builtin_bit_cast(float, i)); }
    }
}

// one workgroup: in-place exclusive scan of counts[0 .. ncells) (counts[ncells] = the total); with `chunks` also the exclusive scan
// of ceil(count / per_chunk) (the work items of the binned query)
__global__ void __launch_bounds__(RR_SCAN_THREADS) k_rr_scan(const RayregGrid* __restrict__ g, uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ chunks, uint32_t per_chunk) {
    __shared__ uint32_t lds[RR_SCAN_THREADS / 64 + 1];
    const uint32_t n = g->ncells;
    uint32_t run = 0, run_c = 0;
    for (uint32_t base = 0; base < n; base += RR_SCAN_THREADS * RR_SCAN_PER) {
        const uint32_t i0 = base + threadIdx.x * RR_SCAN_PER;
        uint32_t v[RR_SCAN_PER], w[RR_SCAN_PER], sv = 0, sw = 0;
#pragma unroll
        for (int k = 0; k < RR_SCAN_PER; k++) {
            v[k] = i0 + k < n ? counts[i0 + k] : 0u;
            w[k] = (v[k] + per_chunk - 1) / per_chunk;
            sv += v[k]; sw += w[k];
        }
        uint32_t tot, tot_c = 0;
        uint32_t ex = run + lae::block_excl_scan<RR_SCAN_THREADS / 64>(sv, &tot, lds);
        uint32_t ex_c = 0;
        if (chunks) ex_c = run_c + lae::block_excl_scan<RR_SCAN_THREADS / 64>(sw, &tot_c, lds);
#pragma unroll
        for (int k = 0; k < RR_SCAN_PER; k++) {
            if (i0 + k < n) { counts[i0 + k] = ex; if (chunks) chunks[i0 + k] = ex_c; }
            ex += v[k]; ex_c += w[k];
        }
        run += tot; run_c += tot_c;
    }
    if (threadIdx.x == 0) { counts[n] = run; if (chunks) chunks[n] = run_c; }
}

// ---------------------------------------------------------------------------------------------------------------- query
__device__ __forceinline__ void store_result(unsigned long long key, float radius, float* __restrict__ d_out, int32_t* __restrict__ nn_out, uint32_t i) {
    const float d = sqrtf(__builtin_bit_cast(float, (uint32_t)(key >> 32)));
    const bool hit = key != ~0ull && d < radius;
    d_out[i] = hit ? d : radius;
    nn_out[i] = hit ? (int32_t)(uint32_t)key : -1;
}

// per query its bin (RR_FAR: answered here); COUNT: also counted per cell
template <bool COUNT>
__global__ void __launch_bounds__(256) k_rr_qcell(const float* __restrict__ x, uint32_t n, const RayregGrid* __restrict__ g, float radius,
                                                  uint32_t* __restrict__ qcell, uint32_t* __restrict__ qcount, float* __restrict__ d_out,
                                                  int32_t* __restrict__ nn_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float px = x[3 * (size_t)i], py = x[3 * (size_t)i + 1], pz = x[3 * (size_t)i + 2];
    uint32_t cx, cy, cz;
    const bool near = g->M && finite3(px, py, pz) && cell_of_query(px, g->lo[0], g->inv_s, g->G[0], &cx) &&
                      cell_of_query(py, g->lo[1], g->inv_s, g->G[1], &cy) && cell_of_query(pz, g->lo[2], g->inv_s, g->G[2], &cz);
    if (!near) { qcell[i] = RR_FAR; d_out[i] = radius; nn_out[i] = -1; return; }
    const uint32_t c = (cz * g->G[1] + cy) * g->G[0] + cx;
    qcell[i] = c;
    if (COUNT) atomicAdd(qcount + c, 1u);
}

__global__ void __launch_bounds__(256) k_rr_qscatter(const uint32_t* __restrict__ qcell, uint32_t n, uint32_t* __restrict__ qcursor,
                                                     uint32_t* __restrict__ qsorted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = qcell[i];
    if (c == RR_FAR) return;
    const uint32_t at = atomicAdd(qcursor + c, 1u);
    if (at < n) qsorted[at] = i;
}

// the nine contiguous point ranges around cell (cx, cy, cz): row r = 3 * (dz + 1) + (dy + 1) -> false when the row is outside
__device__ __forceinline__ bool neighbour_row(const RayregGrid* __restrict__ g, const uint32_t* __restrict__ cell_end, uint32_t cx, uint32_t cy,
                                              uint32_t cz, int r, uint32_t* ps, uint32_t* pe) {
    const int y = (int)cy + r % 3 - 1, z = (int)cz + r / 3 - 1;
    if (y < 0 || z < 0 || y >= (int)g->G[1] || z >= (int)g->G[2]) return false;
    const uint32_t row = ((uint32_t)z * g->G[1] + (uint32_t)y) * g->G[0];
    const uint32_t x0 = cx ? cx - 1 : 0u, x1 = min(cx + 1, g->G[0] - 1);
    *ps = range_start(cell_end, row + x0);
    *pe = cell_end[row + x1];
    return *pe > *ps;
}

// a work item = up to RR_QCH queries of one cell (item -> cell by bisection of the scanned chunk counts)
__global__ void __launch_bounds__(RR_THREADS) k_rr_match(const RayregGrid* __restrict__ g, const uint32_t* __restrict__ cell_end,
                                                         const float4* __restrict__ sorted, const uint32_t* __restrict__ qend,
                                                         const uint32_t* __restrict__ qchunk, const uint32_t* __restrict__ qsorted,
                                                         const float* __restrict__ x, uint32_t n, float radius, float* __restrict__ d_out,
                                                         int32_t* __restrict__ nn_out, unsigned long long* __restrict__ evals) {
    __shared__ float4 tile[RR_TILE];
    const uint32_t ncells = g->ncells, total = qchunk[ncells], M = g->M;
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x) {
        uint32_t lo = 0, hi = ncells;                                   // qchunk[lo] <= item < qchunk[hi]
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (qchunk[mid] <= item) lo = mid; else hi = mid; }
        const uint32_t c = lo;
        const uint32_t qs = min(range_start(qend, c) + (item - qchunk[c]) * RR_QCH, n), qe = min(min(qend[c], qs + RR_QCH), n);
        if (qe <= qs) continue;                                         // (uniform) cannot happen with consistent tables
        const uint32_t cx = c % g->G[0], cy = (c / g->G[0]) % g->G[1], cz = c / (g->G[0] * g->G[1]);
        float px[RR_QPL], py[RR_QPL], pz[RR_QPL];
        unsigned long long best[RR_QPL];
        uint32_t qi[RR_QPL];
#pragma unroll
        for (int k = 0; k < RR_QPL; k++) {
            const uint32_t slot = qs + threadIdx.x + k * RR_THREADS;
            qi[k] = slot < qe ? min(qsorted[slot], n - 1u) : RR_FAR;
            const uint32_t q = slot < qe ? qi[k] : min(qsorted[qs], n - 1u);
            px[k] = x[3 * (size_t)q]; py[k] = x[3 * (size_t)q + 1]; pz[k] = x[3 * (size_t)q + 2];
            best[k] = ~0ull;
        }
        unsigned long long seen = 0;
        for (int r = 0; r < 9; r++) {
            uint32_t ps, pe;
            if (!neighbour_row(g, cell_end, cx, cy, cz, r, &ps, &pe)) continue;
            pe = min(pe, M);
            for (uint32_t t0 = ps; t0 < pe; t0 += RR_TILE) {
                const uint32_t cnt = min((uint32_t)RR_TILE, pe - t0);
                __syncthreads();
                for (uint32_t i = threadIdx.x; i < cnt; i += RR_THREADS) tile[i] = sorted[t0 + i];
                __syncthreads();
#pragma unroll 4
                for (uint32_t i = 0; i < cnt; i++) {
                    const float4 s = tile[i];
                    const uint32_t idx = __builtin_bit_cast(uint32_t, s.w);
#pragma unroll
                    for (int k = 0; k < RR_QPL; k++) {
                        const float dx = px[k] - s.x, dy = py[k] - s.y, dz = pz[k] - s.z;
                        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                        const unsigned long long key = ((unsigned long long)__builtin_bit_cast(uint32_t, d2) << 32) | idx;
                        best[k] = key < best[k] ? key : best[k];
                    }
                }
                seen += cnt;
            }
        }
#pragma unroll
        for (int k = 0; k < RR_QPL; k++)
            if (qi[k] != RR_FAR) store_result(best[k], radius, d_out, nn_out, qi[k]);
        if (threadIdx.x == 0 && evals) atomicAdd(evals, seen * (qe - qs));
    }
}

// the A/B predecessor: a lane per query, the nine ranges read from global memory
__global__ void __launch_bounds__(256) k_rr_gather(const RayregGrid* __restrict__ g, const uint32_t* __restrict__ cell_end,
                                                   const float4* __restrict__ sorted, const uint32_t* __restrict__ qcell,
                                                   const float* __restrict__ x, uint32_t n, float radius, float* __restrict__ d_out,
                                                   int32_t* __restrict__ nn_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = qcell[i];
    if (c == RR_FAR) return;
    const uint32_t cx = c % g->G[0], cy = (c / g->G[0]) % g->G[1], cz = c / (g->G[0] * g->G[1]);
    const float px = x[3 * (size_t)i], py = x[3 * (size_t)i + 1], pz = x[3 * (size_t)i + 2];
    unsigned long long best = ~0ull;
    for (int r = 0; r < 9; r++) {
        uint32_t ps, pe;
        if (!neighbour_row(g, cell_end, cx, cy, cz, r, &ps, &pe)) continue;
        pe = min(pe, g->M);
        for (uint32_t j = ps; j < pe; j++) {
            const float4 s = sorted[j];
            const float dx = px - s.x, dy = py - s.y, dz = pz - s.z;
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            const unsigned long long key = ((unsigned long long)__builtin_bit_cast(uint32_t, d2) << 32) | __builtin_bit_cast(uint32_t, s.w);
            best = key < best ? key : best;
        }
    }
    store_result(best, radius, d_out, nn_out, i);
}

// ------------------------------------------------------------------------------------------------------------ supervise
// stats: [0] R, [1] bits of dmin (+inf when R == 0), [2] bits of dmax, [3] reserved
__global__ void k_rr_stats_init(uint32_t* stats) {
    if (threadIdx.x == 0) { stats[0] = 0; stats[1] = 0x7f800000u; stats[2] = 0; stats[3] = 0; }
}

__device__ __forceinline__ bool registered(float d, int32_t nn, uint32_t M, float reg_dist) { return nn >= 0 && (uint32_t)nn < M && d < reg_dist; }

__global__ void __launch_bounds__(256) k_rr_stats(const float* __restrict__ d, const int32_t* __restrict__ nn, uint32_t n, uint32_t M,
                                                  float reg_dist, uint32_t* __restrict__ stats) {
    uint32_t cnt = 0, lo = 0x7f800000u, hi = 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float di = d[i];
        if (!registered(di, nn[i], M, reg_dist)) continue;
        const uint32_t b = __builtin_bit_cast(uint32_t, fmaxf(di, 0.0f));      // non-negative floats order like their bits
        cnt++; lo = min(lo, b); hi = max(hi, b);
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (uint32_t)__shfl_xor((int)cnt, o); lo = min(lo, (uint32_t)__shfl_xor((int)lo, o)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
    if ((threadIdx.x & 63) == 0 && cnt) { atomicAdd(stats, cnt); atomicMin(stats + 1, lo); atomicMax(stats + 2, hi); }
}

// per row; the arithmetic after the fp32 inputs is fp64 and rounded once (a few rows' worth of work against the search)
__global__ void __launch_bounds__(256) k_rr_rows(const float* __restrict__ d, const int32_t* __restrict__ nn, uint32_t n,
                                                 const float* __restrict__ ref_rgb, const float* __restrict__ ref_dirs, uint32_t M,
                                                 const float* __restrict__ dirs, float reg_dist, float radius, float guide_min, float min_tv,
                                                 const uint32_t* __restrict__ stats, int32_t* __restrict__ nn_reg, float* __restrict__ target,
                                                 float* __restrict__ weight, float* __restrict__ guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float di = d[i];
    const int32_t j = nn[i];
    const bool reg = registered(di, j, M, reg_dist);
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, w = 0.0f;
    if (reg) {
        t0 = ref_rgb[3 * (size_t)j]; t1 = ref_rgb[3 * (size_t)j + 1]; t2 = ref_rgb[3 * (size_t)j + 2];
        const double ax = ref_dirs[3 * (size_t)j], ay = ref_dirs[3 * (size_t)j + 1], az = ref_dirs[3 * (size_t)j + 2];
        const double bx = dirs[3 * (size_t)i], by = dirs[3 * (size_t)i + 1], bz = dirs[3 * (size_t)i + 2];
        const double na = sqrt(ax * ax + ay * ay + az * az), nb = sqrt(bx * bx + by * by + bz * bz);
        const double cs = (ax * bx + ay * by + az * bz) / (fmax(na, 1e-8) * fmax(nb, 1e-8));     // F.cosine_similarity, eps 1e-8
        const double f = (fmin(fmax(cs, -1.0), -0.5) + 1.0) / 0.5;
        const double dmin = __builtin_bit_cast(float, stats[1]), dmax = __builtin_bit_cast(float, stats[2]);
        const double u = dmax > dmin ? ((double)fmaxf(di, 0.0f) - dmin) / (dmax - dmin) : 0.0;    // dmax == dmin: 0, not the reference's 0/0
        w = (float)(fabs(u - 1.0) * f);
    }
    nn_reg[i] = reg ? j : -1;
    target[3 * (size_t)i] = t0; target[3 * (size_t)i + 1] = t1; target[3 * (size_t)i + 2] = t2;
    weight[i] = w;
    const double gm = guide_min, r = radius;
    const double gd = (fmin(fmax((double)di, gm), r) - gm) / (r - gm);
    guide[i] = (float)fmax((double)min_tv, gd);
}

bool bad_radius(float r) { return !(r > 0.0f) || !std::isfinite(r); }

}  // namespace

extern "C" {

uint64_t lae_rayreg_build_bytes(uint32_t M) { return off_sorted(M) + 16ull * std::max(M, 1u); }

uint64_t lae_rayreg_query_bytes(uint32_t n, uint32_t M) { return qoff_evals(n, M) + 256; }

int lae_rayreg_build(const float* ref_x, uint32_t M, float radius, void* grid, void* stream) {
    if (bad_radius(radius) || M > RR_MAX_N) return LAE_EINVAL;
    if (!grid || (M && !ref_x)) return LAE_ENULL;
    if ((uintptr_t)grid & 15) return LAE_EINVAL;
    hipStream_t s = STREAM(stream);
    RayregGrid* g = reinterpret_cast<RayregGrid*>(grid);
    uint32_t* cells = reinterpret_cast<uint32_t*>((char*)grid + off_cells());
    float4* sorted = reinterpret_cast<float4*>((char*)grid + off_sorted(M));
    const uint32_t blocks = std::max(1u, std::min(lae::cdiv(M, 256u), 2048u));
    k_rr_init<<<1, 64, 0, s>>>(g, M);
    if (M) k_rr_bbox<<<blocks, 256, 0, s>>>(ref_x, M, g);
    k_rr_params<<<1, 64, 0, s>>>(g, radius);
    k_rr_zero<<<std::min(lae::cdiv(cell_cap(M) + 1, 256u), 1024u), 256, 0, s>>>(g, cells, nullptr);
    if (M) k_rr_points<false><<<blocks, 256, 0, s>>>(ref_x, M, g, cells, sorted);
    k_rr_scan<<<1, RR_SCAN_THREADS, 0, s>>>(g, cells, nullptr, 1u);
    if (M) k_rr_points<true><<<blocks, 256, 0, s>>>(ref_x, M, g, cells, sorted);
    return lae::check_launch("rayreg_build");
}

int lae_rayreg_query(const void* grid, uint32_t M, const float* x, uint32_t n, float radius, int mode, float* d, int32_t* nn,
                     void* workspace, void* stream) {
    if (bad_radius(radius) || M > RR_MAX_N || n > RR_MAX_N || (mode != LAE_RAYREG_BINNED && mode != LAE_RAYREG_GATHER)) return LAE_EINVAL;
    if (n == 0) return LAE_OK;
    if (!grid || !x || !d || !nn || !workspace) return LAE_ENULL;
    if (((uintptr_t)grid | (uintptr_t)workspace) & 15) return LAE_EINVAL;
    hipStream_t s = STREAM(stream);
    const RayregGrid* g = reinterpret_cast<const RayregGrid*>(grid);
    const uint32_t* cell_end = reinterpret_cast<const uint32_t*>((const char*)grid + off_cells());
    const float4* sorted = reinterpret_cast<const float4*>((const char*)grid + off_sorted(M));
    char* ws = reinterpret_cast<char*>(workspace);
    uint32_t* qcell = reinterpret_cast<uint32_t*>(ws);
    uint32_t* qsorted = reinterpret_cast<uint32_t*>(ws + qoff_sorted(n));
    uint32_t* qend = reinterpret_cast<uint32_t*>(ws + qoff_end(n));
    uint32_t* qchunk = reinterpret_cast<uint32_t*>(ws + qoff_chunk(n, M));
    unsigned long long* evals = reinterpret_cast<unsigned long long*>(ws + qoff_evals(n, M));
    const uint32_t rows = lae::cdiv(n, 256u);
    if (mode == LAE_RAYREG_GATHER) {
        k_rr_qcell<false><<<rows, 256, 0, s>>>(x, n, g, radius, qcell, nullptr, d, nn);
        k_rr_gather<<<rows, 256, 0, s>>>(g, cell_end, sorted, qcell, x, n, radius, d, nn);
        return lae::check_launch("rayreg_query");
    }
    if (hipMemsetAsync(evals, 0, 8, s) != hipSuccess) return LAE_ELAUNCH;
    k_rr_zero<<<std::min(lae::cdiv(cell_cap(M) + 1, 256u), 1024u), 256, 0, s>>>(g, qend, qchunk);
    k_rr_qcell<true><<<rows, 256, 0, s>>>(x, n, g, radius, qcell, qend, d, nn);
    k_rr_scan<<<1, RR_SCAN_THREADS, 0, s>>>(g, qend, qchunk, RR_QCH);
    k_rr_qscatter<<<rows, 256, 0, s>>>(qcell, n, qend, qsorted);
    // at most one partly filled item per occupied cell on top of the full ones
    const uint64_t items = (uint64_t)n / RR_QCH + std::min<uint64_t>(n, cell_cap(M));
    k_rr_match<<<(uint32_t)std::min<uint64_t>(items, 8192), RR_THREADS, 0, s>>>(g, cell_end, sorted, qend, qchunk, qsorted, x, n, radius, d, nn, evals);
    return lae::check_launch("rayreg_query");
}

int lae_rayreg_supervise(const float* d, const int32_t* nn, uint32_t n, const float* ref_rgb, const float* ref_dirs, uint32_t M,
                         const float* dirs, float reg_dist, float radius, float guide_min, float min_tv_factor, int32_t* nn_reg,
                         float* target, float* weight, float* guide, uint32_t* stats, void* stream) {
    if (bad_radius(radius) || !(reg_dist > 0.0f) || !(reg_dist <= radius) || !(guide_min < radius) || !std::isfinite(guide_min) ||
        !std::isfinite(min_tv_factor) || M > RR_MAX_N || n > RR_MAX_N)
        return LAE_EINVAL;
    if (n == 0) return LAE_OK;
    if (!d || !nn || !dirs || !nn_reg || !target || !weight || !guide || !stats || (M && (!ref_rgb || !ref_dirs))) return LAE_ENULL;
    hipStream_t s = STREAM(stream);
    k_rr_stats_init<<<1, 64, 0, s>>>(stats);
    k_rr_stats<<<std::min(lae::cdiv(n, 256u), 1024u), 256, 0, s>>>(d, nn, n, M, reg_dist, stats);
    k_rr_rows<<<lae::cdiv(n, 256u), 256, 0, s>>>(d, nn, n, ref_rgb, ref_dirs, M, dirs, reg_dist, radius, guide_min, min_tv_factor, stats, nn_reg,
                                                target, weight, guide);
    return lae::check_launch("rayreg_supervise");
}

}  // extern "C"
