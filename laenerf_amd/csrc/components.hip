// components.hip -- connected components (6-connectivity) of the inside set {u > threshold} of a dense fp32 lattice, on the
// device: the pass between the density sweep and marching cubes that drops floaters (laenerf_amd/components.py).  The result
// is canonical (include/laenerf.h, lae_components_*): a point's label is the smallest linear index of its component, so the
// schedule cannot change a bit of it.
//
// label: union-find over `labels` itself (labels[p] is p's parent; a root is its own parent; -1 outside), always linking the
// larger index under the smaller, so a tree's root is its smallest member.
//   tile:    one workgroup per CC_TX x CC_TY x CC_TZ tile, z along the lanes: a wave reads one 256-byte row per instruction.
//            The row's ballot gives every point the start of its z run (no union along z inside a tile); runs are joined
//            across y and x by a lock-free union-find in LDS; labels[p] = the global index of the tile-local root.
//   merge:   one thread per lattice point on a low tile face: union(p, the point across the face) with atomicMin on the
//            larger root; a lost race is retried from the value the atomic returned.  Every step lowers an index: no wave
//            ever waits for another.  Every access to `labels` in this kernel and in the next is an agent-scope atomic
//            (other workgroups write what it reads; a CU's L1 is not refreshed by them).
//   flatten: labels[p] = find(labels[p]).
// sizes: zero fill, counts (one add per label a workgroup's waves end with, not one per point), then the statistics (the largest
// component by one 64-bit max of size << 32 | ~root per workgroup): integer atomics only, exact.
// filter: out = u, except threshold at the inside points of components that are not kept.
#include "lae_common.h"

namespace {

constexpr int CC_TX = 4, CC_TY = 4, CC_TZ = 64;          // CC_TZ = one wave: a row's inside mask is one ballot
constexpr int CC_ROWS = CC_TX * CC_TY;
constexpr int CC_THREADS = CC_TY * CC_TZ;                // wave w owns the rows with ly = w; pass q is lx = q
constexpr uint32_t CC_OUTSIDE = 0xffffffffu;
constexpr int CC_POINT_THREADS = 256;
constexpr uint64_t CC_MAX_POINTS = (uint64_t)512 * 512 * 512;
static_assert(CC_TZ == LAE_WAVE && CC_THREADS == 256, "one wave per row");

struct Dims {
    uint32_t nx, ny, nz, nyz, P;
    uint32_t ty, tz;                                     // tiles along y and z
};

__device__ __forceinline__ uint32_t ld_u32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld_lds(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- union-find in a tile's LDS image (lab[l] <= l; CC_OUTSIDE at outside points, which are never passed in)
__device__ __forceinline__ uint32_t lds_find(const uint32_t* lab, uint32_t x) {
    for (uint32_t p; (p = ld_lds(lab + x)) != x;) x = p;
    return x;
}
__device__ __forceinline__ void lds_unite(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {
        a = lds_find(lab, a); b = lds_find(lab, b);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicMin(lab + hi, lo);
        if (old == hi) return;                           // hi was a root and now hangs under lo
        a = old; b = lo;                                 // hi had been linked meanwhile (old < hi): join its parent and lo instead
    }
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_tile(const float* __restrict__ u, Dims d, float thr, int32_t* __restrict__ labels) {
    __shared__ uint32_t lab[CC_ROWS * CC_TZ];
    __shared__ uint64_t rowmask[CC_ROWS];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t t = blockIdx.x;
    const uint32_t tk = t % d.tz; t /= d.tz;
    const uint32_t tj = t % d.ty, ti = t / d.ty;
    const uint32_t i0 = ti * CC_TX, j0 = tj * CC_TY, k0 = tk * CC_TZ;
    const uint32_t j = j0 + w, k = k0 + lane;
    const bool col = j < d.ny && k < d.nz;
    bool in[CC_TX];
    uint64_t mask[CC_TX];
#pragma unroll
    for (int q = 0; q < CC_TX; q++) {
        const uint32_t i = i0 + q, row = q * CC_TY + w;
        in[q] = false;
        if (col && i < d.nx) in[q] = u[(i * d.ny + j) * d.nz + k] > thr;      // strictly above: NaN is outside
        mask[q] = __ballot(in[q]);
        const uint64_t below = ~mask[q] & ((1ull << lane) - 1ull);            // outside points of the row before this one
        const uint32_t start = below ? 64u - (uint32_t)__clzll((long long)below) : 0u;
        lab[row * CC_TZ + lane] = in[q] ? row * CC_TZ + start : CC_OUTSIDE;
        if (lane == 0) rowmask[row] = mask[q];
    }
    __syncthreads();
    // join the z runs across y and x.  A pair whose z predecessors are both inside too is skipped: that pair makes the same join.
#pragma unroll
    for (int q = 0; q < CC_TX; q++) {
        if (!in[q]) continue;
        const uint32_t row = q * CC_TY + w, l = row * CC_TZ + lane;
        const bool prev = lane > 0 && ((mask[q] >> (lane - 1)) & 1ull);
        if (w > 0) {
            const uint64_t mo = rowmask[row - 1];
            if (((mo >> lane) & 1ull) && !(prev && ((mo >> (lane - 1)) & 1ull))) lds_unite(lab, l, l - CC_TZ);
        }
        if (q > 0) {
            const uint64_t mo = rowmask[row - CC_TY];
            if (((mo >> lane) & 1ull) && !(prev && ((mo >> (lane - 1)) & 1ull))) lds_unite(lab, l, l - CC_TY * CC_TZ);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CC_TX; q++) {
        const uint32_t i = i0 + q;
        if (!col || i >= d.nx) continue;
        int32_t out = -1;
        if (in[q]) {
            const uint32_t r = lds_find(lab, (q * CC_TY + w) * CC_TZ + lane);
            const uint32_t rr = r / CC_TZ;                // local order (lx, ly, lz) is the global order: the local root is the
            out = (int32_t)(((i0 + rr / CC_TY) * d.ny + j0 + rr % CC_TY) * d.nz + k0 + r % CC_TZ);   // smallest global index too
        }
        labels[(i * d.ny + j) * d.nz + k] = out;
    }
}

// ---- union-find in global memory: every access an agent-scope atomic
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    uint32_t p = ld_u32(parent + x);
    while (p != x) {
        const uint32_t g = ld_u32(parent + p);
        if (g != p) atomicMin(parent + x, g);            // path halving: g is an ancestor of x below p
        x = p; p = g;
    }
    return x;
}
__device__ __forceinline__ void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a); b = cc_find(parent, b);
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old; b = lo;
    }
}
__device__ __forceinline__ bool cc_inside(const uint32_t* parent, uint32_t p) { return (int32_t)ld_u32(parent + p) >= 0; }

// the pair (p, p - step) across a low tile face; (p - 1, p - 1 - step) makes the same join when both are inside and p - 1 is in
// p's tile (`same`: the caller's statement that it is)
__device__ __forceinline__ void cc_face(uint32_t* parent, uint32_t p, uint32_t mine, uint32_t step, uint32_t other_step, bool same) {
    const uint32_t o = ld_u32(parent + p - step);
    if ((int32_t)o < 0) return;
    if (same && cc_inside(parent, p - other_step) && cc_inside(parent, p - other_step - step)) return;
    cc_unite(parent, mine, o);
}

__global__ void __launch_bounds__(CC_POINT_THREADS) k_cc_merge(uint32_t* __restrict__ parent, Dims d) {
    const uint32_t p = blockIdx.x * CC_POINT_THREADS + threadIdx.x;
    if (p >= d.P) return;
    const uint32_t i = p / d.nyz, rem = p - i * d.nyz, j = rem / d.nz, k = rem - j * d.nz;
    const bool fx = i > 0 && i % CC_TX == 0, fy = j > 0 && j % CC_TY == 0, fz = k > 0 && k % CC_TZ == 0;
    if (!fx && !fy && !fz) return;
    const uint32_t mine = ld_u32(parent + p);
    if ((int32_t)mine < 0) return;
    if (fx) cc_face(parent, p, mine, d.nyz, 1u, k % CC_TZ != 0);
    if (fy) cc_face(parent, p, mine, d.nz, 1u, k % CC_TZ != 0);
    if (fz) cc_face(parent, p, mine, 1u, d.nz, j % CC_TY != 0);
}

__global__ void __launch_bounds__(CC_POINT_THREADS) k_cc_flatten(uint32_t* __restrict__ parent, uint32_t P) {
    const uint32_t p = blockIdx.x * CC_POINT_THREADS + threadIdx.x;
    if (p >= P) return;
    const uint32_t v = ld_u32(parent + p);
    if ((int32_t)v < 0) return;
    const uint32_t r = cc_find(parent, v);
    if (r != v) st_u32(parent + p, r);                   // r is the smallest value parent[p] can take: a racing atomicMin keeps it
}

// ---- sizes
constexpr int CS_THREADS = 1024;                         // count pass: 16 waves share one add per label they all end with
constexpr int CS_WAVES = CS_THREADS / LAE_WAVE;
constexpr uint32_t CS_ITERS = 64;
constexpr uint32_t CS_BATCH = 16;                        // loads in flight per lane of the count pass
static_assert(CS_ITERS % CS_BATCH == 0, "whole batches");
constexpr uint32_t CS_WAVE_POINTS = LAE_WAVE * CS_ITERS;
constexpr uint32_t CS_BLOCK_POINTS = CS_WAVES * CS_WAVE_POINTS;
constexpr int ST_THREADS = 256;
constexpr int ST_WAVES = ST_THREADS / LAE_WAVE;
constexpr uint32_t ST_ITEMS = 64;                        // sizes entries per thread of the statistics pass

// While the statistics pass runs, stats[0..1] hold one 64-bit key, size << 32 | (0x7fffffff - root): its maximum is the largest
// component, the lowest root among equals; stats[2] counts roots and stats[3] points.  k_cc_finish puts them in their places.
__global__ void __launch_bounds__(ST_THREADS) k_cc_zero(int32_t* __restrict__ sizes, uint32_t N, int32_t* __restrict__ stats) {
    const uint32_t p = blockIdx.x * ST_THREADS + threadIdx.x;
    if (p < N) sizes[p] = 0;
    if (p < 4) stats[p] = 0;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, s);
        v = max(v, o);
    }
    return v;
}

// A wave walks CS_WAVE_POINTS consecutive points, 64 at a time.  A lane keeps two (label, count) pairs, the two labels it met
// last, and adds a pair to sizes only when a third label pushes it out: outside points end nothing, and a lane that alternates
// between a solid and a floater next to it keeps both.  What the lanes hold at the end is summed per distinct label over the
// wave, and the wave's largest sum over the workgroup's waves through LDS: a solid costs one add per workgroup that meets it,
// not one per point -- millions of adds to one address are the slowest access there is.
__global__ void __launch_bounds__(CS_THREADS) k_cc_count(const int32_t* __restrict__ labels, uint32_t N, int32_t* __restrict__ sizes) {
    __shared__ int32_t s_lab[CS_WAVES];
    __shared__ uint32_t s_cnt[CS_WAVES];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * CS_BLOCK_POINTS + w * CS_WAVE_POINTS + lane;     // < 2^27 + CS_BLOCK_POINTS
    int32_t c0 = -1, c1 = -1;                            // c0: the label met last
    uint32_t n0 = 0, n1 = 0;
    for (uint32_t it0 = 0; it0 < CS_ITERS; it0 += CS_BATCH) {
        int32_t l[CS_BATCH];                             // the loads of a batch are issued before the first label is looked at
#pragma unroll
        for (uint32_t q = 0; q < CS_BATCH; q++) {
            const uint32_t p = base + (it0 + q) * LAE_WAVE;
            l[q] = p < N ? labels[p] : -1;
        }
#pragma unroll
        for (uint32_t q = 0; q < CS_BATCH; q++) {
            if ((uint32_t)l[q] >= N) continue;           // outside, or not a label: never an index into sizes
            if (l[q] == c0) {
                n0++;
            } else {
                if (l[q] != c1) {
                    if (c1 >= 0) atomicAdd(sizes + c1, (int32_t)n1);
                    c1 = l[q]; n1 = 0;
                }
                const int32_t c = c0; c0 = c1; c1 = c;
                const uint32_t n = n0; n0 = n1 + 1u; n1 = n;
            }
        }
    }
    int32_t lead = -1;                                   // wave-uniform: the label with the wave's largest sum so far
    uint32_t lead_cnt = 0;
    bool done0 = c0 < 0, done1 = c1 < 0;
    for (;;) {
        const uint64_t t0 = __ballot(!done0), t1 = __ballot(!done1);
        if (!(t0 | t1)) break;
        const int32_t lab = t0 ? __shfl(c0, __builtin_ctzll(t0)) : __shfl(c1, __builtin_ctzll(t1));
        const bool m0 = !done0 && c0 == lab, m1 = !done1 && c1 == lab;
        const uint32_t sum = wave_sum((m0 ? n0 : 0u) + (m1 ? n1 : 0u));
        int32_t add = lab;
        uint32_t add_cnt = sum;
        if (sum > lead_cnt) { add = lead; add_cnt = lead_cnt; lead = lab; lead_cnt = sum; }
        if (lane == 0 && add >= 0) atomicAdd(sizes + add, (int32_t)add_cnt);
        done0 |= m0; done1 |= m1;
    }
    if (lane == 0) { s_lab[w] = lead; s_cnt[w] = lead_cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int a = 0; a < CS_WAVES; a++) {
            if (s_lab[a] < 0) continue;
            uint32_t c = s_cnt[a];
            for (int b = a + 1; b < CS_WAVES; b++)
                if (s_lab[b] == s_lab[a]) { c += s_cnt[b]; s_lab[b] = -1; }
            atomicAdd(sizes + s_lab[a], (int32_t)c);
        }
    }
}

// per workgroup that holds a root: one 64-bit max and two adds
__global__ void __launch_bounds__(ST_THREADS) k_cc_stats(const int32_t* __restrict__ sizes, uint32_t N, int32_t* __restrict__ stats) {
    __shared__ uint32_t s_red[2][ST_WAVES];
    __shared__ uint64_t s_key[ST_WAVES];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * (ST_THREADS * ST_ITEMS) + threadIdx.x;
    uint32_t roots = 0, points = 0;
    uint64_t key = 0;
#pragma unroll 16
    for (uint32_t it = 0; it < ST_ITEMS; it++) {
        const uint32_t p = base + it * ST_THREADS;
        const uint32_t s = p < N ? (uint32_t)sizes[p] : 0u;
        if (s > 0u) { roots++; points += s; key = max(key, (uint64_t)s << 32 | (0x7fffffffu - p)); }
    }
    roots = wave_sum(roots); points = wave_sum(points); key = wave_max64(key);
    if (lane == 0) { s_red[0][w] = roots; s_red[1][w] = points; s_key[w] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        roots = points = 0; key = 0;
#pragma unroll
        for (int a = 0; a < ST_WAVES; a++) { roots += s_red[0][a]; points += s_red[1][a]; key = max(key, s_key[a]); }
        if (roots) {
            atomicMax(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)key);
            atomicAdd(stats + 2, (int32_t)roots);
            atomicAdd(stats + 3, (int32_t)points);
        }
    }
}

__global__ void k_cc_finish(int32_t* __restrict__ stats) {
    const uint32_t low = (uint32_t)stats[0];             // the key's halves (little-endian)
    const int32_t size = stats[1], roots = stats[2];
    stats[0] = roots;
    stats[1] = size > 0 ? (int32_t)(0x7fffffffu - low) : -1;
    stats[2] = size;
}

// ---- filter: one thread per 4 points (one 16-byte access per array where the three bases allow it)
constexpr int CF_THREADS = 256;
constexpr int CF_ITEMS = 4;

__device__ __forceinline__ uint32_t filtered(uint32_t bits, int32_t label, const int32_t* __restrict__ sizes, uint32_t N, uint32_t thr_bits,
                                             int32_t min_size, int32_t keep_root) {
    if ((uint32_t)label >= N) return bits;               // outside (-1), or not a label: never an index into sizes
    const bool kept = sizes[label] >= min_size && (keep_root < 0 || label == keep_root);
    return kept ? bits : thr_bits;
}

template <bool VEC>
__global__ void __launch_bounds__(CF_THREADS) k_cc_filter(const uint32_t* u, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ sizes, uint32_t N, uint32_t thr_bits, int32_t min_size,
                                                          int32_t keep_root, uint32_t* out) {
    const uint32_t p0 = (blockIdx.x * CF_THREADS + threadIdx.x) * CF_ITEMS;
    if (p0 >= N) return;
    if (VEC && p0 + CF_ITEMS <= N) {
        const uint4 b = *reinterpret_cast<const uint4*>(u + p0);
        const int4 l = *reinterpret_cast<const int4*>(labels + p0);
        uint4 o;
        o.x = filtered(b.x, l.x, sizes, N, thr_bits, min_size, keep_root);
        o.y = filtered(b.y, l.y, sizes, N, thr_bits, min_size, keep_root);
        o.z = filtered(b.z, l.z, sizes, N, thr_bits, min_size, keep_root);
        o.w = filtered(b.w, l.w, sizes, N, thr_bits, min_size, keep_root);
        *reinterpret_cast<uint4*>(out + p0) = o;
        return;
    }
    for (uint32_t p = p0; p < min(p0 + CF_ITEMS, N); p++) out[p] = filtered(u[p], labels[p], sizes, N, thr_bits, min_size, keep_root);
}

int check_dims(uint32_t nx, uint32_t ny, uint32_t nz, Dims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > 512 || ny > 512 || nz > 512) return LAE_EINVAL;
    d = Dims{nx, ny, nz, ny * nz, nx * ny * nz, lae::cdiv(ny, CC_TY), lae::cdiv(nz, CC_TZ)};
    return LAE_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int lae_components_label(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, double threshold, int32_t* labels, void* stream) {
    Dims d;
    if (check_dims(nx, ny, nz, d)) return LAE_EINVAL;
    if (!u || !labels) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t tiles = lae::cdiv(nx, CC_TX) * d.ty * d.tz;
    k_cc_tile<<<tiles, CC_THREADS, 0, s>>>(u, d, (float)threshold, labels);
    int rc = lae::check_launch("components_label/tile");
    if (rc) return rc;
    uint32_t* parent = reinterpret_cast<uint32_t*>(labels);
    const uint32_t nb = lae::cdiv(d.P, CC_POINT_THREADS);
    k_cc_merge<<<nb, CC_POINT_THREADS, 0, s>>>(parent, d);
    rc = lae::check_launch("components_label/merge");
    if (rc) return rc;
    k_cc_flatten<<<nb, CC_POINT_THREADS, 0, s>>>(parent, d.P);
    return lae::check_launch("components_label/flatten");
}

int lae_components_sizes(const int32_t* labels, uint64_t N, int32_t* sizes, int32_t* stats, void* stream) {
    if (N == 0) return LAE_OK;
    if (N > CC_MAX_POINTS) return LAE_EINVAL;
    if (!labels || !sizes || !stats) return LAE_ENULL;
    if (reinterpret_cast<uintptr_t>(stats) & 7) return LAE_EINVAL;       // stats[0..1] hold a 64-bit key between the passes
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t n = (uint32_t)N;
    k_cc_zero<<<lae::cdiv(n, ST_THREADS), ST_THREADS, 0, s>>>(sizes, n, stats);
    int rc = lae::check_launch("components_sizes/zero");
    if (rc) return rc;
    k_cc_count<<<lae::cdiv(n, CS_BLOCK_POINTS), CS_THREADS, 0, s>>>(labels, n, sizes);
    rc = lae::check_launch("components_sizes/count");
    if (rc) return rc;
    k_cc_stats<<<lae::cdiv(n, ST_THREADS * ST_ITEMS), ST_THREADS, 0, s>>>(sizes, n, stats);
    rc = lae::check_launch("components_sizes/stats");
    if (rc) return rc;
    k_cc_finish<<<1, 1, 0, s>>>(stats);
    return lae::check_launch("components_sizes/finish");
}

int lae_components_filter(const float* u, const int32_t* labels, const int32_t* sizes, uint64_t N, double threshold, int32_t min_size,
                          int32_t keep_root, float* out, void* stream) {
    if (N == 0) return LAE_OK;
    if (N > CC_MAX_POINTS) return LAE_EINVAL;
    if (!u || !labels || !sizes || !out) return LAE_ENULL;
    const float thr = (float)threshold;
    uint32_t thr_bits;
    __builtin_memcpy(&thr_bits, &thr, 4);
    const uint32_t n = (uint32_t)N;
    const uint32_t nb = lae::cdiv(n, CF_THREADS * CF_ITEMS);
    const uint32_t* ub = reinterpret_cast<const uint32_t*>(u);
    uint32_t* ob = reinterpret_cast<uint32_t*>(out);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (aligned16(u) && aligned16(labels) && aligned16(out))
        k_cc_filter<true><<<nb, CF_THREADS, 0, s>>>(ub, labels, sizes, n, thr_bits, min_size, keep_root, ob);
    else
        k_cc_filter<false><<<nb, CF_THREADS, 0, s>>>(ub, labels, sizes, n, thr_bits, min_size, keep_root, ob);
    return lae::check_launch("components_filter");
}

}  // extern "C"
