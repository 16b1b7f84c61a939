// simplify.hip -- quadric vertex clustering of an exported mesh ("Simplification"; simplify.py restates
// the kernels in numpy).  The reference exports the marching-cubes mesh as it is; it has no counterpart of this file.
//
// THE RULE (include/laenerf.h, lae_simplify_*).  Vertices fall into the cells of a lattice of spacing `cell` anchored at `origin`;
// every non-empty cell becomes one output vertex, placed where the planes of the triangles that touch the cell meet best:
//   cluster    ijk = floor(((double)p - (double)origin) / (double)cell) per axis, key = (i ny + j) nz + k (int64)
//   sums       fp64, relative to the cell centre c = origin + (ijk + 0.5) cell.  Over the member vertices: their count, the mean
//              position m, the colour mean.  Over every triangle with a corner in the cluster, once per cluster:
//              n = (p1 - p0) x (p2 - p0), A += n n^T, b += -(n . p0) n, N += n (the squared-area weighting of the plane
//              quadric: nothing is divided, a degenerate triangle adds zero by itself)
//   solve      lambda = reg trace(A) / 3 + 1e-18 cell^4; (A + lambda I) x = lambda m - b (SPD, condition <= 1 + 3 / reg, Cholesky
//              in fp64); x clamped per axis to [-cell / 2, cell / 2]; position = (float)(c + x).  No branch: without faces the
//              floor term gives x = m.  placement "mean" takes x = m.
//   normal     N / |N| rounded to fp32, zero where N is zero; colours: the member mean rounded to fp32
//   triangles  corners through vertex_map; two equal corners: dropped; survivors keep corner order and input order; with dedup
//              only the lowest input index of a vertex SET stays (key: the sorted triple, 3 x 21 bits)
//
// WHO SUMS WHAT.  Ordering is the caller's (simplify.py: stable sorts of the vertex keys and of the (cluster, triangle) pairs,
// and their segment starts); the kernels here never add a floating-point number atomically.  k_simplify_reduce<G> gives a cluster
// to G adjacent lanes (1, 16 or 64): lane l takes items l, l + G, ... of the cluster's two segments in their sorted order, and
// the G partial sums meet in an xor butterfly whose shape depends on G alone -- the same bytes on every call.  The only atomic is
// the integer OR of the error flag.
#include "lae_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int SP_THREADS = 256;
constexpr int N_ACC = 19;                              // m 3, colour 4, A 6 (xx xy xz yy yz zz), b 3, N 3
constexpr int A_M = 0, A_COL = 3, A_A = 7, A_B = 13, A_N = 16;

struct Grid { double o[3]; double cell; uint32_t n[3]; };

__global__ void __launch_bounds__(SP_THREADS) k_simplify_keys(const float* __restrict__ verts, uint32_t V, Grid g, int64_t* __restrict__ keys,
                                                               int32_t* __restrict__ flag) {
    const uint32_t v = blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    int64_t ijk[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double f = floor(((double)verts[3 * (size_t)v + a] - g.o[a]) / g.cell);
        ok = ok && f >= 0.0 && f < (double)g.n[a];     // NaN and infinities fail both comparisons' conjunction
        ijk[a] = ok ? (int64_t)f : 0;
    }
    keys[v] = ok ? (ijk[0] * (int64_t)g.n[1] + ijk[1]) * (int64_t)g.n[2] + ijk[2] : (int64_t)-1;
    if (!ok) atomicOr(flag, LAE_SIMPLIFY_BAD_VERTEX);
}

// the up-to-three (cluster, triangle) pairs of a triangle at slots 3 t + {0, 1, 2} (a corner whose cluster an earlier corner
// named already writes the sentinel V_out, which sorts behind every cluster), its survival flag and its dedup key
__global__ void __launch_bounds__(SP_THREADS) k_simplify_pairs(const int32_t* __restrict__ tris, uint32_t T, const int32_t* __restrict__ vmap,
                                                                uint32_t V, uint32_t V_out, int32_t* __restrict__ pair_cluster,
                                                                uint8_t* __restrict__ surv, int64_t* __restrict__ tri_key,
                                                                int32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * SP_THREADS + threadIdx.x;
    if (t >= T) return;
    const int32_t a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    const bool ok = (uint32_t)a < V && (uint32_t)b < V && (uint32_t)c < V;
    const int32_t none = (int32_t)V_out;
    int32_t m0 = none, m1 = none, m2 = none;
    if (ok) { m0 = vmap[a]; m1 = vmap[b]; m2 = vmap[c]; }
    else atomicOr(flag, LAE_SIMPLIFY_BAD_INDEX);
    pair_cluster[3 * (size_t)t] = m0;
    pair_cluster[3 * (size_t)t + 1] = m1 != m0 ? m1 : none;
    pair_cluster[3 * (size_t)t + 2] = (m2 != m0 && m2 != m1) ? m2 : none;
    const bool alive = ok && m0 != m1 && m1 != m2 && m0 != m2;
    surv[t] = alive ? 1 : 0;
    if (tri_key) {
        int64_t lo = min(m0, min(m1, m2)), hi = max(m0, max(m1, m2));
        int64_t mid = (int64_t)m0 + m1 + m2 - lo - hi;
        tri_key[t] = alive ? ((lo << 42) | (mid << 21) | hi) : INT64_MAX;
    }
}

// keep[] of the dedup: in the stable order of the keys a triangle stays iff it survived and opens its run of equal keys
__global__ void __launch_bounds__(SP_THREADS) k_simplify_first(const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order,
                                                                uint32_t T, uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= T) return;
    const int64_t k = sorted_keys[i], t = order[i];
    if ((uint64_t)t >= T) return;
    keep[t] = (k != INT64_MAX && (i == 0 || sorted_keys[i - 1] != k)) ? 1 : 0;
}

__global__ void __launch_bounds__(SP_THREADS) k_simplify_compact(const int32_t* __restrict__ tris, uint32_t T, const int32_t* __restrict__ vmap,
                                                                  const uint8_t* __restrict__ keep, const int64_t* __restrict__ incl,
                                                                  uint32_t T_out, int32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * SP_THREADS + threadIdx.x;
    if (t >= T || !keep[t]) return;
    const int64_t o = incl[t] - 1;
    if ((uint64_t)o >= T_out) return;
#pragma unroll
    for (int a = 0; a < 3; a++) out[3 * o + a] = vmap[tris[3 * (size_t)t + a]];
}

struct ReduceArgs {
    const float* verts; const float* colors; uint32_t C;
    const int32_t* tris;
    const int64_t* vorder; const int64_t* vkeys; const int64_t* vstart;      // vertices sorted by key; segment starts [V_out + 1]
    const int64_t* porder; const int64_t* pstart;                            // pair slots (3 t + corner) sorted by cluster
    uint32_t V_out, V, T;
    Grid g;
    double reg; int mean;
    float* pos; float* normals; float* colors_out;
};

template <int G>
__global__ void __launch_bounds__(SP_THREADS) k_simplify_reduce(ReduceArgs r) {
    const uint32_t gid = blockIdx.x * SP_THREADS + threadIdx.x;
    const uint32_t c = gid / G, l = gid % G;
    const bool live = c < r.V_out;                     // a group is live or idle as a whole; idle groups walk empty segments
    int64_t v0 = 0, v1 = 0, p0 = 0, p1 = 0;
    double ctr[3] = {0, 0, 0};
    if (live) {
        v0 = r.vstart[c]; v1 = r.vstart[c + 1]; p0 = r.pstart[c]; p1 = r.pstart[c + 1];
        const int64_t key = r.vkeys[v0];
        const int64_t ny = r.g.n[1], nz = r.g.n[2];
        const int64_t ijk[3] = {key / (ny * nz), (key / nz) % ny, key % nz};
#pragma unroll
        for (int a = 0; a < 3; a++) ctr[a] = r.g.o[a] + ((double)ijk[a] + 0.5) * r.g.cell;
    }
    double s[N_ACC];
#pragma unroll
    for (int i = 0; i < N_ACC; i++) s[i] = 0.0;

    for (int64_t q = v0 + l; q < v1; q += G) {
        const uint64_t v = (uint64_t)r.vorder[q];
        if (v >= r.V) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) s[A_M + a] += (double)r.verts[3 * v + a] - ctr[a];
        for (uint32_t k = 0; k < r.C; k++) s[A_COL + k] += (double)r.colors[r.C * v + k];
    }
    for (int64_t q = p0 + l; q < p1; q += G) {
        const uint64_t t = (uint64_t)r.porder[q] / 3u;
        if (t >= r.T) continue;
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t v = (uint32_t)r.tris[3 * t + k];     // range-checked by k_simplify_pairs: a bad triangle has no pair
#pragma unroll
            for (int a = 0; a < 3; a++) p[k][a] = (double)r.verts[3 * (size_t)v + a] - ctr[a];
        }
        double e1[3], e2[3];
#pragma unroll
        for (int a = 0; a < 3; a++) { e1[a] = p[1][a] - p[0][a]; e2[a] = p[2][a] - p[0][a]; }
        const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double d = -((n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2]);
        s[A_A + 0] += n[0] * n[0]; s[A_A + 1] += n[0] * n[1]; s[A_A + 2] += n[0] * n[2];
        s[A_A + 3] += n[1] * n[1]; s[A_A + 4] += n[1] * n[2]; s[A_A + 5] += n[2] * n[2];
#pragma unroll
        for (int a = 0; a < 3; a++) { s[A_B + a] += d * n[a]; s[A_N + a] += n[a]; }
    }
    if (G > 1) {
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
#pragma unroll
            for (int i = 0; i < N_ACC; i++) s[i] += __shfl_xor(s[i], off, G);
        }
    }
    if (!live || l != 0) return;

    const double cnt = (double)(v1 - v0);
    const double m[3] = {s[A_M] / cnt, s[A_M + 1] / cnt, s[A_M + 2] / cnt};
    double x[3] = {m[0], m[1], m[2]};
    if (!r.mean) {
        const double c2 = r.g.cell * r.g.cell;
        const double lam = r.reg * ((s[A_A] + s[A_A + 3]) + s[A_A + 5]) / 3.0 + 1e-18 * (c2 * c2);
        const double M00 = s[A_A] + lam, M10 = s[A_A + 1], M20 = s[A_A + 2], M11 = s[A_A + 3] + lam, M21 = s[A_A + 4], M22 = s[A_A + 5] + lam;
        const double r0 = lam * m[0] - s[A_B], r1 = lam * m[1] - s[A_B + 1], r2 = lam * m[2] - s[A_B + 2];
        const double l00 = sqrt(M00), l10 = M10 / l00, l20 = M20 / l00;
        const double l11 = sqrt(M11 - l10 * l10), l21 = (M21 - l20 * l10) / l11;
        const double l22 = sqrt((M22 - l20 * l20) - l21 * l21);
        const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
        x[2] = y2 / l22;
        x[1] = (y1 - l21 * x[2]) / l11;
        x[0] = ((y0 - l10 * x[1]) - l20 * x[2]) / l00;
    }
    const double h = 0.5 * r.g.cell;
#pragma unroll
    for (int a = 0; a < 3; a++) r.pos[3 * (size_t)c + a] = (float)(ctr[a] + fmin(h, fmax(-h, x[a])));
    if (r.normals) {
        const double len = sqrt((s[A_N] * s[A_N] + s[A_N + 1] * s[A_N + 1]) + s[A_N + 2] * s[A_N + 2]);
#pragma unroll
        for (int a = 0; a < 3; a++) r.normals[3 * (size_t)c + a] = len > 0.0 ? (float)(s[A_N + a] / len) : 0.0f;
    }
    if (r.colors_out)
        for (uint32_t k = 0; k < r.C; k++) r.colors_out[r.C * (size_t)c + k] = (float)(s[A_COL + k] / cnt);
}

bool grid_ok(float ox, float oy, float oz, float cell, uint32_t nx, uint32_t ny, uint32_t nz, Grid& g) {
    if (!(cell > 0.0f) || !(cell <= 3.0e38f) || !(ox - ox == 0.0f) || !(oy - oy == 0.0f) || !(oz - oz == 0.0f)) return false;
    if (!nx || !ny || !nz || (double)nx * (double)ny * (double)nz >= 4.0e18) return false;
    g = Grid{{(double)ox, (double)oy, (double)oz}, (double)cell, {nx, ny, nz}};
    return true;
}

}  // namespace

extern "C" {

int lae_simplify_keys(const float* verts, uint32_t V, float ox, float oy, float oz, float cell, uint32_t nx, uint32_t ny, uint32_t nz,
                      int64_t* keys, int32_t* flag, void* stream) {
    Grid g;
    if (!grid_ok(ox, oy, oz, cell, nx, ny, nz, g)) return LAE_EINVAL;
    if (V == 0) return LAE_OK;
    if (!verts || !keys || !flag) return LAE_ENULL;
    k_simplify_keys<<<lae::cdiv(V, SP_THREADS), SP_THREADS, 0, STREAM(stream)>>>(verts, V, g, keys, flag);
    return lae::check_launch("simplify_keys");
}

int lae_simplify_pairs(const int32_t* tris, uint32_t T, const int32_t* vertex_map, uint32_t V, uint32_t V_out, int32_t* pair_cluster,
                       uint8_t* survives, int64_t* tri_key, int32_t* flag, void* stream) {
    if (V_out > V || V_out > 0x7fffffffu || T > 0x7fffffffu / 3u) return LAE_EINVAL;
    if (tri_key && V_out > LAE_SIMPLIFY_DEDUP_MAX) return LAE_EINVAL;
    if (T == 0) return LAE_OK;
    if (!tris || (V && !vertex_map) || !pair_cluster || !survives || !flag) return LAE_ENULL;
    k_simplify_pairs<<<lae::cdiv(T, SP_THREADS), SP_THREADS, 0, STREAM(stream)>>>(tris, T, vertex_map, V, V_out, pair_cluster, survives,
                                                                                   tri_key, flag);
    return lae::check_launch("simplify_pairs");
}

int lae_simplify_reduce(const float* verts, uint32_t V, const float* colors, uint32_t C, const int32_t* tris, uint32_t T,
                        const int64_t* vorder, const int64_t* vkeys_sorted, const int64_t* vstart, const int64_t* porder,
                        const int64_t* pstart, uint32_t V_out, float ox, float oy, float oz, float cell, uint32_t nx, uint32_t ny,
                        uint32_t nz, double reg, int placement, int lanes, float* pos, float* normals, float* colors_out, void* stream) {
    Grid g;
    if (!grid_ok(ox, oy, oz, cell, nx, ny, nz, g)) return LAE_EINVAL;
    if (!(reg > 0.0) || !(reg <= 1.0e6) || C > 4 || (placement != LAE_SIMPLIFY_QUADRIC && placement != LAE_SIMPLIFY_MEAN)) return LAE_EINVAL;
    if (lanes != 0 && lanes != 1 && lanes != 16 && lanes != 64) return LAE_EINVAL;
    if (V_out > V) return LAE_EINVAL;
    if (V_out == 0) return LAE_OK;
    if (!verts || !vorder || !vkeys_sorted || !vstart || !pstart || !pos || (T && (!tris || !porder))) return LAE_ENULL;
    if ((colors_out && !colors) || (colors_out && C == 0)) return LAE_ENULL;
    // lanes per cluster.  Measured on the teacher scene of tools/simplify_bench.py, R = 256 / 512, reduce
    // kernel in us with 1 / 16 / 64 lanes -- cell 2 (8 items a cluster): 120 / 779 / 3952 and 782 / 5690 / 27691; cell 4 (20 - 25):
    // 230 / 352 / 1586 and 1071 / 2486 / 10322; cell 8 (80 - 90): 772 / 187 / 447 and 1819 / 1082 / 3038.  The butterfly of 19 doubles
    // is a fixed cost per cluster that a thread per cluster does not pay; it is won back once a cluster holds some tens of items.
    // (V + T) / V_out is what the host knows of that without a read; a wave per cluster never won.
    if (lanes == 0) lanes = lae::env_int("LAE_SIMPLIFY_LANES", ((uint64_t)V + T) / V_out >= LAE_SIMPLIFY_WIDE_ITEMS ? 16 : 1, {1, 16, 64});
    const ReduceArgs r{verts, colors, colors_out ? C : 0u, tris, vorder, vkeys_sorted, vstart, porder, pstart, V_out, V, T, g, reg,
                       placement == LAE_SIMPLIFY_MEAN, pos, normals, colors_out};
    const uint32_t nb = lae::cdiv((uint64_t)V_out * lanes, SP_THREADS);
    hipStream_t s = STREAM(stream);
    if (lanes == 1) k_simplify_reduce<1><<<nb, SP_THREADS, 0, s>>>(r);
    else if (lanes == 16) k_simplify_reduce<16><<<nb, SP_THREADS, 0, s>>>(r);
    else k_simplify_reduce<64><<<nb, SP_THREADS, 0, s>>>(r);
    return lae::check_launch("simplify_reduce");
}

int lae_simplify_first(const int64_t* sorted_keys, const int64_t* order, uint32_t T, uint8_t* keep, void* stream) {
    if (T == 0) return LAE_OK;
    if (!sorted_keys || !order || !keep) return LAE_ENULL;
    k_simplify_first<<<lae::cdiv(T, SP_THREADS), SP_THREADS, 0, STREAM(stream)>>>(sorted_keys, order, T, keep);
    return lae::check_launch("simplify_first");
}

int lae_simplify_compact(const int32_t* tris, uint32_t T, const int32_t* vertex_map, const uint8_t* keep, const int64_t* keep_incl,
                         uint32_t T_out, int32_t* out, void* stream) {
    if (T_out > T) return LAE_EINVAL;
    if (T == 0 || T_out == 0) return LAE_OK;
    if (!tris || !vertex_map || !keep || !keep_incl || !out) return LAE_ENULL;
    k_simplify_compact<<<lae::cdiv(T, SP_THREADS), SP_THREADS, 0, STREAM(stream)>>>(tris, T, vertex_map, keep, keep_incl, T_out, out);
    return lae::check_launch("simplify_compact");
}

}  // extern "C"
