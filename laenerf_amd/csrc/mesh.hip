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
//
// Export (lae_mesh_vertex_attrs, lae_mesh_pack_ply): per-vertex position in the box, normal and view direction from the field
// the mesh was cut from, and the binary PLY bodies assembled on the device.  The specification is in include/laenerf.h.
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

// ---- vertex attributes: one thread per vertex
constexpr int VA_THREADS = 256;

struct Box {
    float bmin[3], bmax[3];
};

// central difference of u along every axis at the lattice point p (one-sided on a border); p is inside the lattice, so is
// every index read here
__device__ __forceinline__ void lattice_gradient(const float* __restrict__ u, const Dims& d, const int (&p)[3], float (&g)[3]) {
    const int n[3] = {(int)d.nx, (int)d.ny, (int)d.nz};
    const uint32_t step[3] = {d.nyz, d.nz, 1u};
    const uint32_t at = ((uint32_t)p[0] * d.ny + (uint32_t)p[1]) * d.nz + (uint32_t)p[2];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool lo = p[a] > 0, hi = p[a] + 1 < n[a];
        const float diff = __fsub_rn(u[hi ? at + step[a] : at], u[lo ? at - step[a] : at]);
        g[a] = lo && hi ? __fmul_rn(diff, 0.5f) : diff;
    }
}

__global__ void __launch_bounds__(VA_THREADS) k_mesh_vertex_attrs(const float* __restrict__ u, Dims d, const float* __restrict__ verts,
                                                                  uint32_t V, Box box, float* __restrict__ pos,
                                                                  float* __restrict__ normals, float* __restrict__ dirs) {
    const uint32_t i = blockIdx.x * VA_THREADS + threadIdx.x;
    if (i >= V) return;
    const int n[3] = {(int)d.nx, (int)d.ny, (int)d.nz};
    float v[3], ext[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        v[a] = verts[3 * (uint64_t)i + a];
        if (!__builtin_isfinite(v[a])) v[a] = 0.0f;
        ext[a] = __fsub_rn(box.bmax[a], box.bmin[a]);
    }
    if (pos) {
#pragma unroll
        for (int a = 0; a < 3; a++)      // v / (n - 1) * (bmax - bmin) + bmin in fp64, each step rounded, one rounding to fp32
            pos[3 * (uint64_t)i + a] = (float)__dadd_rn(__dmul_rn(__ddiv_rn((double)v[a], (double)(n[a] - 1)), (double)ext[a]), (double)box.bmin[a]);
    }
    if (!normals && !dirs) return;
    int base[3], q[3];
    float t = 0.0f;
    int axis = -1;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float b = fminf(fmaxf(floorf(v[a]), 0.0f), (float)(n[a] - 1));      // clamped as a float: the conversion cannot overflow
        base[a] = q[a] = (int)b;
        const float frac = __fsub_rn(v[a], b);
        if (axis < 0 && frac > 0.0f) { axis = a; t = frac; }
    }
    float g0[3], w[3];
    lattice_gradient(u, d, base, g0);
    if (axis >= 0) {
        q[axis] = min(base[axis] + 1, n[axis] - 1);
        float g1[3];
        lattice_gradient(u, d, q, g1);
#pragma unroll
        for (int a = 0; a < 3; a++) g0[a] = __fadd_rn(g0[a], __fmul_rn(t, __fsub_rn(g1[a], g0[a])));
    }
#pragma unroll
    for (int a = 0; a < 3; a++) w[a] = __fmul_rn(g0[a], __fdiv_rn((float)(n[a] - 1), ext[a]));
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], w[0]), __fmul_rn(w[1], w[1])), __fmul_rn(w[2], w[2])));
    const bool ok = len > 0.0f && __builtin_isfinite(len);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float r = ok ? __fdiv_rn(w[a], len) : (a == 2 ? 1.0f : 0.0f);
        if (dirs) dirs[3 * (uint64_t)i + a] = r;
        if (normals) normals[3 * (uint64_t)i + a] = ok ? -r : 0.0f;
    }
}

// ---- PLY bodies: a workgroup builds PK_RECORDS records in an LDS image and stores the image as whole dwords.  PK_RECORDS is a
// multiple of 4, so every workgroup's part of the buffer starts on a dword whatever the record size; only the buffer's last
// 1-3 bytes (last workgroup) go out as bytes.
constexpr int PK_THREADS = 256;
constexpr uint32_t PK_RECORDS = PK_THREADS;
constexpr uint32_t PK_MAX_STRIDE = 27;

// `clip(x, 0, 1) * 255`, truncated (evaluate.hip to_u8); NaN -> 0
__device__ __forceinline__ uint32_t color_u8(float x) { return (uint32_t)(int)__fmul_rn(lae::clampf(x, 0.0f, 1.0f), 255.0f); }

// a little-endian 32-bit word at byte offset `at` of the image: one dword store where it is aligned, four byte stores where not
__device__ __forceinline__ void put32(uint32_t* img, uint32_t at, uint32_t w) {
    if ((at & 3u) == 0u) {
        img[at >> 2] = w;
    } else {
        uint8_t* b = reinterpret_cast<uint8_t*>(img) + at;
        b[0] = (uint8_t)w; b[1] = (uint8_t)(w >> 8); b[2] = (uint8_t)(w >> 16); b[3] = (uint8_t)(w >> 24);
    }
}

// FACES: records of 13 bytes (uchar 3, int[3]) from rec_a = tris; else vertex records of `stride` bytes from rec_a = pos,
// rec_b = normals or NULL, rec_c = rgb or NULL
template <bool FACES>
__global__ void __launch_bounds__(PK_THREADS) k_mesh_pack(const void* __restrict__ rec_a, const float* __restrict__ rec_b,
                                                          const float* __restrict__ rec_c, uint32_t count, uint32_t stride,
                                                          uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t img[PK_RECORDS * (FACES ? 13u : PK_MAX_STRIDE) / 4];
    const uint32_t first = blockIdx.x * PK_RECORDS;
    const uint32_t here = min(PK_RECORDS, count - first);                 // the grid has no empty workgroup
    const uint32_t r = threadIdx.x;
    if (r < here) {
        const uint64_t rec = (uint64_t)first + r;
        uint32_t at = r * stride;
        if (FACES) {
            const int32_t* tri = static_cast<const int32_t*>(rec_a) + 3 * rec;
            reinterpret_cast<uint8_t*>(img)[at] = 3;
#pragma unroll
            for (int c = 0; c < 3; c++) put32(img, at + 1 + 4 * c, (uint32_t)tri[c]);
        } else {
            const float* p = static_cast<const float*>(rec_a) + 3 * rec;
#pragma unroll
            for (int c = 0; c < 3; c++) put32(img, at + 4 * c, __float_as_uint(p[c]));
            at += 12;
            if (rec_b) {
#pragma unroll
                for (int c = 0; c < 3; c++) put32(img, at + 4 * c, __float_as_uint(rec_b[3 * rec + c]));
                at += 12;
            }
            if (rec_c) {
#pragma unroll
                for (int c = 0; c < 3; c++) reinterpret_cast<uint8_t*>(img)[at + c] = (uint8_t)color_u8(rec_c[3 * rec + c]);
            }
        }
    }
    __syncthreads();
    const uint32_t bytes = here * stride, dwords = bytes >> 2;
    uint8_t* dst = out + (uint64_t)first * stride;                        // 4-byte aligned: first % 4 == 0 and so is `out`
    uint32_t w0 = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {                   // 16-byte stores while whole quads are left
        const uint32_t quads = dwords >> 2;
        for (uint32_t w = threadIdx.x; w < quads; w += PK_THREADS)
            reinterpret_cast<uint4*>(dst)[w] = reinterpret_cast<const uint4*>(img)[w];
        w0 = quads << 2;
    }
    for (uint32_t w = w0 + threadIdx.x; w < dwords; w += PK_THREADS) reinterpret_cast<uint32_t*>(dst)[w] = img[w];
    const uint32_t tail = dwords << 2;
    if (tail + threadIdx.x < bytes) dst[tail + threadIdx.x] = reinterpret_cast<const uint8_t*>(img)[tail + threadIdx.x];
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

int lae_mesh_vertex_attrs(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, const float* verts, uint32_t V, float bmin_x,
                          float bmin_y, float bmin_z, float bmax_x, float bmax_y, float bmax_z, float* pos, float* normals, float* dirs,
                          void* stream) {
    Dims d;
    if (check_dims(nx, ny, nz, d)) return LAE_EINVAL;
    if (V == 0) return LAE_OK;
    if (!u || !verts) return LAE_ENULL;
    if (!pos && !normals && !dirs) return LAE_OK;
    const Box box{{bmin_x, bmin_y, bmin_z}, {bmax_x, bmax_y, bmax_z}};
    k_mesh_vertex_attrs<<<lae::cdiv(V, VA_THREADS), VA_THREADS, 0, reinterpret_cast<hipStream_t>(stream)>>>(u, d, verts, V, box, pos,
                                                                                                             normals, dirs);
    return lae::check_launch("mesh_vertex_attrs");
}

int lae_mesh_pack_ply(const float* pos, const float* normals, const float* rgb, uint32_t V, const int32_t* tris, uint32_t T,
                      uint8_t* vertex_bytes, uint8_t* face_bytes, void* stream) {
    if ((reinterpret_cast<uintptr_t>(vertex_bytes) & 3) || (reinterpret_cast<uintptr_t>(face_bytes) & 3)) return LAE_EINVAL;
    if ((vertex_bytes && V && !pos) || (face_bytes && T && !tris)) return LAE_ENULL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (vertex_bytes && V) {
        const uint32_t stride = 12u + (normals ? 12u : 0u) + (rgb ? 3u : 0u);
        k_mesh_pack<false><<<lae::cdiv(V, PK_RECORDS), PK_THREADS, 0, s>>>(pos, normals, rgb, V, stride, vertex_bytes);
        int rc = lae::check_launch("mesh_pack_ply/vertices");
        if (rc) return rc;
    }
    if (face_bytes && T) {
        k_mesh_pack<true><<<lae::cdiv(T, PK_RECORDS), PK_THREADS, 0, s>>>(tris, nullptr, nullptr, T, 13u, face_bytes);
        return lae::check_launch("mesh_pack_ply/faces");
    }
    return LAE_OK;
}

}  // extern "C"
