// region.hip -- move, rotate, scale, copy or delete the selected region of a trained NeRF at render time (DESIGN.md section 4c,
// "Region transform"; laenerf_amd/editing/region_transform.py restates both entry points in numpy).
//
// The selection is an edit bitfield (the layout of density_bitfield: cascade-major, Morton order inside a cascade).  A similarity
// x_new = s R (x - pivot) + pivot + t places the selected object; the host forms the forward map M [3,4], its inverse Minv [3,4]
// and Rt = R^T [3,3] in float64 and rounds each once to fp32.  Nothing is resampled: the field is evaluated where the object
// CAME FROM.
//
// sel(q): the selection bit of q's cell at q's OWN cascade -- level = cascade_of(max |q_i|, C), the cell index is probe_at's
// (raymarch_common.h) with dt left out, statement for statement.
//
// lae_region_warp, one sample row (x, d) per thread.  p = Minv (x, 1), each component ((m0 x + m1 y) + m2 z) + m3, one rounding per
// operation (-ffp-contract=off):
//   moved    mode != DELETE, |p_i| <= bound for every i and sel(p):  xyz = p, dir = Rt d ((r0 dx + r1 dy) + r2 dz), sigma_scale = 1/s.
//            The moved object wins over whatever stood at the target (paste-over).  delta stays the marcher's world step, so the
//            density is divided by s: the object keeps its opacity per object length.
//   vacated  else, mode != COPY and sel(x):                           the row is unchanged, sigma_scale = 0.
//   kept     otherwise:                                               the row is unchanged, sigma_scale = 1.
// A NaN p fails the box test; rows the marcher left as zeros take one of the three branches like any other row.
//
// lae_region_occupancy: the bitfield the marcher walks, a conservative superset of where the edited scene has density.
//   keep     out = occ; in modes MOVE and DELETE the bit of a cell is cleared when its selection bit is set and the cell is of its
//            own cascade (cascade 0, or at c > 0 not all three coordinates in [H/4, 3H/4): outside the half cascade c - 1 covers).
//            No other bit is cleared.
//   image    modes MOVE and COPY.  Every selected, occupied SOURCE cell maps its 8 corners with M, takes their axis-aligned box,
//            widens it by `margin` and sets the bit of every cell the box overlaps at EVERY cascade (clipped to the cascade's
//            domain): the marcher may probe any level at or above a point's own.  The image of a cube is inside the box of its
//            corner images, so the result is conservative up to rounding, which `margin` covers (derived from the fp32 error of
//            the two maps in region_transform.py; a small fraction of a cell).  Source cells are the own-cascade cells plus, at
//            c > 0, the layer with a coordinate equal to H/4: a point with a coordinate of exactly -2^(c-1) has level c and
//            looks its bit up there.  Cell ranges come from the marcher's own position-to-cell statement, which is monotone, so
//            box corners and sample points round the same way.
//   Bits are set with 32-bit atomicOr (after a plain look at the word); OR does not depend on order: two calls give the same bytes.
#include <algorithm>

#include "raymarch_common.h"

namespace {

struct Affine { float m[12]; };     // rows [m0 m1 m2 | m3]
struct Rot { float r[9]; };

__device__ __forceinline__ float affine_row(const float* m, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}
__device__ __forceinline__ float rot_row(const float* r, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)), __fmul_rn(r[2], z));
}

// probe_at's cell coordinate of v at a level whose reciprocal mip bound is rb (raymarch_common.h:82)
__device__ __forceinline__ int cell_coord(const MarchCfg& c, float v, float rb) {
    return (int)clampf((0.5f * fmaf(v, rb, 1.0f)) * c.Hf, 0.0f, c.Hm1);
}

__device__ __forceinline__ bool sel_at(const MarchCfg& c, const uint8_t* __restrict__ sel, float x, float y, float z) {
    const float amax = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    const int level = cascade_of(amax, c.Cf);
    float mb, rb;
    mip_bounds(c, level, mb, rb);
    const uint32_t index = (uint32_t)level * c.H3 +
                           morton_encode((uint32_t)cell_coord(c, x, rb), (uint32_t)cell_coord(c, y, rb), (uint32_t)cell_coord(c, z, rb));
    return (sel[index >> 3] >> (index & 7u)) & 1u;
}

__device__ __forceinline__ void warp_row(const MarchCfg& c, const uint8_t* __restrict__ sel, const Affine& A, const Rot& R,
                                         float inv_s, int mode, float& x, float& y, float& z, float& dx, float& dy, float& dz, float& s) {
    const float px = affine_row(A.m, x, y, z), py = affine_row(A.m + 4, x, y, z), pz = affine_row(A.m + 8, x, y, z);
    const bool inside = fabsf(px) <= c.bound && fabsf(py) <= c.bound && fabsf(pz) <= c.bound;
    if (mode != LAE_REGION_DELETE && inside && sel_at(c, sel, px, py, pz)) {
        const float qx = rot_row(R.r, dx, dy, dz), qy = rot_row(R.r + 3, dx, dy, dz), qz = rot_row(R.r + 6, dx, dy, dz);
        x = px; y = py; z = pz; dx = qx; dy = qy; dz = qz; s = inv_s;
    } else if (mode != LAE_REGION_COPY && sel_at(c, sel, x, y, z)) {
        s = 0.0f;
    } else {
        s = 1.0f;
    }
}

// Streaming: 24 bytes in, 28 out per row, the bitfield gathers stay in L2.  A thread owns 4 consecutive rows = three 16-byte
// loads per array (48 contiguous bytes a lane, 3 KiB a wave instruction triple), all issued before the first use; the grid is capped
// and strides.  In-place use is safe: a thread reads its rows before it writes them and no other thread touches them.
constexpr int RW_THREADS = 256, RW_ROWS = 4, RW_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(RW_THREADS) void k_region_warp4(const float4* xyzs, const float4* dirs, uint32_t quads,
                                                             const uint8_t* __restrict__ sel, Affine A, Rot R, float inv_s, int mode,
                                                             MarchCfg c, float4* xyzs_out, float4* dirs_out, float4* __restrict__ scale_out) {
    for (uint32_t q = blockIdx.x * RW_THREADS + threadIdx.x; q < quads; q += gridDim.x * RW_THREADS) {
        const float4 a0 = xyzs[3 * (size_t)q], a1 = xyzs[3 * (size_t)q + 1], a2 = xyzs[3 * (size_t)q + 2];
        const float4 b0 = dirs[3 * (size_t)q], b1 = dirs[3 * (size_t)q + 1], b2 = dirs[3 * (size_t)q + 2];
        float x[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        float d[12] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
        float s[RW_ROWS];
#pragma unroll
        for (int k = 0; k < RW_ROWS; k++)
            warp_row(c, sel, A, R, inv_s, mode, x[3 * k], x[3 * k + 1], x[3 * k + 2], d[3 * k], d[3 * k + 1], d[3 * k + 2], s[k]);
        xyzs_out[3 * (size_t)q] = make_float4(x[0], x[1], x[2], x[3]);
        xyzs_out[3 * (size_t)q + 1] = make_float4(x[4], x[5], x[6], x[7]);
        xyzs_out[3 * (size_t)q + 2] = make_float4(x[8], x[9], x[10], x[11]);
        dirs_out[3 * (size_t)q] = make_float4(d[0], d[1], d[2], d[3]);
        dirs_out[3 * (size_t)q + 1] = make_float4(d[4], d[5], d[6], d[7]);
        dirs_out[3 * (size_t)q + 2] = make_float4(d[8], d[9], d[10], d[11]);
        scale_out[q] = make_float4(s[0], s[1], s[2], s[3]);
    }
}

// rows [first, M): the up-to-3 rows after the last whole quad, or every row when a base address is not 16-byte aligned
__global__ __launch_bounds__(RW_THREADS) void k_region_warp1(const float* xyzs, const float* dirs, uint32_t first,
                                                             uint32_t M, const uint8_t* __restrict__ sel, Affine A, Rot R, float inv_s,
                                                             int mode, MarchCfg c, float* xyzs_out, float* dirs_out,
                                                             float* __restrict__ scale_out) {
    for (size_t i = (size_t)first + blockIdx.x * RW_THREADS + threadIdx.x; i < M; i += (size_t)gridDim.x * RW_THREADS) {
        float x = xyzs[3 * i], y = xyzs[3 * i + 1], z = xyzs[3 * i + 2];
        float dx = dirs[3 * i], dy = dirs[3 * i + 1], dz = dirs[3 * i + 2], s;
        warp_row(c, sel, A, R, inv_s, mode, x, y, z, dx, dy, dz, s);
        xyzs_out[3 * i] = x; xyzs_out[3 * i + 1] = y; xyzs_out[3 * i + 2] = z;
        dirs_out[3 * i] = dx; dirs_out[3 * i + 1] = dy; dirs_out[3 * i + 2] = dz;
        scale_out[i] = s;
    }
}

// ---- occupancy
__device__ __forceinline__ bool in_inner_half(uint32_t n, uint32_t lo, uint32_t H) { return n >= lo && n < 3u * (H >> 2); }

// keep part: one 32-bit word (32 consecutive Morton cells of one cascade) per thread
__global__ __launch_bounds__(256) void k_region_keep(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ sel, uint32_t words,
                                                     uint32_t cshift, uint32_t H, int mode, uint32_t* __restrict__ out) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= words) return;
    const uint32_t o = occ[w];
    uint32_t clear = mode == LAE_REGION_COPY ? 0u : sel[w];
    if (clear && ((w << 5) >> cshift) > 0u) {             // cascade > 0: only cells outside the inner half are its own
        const uint32_t m0 = (w << 5) & ((1u << cshift) - 1u);
        for (uint32_t b = 0; b < 32u; b++) {
            const uint32_t m = m0 + b;
            if (((clear >> b) & 1u) && in_inner_half(morton_compact(m), H >> 2, H) && in_inner_half(morton_compact(m >> 1), H >> 2, H) &&
                in_inner_half(morton_compact(m >> 2), H >> 2, H))
                clear &= ~(1u << b);
        }
    }
    out[w] = o & ~clear;
}

// image part: one cell per thread; a source cell walks every target cascade
__global__ __launch_bounds__(256) void k_region_image(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ sel, uint32_t total,
                                                      uint32_t cshift, uint32_t C, Affine A, float margin, MarchCfg c, uint32_t* out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    if (!(((occ[g >> 5] & sel[g >> 5]) >> (g & 31u)) & 1u)) return;
    const uint32_t cas = g >> cshift, m = g & ((1u << cshift) - 1u), H = 1u << (cshift / 3u);
    const uint32_t nx = morton_compact(m), ny = morton_compact(m >> 1), nz = morton_compact(m >> 2);
    // at cascade > 0 the cells strictly inside the inner half are never a point's own (the layer at H/4 is: see the header)
    if (cas > 0u && in_inner_half(nx, (H >> 2) + 1u, H) && in_inner_half(ny, (H >> 2) + 1u, H) && in_inner_half(nz, (H >> 2) + 1u, H)) return;
    float mb, rb;
    mip_bounds(c, (int)cas, mb, rb);
    // the cell's faces, the inverse of the marcher's cell lookup: (((n / H) * 2) - 1) * mip_bound, exact in fp32
    const float fx[2] = {(((float)nx * c.rH) * 2.0f - 1.0f) * mb, (((float)(nx + 1u) * c.rH) * 2.0f - 1.0f) * mb};
    const float fy[2] = {(((float)ny * c.rH) * 2.0f - 1.0f) * mb, (((float)(ny + 1u) * c.rH) * 2.0f - 1.0f) * mb};
    const float fz[2] = {(((float)nz * c.rH) * 2.0f - 1.0f) * mb, (((float)(nz + 1u) * c.rH) * 2.0f - 1.0f) * mb};
    float lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float x = fx[k & 1], y = fy[(k >> 1) & 1], z = fz[k >> 2];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = affine_row(A.m + 4 * a, x, y, z);
            lo[a] = k ? fminf(lo[a], v) : v;
            hi[a] = k ? fmaxf(hi[a], v) : v;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) { lo[a] = __fsub_rn(lo[a], margin); hi[a] = __fadd_rn(hi[a], margin); }
    for (uint32_t t = 0; t < C; t++) {
        float tb, trb;
        mip_bounds(c, (int)t, tb, trb);
        if (lo[0] > tb || lo[1] > tb || lo[2] > tb || hi[0] < -tb || hi[1] < -tb || hi[2] < -tb) continue;     // outside this cascade's domain
        const int x0 = cell_coord(c, lo[0], trb), x1 = cell_coord(c, hi[0], trb);
        const int y0 = cell_coord(c, lo[1], trb), y1 = cell_coord(c, hi[1], trb);
        const int z0 = cell_coord(c, lo[2], trb), z1 = cell_coord(c, hi[2], trb);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) {
                    const uint32_t idx = (t << cshift) + morton_encode((uint32_t)x, (uint32_t)y, (uint32_t)z);     // < total: 0 <= x, y, z < H
                    const uint32_t bit = 1u << (idx & 31u);
                    if (!(__hip_atomic_load(out + (idx >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(out + (idx >> 5), bit);
                }
    }
}

// what both entries ask of the grid: H a power of two in [4, 128], 1 <= C <= 2 (the shipped bounds 1 and 2; the image part's
// per-cell box walk is unmeasured beyond, where a coarse cell's box covers ever more fine cells), bound = 2^(C-1) (the renderer's cascade rule for a
// power-of-two bound: every level's mip bound is 2^level), and a bitfield of exactly C H^3 / 8 bytes.  -> log2(H), or -1
static int grid_shape_ok(float bound, uint32_t C, uint32_t H, uint64_t bytes) {
    if (H < 4 || H > 128 || (H & (H - 1)) != 0 || C == 0 || C > 2) return -1;
    if (!(bound == (float)(1u << (C - 1)))) return -1;
    int lg = 0;
    while ((1u << lg) < H) lg++;
    if (bytes != ((uint64_t)C << (3 * lg)) / 8) return -1;
    return lg;
}
static bool finite_all(const float* v, int n) {
    for (int i = 0; i < n; i++)
        if (!(v[i] - v[i] == 0.0f)) return false;
    return true;
}
static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int lae_region_warp(const float* xyzs, const float* dirs, uint32_t M, const uint8_t* sel, uint64_t sel_bytes, const float* Minv,
                    const float* Rt, float inv_scale, int mode, float bound, uint32_t C, uint32_t H, float* xyzs_out, float* dirs_out,
                    float* sigma_scale, void* stream) {
    if (!xyzs || !dirs || !sel || !Minv || !Rt || !xyzs_out || !dirs_out || !sigma_scale) return LAE_EINVAL;
    if (mode < LAE_REGION_MOVE || mode > LAE_REGION_DELETE) return LAE_EINVAL;
    if (!(inv_scale >= 0.5f && inv_scale <= 2.0f)) return LAE_EINVAL;                 // s in [0.5, 2]; a NaN fails both
    if (grid_shape_ok(bound, C, H, sel_bytes) < 0 || !finite_all(Minv, 12) || !finite_all(Rt, 9)) return LAE_EINVAL;
    if (!aligned(xyzs, 4) || !aligned(dirs, 4) || !aligned(xyzs_out, 4) || !aligned(dirs_out, 4) || !aligned(sigma_scale, 4)) return LAE_EINVAL;
    if (M == 0) return LAE_OK;
    Affine A; Rot R;
    for (int i = 0; i < 12; i++) A.m[i] = Minv[i];
    for (int i = 0; i < 9; i++) R.r[i] = Rt[i];
    const MarchCfg c = make_cfg(bound, 0.0f, 1024, C, H);
    hipStream_t s = STREAM(stream);
    const bool vec = aligned(xyzs, 16) && aligned(dirs, 16) && aligned(xyzs_out, 16) && aligned(dirs_out, 16) && aligned(sigma_scale, 16);
    const uint32_t quads = vec ? M / RW_ROWS : 0u, first = quads * RW_ROWS;
    if (quads)
        k_region_warp4<<<std::min(lae::cdiv(quads, (uint32_t)RW_THREADS), (uint32_t)RW_MAX_BLOCKS), RW_THREADS, 0, s>>>(
            reinterpret_cast<const float4*>(xyzs), reinterpret_cast<const float4*>(dirs), quads, sel, A, R, inv_scale, mode, c,
            reinterpret_cast<float4*>(xyzs_out), reinterpret_cast<float4*>(dirs_out), reinterpret_cast<float4*>(sigma_scale));
    if (first < M)
        k_region_warp1<<<std::min(lae::cdiv(M - first, (uint32_t)RW_THREADS), (uint32_t)RW_MAX_BLOCKS), RW_THREADS, 0, s>>>(
            xyzs, dirs, first, M, sel, A, R, inv_scale, mode, c, xyzs_out, dirs_out, sigma_scale);
    return lae::check_launch("region_warp");
}

int lae_region_occupancy(const uint8_t* occ, const uint8_t* sel, uint64_t bytes, const float* M, float margin, int mode, float bound,
                         uint32_t C, uint32_t H, uint8_t* out, void* stream) {
    if (!occ || !sel || !out || (mode != LAE_REGION_DELETE && !M)) return LAE_EINVAL;
    if (mode < LAE_REGION_MOVE || mode > LAE_REGION_DELETE) return LAE_EINVAL;
    const int lg = grid_shape_ok(bound, C, H, bytes);
    if (lg < 0 || out == occ || out == sel || !aligned(occ, 4) || !aligned(sel, 4) || !aligned(out, 4)) return LAE_EINVAL;
    // the margin is a rounding allowance: never a quarter of the finest cell (2 / H), let alone a whole one
    if (mode != LAE_REGION_DELETE && (!finite_all(M, 12) || !(margin >= 0.0f && margin < 0.5f / (float)H))) return LAE_EINVAL;
    const uint32_t cshift = 3u * (uint32_t)lg, total = C << cshift, words = total >> 5;
    hipStream_t s = STREAM(stream);
    k_region_keep<<<lae::cdiv(words, 256u), 256, 0, s>>>(reinterpret_cast<const uint32_t*>(occ), reinterpret_cast<const uint32_t*>(sel), words,
                                                        cshift, H, mode, reinterpret_cast<uint32_t*>(out));
    if (mode != LAE_REGION_DELETE) {
        Affine A;
        for (int i = 0; i < 12; i++) A.m[i] = M[i];
        k_region_image<<<lae::cdiv(total, 256u), 256, 0, s>>>(reinterpret_cast<const uint32_t*>(occ), reinterpret_cast<const uint32_t*>(sel), total,
                                                             cshift, C, A, margin, make_cfg(bound, 0.0f, 1024, C, H), reinterpret_cast<uint32_t*>(out));
    }
    return lae::check_launch("region_occupancy");
}

}  // extern "C"
