// insert.hip -- insert the selected object of one trained NeRF (the SOURCE) into another scene (the DESTINATION) at render time
// ("Scene insert"; laenerf_amd/editing/scene_insert.py restates the three entry points in numpy).
//
// The rule is the region transform's (region.hip), across two fields.  The selection is a bitfield of the SOURCE grid (C_s cascades
// of H_s^3 cells, bound_s = 2^(C_s-1)); a similarity x_dst = s R (x_src - pivot) + position places the object in the destination
// (C_d, H_d, bound_d).  The host forms the forward map M [3,4], its inverse Minv [3,4] and Rt = R^T [3,3] in float64 and rounds each
// once to fp32.  Nothing is resampled: a destination sample is evaluated by the source field where the object CAME FROM, and the
// two fields' results are blended per sample.  Every operation that decides a branch or produces an output is one rounded fp32
// operation (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, -ffp-contract=off).
//
// bit(g, q): the bit of q's cell at q's OWN cascade in the source bitfield g -- level = cascade_of(max |q_i|, C_s), the cell index is
// probe_at's (raymarch_common.h) with dt left out, statement for statement (region.hip's sel_at).
//
// lae_insert_route, one sample row (x, d) per thread.  p = Minv (x, 1), each component ((m0 x + m1 y) + m2 z) + m3; q = Rt d,
// (r0 dx + r1 dy) + r2 dz.  The row is INSERTED iff
//     deltas == NULL or deltas[2 i] != 0          (the marcher's padding rows have a zero step and are skipped)
//     |p_i| <= bound_s for every i                (a NaN p fails)
//     bit(src_sel, p) and bit(src_occ, p).
// An inserted row gets slot = its rank among the inserted rows in ascending row order, and (p, q) go to row `slot` of xyzs_src /
// dirs_src; every other row gets slot = -1; *count = the number of inserted rows.  Rows of xyzs_src / dirs_src at and beyond
// *count are not written.  Three launches, none of which waits for another workgroup:
//     mark     a workgroup owns IR_TILE consecutive rows; a wave ballots its 64 predicates, a lane's rank in the wave is the
//              popcount of the ballot below it, the wave totals go through LDS: slot[i] = rank INSIDE the workgroup (or -1),
//              block_counts[b] = the workgroup's total
//     scan     one workgroup: exclusive prefix of block_counts in place, IR_SCAN_THREADS counts a pass with a carry between
//              passes (a pass covers IR_SCAN_THREADS * IR_TILE rows); *count = the sum
//     scatter  rows with slot >= 0 add their workgroup's offset, compute (p, q) again (the same statements: the same bits) and
//              write the compacted rows; other rows are not touched again
// Integer arithmetic only decides the order: two calls give the same bytes.  No atomics, no host read, no allocation: capturable.
//
// lae_insert_blend, one row per thread.  slot < 0 (or >= n_src, the rows the source arrays hold: lae_insert_route writes no such
// slot, and nothing is read outside the arrays): (sigma, rgb) = the destination's.  Otherwise ss = sigma_s[slot] * inv_scale
// (delta stays the marcher's destination step, so the density is divided by s: the object keeps its opacity per object length) and
//     REPLACE  sigma = ss, rgb = rgb_s[slot]: the object is pasted over what stood there (the region transform's semantics)
//     ADD      sigma = sigma_d + ss; rgb = sigma > 0 ? rgb_d + (ss / sigma) * (rgb_s - rgb_d) : rgb_d -- the exact mixture of two
//              participating media: densities add, colours average by density.
// Inputs are fp16 or fp32 each (converted to fp32 exactly), outputs fp32; an output may be the destination input it replaces when
// that input is fp32 (a thread reads its row before it writes it).
//
// lae_insert_occupancy: the bitfield the destination's marcher walks, a conservative superset of where the composed scene has
// density.  out = dst_occ, plus for every SOURCE cell that is selected, occupied and of its own cascade (cascade 0; at c > 0 not
// all three coordinates in (H_s/4, 3H_s/4): the layer with a coordinate equal to H_s/4 counts, a coordinate of exactly -2^(c-1)
// looks its bit up there -- k_region_image's rule) the image box: the 8 corners mapped with M, their axis-aligned box widened by
// `margin`, and the bit of every DESTINATION cell the box overlaps at EVERY destination cascade, clipped to the cascade's domain.
// Cell ranges come from the destination marcher's own position-to-cell statement, which is monotone.  No bit is cleared.  Bits are
// set with 32-bit atomicOr (after a plain look at the word): the same bytes from every call.
#include <algorithm>

#include "raymarch_common.h"

namespace {

typedef _Float16 half_t;

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

// bit index of (x, y, z)'s cell at its own cascade; < C H^3 for every input (the coordinates are clamped, a NaN gives 0)
__device__ __forceinline__ uint32_t own_cell(const MarchCfg& c, float x, float y, float z) {
    const float amax = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    const int level = cascade_of(amax, c.Cf);
    float mb, rb;
    mip_bounds(c, level, mb, rb);
    return (uint32_t)level * c.H3 + morton_encode((uint32_t)cell_coord(c, x, rb), (uint32_t)cell_coord(c, y, rb), (uint32_t)cell_coord(c, z, rb));
}

// ---- route
constexpr int IR_THREADS = 256, IR_WAVES = IR_THREADS / LAE_WAVE, IR_TRIPS = 4;
constexpr uint32_t IR_TILE = IR_THREADS * IR_TRIPS;          // rows a workgroup owns
constexpr int IR_SCAN_THREADS = 1024;                        // workgroup counts one pass of the scan takes

// the row's pre-image and whether the row is inserted
__device__ __forceinline__ bool route_row(const MarchCfg& c, const float* __restrict__ xyzs, const float* __restrict__ deltas,
                                          const uint8_t* __restrict__ sel, const uint8_t* __restrict__ occ, const Affine& A, size_t i,
                                          float& px, float& py, float& pz) {
    const float x = xyzs[3 * i], y = xyzs[3 * i + 1], z = xyzs[3 * i + 2];
    px = affine_row(A.m, x, y, z); py = affine_row(A.m + 4, x, y, z); pz = affine_row(A.m + 8, x, y, z);
    if (deltas && deltas[2 * i] == 0.0f) return false;
    if (!(fabsf(px) <= c.bound && fabsf(py) <= c.bound && fabsf(pz) <= c.bound)) return false;
    const uint32_t index = own_cell(c, px, py, pz);
    return ((sel[index >> 3] & occ[index >> 3]) >> (index & 7u)) & 1u;
}

// trip j of workgroup b covers the rows b IR_TILE + j IR_THREADS + (0 .. IR_THREADS - 1): consecutive lanes, consecutive rows
__global__ __launch_bounds__(IR_THREADS) void k_insert_mark(const float* __restrict__ xyzs, const float* __restrict__ deltas, uint32_t M,
                                                            const uint8_t* __restrict__ sel, const uint8_t* __restrict__ occ, Affine A,
                                                            MarchCfg c, int32_t* __restrict__ slot, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t wave_count[IR_TRIPS * IR_WAVES];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t rank[IR_TRIPS];
#pragma unroll
    for (int j = 0; j < IR_TRIPS; j++) {
        const size_t i = (size_t)blockIdx.x * IR_TILE + (size_t)j * IR_THREADS + threadIdx.x;
        float px, py, pz;
        const bool in = i < M && route_row(c, xyzs, deltas, sel, occ, A, i, px, py, pz);
        const uint64_t votes = __ballot(in);
        rank[j] = in ? (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)) : 0xffffffffu;
        if (lane == 0) wave_count[j * IR_WAVES + w] = (uint32_t)__popcll(votes);
    }
    __syncthreads();
    // the waves' totals stand in row order (trip-major, wave-minor): a row's rank adds the totals before its own (trip, wave)
    uint32_t total = 0, before[IR_TRIPS] = {};
#pragma unroll
    for (int k = 0; k < IR_TRIPS * IR_WAVES; k++) {
        const uint32_t v = wave_count[k];
        total += v;
#pragma unroll
        for (int j = 0; j < IR_TRIPS; j++)
            if (k < j * IR_WAVES + (int)w) before[j] += v;
    }
#pragma unroll
    for (int j = 0; j < IR_TRIPS; j++) {
        const size_t i = (size_t)blockIdx.x * IR_TILE + (size_t)j * IR_THREADS + threadIdx.x;
        if (i < M) slot[i] = rank[j] == 0xffffffffu ? -1 : (int32_t)(rank[j] + before[j]);
    }
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// one workgroup: exclusive prefix of the workgroup counts in place, *count = the sum
__global__ __launch_bounds__(IR_SCAN_THREADS) void k_insert_scan(uint32_t* __restrict__ block_counts, uint32_t nb, uint32_t* __restrict__ count) {
    __shared__ uint32_t lds[IR_SCAN_THREADS / LAE_WAVE + 1];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += IR_SCAN_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? block_counts[i] : 0u;
        uint32_t total;
        const uint32_t ex = lae::block_excl_scan<IR_SCAN_THREADS / LAE_WAVE>(v, &total, lds);
        if (i < nb) block_counts[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(IR_THREADS) void k_insert_scatter(const float* __restrict__ xyzs, const float* __restrict__ dirs, uint32_t M,
                                                               Affine A, Rot R, const uint32_t* __restrict__ block_offsets,
                                                               int32_t* __restrict__ slot, float* __restrict__ xyzs_src,
                                                               float* __restrict__ dirs_src) {
    const uint32_t off = block_offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < IR_TRIPS; j++) {
        const size_t i = (size_t)blockIdx.x * IR_TILE + (size_t)j * IR_THREADS + threadIdx.x;
        if (i >= M) continue;
        const int32_t local = slot[i];
        if (local < 0) continue;
        const size_t k = (size_t)off + (uint32_t)local;          // < *count <= M
        slot[i] = (int32_t)k;
        const float x = xyzs[3 * i], y = xyzs[3 * i + 1], z = xyzs[3 * i + 2];
        const float dx = dirs[3 * i], dy = dirs[3 * i + 1], dz = dirs[3 * i + 2];
        xyzs_src[3 * k] = affine_row(A.m, x, y, z);
        xyzs_src[3 * k + 1] = affine_row(A.m + 4, x, y, z);
        xyzs_src[3 * k + 2] = affine_row(A.m + 8, x, y, z);
        dirs_src[3 * k] = rot_row(R.r, dx, dy, dz);
        dirs_src[3 * k + 1] = rot_row(R.r + 3, dx, dy, dz);
        dirs_src[3 * k + 2] = rot_row(R.r + 6, dx, dy, dz);
    }
}

// ---- blend
template <bool HALF>
__device__ __forceinline__ float load_as_f32(const void* p, size_t i) {
    if (HALF) return (float)static_cast<const half_t*>(p)[i];
    return static_cast<const float*>(p)[i];
}

struct BlendArgs {
    const void* sigma_d; const void* rgb_d; const void* sigma_s; const void* rgb_s;
    const int32_t* slot;
    float inv_scale;
    int mode;
    float* sigma; float* rgb;
    uint32_t M, n_src;
};

// SDH, RDH, SSH, RSH: sigma_d, rgb_d, sigma_s, rgb_s is fp16 (each array has its own dtype code)
template <bool SDH, bool RDH, bool SSH, bool RSH>
__global__ __launch_bounds__(256) void k_insert_blend(BlendArgs a) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.M) return;
    const int32_t k = a.slot[i];
    float sg = load_as_f32<SDH>(a.sigma_d, i);
    float r = load_as_f32<RDH>(a.rgb_d, 3 * i), g = load_as_f32<RDH>(a.rgb_d, 3 * i + 1), b = load_as_f32<RDH>(a.rgb_d, 3 * i + 2);
    if (k >= 0 && (uint32_t)k < a.n_src) {                   // a slot the source arrays do not hold is no slot: nothing is read there
        const float ss = __fmul_rn(load_as_f32<SSH>(a.sigma_s, (size_t)k), a.inv_scale);
        const float rs = load_as_f32<RSH>(a.rgb_s, 3 * (size_t)k), gs = load_as_f32<RSH>(a.rgb_s, 3 * (size_t)k + 1),
                    bs = load_as_f32<RSH>(a.rgb_s, 3 * (size_t)k + 2);
        if (a.mode == LAE_INSERT_REPLACE) {
            sg = ss; r = rs; g = gs; b = bs;
        } else {
            sg = __fadd_rn(sg, ss);
            if (sg > 0.0f) {
                const float w = __fdiv_rn(ss, sg);
                r = __fadd_rn(r, __fmul_rn(w, __fsub_rn(rs, r)));
                g = __fadd_rn(g, __fmul_rn(w, __fsub_rn(gs, g)));
                b = __fadd_rn(b, __fmul_rn(w, __fsub_rn(bs, b)));
            }
        }
    }
    a.sigma[i] = sg;
    a.rgb[3 * i] = r; a.rgb[3 * i + 1] = g; a.rgb[3 * i + 2] = b;
}

template <bool SDH, bool RDH, bool SSH>
static void launch_blend3(bool rsh, const BlendArgs& a, hipStream_t s) {
    const uint32_t nb = lae::cdiv(a.M, 256u);
    if (rsh) k_insert_blend<SDH, RDH, SSH, true><<<nb, 256, 0, s>>>(a);
    else k_insert_blend<SDH, RDH, SSH, false><<<nb, 256, 0, s>>>(a);
}
template <bool SDH, bool RDH>
static void launch_blend2(bool ssh, bool rsh, const BlendArgs& a, hipStream_t s) {
    if (ssh) launch_blend3<SDH, RDH, true>(rsh, a, s);
    else launch_blend3<SDH, RDH, false>(rsh, a, s);
}
template <bool SDH>
static void launch_blend1(bool rdh, bool ssh, bool rsh, const BlendArgs& a, hipStream_t s) {
    if (rdh) launch_blend2<SDH, true>(ssh, rsh, a, s);
    else launch_blend2<SDH, false>(ssh, rsh, a, s);
}

// ---- occupancy
__device__ __forceinline__ bool in_inner_half(uint32_t n, uint32_t lo, uint32_t H) { return n >= lo && n < 3u * (H >> 2); }

__global__ __launch_bounds__(256) void k_insert_copy(const uint32_t* __restrict__ in, uint32_t words, uint32_t* __restrict__ out) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < words) out[w] = in[w];
}

// one SOURCE cell per thread; the cell walks its image box at every DESTINATION cascade.  cs / cd: the source's / the destination's
// grid; sshift / dshift = 3 log2(H_s) / 3 log2(H_d)
__global__ __launch_bounds__(256) void k_insert_image(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ sel, uint32_t total,
                                                      uint32_t sshift, MarchCfg cs, Affine A, float margin, uint32_t Cd, uint32_t dshift,
                                                      MarchCfg cd, uint32_t* out) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total) return;
    if (!(((occ[g >> 5] & sel[g >> 5]) >> (g & 31u)) & 1u)) return;
    const uint32_t cas = g >> sshift, m = g & ((1u << sshift) - 1u), H = 1u << (sshift / 3u);
    const uint32_t nx = morton_compact(m), ny = morton_compact(m >> 1), nz = morton_compact(m >> 2);
    // at cascade > 0 the cells strictly inside the inner half are never a point's own (the layer at H/4 is: see the header)
    if (cas > 0u && in_inner_half(nx, (H >> 2) + 1u, H) && in_inner_half(ny, (H >> 2) + 1u, H) && in_inner_half(nz, (H >> 2) + 1u, H)) return;
    float mb, rb;
    mip_bounds(cs, (int)cas, mb, rb);
    // the cell's faces, the inverse of the marcher's cell lookup: (((n / H) * 2) - 1) * mip_bound, exact in fp32
    const float fx[2] = {(((float)nx * cs.rH) * 2.0f - 1.0f) * mb, (((float)(nx + 1u) * cs.rH) * 2.0f - 1.0f) * mb};
    const float fy[2] = {(((float)ny * cs.rH) * 2.0f - 1.0f) * mb, (((float)(ny + 1u) * cs.rH) * 2.0f - 1.0f) * mb};
    const float fz[2] = {(((float)nz * cs.rH) * 2.0f - 1.0f) * mb, (((float)(nz + 1u) * cs.rH) * 2.0f - 1.0f) * mb};
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
    for (uint32_t t = 0; t < Cd; t++) {
        float tb, trb;
        mip_bounds(cd, (int)t, tb, trb);
        if (lo[0] > tb || lo[1] > tb || lo[2] > tb || hi[0] < -tb || hi[1] < -tb || hi[2] < -tb) continue;     // outside this cascade's domain
        const int x0 = cell_coord(cd, lo[0], trb), x1 = cell_coord(cd, hi[0], trb);
        const int y0 = cell_coord(cd, lo[1], trb), y1 = cell_coord(cd, hi[1], trb);
        const int z0 = cell_coord(cd, lo[2], trb), z1 = cell_coord(cd, hi[2], trb);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) {
                    const uint32_t idx = (t << dshift) + morton_encode((uint32_t)x, (uint32_t)y, (uint32_t)z);     // < Cd H_d^3: 0 <= x, y, z < H_d
                    const uint32_t bit = 1u << (idx & 31u);
                    if (!(__hip_atomic_load(out + (idx >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(out + (idx >> 5), bit);
                }
    }
}

// what every entry asks of a grid: H a power of two in [4, 128], C = 1 or 2, bound = 2^(C-1) (region.hip's rules), and, where a
// bitfield comes with it, exactly C H^3 / 8 bytes.  -> log2(H), or -1
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
// do [a, a + na) and [b, b + nb) share a byte?
static bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

}  // namespace

extern "C" {

uint64_t lae_insert_route_scratch_bytes(uint32_t M) { return (uint64_t)4 * (lae::cdiv(M, IR_TILE) + 1); }

int lae_insert_route(const float* xyzs, const float* dirs, const float* deltas, uint32_t M, const uint8_t* src_sel, const uint8_t* src_occ,
                     uint64_t src_bytes, const float* Minv, const float* Rt, float bound_s, uint32_t C_s, uint32_t H_s, int32_t* slot,
                     float* xyzs_src, float* dirs_src, uint32_t* count, void* scratch, void* stream) {
    if (!src_sel || !src_occ || !Minv || !Rt || !count) return LAE_EINVAL;
    if (M && (!xyzs || !dirs || !slot || !xyzs_src || !dirs_src || !scratch)) return LAE_EINVAL;     // (an empty array may have no address)
    if (grid_shape_ok(bound_s, C_s, H_s, src_bytes) < 0 || !finite_all(Minv, 12) || !finite_all(Rt, 9)) return LAE_EINVAL;
    if (M > 0x7fffffffu) return LAE_EINVAL;                                              // int32 slots
    const void* bases[] = {xyzs, dirs, deltas, slot, xyzs_src, dirs_src, count, scratch};
    for (const void* p : bases)
        if (!aligned(p, 4)) return LAE_EINVAL;
    // outputs alias neither an input nor one another
    const uint64_t rows3 = (uint64_t)12 * M, nscr = lae_insert_route_scratch_bytes(M);
    struct Span { const void* p; uint64_t n; };
    const Span outs[] = {{slot, (uint64_t)4 * M}, {xyzs_src, rows3}, {dirs_src, rows3}, {count, 4}, {scratch, nscr}};
    const Span ins[] = {{xyzs, rows3}, {dirs, rows3}, {deltas, deltas ? (uint64_t)8 * M : 0}, {src_sel, src_bytes}, {src_occ, src_bytes}};
    for (int a = 0; a < 5; a++) {
        for (int b = a + 1; b < 5; b++)
            if (overlap(outs[a].p, outs[a].n, outs[b].p, outs[b].n)) return LAE_EINVAL;
        for (const Span& in : ins)
            if (overlap(outs[a].p, outs[a].n, in.p, in.n)) return LAE_EINVAL;
    }
    hipStream_t s = STREAM(stream);
    if (M == 0) {
        if (hipMemsetAsync(count, 0, sizeof(uint32_t), s) != hipSuccess) return lae::check_launch("insert_route");
        return LAE_OK;
    }
    Affine A; Rot R;
    for (int i = 0; i < 12; i++) A.m[i] = Minv[i];
    for (int i = 0; i < 9; i++) R.r[i] = Rt[i];
    const MarchCfg c = make_cfg(bound_s, 0.0f, 1024, C_s, H_s);
    const uint32_t nb = lae::cdiv(M, IR_TILE);
    uint32_t* offs = static_cast<uint32_t*>(scratch);
    k_insert_mark<<<nb, IR_THREADS, 0, s>>>(xyzs, deltas, M, src_sel, src_occ, A, c, slot, offs);
    int rc = lae::check_launch("insert_route/mark");
    if (rc) return rc;
    k_insert_scan<<<1, IR_SCAN_THREADS, 0, s>>>(offs, nb, count);
    rc = lae::check_launch("insert_route/scan");
    if (rc) return rc;
    k_insert_scatter<<<nb, IR_THREADS, 0, s>>>(xyzs, dirs, M, A, R, offs, slot, xyzs_src, dirs_src);
    return lae::check_launch("insert_route/scatter");
}

int lae_insert_blend(const void* sigma_d, int sigma_d_dtype, const void* rgb_d, int rgb_d_dtype, const void* sigma_s, int sigma_s_dtype,
                     const void* rgb_s, int rgb_s_dtype, uint32_t n_src, const int32_t* slot, uint32_t M, float inv_scale, int mode,
                     float* sigma, float* rgb, void* stream) {
    if (M && (!sigma_d || !rgb_d || !slot || !sigma || !rgb)) return LAE_EINVAL;                    // (an empty array may have no address)
    if (n_src && (!sigma_s || !rgb_s)) return LAE_EINVAL;
    if (mode < LAE_INSERT_REPLACE || mode > LAE_INSERT_ADD) return LAE_EINVAL;
    if (!(inv_scale >= 0.5f && inv_scale <= 2.0f)) return LAE_EINVAL;                 // s in [0.5, 2]; a NaN fails both
    const int codes[] = {sigma_d_dtype, rgb_d_dtype, sigma_s_dtype, rgb_s_dtype};
    for (const int code : codes)
        if (code != LAE_F32 && code != LAE_F16) return LAE_EINVAL;
    const void* ptrs[] = {sigma_d, rgb_d, sigma_s, rgb_s};
    for (int k = 0; k < 4; k++)
        if (!aligned(ptrs[k], codes[k] == LAE_F16 ? 2 : 4)) return LAE_EINVAL;
    if (!aligned(slot, 4) || !aligned(sigma, 4) || !aligned(rgb, 4)) return LAE_EINVAL;
    // an output may BE the fp32 destination array it replaces; it overlaps nothing else
    const uint64_t e_sd = sigma_d_dtype == LAE_F16 ? 2 : 4, e_rd = rgb_d_dtype == LAE_F16 ? 2 : 4;
    const uint64_t e_ss = sigma_s_dtype == LAE_F16 ? 2 : 4, e_rs = rgb_s_dtype == LAE_F16 ? 2 : 4;
    const uint64_t n_sig = (uint64_t)4 * M, n_rgb = (uint64_t)12 * M;
    if (overlap(sigma, n_sig, rgb, n_rgb) || overlap(sigma, n_sig, slot, n_sig) || overlap(rgb, n_rgb, slot, n_sig)) return LAE_EINVAL;
    if (overlap(sigma, n_sig, sigma_s, e_ss * n_src) || overlap(sigma, n_sig, rgb_s, 3 * e_rs * n_src)) return LAE_EINVAL;
    if (overlap(rgb, n_rgb, sigma_s, e_ss * n_src) || overlap(rgb, n_rgb, rgb_s, 3 * e_rs * n_src)) return LAE_EINVAL;
    if (overlap(sigma, n_sig, rgb_d, 3 * e_rd * M) || overlap(rgb, n_rgb, sigma_d, e_sd * M)) return LAE_EINVAL;
    if (overlap(sigma, n_sig, sigma_d, e_sd * M) && !(sigma_d_dtype == LAE_F32 && sigma == sigma_d)) return LAE_EINVAL;
    if (overlap(rgb, n_rgb, rgb_d, 3 * e_rd * M) && !(rgb_d_dtype == LAE_F32 && rgb == rgb_d)) return LAE_EINVAL;
    if (M == 0) return LAE_OK;
    BlendArgs a{sigma_d, rgb_d, sigma_s, rgb_s, slot, inv_scale, mode, sigma, rgb, M, n_src};
    hipStream_t s = STREAM(stream);
    if (sigma_d_dtype == LAE_F16) launch_blend1<true>(rgb_d_dtype == LAE_F16, sigma_s_dtype == LAE_F16, rgb_s_dtype == LAE_F16, a, s);
    else launch_blend1<false>(rgb_d_dtype == LAE_F16, sigma_s_dtype == LAE_F16, rgb_s_dtype == LAE_F16, a, s);
    return lae::check_launch("insert_blend");
}

int lae_insert_occupancy(const uint8_t* dst_occ, uint64_t dst_bytes, const uint8_t* src_sel, const uint8_t* src_occ, uint64_t src_bytes,
                         const float* M, float margin, float bound_s, uint32_t C_s, uint32_t H_s, float bound_d, uint32_t C_d, uint32_t H_d,
                         uint8_t* out, void* stream) {
    if (!dst_occ || !src_sel || !src_occ || !M || !out) return LAE_EINVAL;
    const int lgs = grid_shape_ok(bound_s, C_s, H_s, src_bytes), lgd = grid_shape_ok(bound_d, C_d, H_d, dst_bytes);
    if (lgs < 0 || lgd < 0 || !finite_all(M, 12)) return LAE_EINVAL;
    // the margin is a rounding allowance: never a quarter of the finest destination cell (2 / H_d), let alone a whole one
    if (!(margin >= 0.0f && margin < 0.5f / (float)H_d)) return LAE_EINVAL;
    if (!aligned(dst_occ, 4) || !aligned(src_sel, 4) || !aligned(src_occ, 4) || !aligned(out, 4)) return LAE_EINVAL;
    if (overlap(out, dst_bytes, dst_occ, dst_bytes) || overlap(out, dst_bytes, src_sel, src_bytes) || overlap(out, dst_bytes, src_occ, src_bytes))
        return LAE_EINVAL;
    const uint32_t sshift = 3u * (uint32_t)lgs, dshift = 3u * (uint32_t)lgd, total = C_s << sshift, words = (C_d << dshift) >> 5;
    hipStream_t s = STREAM(stream);
    k_insert_copy<<<lae::cdiv(words, 256u), 256, 0, s>>>(reinterpret_cast<const uint32_t*>(dst_occ), words, reinterpret_cast<uint32_t*>(out));
    Affine A;
    for (int i = 0; i < 12; i++) A.m[i] = M[i];
    k_insert_image<<<lae::cdiv(total, 256u), 256, 0, s>>>(reinterpret_cast<const uint32_t*>(src_occ), reinterpret_cast<const uint32_t*>(src_sel), total,
                                                         sshift, make_cfg(bound_s, 0.0f, 1024, C_s, H_s), A, margin, C_d, dshift,
                                                         make_cfg(bound_d, 0.0f, 1024, C_d, H_d), reinterpret_cast<uint32_t*>(out));
    return lae::check_launch("insert_occupancy");
}

}  // extern "C"
