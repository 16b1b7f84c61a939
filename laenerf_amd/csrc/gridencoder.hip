// gridencoder.hip -- multiresolution hash / tiled grid encoder for gfx950.
//
// Replaces gridencoder/src/gridencoder.cu of the reference (cited per kernel).
//
// MI355X mapping: one lane = one (sample, level).  Blocks are dealt round-robin
// over the 8 XCDs (block b and b+8 share an XCD, MI355X_MICROARCH "Workgroup
// dispatch"), and each XCD has a private 4 MiB L2.  When L is a multiple of 8 the
// blockIdx -> (level, chunk) map sends all blocks of level l to XCD (l mod 8), one
// level at a time, so a hashed level's table (2 MiB fp16 / 4 MiB fp32 at T=2^19)
// is gathered out of ONE L2 instead of being replicated into all eight.
//
// Per-level scale = exp2(level*S)*H - 1 is evaluated once on the host (the
// reference evaluates exp2f per thread, gridencoder.cu:138) and passed by value;
// the oracle uses the same host libm, so fp32 results are bit-identical to it.
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include "grid_levels.h"
#include <vector>

namespace {

// accumulate r += w * v with the reference's rounding (`results[ch] += w * grid[..]`, :187): fp32 -> one FMA (nvcc
// contraction).  scalar_t = at::Half: `float * Half` is a float, and the only viable `Half += float` is
// operator+=(Half&, const Half&) -- the product is ROUNDED TO HALF first, then the two halves are added (through float,
// rounded once: exactly the correctly rounded half sum).  Checked against torch's own Half header: 0 mismatches in 2e6
// random cases, 15 % mismatches for a model that keeps the product in fp32.
__device__ __forceinline__ void accum(float& r, float w, float v) { r = fmaf(w, v, r); }
__device__ __forceinline__ void accum(half_t& r, float w, half_t v) { r = r + (half_t)(w * (float)v); }

// ---------------------------------------------------------------- K13
// gridencoder.cu:87-245.  out index = b*os_b + level*os_l + ch  ([L,B,C]: os_b=C, os_l=B*C; [B,L*C]: os_b=L*C, os_l=C)
template <typename T, int D, int C>
__global__ __launch_bounds__(GRID_BLOCK) void k_grid_fwd(
    const float* __restrict__ inputs, const T* __restrict__ grid, const int32_t* __restrict__ offsets,
    T* __restrict__ outputs, uint32_t B, uint32_t L, LevelScales sc, T* __restrict__ dy_dx, uint32_t gridtype,
    bool align_corners, uint32_t interp, uint32_t nb, bool xcd_mode, uint64_t os_b, uint64_t os_l,
    const uint32_t* __restrict__ B_dev) {
    uint32_t level, chunk;
    block_to_level_chunk(nb, xcd_mode, level, chunk);
    if (level >= L) return;
    const uint32_t b = chunk * GRID_BLOCK + threadIdx.x;
    // B_dev (frame loop): the live row count is produced on the device; B stays the capacity the strides are built from
    if (B_dev) B = min(B, *B_dev);
    if (b >= B) return;
    const LevelInfo<D> li = level_info<D>(sc, offsets, level, gridtype, align_corners);
    const T* __restrict__ tab = grid + (size_t)li.table_off * C;

    float x[D];
    bool oob = false;
#pragma unroll
    for (int d = 0; d < D; d++) {
        x[d] = (inputs[(size_t)b * D + d] + sc.in_shift) * sc.in_scale;
        oob |= (x[d] < 0.0f) | (x[d] > 1.0f);
    }
    T* out = outputs + (size_t)b * os_b + (size_t)level * os_l;
    T* dout = dy_dx ? dy_dx + (size_t)b * D * L * C + (size_t)level * D * C : nullptr;
    if (oob) {                                             // :118-135
#pragma unroll
        for (int ch = 0; ch < C; ch++) out[ch] = (T)0.0f;
        if (dout) {
#pragma unroll
            for (int i = 0; i < D * C; i++) dout[i] = (T)0.0f;
        }
        return;
    }

    float frac[D], dfrac[D];
    uint32_t pg[D];
#pragma unroll
    for (int d = 0; d < D; d++) {                          // :146-159
        float p = fmaf(x[d], li.scale, align_corners ? 0.0f : 0.5f);
        const float fl = floorf(p);
        pg[d] = (uint32_t)fl;
        p -= (float)pg[d];
        if (interp == 1) { dfrac[d] = 6 * p * (1.0f - p); p = p * p * (3.0f - 2.0f * p); }
        else dfrac[d] = 1.0f;
        frac[d] = p;
    }

    T res[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) res[ch] = (T)0.0f;
    if constexpr (D == 3 && C == 2) {
        // Corner pairs (x, x+1): the two entries are adjacent and pair-aligned whenever idx(x+1) == idx(x) ^ 1 -- on
        // hashed levels for every even x ((x ^ h) and ((x|1) ^ h) differ in bit 0 only), on dense levels for even
        // idx -- and are then fetched with ONE 8/16-byte load.  The kernel is bound by the number of cache lines the
        // texture path touches (~1 line / cycle / CU, profiles/r1_grid_fwd_pmc.txt); this removes ~25 % of them.
        // Accumulation order is unchanged (idx = x + 2y + 4z), so results stay bit-identical.
        using V2 = typename std::conditional<sizeof(T) == 2, half2_t, float2>::type;
        const V2* __restrict__ tab2 = reinterpret_cast<const V2*>(tab);
        T cv[8][2];
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
            uint32_t pl[3] = {pg[0], pg[1] + (yz & 1), pg[2] + (yz >> 1)};
            const uint32_t i0 = cell_index<D>(li, pl);
            pl[0] = pg[0] + 1;
            const uint32_t i1 = cell_index<D>(li, pl);
            V2 a, b;
            if (i1 == (i0 ^ 1u)) {
                if constexpr (sizeof(T) == 2) {
                    const uint2 w = *reinterpret_cast<const uint2*>(tab2 + (i0 & ~1u));
                    const half2_t lo = __builtin_bit_cast(half2_t, w.x), hi = __builtin_bit_cast(half2_t, w.y);
                    a = (i0 & 1u) ? hi : lo; b = (i0 & 1u) ? lo : hi;
                } else {
                    const float4 w = *reinterpret_cast<const float4*>(tab2 + (i0 & ~1u));
                    a = (i0 & 1u) ? make_float2(w.z, w.w) : make_float2(w.x, w.y);
                    b = (i0 & 1u) ? make_float2(w.x, w.y) : make_float2(w.z, w.w);
                }
            } else { a = tab2[i0]; b = tab2[i1]; }
            if constexpr (sizeof(T) == 2) { cv[2 * yz][0] = a[0]; cv[2 * yz][1] = a[1]; cv[2 * yz + 1][0] = b[0]; cv[2 * yz + 1][1] = b[1]; }
            else { cv[2 * yz][0] = a.x; cv[2 * yz][1] = a.y; cv[2 * yz + 1][0] = b.x; cv[2 * yz + 1][1] = b.y; }
        }
#pragma unroll
        for (int idx = 0; idx < 8; idx++) {
            const float w = (((idx & 1) ? frac[0] : 1 - frac[0]) * ((idx & 2) ? frac[1] : 1 - frac[1])) * ((idx & 4) ? frac[2] : 1 - frac[2]);
            accum(res[0], w, cv[idx][0]);
            accum(res[1], w, cv[idx][1]);
        }
    } else {
#pragma unroll
    for (int idx = 0; idx < (1 << D); idx++) {             // :166-191
        float w = 1.0f;
        uint32_t pgl[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            if ((idx & (1 << d)) == 0) { w *= 1 - frac[d]; pgl[d] = pg[d]; }
            else { w *= frac[d]; pgl[d] = pg[d] + 1; }
        }
        const uint32_t gi = cell_index<D>(li, pgl) * C;
        T v[C];
#pragma unroll
        for (int ch = 0; ch < C; ch++) v[ch] = tab[gi + ch];
#pragma unroll
        for (int ch = 0; ch < C; ch++) accum(res[ch], w, v[ch]);
    }
    }
    if constexpr (C == 2 && sizeof(T) == 2) {
        half2_t h = {res[0], res[1]};
        *reinterpret_cast<half2_t*>(out) = h;
    } else if constexpr (C == 2 && sizeof(T) == 4) {
        *reinterpret_cast<float2*>(out) = make_float2(res[0], res[1]);
    } else {
#pragma unroll
        for (int ch = 0; ch < C; ch++) out[ch] = res[ch];
    }

    if (dout) {                                            // :201-243
#pragma unroll
        for (int gd = 0; gd < D; gd++) {
            T rg[C];
#pragma unroll
            for (int ch = 0; ch < C; ch++) rg[ch] = (T)0.0f;
#pragma unroll
            for (int idx = 0; idx < (1 << (D - 1)); idx++) {
                float w = li.scale;
                uint32_t pgl[D];
#pragma unroll
                for (int nd = 0; nd < D - 1; nd++) {
                    const int d = (nd >= gd) ? nd + 1 : nd;
                    if ((idx & (1 << nd)) == 0) { w *= 1 - frac[d]; pgl[d] = pg[d]; }
                    else { w *= frac[d]; pgl[d] = pg[d] + 1; }
                }
                pgl[gd] = pg[gd];
                const uint32_t il = cell_index<D>(li, pgl) * C;
                pgl[gd] = pg[gd] + 1;
                const uint32_t ir = cell_index<D>(li, pgl) * C;
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    if constexpr (sizeof(T) == 2) {
                        const half_t diff = (half_t)((float)tab[ir + ch] - (float)tab[il + ch]);
                        rg[ch] = rg[ch] + (half_t)(w * (float)diff * dfrac[gd]);     // Half += float: see accum()
                    } else {
                        rg[ch] = fmaf(w * (tab[ir + ch] - tab[il + ch]), dfrac[gd], rg[ch]);   // `+=` of a product: nvcc contracts (:236)
                    }
                }
            }
#pragma unroll
            for (int ch = 0; ch < C; ch++) dout[gd * C + ch] = rg[ch];
        }
    }
}

// ---------------------------------------------------------------- K13, hot configuration
// fp16 table, D = 3, C = 2, linear interpolation, align_corners = false, hash grid type, no dy_dx: every shipped config
// (grid.py:96-161 defaults under autocast).  Same arithmetic per sample as k_grid_fwd (bit-identical results), but
//  * the three level kinds are separate, branch-free code paths selected by a block-uniform switch:
//    hashed with a power-of-two size -- the y / z hash terms cost one multiply + one add each instead of eight
//    multiplies, byte offsets are formed before the xor (no per-corner shift), whether (x, x+1) share an aligned
//    8-byte pair is decided once per lane (x even) instead of once per corner row, 32-bit offsets against a uniform
//    base; dense without wrap-around -- eight plain loads off one base index (the divergent pair path cost more than
//    it saved: an unaligned 8-byte load is issued as two), no modulo; anything else -- the generic index.
//    110 VALU instructions per (sample, level) instead of ~200: measured alone on one XCD (tools/ubench/
//    grid_fwd_variants.hip, 433 k samples) a dense level takes 15.5 us instead of 29, level 11 44 instead of 57.
//  * work is dealt to the XCDs by a host-built schedule (FwdSched) instead of the fixed (l, l + 8) pairing: a level's
//    cost is set by its vector-memory instruction issue (coarse levels) or by the L2 request rate of its XCD (fine
//    levels, one 64-byte sector per (y, z) corner row and sample: ~57 us per level and 433 k samples whatever the
//    kernel does), so whole hashed levels are packed longest-first and the cheap dense levels (tables <= 0.8 MB, harmless
//    to replicate in several L2s) fill the gaps in eighths.
struct FwdSeg { uint32_t level, c0, n, cnt; };             // chunks [c0, c0 + n) of `level`; cnt > 0: the n chunks (j / cnt) * 8 + c0 + j % cnt instead (residues c0 .. c0 + cnt - 1 mod 8)
constexpr int FWD_MAX_SEG = 12;
struct FwdSched { uint32_t nseg[8]; FwdSeg seg[8][FWD_MAX_SEG]; };

// one (sample row, level) of the lean forward: shared by k_grid_fwd_lean and by the frame loop's overflow launch below
__device__ __forceinline__ void grid_fwd_lean_row(const float* __restrict__ inputs, const half_t* __restrict__ grid, const int32_t* __restrict__ offsets,
                                                  half_t* __restrict__ outputs, const LevelScales& sc, uint64_t os_b, uint64_t os_l, uint32_t level, uint32_t b) {
#include "grid_fwd_lean_row.inc"
}

__global__ __launch_bounds__(GRID_BLOCK) void k_grid_fwd_lean(
    const float* __restrict__ inputs, const half_t* __restrict__ grid, const int32_t* __restrict__ offsets,
    half_t* __restrict__ outputs, uint32_t B, LevelScales sc, FwdSched sched, uint64_t os_b, uint64_t os_l,
    const uint32_t* __restrict__ B_dev
#ifdef LAE_GRID_FWD_LOOP_PROBE
    , uint32_t pass_chunks                                 // fault probe only (below): 0 = one trip
#endif
    ) {
    const uint32_t xcd = blockIdx.x & 7u;
#ifdef LAE_GRID_STAMPS
    const unsigned long long st_t0 = wall_clock64();
#endif
    uint32_t j = blockIdx.x >> 3, level = 0xffffffffu, chunk = 0;
    const uint32_t ns = sched.nseg[xcd];
    for (uint32_t q = 0; q < ns; q++) {
        const uint32_t n = sched.seg[xcd][q].n;
        if (j < n) {
            const uint32_t cnt = sched.seg[xcd][q].cnt;
            level = sched.seg[xcd][q].level;
            chunk = cnt ? (j / cnt) * 8u + sched.seg[xcd][q].c0 + j % cnt : sched.seg[xcd][q].c0 + j;
            break;
        }
        j -= n;
    }
    if (level == 0xffffffffu) return;
#ifndef LAE_GRID_FWD_LOOP_PROBE
    const uint32_t b = chunk * GRID_BLOCK + threadIdx.x;
    if (B_dev) B = min(B, *B_dev);
    if (b >= B) return;
    grid_fwd_lean_row(inputs, grid, offsets, outputs, sc, os_b, os_l, level, b);
#else
    // FAULT PROBE, never in the shipped library (tools/grid_loop_fault.sh builds it into tools/ubench/bin/): round 4's reverted
    // "workgroups loop over the overflow rows" form of this kernel (commit 4541188).  With the row statements inside a
    // by-reference lambda inside this loop (variant 1) a few hundred rays of a frame differed from run to run as soon as a SECOND
    // PROCESS rendered frames on the GPU -- also with one trip (pass_chunks = 0, what the probe launches); the same loop around the
    // __forceinline__ function (variant 2) never did.  Round 5 bisected the two listings (they differ in the scalar prologue's
    // schedule and in ONE vector instruction) by hand-patched assembly: the instruction is
    //       v_pk_mul_f32 v[20:21], v[6:7], v[22:23] op_sel:[0,1] op_sel_hi:[0,1]          (variant 2: v[22:23], v[6:7] op_sel:[1,0] op_sel_hi:[1,0])
    // i.e. the gfx950 packed-fp32 erratum of laenerf_amd/build.py: beside the other process's MFMA kernels the low product is
    // sometimes a.lo x 0.  Built with the compiler's defaults (--packed-fp32) the probe still shows it; built like the shipped
    // library (no packed-fp32 instructions) it is gone.
    if (B_dev) B = min(B, *B_dev);
    for (uint32_t b = chunk * GRID_BLOCK + threadIdx.x; b < B; b += pass_chunks * GRID_BLOCK) {
#if LAE_GRID_FWD_LOOP_PROBE == 2
        grid_fwd_lean_row(inputs, grid, offsets, outputs, sc, os_b, os_l, level, b);
#else
        [&]() {
#include "grid_fwd_lean_row.inc"
        }();
#endif
        if (pass_chunks == 0u) break;
    }
#endif
#ifdef LAE_GRID_STAMPS
    if (threadIdx.x == 0 && blockIdx.x < 32768u * 8u) {            // (same-address atomics per XCD stretched the launch from 50 to 290 us: plain stores, a slot per block)
        g_grid_stamps[(size_t)blockIdx.x * 4] = st_t0; g_grid_stamps[(size_t)blockIdx.x * 4 + 1] = wall_clock64(); g_grid_stamps[(size_t)blockIdx.x * 4 + 2] = level;
    }
#endif
}


// Frame loop, rows [b0, *B_dev): the rows beyond what the host EXPECTED when it sized the lean launch (its lagging bound of the rays
// alive x the n_step that bound implies).  A launch sized for the worst case -- the row budget -- had 130 k of its 216 k workgroups
// find no rows in the iterations of a 1080p frame (~0.3 ns each: 40 of 245 us).  Rows exist here only in the few iterations after
// n_step rose on the device; then one workgroup takes 256 rows through ALL levels (straight-line code, one copy per level: no
// XCD placement for these rows, and no loop around the row code -- see DESIGN.md section 8).
__global__ __launch_bounds__(GRID_BLOCK) void k_grid_fwd_lean_tail(
    const float* __restrict__ inputs, const half_t* __restrict__ grid, const int32_t* __restrict__ offsets,
    half_t* __restrict__ outputs, uint32_t B, LevelScales sc, uint32_t L, uint64_t os_b, uint64_t os_l,
    const uint32_t* __restrict__ B_dev, uint32_t b0) {
    const uint32_t b = b0 + blockIdx.x * GRID_BLOCK + threadIdx.x;
    B = min(B, *B_dev);
    if (b >= B) return;
#pragma unroll
    for (uint32_t level = 0; level < 16u; level++)
        if (level < L) grid_fwd_lean_row(inputs, grid, offsets, outputs, sc, os_b, os_l, level, b);
}
// [L][B][2] -> [B][L][2] through an LDS tile: the gather kernel writes level-major (each level's block stores 256
// consecutive pairs = full lines); storing 4 B per lane at a 64 B stride straight into [B, L*2] measured 123 MB of
// HBM writes for 16 MB of output (profiles/r1_pmc_fetch_write_per_kernel.csv).
template <typename T>
__global__ __launch_bounds__(256) void k_out_transpose(const T* __restrict__ in, T* __restrict__ out, uint32_t B, uint32_t L) {
    using V = typename std::conditional<sizeof(T) == 2, uint32_t, uint2>::type;
    __shared__ V tile[256 * 33];
    const uint32_t b0 = blockIdx.x * 256;
    const uint32_t nb = min(256u, B - b0);
    const V* src = reinterpret_cast<const V*>(in);
    for (uint32_t e = threadIdx.x; e < nb * L; e += 256) {
        const uint32_t l = e / nb, b = e % nb;
        tile[b * (L + 1) + l] = src[(size_t)l * B + b0 + b];
    }
    __syncthreads();
    V* dstv = reinterpret_cast<V*>(out) + (size_t)b0 * L;
    for (uint32_t e = threadIdx.x; e < nb * L; e += 256) dstv[e] = tile[(e / L) * (L + 1) + (e % L)];
}

// ---------------------------------------------------------------- input gradient without dy_dx (lae_grid_input_grad)
// d loss / d x of the samples from the level-major feature gradients [L, M, 2] (what lae_nerf_field_backward leaves in grad_enc), for
// the fp16 table, D = 3, C = 2, linear interpolation.  K13 + K15 need a dy_dx buffer of L * D * C values per sample and sum in fp16;
// here every (sample, level) recomputes its cell and fractional position with the forward's statements (level_info, cell_index, the
// fmaf of k_grid_fwd), gathers the forward's eight corners again and sums, per axis gd and in fp32,
//     scale * w(other two axes) * (table[right] - table[left]) * grad_feats[l, b, ch]      over the 4 corner pairs and 2 channels.
// Layout: a workgroup owns IG_ROWS = 64 consecutive samples; lane = sample, wave w takes the levels w, w + IG_WAVES, ... (a coarse and
// a fine level for L = 16, as the (l, l + 8) pairing of k_grid_fwd), so that every load of x and of grad_feats is one contiguous run
// per wave and all lanes of a wave gather from the same level's table.  The waves' partial sums meet in LDS and wave 0 adds them in
// wave order: one owner per output row, no atomics, the same bits on every run.  A row outside [0,1]^3 gives zeros (the forward's rule).
constexpr int IG_ROWS = 64, IG_WAVES = 8;

__global__ __launch_bounds__(IG_ROWS * IG_WAVES) void k_grid_input_grad(
    const float* __restrict__ inputs, const half_t* __restrict__ grid, const int32_t* __restrict__ offsets,
    const half_t* __restrict__ grad_feats, float* __restrict__ grad_x, uint32_t M, uint32_t L, LevelScales sc, uint32_t gridtype,
    bool align_corners) {
    __shared__ float part[IG_WAVES][3][IG_ROWS];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t b = blockIdx.x * IG_ROWS + lane;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (b < M) {
        float x01[3];
        bool oob = false;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            x01[d] = (inputs[(size_t)b * 3 + d] + sc.in_shift) * sc.in_scale;
            oob |= (x01[d] < 0.0f) | (x01[d] > 1.0f);
        }
        if (!oob) {
            for (uint32_t level = wave; level < L; level += IG_WAVES) {
                const LevelInfo<3> li = level_info<3>(sc, offsets, level, gridtype, align_corners);
                const uint32_t* __restrict__ tab = reinterpret_cast<const uint32_t*>(grid) + li.table_off;   // one word = the entry's two halves
                float fr[3];
                uint32_t pg[3];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const float p = fmaf(x01[d], li.scale, align_corners ? 0.0f : 0.5f);
                    pg[d] = (uint32_t)floorf(p);
                    fr[d] = p - (float)pg[d];
                }
                float v[8][2];                             // corner idx = x + 2y + 4z
#pragma unroll
                for (int idx = 0; idx < 8; idx++) {
                    const uint32_t pl[3] = {pg[0] + (idx & 1), pg[1] + ((idx >> 1) & 1), pg[2] + (idx >> 2)};
                    const half2_t h = __builtin_bit_cast(half2_t, tab[cell_index<3>(li, pl)]);
                    v[idx][0] = (float)h[0]; v[idx][1] = (float)h[1];
                }
                const half2_t gh = *reinterpret_cast<const half2_t*>(grad_feats + ((size_t)level * M + b) * 2);
                const float g0 = (float)gh[0], g1 = (float)gh[1];
#pragma unroll
                for (int gd = 0; gd < 3; gd++) {
                    const int da = gd == 0 ? 1 : 0, db = gd == 2 ? 1 : 2;              // the other two axes, in order
#pragma unroll
                    for (int pr = 0; pr < 4; pr++) {
                        const float wa = (pr & 1) ? fr[da] : 1.0f - fr[da];
                        const float wb = (pr & 2) ? fr[db] : 1.0f - fr[db];
                        const float w = li.scale * (wa * wb);
                        const int il = ((pr & 1) << da) | (((pr >> 1) & 1) << db), ir = il | (1 << gd);
                        acc[gd] = fmaf(w, (v[ir][0] - v[il][0]) * g0, acc[gd]);
                        acc[gd] = fmaf(w, (v[ir][1] - v[il][1]) * g1, acc[gd]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) part[wave][d][lane] = acc[d];
    __syncthreads();
    if (wave == 0 && b < M) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
            float s = part[0][d][lane];
#pragma unroll
            for (int w = 1; w < IG_WAVES; w++) s += part[w][d][lane];
            grad_x[(size_t)b * 3 + d] = s * sc.in_scale;
        }
    }
}

// ---------------------------------------------------------------- K16
// gridencoder.cu:506-610 (fp32 only: grid.py:165 runs it with autocast disabled)
template <int D, int C>
__global__ __launch_bounds__(GRID_BLOCK) void k_grad_tv(const float* __restrict__ inputs, const float* __restrict__ grid,
                                                         float* __restrict__ grad, const int32_t* __restrict__ offsets,
                                                         float weight, uint32_t B, uint32_t L, LevelScales sc,
                                                         uint32_t gridtype, bool align_corners, uint32_t nb) {
    uint32_t level, chunk;
    block_to_level_chunk(nb, false, level, chunk);
    if (level >= L) return;
    const uint32_t b = chunk * GRID_BLOCK + threadIdx.x;
    if (b >= B) return;
    const LevelInfo<D> li = level_info<D>(sc, offsets, level, gridtype, align_corners);
    const float* tab = grid + (size_t)li.table_off * C;
    float* gtab = grad + (size_t)li.table_off * C;
    uint32_t pg[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        const float xv = inputs[(size_t)b * D + d];
        if (xv < 0.0f || xv > 1.0f) return;
        pg[d] = (uint32_t)floorf(fmaf(xv, li.scale, align_corners ? 0.0f : 0.5f));
    }
    float res[C], idelta[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) { res[ch] = 0; idelta[ch] = 0; }
    const uint32_t index = cell_index<D>(li, pg) * C;
    const float w = weight / (float)(2 * D);
#pragma unroll
    for (int d = 0; d < D; d++) {
        const uint32_t cur = pg[d];
        if (cur < li.resolution) {
            pg[d] = cur + 1;
            const uint32_t ir = cell_index<D>(li, pg) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) { const float gv = tab[index + ch] - tab[ir + ch]; res[ch] += gv; idelta[ch] += gv * gv; }
        }
        if (cur > 0) {
            pg[d] = cur - 1;
            const uint32_t il = cell_index<D>(li, pg) * C;
#pragma unroll
            for (int ch = 0; ch < C; ch++) { const float gv = tab[index + ch] - tab[il + ch]; res[ch] += gv; idelta[ch] += gv * gv; }
        }
        pg[d] = cur;
    }
#pragma unroll
    for (int ch = 0; ch < C; ch++) atomicAdd(gtab + index + ch, w * res[ch] * (1.0f / sqrtf(idelta[ch] + 1e-9f)));
}

// ---------------------------------------------------------------- host dispatch
struct FwdArgs {
    const float* inputs; const void* emb; const int32_t* offsets; void* out; uint32_t B, L; LevelScales sc;
    void* dy_dx; uint32_t gridtype; bool align; uint32_t interp; uint64_t os_b, os_l; hipStream_t stream;
    const uint32_t* B_dev = nullptr; uint32_t B_launch = 0;     // frame loop: device-side row count, host bound for the launch
    uint32_t B_likely = 0;                                      // frame loop: the rows the host expects (<= B_launch): the scheduled launch covers them, k_grid_fwd_lean_tail the rest
    const int32_t* offsets_host = nullptr;                      // the caller's host copy of `offsets` (L + 1 ints) or NULL
    const float* level_cost = nullptr;                          // frame loop: measured per-level chunk costs (balance only) or NULL
};

// ---- schedule of k_grid_fwd_lean (see the kernel's header).  Relative cost of one chunk of a level, calibrated on the
// bench batches (tools/ubench/grid_fwd_variants.hip, then a sweep with tools/grid_fwd_bench.py on one-view and 16-view
// batches): dense 1; hashed 1.25 up to resolution ~80, rising with log2(resolution) to 2.3 at ~550 (consecutive samples of a
// ray stop sharing cache lines) and 4.5 from ~1000 on (every corner row is its own L2 request).  Only the balance depends on it, never a result.
// (round 3, tools/grid_fwd_spans.py -- per-block stamps of one launch: with this table the XCDs end at 38.5-41 us (one finest level
// each) and 45-47 us (two middle levels + dense eighths); a table re-fitted to those spans (middle levels 2.0-2.9 instead of
// 1.4-2.4) moves the late end to the XCDs that carry levels 11 / 12 + dense eighths and the launch still spans 46.5 us: two levels
// sharing an XCD overlap better than their solo costs add up, and the dense eighths run last on every XCD.  Kept as calibrated.)
static float fwd_level_cost(bool hashed, uint32_t resolution) {
    if (!hashed) return 1.0f;
    const float lr = log2f((float)resolution);
    if (lr <= 6.3f) return 1.25f;
    if (lr <= 9.1f) return 1.25f + (lr - 6.3f) * (1.05f / 2.8f);
    if (lr <= 10.0f) return 2.3f + (lr - 9.1f) * (2.2f / 0.9f);
    return 4.5f;
}
// The same for a FRAME's rows (ray-major: neighbouring rows are neighbouring samples of one ray, neighbouring rays neighbouring
// pixels), from per-block stamps of frame-loop launches (tools/frame_grid_spans.py, profiles/r4_frame_grid_spans.txt): a level
// alone on an XCD took 27 / 32 / 33 / 39 / 40 / 44 / 46 / 54 / 58 / 71 / 83 us for resolutions 80 ... 2048 and a dense level 21 --
// the finest levels cost 2.8-4x a dense one, not 4.5x, and rise steadily instead of jumping at ~1000: with the training table
// the XCDs that carry ONE fine level finished at 58 / 71 us of an 87 us launch.
static float fwd_level_cost_frame(bool hashed, uint32_t resolution) {
    if (!hashed) return 1.0f;
    const float lr = log2f((float)resolution);
    if (lr <= 6.3f) return 1.29f;
    if (lr <= 9.1f) return 1.29f + (lr - 6.3f) * (0.91f / 2.8f);
    if (lr <= 11.0f) return 2.2f + (lr - 9.1f) * (1.75f / 1.9f);
    static const float top_slope = [] { const char* e = getenv("LAE_GRID_FWD_FRAME_SLOPE"); return e ? (float)atof(e) : 0.5f; }();   // beyond resolution 2048 (bound-2 scenes: finest levels 2819 / 4096) the rise flattens: slope 0.92 / 0.5 / 0.2 / 0 -> 1080p frame 60.8 / 59.7 / 59.9 / 61.4 ms
    return 3.95f + (lr - 11.0f) * top_slope;
}
static int g_fwd_frame_sched = -1;                         // LAE_GRID_FWD_FRAME_SCHED: 0 training table, 1 (default) frame table, 2 frame table + the costliest levels in halves
// (measured, 800x800 / 1080p / one rank's shard of it: 0: 10.9 / 67.2 / 11.15 ms, 1: 10.95 / 62.2 / 10.9, 2: 11.1 / 63.7 / 10.9 -- a level in two
// halves costs 2 x 48 us against 83 whole: its table then streams into two L2s)
static void fwd_sched_default(FwdSched& fs, uint32_t L, uint32_t nb) {     // level l on XCD l mod 8, one level at a time
    for (int x = 0; x < 8; x++) fs.nseg[x] = 0;
    for (uint32_t l = 0; l < L; l++) {
        const uint32_t x = l & 7u;
        fs.seg[x][fs.nseg[x]++] = FwdSeg{l, 0u, nb, 0u};
    }
}
// returns the largest number of blocks any XCD owns
static uint32_t fwd_sched_build(FwdSched& fs, uint32_t L, uint32_t nb, const LevelScales& sc, const int32_t* offs, bool frame = false,
                                const float* cost_override = nullptr) {
    bool ok = offs != nullptr && L <= 32 && nb >= 64;
    float cost[MAX_LEVELS]; bool dense[MAX_LEVELS];
    if (g_fwd_frame_sched < 0) { const char* e = getenv("LAE_GRID_FWD_FRAME_SCHED"); g_fwd_frame_sched = e ? atoi(e) : 1; }
    const int fmode = frame ? g_fwd_frame_sched : 0;
    if (ok) {
        float total = 0.f;
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t res = (uint32_t)ceilf(sc.scale[l]) + 1;
            const uint64_t size = (uint64_t)(offs[l + 1] - offs[l]);
            const uint64_t full = (uint64_t)(res + 1) * (res + 1) * (res + 1);
            dense[l] = full <= size;
            cost[l] = fmode ? fwd_level_cost_frame(!dense[l], res) : fwd_level_cost(!dense[l], res);
            if (frame && cost_override) cost[l] = cost_override[l];
            total += cost[l];
        }
        // a whole hashed level is one item (its 2 MB table then lives in ONE L2); in a frame a level that alone exceeds an XCD's
        // fair share would set the launch's span, so it goes out as two halves of its chunk range (two L2s hold its table)
        struct Item { float cost; uint32_t level; bool piece; uint32_t c0, n; };
        std::vector<Item> items;
        const uint32_t piece = lae::cdiv(nb, 8u);
        for (uint32_t l = 0; l < L; l++) {
            if (!dense[l]) {
                if (fmode == 2 && cost[l] > 0.97f * total / 8.0f) {
                    const uint32_t h = nb / 2;
                    items.push_back(Item{cost[l] * h, l, false, 0u, h});
                    items.push_back(Item{cost[l] * (nb - h), l, false, h, nb - h});
                } else items.push_back(Item{cost[l] * nb, l, false, 0u, nb});
            }
            else for (uint32_t k = 0; k < 8 && k * piece < nb; k++) items.push_back(Item{cost[l] * std::min(piece, nb - k * piece), l, true, 0u, 0u});
        }
        std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.cost > b.cost; });
        float load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t pieces[8][MAX_LEVELS] = {};
        for (int x = 0; x < 8; x++) fs.nseg[x] = 0;
        for (const Item& it : items) {
            int best = 0;
            for (int x = 1; x < 8; x++) if (load[x] < load[best]) best = x;
            load[best] += it.cost;
            if (it.piece) pieces[best][it.level]++;
            else if (fs.nseg[best] < FWD_MAX_SEG) fs.seg[best][fs.nseg[best]++] = FwdSeg{it.level, it.c0, it.n, 0u};
            else ok = false;
        }
        for (uint32_t l = 0; l < L && ok; l++) {
            if (!dense[l]) continue;
            uint32_t c0 = 0;
            if (fmode) {
                // a frame's launch is sized by a host BOUND of the row count: the chunks beyond the live rows are empty, and with
                // contiguous eighths the XCDs holding the last ones would idle while the first ones do all of a dense level
                // (1080p frame: 86-93 us of dense work on two XCDs, 6 on another) -- an XCD takes every 8th chunk instead
                for (int x = 0; x < 8; x++) {
                    if (!pieces[x][l]) continue;
                    if (fs.nseg[x] < FWD_MAX_SEG) fs.seg[x][fs.nseg[x]++] = FwdSeg{l, c0, lae::cdiv(nb, 8u) * pieces[x][l], pieces[x][l]}; else ok = false;
                    c0 += pieces[x][l];
                }
                if (c0 != std::min(8u, lae::cdiv(nb, piece))) ok = false;
                continue;
            }
            for (int x = 0; x < 8; x++) {
                if (!pieces[x][l]) continue;
                const uint32_t n = std::min(pieces[x][l] * piece, nb - c0);
                if (fs.nseg[x] < FWD_MAX_SEG) fs.seg[x][fs.nseg[x]++] = FwdSeg{l, c0, n, 0u}; else ok = false;
                c0 += n;
            }
            if (c0 != nb) ok = false;
        }
    }
    if (!ok) fwd_sched_default(fs, L, nb);
    uint32_t mx = 0;
    for (int x = 0; x < 8; x++) {
        uint32_t t = 0;
        for (uint32_t q = 0; q < fs.nseg[x]; q++) t += fs.seg[x][q].n;
        mx = std::max(mx, t);
    }
    return mx;
}
static int g_fwd_mode = 0;                                 // 0: lean kernel + balanced schedule, 1: lean + (l, l+8) map, 2: generic kernel

template <typename T, int D, int C>
static void launch_fwd(const FwdArgs& a) {
    const uint32_t nb_safe = lae::cdiv(a.B_dev ? a.B_launch : a.B, GRID_BLOCK);
    // frame, lean kernel: the scheduled launch is sized for the expected rows (a multiple of 8 chunks: strided dense pieces)
    // -- when that spares enough workgroups to pay for the second launch (~4 us in the iteration's chain against ~0.3 ns per
    // workgroup that finds no rows, L of them per chunk: from ~2000 chunks on; an 800x800 frame stays with one launch)
    static const uint32_t tail_min_chunks = [] { const char* e = getenv("LAE_GRID_FWD_TAIL_MIN"); return e ? (uint32_t)atoi(e) : 2048u; }();
    uint32_t nb = a.B_dev && a.B_likely ? std::min((lae::cdiv(a.B_likely, GRID_BLOCK) + 7u) / 8u * 8u, nb_safe) : nb_safe;
    if (nb_safe - nb < tail_min_chunks) nb = nb_safe;
    if constexpr (std::is_same<T, half_t>::value && D == 3 && C == 2) {
        if (g_fwd_mode != 2 && !a.dy_dx && a.interp == 0 && !a.align && a.gridtype == 0 && a.L <= 8 * FWD_MAX_SEG && a.L <= MAX_LEVELS) {
            FwdSched fs;
            static const std::vector<float> env_cost = [] {      // probe: LAE_GRID_FWD_COSTS="c0,c1,...": per-level chunk costs of frame launches
                std::vector<float> v; const char* e = getenv("LAE_GRID_FWD_COSTS");
                while (e && *e) { char* end; v.push_back(strtof(e, &end)); if (end == e) break; e = *end ? end + 1 : end; }
                return v; }();
            const float* co = a.level_cost ? a.level_cost : (env_cost.size() >= a.L ? env_cost.data() : nullptr);
            const uint32_t per_xcd = fwd_sched_build(fs, a.L, nb, a.sc, g_fwd_mode == 0 ? a.offsets_host : nullptr, a.B_dev != nullptr, co);
            k_grid_fwd_lean<<<per_xcd * 8, GRID_BLOCK, 0, a.stream>>>(a.inputs, (const half_t*)a.emb, a.offsets, (half_t*)a.out, std::min(a.B, nb * (uint32_t)GRID_BLOCK), a.sc,
                                                                      fs, a.os_b, a.os_l, a.B_dev
#ifdef LAE_GRID_FWD_LOOP_PROBE
                                                                      , 0u
#endif
                                                                      );
            if (nb < nb_safe)                                  // rows beyond the expected ones, if the device has any
                k_grid_fwd_lean_tail<<<nb_safe - nb, GRID_BLOCK, 0, a.stream>>>(a.inputs, (const half_t*)a.emb, a.offsets, (half_t*)a.out, a.B, a.sc, a.L,
                                                                                 a.os_b, a.os_l, a.B_dev, nb * (uint32_t)GRID_BLOCK);
            return;
        }
    }
    const bool xcd = (a.L % 8) == 0;
    k_grid_fwd<T, D, C><<<nb_safe * a.L, GRID_BLOCK, 0, a.stream>>>(a.inputs, (const T*)a.emb, a.offsets, (T*)a.out, a.B, a.L,
                                                                a.sc, (T*)a.dy_dx, a.gridtype, a.align, a.interp, nb_safe,
                                                                xcd, a.os_b, a.os_l, a.B_dev);
}
template <typename T, int D>
static int dispatch_fwd_c(const FwdArgs& a, uint32_t C) {
    switch (C) {
        case 1: launch_fwd<T, D, 1>(a); return LAE_OK;
        case 2: launch_fwd<T, D, 2>(a); return LAE_OK;
        case 4: launch_fwd<T, D, 4>(a); return LAE_OK;
        case 8: launch_fwd<T, D, 8>(a); return LAE_OK;
        default: return LAE_EINVAL;     // gridencoder.cu:381 "C must be 1, 2, 4, or 8"
    }
}
template <typename T>
static int dispatch_fwd_d(const FwdArgs& a, uint32_t D, uint32_t C) {
    switch (D) {
        case 2: return dispatch_fwd_c<T, 2>(a, C);
        case 3: return dispatch_fwd_c<T, 3>(a, C);
        case 4: return dispatch_fwd_c<T, 4>(a, C);
        case 5: return dispatch_fwd_c<T, 5>(a, C);
        default: return LAE_EINVAL;     // gridencoder.cu:398
    }
}

static int grid_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B,
                        uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx, uint32_t gridtype,
                        int align_corners, uint32_t interp, int dtype, bool blc, void* stream, float in_shift = 0.0f,
                        float in_scale = 1.0f, const int32_t* offsets_host = nullptr) {
    if (B == 0) return LAE_OK;
    if (!inputs || !embeddings || !offsets || !outputs) return LAE_ENULL;
    if (gridtype > 1 || interp > 1) return LAE_EINVAL;
    FwdArgs a;
    a.offsets_host = offsets_host;
    a.inputs = inputs; a.emb = embeddings; a.offsets = offsets; a.out = outputs; a.B = B; a.L = L;
    int rc = fill_scales(a.sc, L, S, H);
    if (rc) return rc;
    a.sc.in_shift = in_shift; a.sc.in_scale = in_scale;
    a.dy_dx = dy_dx; a.gridtype = gridtype; a.align = align_corners != 0; a.interp = interp;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    if (dtype != LAE_F32 && dtype != LAE_F16) return LAE_EINVAL;
    // [B, L*C] output with C == 2: gather level-major into the workspace, then one tiled transpose
    const bool staged = blc && C == 2 && L <= 32;
    void* lbc = nullptr;
    if (staged) {
        lbc = lae::workspace(lae::WS_GRID_OUT_T, (size_t)B * L * C * (dtype == LAE_F16 ? 2 : 4), a.stream);
        if (!lbc) return LAE_ELAUNCH;
        a.out = lbc;
    }
    const bool level_major = !blc || staged;
    a.os_b = level_major ? C : (uint64_t)L * C;
    a.os_l = level_major ? (uint64_t)B * C : C;
    if (dtype == LAE_F32) rc = dispatch_fwd_d<float>(a, D, C);
    else rc = dispatch_fwd_d<half_t>(a, D, C);
    if (rc) return rc;
    if (staged) {
        if (dtype == LAE_F16) k_out_transpose<half_t><<<lae::cdiv(B, 256), 256, 0, a.stream>>>((const half_t*)lbc, (half_t*)outputs, B, L);
        else k_out_transpose<float><<<lae::cdiv(B, 256), 256, 0, a.stream>>>((const float*)lbc, (float*)outputs, B, L);
    }
    return lae::check_launch("grid_encode_forward");
}

template <int D>
static int tv_c(const float* inputs, const float* emb, float* grad, const int32_t* offsets, float weight, uint32_t B,
                uint32_t C, uint32_t L, const LevelScales& sc, uint32_t gridtype, bool align, hipStream_t s) {
    const uint32_t nb = lae::cdiv(B, GRID_BLOCK);
    switch (C) {
        case 1: k_grad_tv<D, 1><<<nb * L, GRID_BLOCK, 0, s>>>(inputs, emb, grad, offsets, weight, B, L, sc, gridtype, align, nb); break;
        case 2: k_grad_tv<D, 2><<<nb * L, GRID_BLOCK, 0, s>>>(inputs, emb, grad, offsets, weight, B, L, sc, gridtype, align, nb); break;
        case 4: k_grad_tv<D, 4><<<nb * L, GRID_BLOCK, 0, s>>>(inputs, emb, grad, offsets, weight, B, L, sc, gridtype, align, nb); break;
        case 8: k_grad_tv<D, 8><<<nb * L, GRID_BLOCK, 0, s>>>(inputs, emb, grad, offsets, weight, B, L, sc, gridtype, align, nb); break;
        default: return LAE_EINVAL;
    }
    return LAE_OK;
}

}  // namespace

// frame loop (frame.hip lae_render_frame): fp16 table, D=3, C=2, level-major output [L, B_cap, 2]; rows beyond
// *B_dev are not touched.  B_launch = host upper bound of *B_dev (sizes the launch only).
int lae::grid_forward_frame(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs, uint32_t B_cap,
                            uint32_t B_launch, const uint32_t* B_dev, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                            int align_corners, uint32_t interp, float in_shift, float in_scale, hipStream_t stream,
                            const int32_t* offsets_host, uint32_t B_likely) {
    if (B_launch == 0) return LAE_OK;
    FwdArgs a;
    a.offsets_host = offsets_host;
    a.inputs = inputs; a.emb = embeddings; a.offsets = offsets; a.out = outputs; a.B = B_cap; a.L = L;
    int rc = fill_scales(a.sc, L, S, H);
    if (rc) return rc;
    a.sc.in_shift = in_shift; a.sc.in_scale = in_scale;
    a.dy_dx = nullptr; a.gridtype = gridtype; a.align = align_corners != 0; a.interp = interp;
    a.stream = stream; a.os_b = 2; a.os_l = (uint64_t)B_cap * 2;
    a.B_dev = B_dev; a.B_launch = std::min(B_launch, B_cap); a.B_likely = std::min(B_likely, a.B_launch);
    launch_fwd<half_t, 3, 2>(a);
    return LAE_OK;
}

extern "C" {

int lae_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                            uint32_t gridtype, int align_corners, uint32_t interp, int dtype, void* stream) {
    return grid_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners, interp,
                        dtype, false, stream);
}
int lae_grid_encode_forward_ex(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                               uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                               uint32_t gridtype, int align_corners, uint32_t interp, int dtype, int blc, float in_shift,
                               float in_scale, const int32_t* offsets_host, void* stream) {
    return grid_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners, interp,
                        dtype, blc != 0, stream, in_shift, in_scale, offsets_host);
}
int lae_grid_input_grad(const float* inputs, const void* embeddings, const int32_t* offsets, const void* grad_feats, float* grad_x,
                        uint32_t M, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                        uint32_t interp, int dtype, float in_shift, float in_scale, void* stream) {
    if (D != 3 || C != 2 || dtype != LAE_F16 || interp != LAE_INTERP_LINEAR || gridtype > 1) return LAE_EINVAL;
    LevelScales sc;
    if (const int rc = fill_scales(sc, L, S, H)) return rc;                     // L = 0 or L > 32
    if (M == 0) return LAE_OK;
    if (!inputs || !embeddings || !offsets || !grad_feats || !grad_x) return LAE_ENULL;
    sc.in_shift = in_shift; sc.in_scale = in_scale;
    hipLaunchKernelGGL(k_grid_input_grad, dim3(lae::cdiv(M, IG_ROWS)), dim3(IG_ROWS * IG_WAVES), 0, reinterpret_cast<hipStream_t>(stream),
                       inputs, (const half_t*)embeddings, offsets, (const half_t*)grad_feats, grad_x, M, L, sc, gridtype,
                       align_corners != 0);
    return lae::check_launch("grid_input_grad");
}

int lae_grid_forward_schedule(const int32_t* offsets_host, uint32_t L, float S, uint32_t H, uint32_t n_chunks, uint32_t* nseg_out,
                              uint32_t* segs_out) {
    if (!offsets_host || !nseg_out || !segs_out) return LAE_ENULL;
    LevelScales sc;
    if (fill_scales(sc, L, S, H) != LAE_OK || L > 8 * FWD_MAX_SEG) return LAE_EINVAL;
    FwdSched fs;
    const uint32_t per_xcd = fwd_sched_build(fs, L, n_chunks, sc, offsets_host);
    for (int x = 0; x < 8; x++) {
        nseg_out[x] = fs.nseg[x];
        for (uint32_t q = 0; q < fs.nseg[x]; q++) {
            uint32_t* o = segs_out + ((size_t)x * FWD_MAX_SEG + q) * 3;
            o[0] = fs.seg[x][q].level; o[1] = fs.seg[x][q].c0; o[2] = fs.seg[x][q].n;
        }
    }
    return (int)per_xcd;
}

int lae_grid_set_forward_mode(int mode) {
    if (mode < 0 || mode > 2) return LAE_EINVAL;
    g_fwd_mode = mode;
    return LAE_OK;
}

int lae_grad_total_variation(const void* inputs, const void* embeddings, void* grad, const int32_t* offsets,
                             float weight, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             uint32_t gridtype, int align_corners, int dtype, void* stream) {
    if (B == 0) return LAE_OK;
    if (!inputs || !embeddings || !grad || !offsets) return LAE_ENULL;
    if (dtype != LAE_F32 || gridtype > 1) return LAE_EINVAL;
    LevelScales sc;
    int rc = fill_scales(sc, L, S, H);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool al = align_corners != 0;
    const float* in = (const float*)inputs; const float* e = (const float*)embeddings; float* g = (float*)grad;
    switch (D) {
        case 2: rc = tv_c<2>(in, e, g, offsets, weight, B, C, L, sc, gridtype, al, s); break;
        case 3: rc = tv_c<3>(in, e, g, offsets, weight, B, C, L, sc, gridtype, al, s); break;
        case 4: rc = tv_c<4>(in, e, g, offsets, weight, B, C, L, sc, gridtype, al, s); break;
        case 5: rc = tv_c<5>(in, e, g, offsets, weight, B, C, L, sc, gridtype, al, s); break;
        default: rc = LAE_EINVAL;
    }
    if (rc) return rc;
    return lae::check_launch("grad_total_variation");
}

}  // extern "C"

#ifdef LAE_GRID_STAMPS
GRID_STAMPS_READER(lae_debug_grid_stamps)
#endif
