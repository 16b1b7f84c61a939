// gridbackward.hip -- backward of the multiresolution hash / tiled grid encoder for gfx950 (forward: gridencoder.hip).
//
// Replaces kernel_grid_backward / kernel_input_backward of gridencoder/src/gridencoder.cu of the reference (cited per kernel).
// Two forms: k_grid_bwd, the reference's scatter with global atomics (any D, C), and for D = 3, C = 2 the binned pipeline
// k_bwd_walk<COUNT> -> scans -> k_bwd_walk<FILL> -> k_bwd_acc, which routes the contributions to the owners of table partitions and
// needs no global float atomics.  lae_nerf_field_backward runs the MLP head's backward in front of it and lets the reduction of
// the weight gradients ride in the accumulate pass.
#include <stdlib.h>
#include <algorithm>
#include <mutex>
#include <vector>
#include "grid_levels.h"
#include "dw_reduce.h"

namespace {

// ---------------------------------------------------------------- K14
// gridencoder.cu:248-340: scatter w*grad into grad_grid.  v1: one no-return atomic per
// (corner, channel pair): global_atomic_add_f32 / global_atomic_pk_add_f16.
// ---- constants and predicates of the binned backward (defined here because the generic kernel below is its companion)
constexpr uint32_t PART_SHIFT = 12, PART = 1u << PART_SHIFT;   // table entries per partition (= per accumulate workgroup)
constexpr uint32_t BK_MAX = 512;              // partitions per level the binned path handles (level size <= 2^21 entries)
constexpr uint32_t BK_TARGET = 32;            // target workgroups per level (levels with fewer partitions are split into sub-ranges).  Round 4: 16 -> 32
                                              // (same-box A/B, 16 / 32 / 64: lego step 0.3514 / 0.3508 / 0.3547 ms, style step 0.396 / 0.367 / 0.368, flower step 0.700 / 0.666 / 0.647:
                                              // the smallest levels' few cells take every sample's LDS atomics, more sub-ranges spread them over more CUs)

struct LevelBins { uint32_t P, SUB; };
__host__ __device__ __forceinline__ LevelBins level_bins_of(uint32_t hashmap_size, uint32_t bk_target = BK_TARGET) {
    LevelBins lb;
    lb.P = (hashmap_size + PART - 1) >> PART_SHIFT;
    lb.SUB = lb.P >= bk_target ? 1u : (bk_target + lb.P - 1) / lb.P;
    return lb;
}
// A level goes through the binned pipeline when its partitions fit the directory rows; anything larger is left to the
// generic atomic kernel.
__host__ __device__ __forceinline__ bool level_is_binned(uint32_t hashmap_size) { return level_bins_of(hashmap_size).P <= BK_MAX; }


template <typename T, int D, int C>
__global__ __launch_bounds__(GRID_BLOCK) void k_grid_bwd(
    const T* __restrict__ grad, const float* __restrict__ inputs, const int32_t* __restrict__ offsets,
    T* __restrict__ grad_grid, uint32_t B, uint32_t L, LevelScales sc, uint32_t gridtype, bool align_corners,
    uint32_t interp, uint32_t nb, bool xcd_mode, uint64_t gs_b, uint64_t gs_l, bool only_unbinned,
    uint32_t* __restrict__ grad_dirty = nullptr) {
    // the accumulator's "dirty" word (see k_bwd_walk<FILL>): these atomics add on top of whatever is there and leave it non-zero
    if (grad_dirty && blockIdx.x == 0 && threadIdx.x == 0) *grad_dirty = 1u;
    uint32_t level, chunk;
    block_to_level_chunk(nb, xcd_mode, level, chunk);
    if (level >= L) return;
    const uint32_t b = chunk * GRID_BLOCK + threadIdx.x;
    if (b >= B) return;
    const LevelInfo<D> li = level_info<D>(sc, offsets, level, gridtype, align_corners);
    if (only_unbinned) {      // companion of the binned fast path: only the levels it leaves out
        if constexpr (D == 3) { if (level_is_binned(li.hashmap_size)) return; }
    }
    T* __restrict__ tab = grad_grid + (size_t)li.table_off * C;

    float frac[D];
    uint32_t pg[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        const float xv = (inputs[(size_t)b * D + d] + sc.in_shift) * sc.in_scale;
        if (xv < 0.0f || xv > 1.0f) return;                // :276-281
        float p = fmaf(xv, li.scale, align_corners ? 0.0f : 0.5f);
        const float fl = floorf(p);
        pg[d] = (uint32_t)fl;
        p -= (float)pg[d];
        if (interp == 1) p = p * p * (3.0f - 2.0f * p);
        frac[d] = p;
    }
    const T* g = grad + (size_t)b * gs_b + (size_t)level * gs_l;
    float gc[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++) gc[ch] = (float)g[ch];

#pragma unroll
    for (int idx = 0; idx < (1 << D); idx++) {
        float w = 1.0f;
        uint32_t pgl[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            if ((idx & (1 << d)) == 0) { w *= 1 - frac[d]; pgl[d] = pg[d]; }
            else { w *= frac[d]; pgl[d] = pg[d] + 1; }
        }
        const uint32_t gi = cell_index<D>(li, pgl) * C;
        if constexpr (sizeof(T) == 2) {
            static_assert(C % 2 == 0 || sizeof(T) == 4, "fp16 grads need an even channel count");
#pragma unroll
            for (int ch = 0; ch < C; ch += 2) {
                half2_t v = {(half_t)(w * gc[ch]), (half_t)(w * gc[ch + 1])};      // :329
                __builtin_amdgcn_global_atomic_fadd_v2f16(
                    (__attribute__((address_space(1))) half2_t*)(tab + gi + ch), v);
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < C; ch++) atomicAdd(tab + gi + ch, w * gc[ch]);     // :336
        }
    }
}

// ---------------------------------------------------------------- K14, MI355X form (D = 3, C = 2), round 2
// Scattered global float atomics execute at the memory side on gfx950 (~20 G requests/s chip-wide, MI355X_MICROARCH
// "Global float atomics"): 128 of them per sample made k_grid_bwd 54 % of the first train step.  Instead the gradient
// table is cut into partitions of PART = 4096 entries and the contributions are ROUTED to the partition's owner by a
// counting sort:
//
//   k_bwd_walk<COUNT> : block = UNIT = (level, 1024 consecutive samples), 4 consecutive samples per lane.  While the cell
//                is unchanged the 8 corner contributions are summed in registers; every finished cell yields ITEMS: one
//                per (y', z') corner row = {key: entry e0 inside the partition | how to get e1 from e0, values of the x
//                and x+1 corners} (10 bytes for fp16 gradients) -- both x corners share a partition unless the pair
//                straddles a partition boundary, which costs two single-corner items.  COUNT only needs the positions:
//                items per partition (LDS histogram) -> the unit's counter row + its column of the per-partition table.
//   k_bwd_scan_units / k_bwd_scan_parts : exclusive scans over the units of a partition and over the partitions:
//                where every unit's run of every partition starts in the queue.
//   k_bwd_walk<FILL>  : same walk with the gradients; items are ranked inside the block (LDS counters), laid out
//                partition by partition in an LDS staging area and leave for the queue as whole runs (consecutive lanes,
//                consecutive slots: in round 1 every 16-byte item was its own L2 request and the pass ran at the L2
//                request rate).  No global atomics anywhere.
//   k_bwd_acc  : one workgroup per (level, partition[, sub-range]) -- handed out through a device-side ticket, fullest
//                first -- streams its contiguous queue range, accumulates in LDS and adds the partition to the table with
//                coalesced read-modify-writes.  fp16 gradients accumulate EXACTLY as 2^-24 fixed point in int64 LDS words
//                (every fp16 value is a multiple of 2^-24; random-address ds_add_u64 costs ~0.3 cycles per lane-op,
//                tools/ubench/lds_acc2.hip), and the table entry becomes RN_half(old + sum) with ONE rounding: order
//                independent, deterministic.  A non-finite contribution (overflowed loss scale) marks its entry, which is
//                written as NaN so that the optimizer's non-finite scan sees it (an integer accumulator would otherwise
//                silently turn Inf into a finite number).  fp32 gradients use ds_add_f32.
// Levels with few partitions are split into SUB sub-ranges so that bk_target workgroups (the host's choice: BK_TARGET = 32, 64 from
// 400 k samples on) share every level; each adds its exact partial sums (int64: the adds commute) into the partition's merge
// record with device-scope atomics and the last to arrive takes them out (no float atomics: same bits whatever the order).
// Levels with more than BK_MAX partitions (T > 2^21) are left to k_grid_bwd.
template <typename T> struct BVal;
template <> struct BVal<half_t> { using type = uint2; };       // {half2 of corner x, half2 of corner x+1}
template <> struct BVal<float> { using type = float4; };
constexpr int FILL_THREADS = 256;
constexpr int SPT = 4;                                         // consecutive samples per lane
constexpr uint32_t UNIT_SAMPLES = FILL_THREADS * SPT;          // 1024: the samples of one block = one UNIT
constexpr uint32_t STAGE_CAP = 4096 + 256;                     // items staged in LDS: a fine level's unit is 1024 cells x 4 pair rows = 4096 items
                                                               // PLUS 4 for every cell whose x-neighbour lies in the next partition (1 cell in 4096);
                                                               // with a cap of exactly 4096, 22 % of the fine levels' units took the unstaged path
constexpr uint32_t KEY_SINGLE = 15u;                           // key code: 0..11 -> e1 = e0 ^ ((2 << code) - 1) (e0 + 1 is such an xor too: the trailing ones of e0 and the zero above them flip)
constexpr int ACC_THREADS = 1024;
constexpr uint32_t BWD_MAX_SAMPLES = 1u << 24;                  // byte offsets of the buffer loads (walk: 12 B per sample; accumulate: 8 B per item, 8 items per sample and level) stay below 2^31
constexpr uint32_t COARSE_RES = 64;                            // levels coarser than this: consecutive queue items often repeat an entry (same ray, same cell)
                                                               // (16 samples per lane on those levels was tried in round 3 and dropped: accumulate 62.4 -> 58.4 us, but fill 58.3 -> 80.1
                                                               // and count 27.5 -> 38.0, step 0.356 -> 0.433 ms; docs/DESIGN_LOG.md)
constexpr uint32_t SUB_RECS = 64;                              // merge records per level: one per partition of a level that is split (P < bk_target)
constexpr uint32_t TICKET_ARRIVALS = 2;                        // tickets[0] = work queue; [2 + level * SUB_RECS + p] = arrivals
constexpr uint32_t TICKET_WORDS = TICKET_ARRIVALS + MAX_LEVELS * SUB_RECS;
template <typename T> constexpr uint32_t sub_rec_words() { return (sizeof(T) == 2 ? 2 * PART : PART) + PART / 64; }

// the plan: everything the fill / accumulate passes need to know about where items go (positions only)
struct BwdPlan {
    uint16_t* cnt;        // [L * U][BK_MAX]   per unit: items per (partition, lane copy) counter
    uint32_t* part_cnt;   // [L][BK_MAX][U]    per partition: items of every unit, then (in place) their exclusive prefix
    uint32_t* totals;     // [L][BK_MAX]       items per partition
    uint32_t* offs;       // [L][BK_MAX]       first queue slot of every partition
    uint32_t* tickets;    // [TICKET_WORDS]
};

// behind the ticket words (plan_layout leaves room), written by the fill pass for the accumulate pass: its tail job, and the
// snapshot of the accumulator's "dirty" word (0 = the table gradient is all zero, no old values are needed).  Not among the
// tickets: every workgroup's atomics keep the line of tickets[0] busy, and a load from it waits behind them.
__host__ __device__ __forceinline__ lae_dw::DwTailJob* plan_tail_job(const BwdPlan& plan) {
    static_assert((TICKET_WORDS * 4) % alignof(lae_dw::DwTailJob) == 0, "the tail job sits right behind the tickets");
    return reinterpret_cast<lae_dw::DwTailJob*>(plan.tickets + TICKET_WORDS);
}
__host__ __device__ __forceinline__ uint32_t* plan_dirty_snapshot(const BwdPlan& plan) {
    return plan.tickets + TICKET_WORDS + sizeof(lae_dw::DwTailJob) / 4;
}

__device__ __forceinline__ uint32_t pack_half2(float a, float b) {
    const half2_t h = {(half_t)a, (half_t)b};
    return __builtin_bit_cast(uint32_t, h);
}

// ---------------------------------------------------------------- stages of k_bwd_walk
// what the stages of a walk block know about its unit; all of it is block-uniform (SGPRs)
struct WalkUnit {
    LevelInfo<3> li;
    uint32_t level, u, U, B;   // the unit: samples [u * UNIT_SAMPLES, (u + 1) * UNIT_SAMPLES) of the B of `level`; U units per level
    // P: partitions of the level.  few partitions: all lanes of a wave count into the same one or two counters, and same-address
    // LDS atomics of one instruction serialise -> NC copies per partition, lane l uses copy l mod NC (sub-runs inside the
    // partition's run).  Coarse levels keep arrival order instead: the accumulate pass merges neighbouring repeats.
    uint32_t P, NC, interp;
    bool align_corners;
};

// ---- positions (and gradients) of SPT consecutive samples of a lane: 16-byte buffer loads, the hardware range check
// returns zeros past the end of the batch (no ragged-tail path for the compiler to blend into the wide one)
struct SampleGroup { float xs[SPT][3], g0[SPT], g1[SPT]; };
template <typename T, bool FILL>
__device__ __forceinline__ SampleGroup load_group(const float* __restrict__ inputs, const T* __restrict__ g_lvl, uint32_t B, uint32_t bs) {
    SampleGroup sg;
    static_assert(SPT == 4, "the wide reads below take 4 samples per lane");
    using u4 = __attribute__((__vector_size__(16))) uint32_t;
    // (the range check is all-or-nothing per 16-byte load: the records end with the last whole group of 4 samples,
    // the one lane that holds the batch's last 1-3 samples reads them with plain loads below)
    const uint32_t B4 = B & ~3u;
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(inputs), 0, (int)(B4 * 12u), 0x00020000);
    const u4 x0 = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (int)(bs * 12u), 0, 0);
    const u4 x1 = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (int)(bs * 12u + 16u), 0, 0);
    const u4 x2 = __builtin_amdgcn_raw_buffer_load_b128(rs_in, (int)(bs * 12u + 32u), 0, 0);
    u4 ga = {0, 0, 0, 0}, gb = {0, 0, 0, 0};
    if constexpr (FILL) {
        const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(g_lvl), 0, (int)(B4 * 2u * (uint32_t)sizeof(T)), 0x00020000);
        ga = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (int)(bs * 2u * (uint32_t)sizeof(T)), 0, 0);
        if constexpr (sizeof(T) == 4) gb = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (int)(bs * 8u + 16u), 0, 0);
    }
    uint32_t t[12] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3], x2[0], x2[1], x2[2], x2[3]};
    uint32_t gw[8] = {ga[0], ga[1], ga[2], ga[3], gb[0], gb[1], gb[2], gb[3]};
    if (bs == B4 && B4 != B) {                             // the ragged tail
#pragma unroll
        for (int s_ = 0; s_ < 3; s_++) {
            if (bs + s_ >= B) break;
#pragma unroll
            for (int d = 0; d < 3; d++) t[3 * s_ + d] = __builtin_bit_cast(uint32_t, inputs[(size_t)(bs + s_) * 3 + d]);
            if constexpr (FILL && sizeof(T) == 2) gw[s_] = reinterpret_cast<const uint32_t*>(g_lvl)[bs + s_];
            else if constexpr (FILL) { gw[2 * s_] = reinterpret_cast<const uint32_t*>(g_lvl)[2 * (bs + s_)]; gw[2 * s_ + 1] = reinterpret_cast<const uint32_t*>(g_lvl)[2 * (bs + s_) + 1]; }
        }
    }
#pragma unroll
    for (int s_ = 0; s_ < SPT; s_++) {
#pragma unroll
        for (int d = 0; d < 3; d++) sg.xs[s_][d] = __builtin_bit_cast(float, t[3 * s_ + d]);
        if constexpr (FILL && sizeof(T) == 2) { const half2_t h = __builtin_bit_cast(half2_t, gw[s_]); sg.g0[s_] = (float)h[0]; sg.g1[s_] = (float)h[1]; }
        else if constexpr (FILL) { sg.g0[s_] = __builtin_bit_cast(float, gw[2 * s_]); sg.g1[s_] = __builtin_bit_cast(float, gw[2 * s_ + 1]); }
        else { sg.g0[s_] = 0.f; sg.g1[s_] = 0.f; }
    }
    return sg;
}

// ---- where the samples of a group lie on the level: cell coordinates, fractions and the range test
struct PlacedGroup { uint32_t pg[SPT][3]; float fr[SPT][3]; bool ok[SPT]; };
__device__ __forceinline__ PlacedGroup place_group(const SampleGroup& sg, const WalkUnit& w, const LevelScales& sc, uint32_t bs) {
    PlacedGroup pl;
#pragma unroll
    for (int s_ = 0; s_ < SPT; s_++) {
        bool ok = bs + s_ < w.B;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const float xv = (sg.xs[s_][d] + sc.in_shift) * sc.in_scale;
            ok = ok && !(xv < 0.0f) && !(xv > 1.0f);                     // gridencoder.cu:276-281
            float pp = fmaf(xv, w.li.scale, w.align_corners ? 0.0f : 0.5f);
            const float fl = floorf(pp);
            pl.pg[s_][d] = (uint32_t)fl;
            pp -= (float)pl.pg[s_][d];
            if (w.interp == 1) pp = pp * pp * (3.0f - 2.0f * pp);
            pl.fr[s_][d] = pp;
        }
        pl.ok[s_] = ok;
    }
    return pl;
}
// the walk's cell test: sample s_ of the group leaves the cell cp (or there is none yet)
__device__ __forceinline__ bool leaves_cell(const PlacedGroup& pl, int s_, bool have, const uint32_t (&cp)[3]) {
    return !have || pl.pg[s_][0] != cp[0] || pl.pg[s_][1] != cp[1] || pl.pg[s_][2] != cp[2];
}

// ---- items of the cell cp, one row of x-neighbours (y, z corner) at a time: a PAIR item {counter c0, key k0} when both
// entries sit in one partition a low-bit xor apart, else two single items {c0, k0}, {c1, k1}
struct Rows { uint32_t c0[4], k0[4], c1[4], k1[4], i0[4], i1[4]; bool pair[4]; };   // i0 / i1: the two entries of the row (count pass only)
__device__ __forceinline__ void cell_rows(const WalkUnit& w, uint32_t lane, const uint32_t (&cp)[3], Rows& r) {
    const LevelInfo<3>& li = w.li;
    const uint32_t NC = w.NC, lane_copy = lane & (NC - 1);
    if (li.use_hash && li.pow2) {
        // hashed level with a power-of-two table: the x-neighbour is i1 = i0 ^ dx on EVERY row, dx = the low-bit mask
        // (x ^ (x + 1)) & (size - 1), so whether the row is a pair item and its key code are decided once per cell
        // (the pass is bound by its instruction count: ~30 instructions per row -> ~9)
        const uint32_t m = li.hashmap_size - 1u;
        const uint32_t dx = (cp[0] ^ (cp[0] + 1u)) & m;
        const bool pr = dx != 0u && dx < PART;
        const uint32_t code = (pr ? (uint32_t)(__builtin_popcount(dx) - 1) : KEY_SINGLE) << 12;
        const uint32_t hy0 = cp[1] * 2654435761u, hy1 = hy0 + 2654435761u, hz0 = cp[2] * 805459861u, hz1 = hz0 + 805459861u;
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
            const uint32_t i0 = (cp[0] ^ ((yz & 1) ? hy1 : hy0) ^ ((yz & 2) ? hz1 : hz0)) & m, i1 = i0 ^ dx;
            r.c0[yz] = (i0 >> PART_SHIFT) * NC + lane_copy; r.c1[yz] = (i1 >> PART_SHIFT) * NC + lane_copy;
            r.i0[yz] = i0; r.i1[yz] = i1;
            r.pair[yz] = pr;
            r.k0[yz] = (i0 & (PART - 1)) | code;
            r.k1[yz] = (i1 & (PART - 1)) | (KEY_SINGLE << 12);
        }
        return;
    }
    uint32_t hy0 = 0, hy1 = 0, hz0 = 0, hz1 = 0, key0 = 0;
    if (li.use_hash) {
        hy0 = cp[1] * 2654435761u; hy1 = hy0 + 2654435761u;
        hz0 = cp[2] * 805459861u; hz1 = hz0 + 805459861u;
    } else key0 = cp[0] * li.stride[0] + cp[1] * li.stride[1] + cp[2] * li.stride[2];
#pragma unroll
    for (int yz = 0; yz < 4; yz++) {
        uint32_t i0, i1;
        if (li.use_hash) {
            const uint32_t h = ((yz & 1) ? hy1 : hy0) ^ ((yz & 2) ? hz1 : hz0);
            i0 = cp[0] ^ h; i1 = (cp[0] + 1) ^ h;
        } else {
            i0 = key0 + ((yz & 1) ? li.stride[1] : 0u) + ((yz & 2) ? li.stride[2] : 0u);
            i1 = i0 + li.stride[0];
        }
        if (li.pow2) { i0 &= li.hashmap_size - 1; i1 &= li.hashmap_size - 1; }
        else if (li.use_hash || !li.nowrap) { i0 %= li.hashmap_size; i1 %= li.hashmap_size; }
        const uint32_t e0 = i0 & (PART - 1), e1 = i1 & (PART - 1), d = e0 ^ e1;
        const bool same_part = (i0 >> PART_SHIFT) == (i1 >> PART_SHIFT) && d != 0;
        r.c0[yz] = (i0 >> PART_SHIFT) * NC + lane_copy; r.c1[yz] = (i1 >> PART_SHIFT) * NC + lane_copy;
        r.i0[yz] = i0; r.i1[yz] = i1;
        r.pair[yz] = same_part && (d & (d + 1)) == 0;
        r.k0[yz] = e0 | ((r.pair[yz] ? (uint32_t)(__builtin_popcount(d) - 1) : KEY_SINGLE) << 12);
        r.k1[yz] = e1 | (KEY_SINGLE << 12);
    }
}

// ---- the count unit: how many items does each (partition, copy) counter get from this unit
// lines: LDS copy of the level's bits of the caller's "ever touched" bitmap, or NULL (no marking)
__device__ __forceinline__ void count_cell(const WalkUnit& w, uint32_t lane, const uint32_t (&cp)[3], uint32_t* hist, uint32_t* lines, uint32_t line_shift) {
    Rows r;
    cell_rows(w, lane, cp, r);
#pragma unroll
    for (int yz = 0; yz < 4; yz++) atomicAdd(&hist[r.c0[yz]], 1u);
    if (lines) {
        // "ever touched" bitmap of the caller, one bit per 8 entries (a 64-byte line of the fp32 table): the block
        // notes the lines of its cells' corners in LDS (a superset of the lines that get a non-zero gradient is fine)
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
            const uint32_t l0 = line_shift + (r.i0[yz] >> 3), l1 = line_shift + (r.i1[yz] >> 3);
            atomicOr(&lines[l0 >> 5], 1u << (l0 & 31u));
            if (l1 != l0) atomicOr(&lines[l1 >> 5], 1u << (l1 & 31u));
        }
    }
    if (!(r.pair[0] && r.pair[1] && r.pair[2] && r.pair[3])) {
#pragma unroll
        for (int yz = 0; yz < 4; yz++) if (!r.pair[yz]) atomicAdd(&hist[r.c1[yz]], 1u);
    }
}
// the unit's histogram -> its counter row and its column of the per-partition table
__device__ __forceinline__ void publish_counts(const WalkUnit& w, const BwdPlan& plan, const uint32_t* hist) {
    const uint32_t tid = threadIdx.x, unit = w.level * w.U + w.u;
    for (uint32_t k = tid; k < BK_MAX / 2; k += FILL_THREADS)
        reinterpret_cast<uint32_t*>(plan.cnt + (size_t)unit * BK_MAX)[k] = hist[2 * k] | (hist[2 * k + 1] << 16);   // <= 8192 each
    for (uint32_t k = tid; k < w.P; k += FILL_THREADS) {
        uint32_t n = 0;
        for (uint32_t c = 0; c < w.NC; c++) n += hist[k * w.NC + c];
        plan.part_cnt[((size_t)w.level * BK_MAX + k) * w.U + w.u] = n;
    }
}
// new line bits of this block -> the caller's bitmap (a plain read first); a block that sees every line of the level marked
// sets level_full[level].  Every thread of the block calls it (one barrier inside).
__device__ __forceinline__ void publish_touched(const WalkUnit& w, uint32_t* __restrict__ touched, uint32_t* __restrict__ level_full,
                                                const uint32_t* lines, uint32_t line_shift, uint32_t line_words) {
    const uint32_t tid = threadIdx.x;
    uint32_t* gw = touched + ((w.li.table_off >> 3) >> 5);
    const uint32_t n_lines = (w.li.hashmap_size + 7u) >> 3;
    bool full = true;
    for (uint32_t k = tid; k < line_words; k += FILL_THREADS) {
        const uint32_t wd = lines[k], cur = gw[k];
        if (wd && (cur & wd) != wd) atomicOr(&gw[k], wd);
        // bits of word k that belong to this level: [line_shift, line_shift + n_lines) in the level's bit space
        const uint32_t lo_bit = k == 0 ? line_shift : 0u;
        const uint32_t end = line_shift + n_lines - 32u * k;          // bits of this word below `end` are the level's
        uint32_t mask = end >= 32u ? 0xffffffffu : ((1u << end) - 1u);
        mask &= ~((1u << lo_bit) - 1u);
        full = full && (((cur | wd) & mask) == mask);
    }
    if (__syncthreads_and(full ? 1 : 0) && tid == 0) level_full[w.level] = 1u;
}

__device__ __forceinline__ void walk_count_unit(const WalkUnit& w, const LevelScales& sc, const float* __restrict__ inputs, const BwdPlan& plan,
                                                uint32_t* __restrict__ touched_, uint32_t* __restrict__ level_full) {
    __shared__ uint32_t hist[BK_MAX];
    extern __shared__ uint32_t s_lines[];                  // with `touched`: line bits of this level, aligned to the global words
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // bit of entry e of this level in the caller's bitmap: (table_off + e) / 8; the LDS copy starts at the bitmap word that
    // holds the level's first line
    const uint32_t line_shift = (w.li.table_off >> 3) & 31u;
    const uint32_t line_words = (line_shift + ((w.li.hashmap_size + 7u) >> 3) + 31u) >> 5;
    // a level all of whose lines are marked has nothing to add: level_full[level] (set below by a block that sees it) switches
    // the marking of that level off for good (on the bench scene: levels 9-15 after a few steps)
    // The decision is made ONCE per block (thread 0 reads the flag, the block agrees through LDS): blocks of this very launch
    // set level_full[level], so a per-thread read could split a block's waves between marking and not marking -- mismatched
    // barrier counts below and uninitialised LDS words ORed into the bitmap.
    __shared__ uint32_t s_mark;
    if (tid == 0) s_mark = (touched_ && !level_full[w.level]) ? 1u : 0u;
    __syncthreads();
    uint32_t* __restrict__ touched = s_mark ? touched_ : nullptr;
    if (touched) { for (uint32_t k = tid; k < line_words; k += FILL_THREADS) s_lines[k] = 0u; }
    for (uint32_t k = tid; k < BK_MAX; k += FILL_THREADS) hist[k] = 0;
    const uint32_t bs = (w.u * FILL_THREADS + tid) * SPT;
    const PlacedGroup pl = place_group(load_group<float, false>(inputs, nullptr, w.B, bs), w, sc, bs);
    __syncthreads();
    uint32_t cpg[3] = {0, 0, 0}; bool have = false;
#pragma unroll
    for (int s_ = 0; s_ < SPT; s_++) {
        if (!pl.ok[s_]) continue;
        if (leaves_cell(pl, s_, have, cpg)) {
            if (have) count_cell(w, lane, cpg, hist, touched ? s_lines : nullptr, line_shift);
            cpg[0] = pl.pg[s_][0]; cpg[1] = pl.pg[s_][1]; cpg[2] = pl.pg[s_][2]; have = true;
        }
    }
    if (have) count_cell(w, lane, cpg, hist, touched ? s_lines : nullptr, line_shift);
    __syncthreads();
    publish_counts(w, plan, hist);
    if (touched) publish_touched(w, touched, level_full, s_lines, line_shift, line_words);
}

// ---- the fill unit
// the counters of a fill block (LDS), and where its items go: the LDS staging area s_vals / s_keys (STAGE_CAP items), or straight to the queue
struct __attribute__((aligned(16))) FillLds {
    uint32_t hist[BK_MAX];         // items per (partition, copy) counter, then the running slot of its sub-run
    uint32_t start[BK_MAX + 1];    // first slot of every sub-run in the staging area (+ the unit's total)
    uint32_t gbase[BK_MAX];        // the unit's first queue slot of every partition
};
template <typename T>
struct FillQueue { typename BVal<T>::type* __restrict__ vals; uint16_t* __restrict__ keys; bool staged; };   // staged: the unit's items fit the staging area
// exclusive scan over the counters (one wave, 8 counters per lane) -> where each sub-run starts in the staging area
__device__ __forceinline__ void scan_counters(uint32_t* hist, uint32_t* start) {
    const uint32_t tid = threadIdx.x;
    if (tid < 64) {
        uint32_t v[BK_MAX / 64], sum = 0;
#pragma unroll
        for (int k = 0; k < (int)(BK_MAX / 64); k++) { v[k] = hist[tid * (BK_MAX / 64) + k]; sum += v[k]; }
        uint32_t run = lae::wave_incl_scan(sum) - sum;
#pragma unroll
        for (int k = 0; k < (int)(BK_MAX / 64); k++) {     // hist becomes the running slot of its sub-run
            start[tid * (BK_MAX / 64) + k] = run; hist[tid * (BK_MAX / 64) + k] = run; run += v[k];
        }
        if (tid == 63) start[BK_MAX] = run;
    }
}
// one item {corner x: (x0, x1), corner x+1: (y0, y1) -- zeros in a single-corner item} into slot `slot` of counter ci's sub-run
template <typename T>
__device__ __forceinline__ void put_item(FillLds& lds, typename BVal<T>::type* s_vals, uint16_t* s_keys, const FillQueue<T>& q, uint32_t NC, uint32_t slot, uint32_t ci, uint32_t key, float x0, float x1, float y0, float y1) {
    typename BVal<T>::type val;
    if constexpr (sizeof(T) == 2) { val.x = pack_half2(x0, x1); val.y = pack_half2(y0, y1); }
    else { val.x = x0; val.y = x1; val.z = y0; val.w = y1; }
    if (q.staged) { s_vals[slot] = val; s_keys[slot] = (uint16_t)key; }
    else {          // more items than the staging area holds (split corner pairs): straight to the queue
        const uint32_t k = ci / NC, dst = lds.gbase[k] + (slot - lds.start[k * NC]);
        q.vals[dst] = val; q.keys[dst] = (uint16_t)key;
    }
}
// sums + emission of the finished cell cp, sorted by partition (slot = sub-run start + arrival order inside it)
template <typename T>
__device__ __forceinline__ void emit_cell(const WalkUnit& w, uint32_t lane, const uint32_t (&cp)[3], FillLds& lds, typename BVal<T>::type* s_vals, uint16_t* s_keys, const FillQueue<T>& q, float (&a0)[8], float (&a1)[8]) {
    Rows r;
    cell_rows(w, lane, cp, r);
    // the slots of all rows first (independent LDS atomics in flight together), then the writes
    uint32_t sl0[4], sl1[4];
#pragma unroll
    for (int yz = 0; yz < 4; yz++) sl0[yz] = atomicAdd(&lds.hist[r.c0[yz]], 1u);
    // four pair rows is the common cell: one test instead of a divergent branch per row and phase
    const bool all_pairs = r.pair[0] && r.pair[1] && r.pair[2] && r.pair[3];
    if (!all_pairs) {
#pragma unroll
        for (int yz = 0; yz < 4; yz++) sl1[yz] = r.pair[yz] ? 0u : atomicAdd(&lds.hist[r.c1[yz]], 1u);
    }
    if (all_pairs) {
#pragma unroll
        for (int yz = 0; yz < 4; yz++) put_item<T>(lds, s_vals, s_keys, q, w.NC, sl0[yz], r.c0[yz], r.k0[yz], a0[2 * yz], a1[2 * yz], a0[2 * yz + 1], a1[2 * yz + 1]);
    } else {
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
            const bool pr = r.pair[yz];
            // (fp16: a pair of zeros packs to the word 0)
            put_item<T>(lds, s_vals, s_keys, q, w.NC, sl0[yz], r.c0[yz], r.k0[yz], a0[2 * yz], a1[2 * yz], pr ? a0[2 * yz + 1] : 0.f, pr ? a1[2 * yz + 1] : 0.f);
            if (!pr) put_item<T>(lds, s_vals, s_keys, q, w.NC, sl1[yz], r.c1[yz], r.k1[yz], a0[2 * yz + 1], a1[2 * yz + 1], 0.f, 0.f);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; c++) { a0[c] = 0.f; a1[c] = 0.f; }
}
// ---- the staged runs leave for the queue, one partition at a time per wave: consecutive lanes, consecutive slots
// a wave owns a contiguous range of partitions; the (start, end, queue base) triples of up to 64 of them are
// read by the lanes at once and handed round through SGPRs, so the copies of consecutive runs do not wait
// for one another's LDS reads
template <typename T>
__device__ __forceinline__ void drain_staged_runs(const WalkUnit& w, FillLds& lds, typename BVal<T>::type* s_vals, uint16_t* s_keys, const FillQueue<T>& q) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, P = w.P, NC = w.NC;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t per = (P + FILL_THREADS / 64 - 1) / (FILL_THREADS / 64);
    const uint32_t kend = min(P, (wv + 1) * per);
    for (uint32_t kb = wv * per; kb < kend; kb += 64) {
        const uint32_t k = kb + lane;
        uint32_t s0v = 0, s1v = 0, gbv = 0;
        if (k < kend) { s0v = lds.start[k * NC]; s1v = lds.start[(k + 1) * NC]; gbv = lds.gbase[k]; }
        const uint32_t np = min(64u, kend - kb);
        // two runs at a time, one per half of the wave (a run of a fine level holds ~32 items)
#pragma unroll 4
        for (uint32_t r = 0; r < np; r += 2) {
            const int src = (int)(r + (lane >> 5));                  // lanes past np hold zeros: an empty run
            const uint32_t s0 = __shfl(s0v, src, 64), s1 = __shfl(s1v, src, 64), gb = __shfl(gbv, src, 64);
            for (uint32_t i = s0 + (lane & 31u); i < s1; i += 32) { q.vals[gb + (i - s0)] = s_vals[i]; q.keys[gb + (i - s0)] = s_keys[i]; }
        }
    }
}

template <typename T>
__device__ __forceinline__ void walk_fill_unit(const WalkUnit& w, const LevelScales& sc, const T* __restrict__ g_lvl, const float* __restrict__ inputs,
                                               const BwdPlan& plan, typename BVal<T>::type* __restrict__ qvals, uint16_t* __restrict__ qkeys) {
    __shared__ FillLds lds;
    __shared__ __attribute__((aligned(16))) typename BVal<T>::type s_vals[STAGE_CAP];
    __shared__ __attribute__((aligned(16))) uint16_t s_keys[STAGE_CAP];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, unit = w.level * w.U + w.u;
    const uint32_t bs = (w.u * FILL_THREADS + tid) * SPT;
    // every global read of the unit is issued before the first one is consumed: one memory latency, not three
    static_assert(BK_MAX / 2 == FILL_THREADS && BK_MAX == 2 * FILL_THREADS, "one counter word and two partitions per lane");
    // the unit's own counters (from the count pass) and where its run of every partition starts in the queue
    const uint32_t w_cnt = reinterpret_cast<const uint32_t*>(plan.cnt + (size_t)unit * BK_MAX)[tid];
    uint32_t gb_off[2] = {0, 0}, gb_cnt[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t k = tid + i * FILL_THREADS;
        if (k < w.P) { gb_off[i] = plan.offs[w.level * BK_MAX + k]; gb_cnt[i] = plan.part_cnt[((size_t)w.level * BK_MAX + k) * w.U + w.u]; }
    }
    const SampleGroup sg = load_group<T, true>(inputs, g_lvl, w.B, bs);
    lds.hist[2 * tid] = w_cnt & 0xffffu; lds.hist[2 * tid + 1] = w_cnt >> 16;
#pragma unroll
    for (int i = 0; i < 2; i++) { const uint32_t k = tid + i * FILL_THREADS; if (k < w.P) lds.gbase[k] = gb_off[i] + gb_cnt[i]; }
    const PlacedGroup pl = place_group(sg, w, sc, bs);
    GRID_STAMP(blockIdx.x, 1);
    __syncthreads();
    GRID_STAMP(blockIdx.x, 2);
    scan_counters(lds.hist, lds.start);
    __syncthreads();
    GRID_STAMP(blockIdx.x, 3);
    const uint32_t total = lds.start[BK_MAX];
    const FillQueue<T> q = {qvals, qkeys, total <= STAGE_CAP};
    uint32_t cpg[3] = {0, 0, 0}; bool have = false;
    float a0[8], a1[8];
#pragma unroll
    for (int c = 0; c < 8; c++) { a0[c] = 0.f; a1[c] = 0.f; }
#pragma unroll
    for (int s_ = 0; s_ < SPT; s_++) {
        GRID_STAMP(blockIdx.x, 8 + s_);
        if (!pl.ok[s_]) continue;
        if (leaves_cell(pl, s_, have, cpg)) {
            if (have) emit_cell<T>(w, lane, cpg, lds, s_vals, s_keys, q, a0, a1);
            cpg[0] = pl.pg[s_][0]; cpg[1] = pl.pg[s_][1]; cpg[2] = pl.pg[s_][2]; have = true;
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const float wt = (((c & 1) ? pl.fr[s_][0] : 1 - pl.fr[s_][0]) * ((c & 2) ? pl.fr[s_][1] : 1 - pl.fr[s_][1])) * ((c & 4) ? pl.fr[s_][2] : 1 - pl.fr[s_][2]);
            a0[c] = fmaf(wt, sg.g0[s_], a0[c]); a1[c] = fmaf(wt, sg.g1[s_], a1[c]);
        }
    }
    GRID_STAMP(blockIdx.x, 12);
    if (have) emit_cell<T>(w, lane, cpg, lds, s_vals, s_keys, q, a0, a1);
    GRID_STAMP(blockIdx.x, 4);
    __syncthreads();
    GRID_STAMP(blockIdx.x, 5);
    if (q.staged) drain_staged_runs<T>(w, lds, s_vals, s_keys, q);
    GRID_STAMP(blockIdx.x, 6);
    GRID_NOTE(blockIdx.x, 7, total);
}

// block 0 of the fill pass opens the accumulate pass of this backward: tickets, the accumulator's "dirty" word, the tail job
__device__ __forceinline__ void open_accumulate_pass(const BwdPlan& plan, uint32_t* __restrict__ grad_dirty, const lae_dw::DwTailJob& tail) {
    for (uint32_t k = threadIdx.x; k < TICKET_WORDS; k += FILL_THREADS) plan.tickets[k] = 0;   // work queue / arrival counters of the accumulate pass
    // the caller's "dirty" word of the gradient accumulator (0: nothing but zeros in it, the optimizer's apply kernel has just
    // consumed it): the accumulate pass of THIS backward gets its value, and from here on the accumulator counts as written.
    // No block of this launch reads either word and the accumulate pass is a later launch on the stream: no counter, no fence.
    // Without a word the accumulator may hold anything.
    if (threadIdx.x == 0) {
        *plan_dirty_snapshot(plan) = grad_dirty ? *grad_dirty : 1u;
        if (grad_dirty) *grad_dirty = 1u;
        // the accumulate pass's tail job (n_tasks == 0: none) travels through the plan as well: as an argument of that launch
        // its 26 words would stay in scalar registers for the whole pass, which has none to spare
        *plan_tail_job(plan) = tail;
    }
}

// PLAIN: linear interpolation, align_corners = false, hash grid type (every shipped config) as compile-time facts -- the pass
// is bound by its instruction count
template <typename T, bool FILL, bool PLAIN>
__global__ __launch_bounds__(FILL_THREADS) void k_bwd_walk(
    const T* __restrict__ gradT, const float* __restrict__ inputs, const int32_t* __restrict__ offsets, uint32_t B,
    uint32_t L, LevelScales sc, uint32_t gridtype_, bool align_corners_, uint32_t interp_, uint32_t U, BwdPlan plan,
    typename BVal<T>::type* __restrict__ qvals, uint16_t* __restrict__ qkeys, uint32_t* __restrict__ touched_,
    uint32_t* __restrict__ level_full, uint32_t* __restrict__ grad_dirty = nullptr, lae_dw::DwTailJob tail = lae_dw::DwTailJob{}) {
    const uint32_t gridtype = PLAIN ? 0u : gridtype_;
    WalkUnit w;
    w.interp = PLAIN ? 0u : interp_; w.align_corners = PLAIN ? false : align_corners_;
    if constexpr (FILL) GRID_STAMP(blockIdx.x, 0);
    w.level = blockIdx.x / U; w.u = blockIdx.x % U; w.U = U; w.B = B;
    if (FILL && blockIdx.x == 0) open_accumulate_pass(plan, grad_dirty, tail);
    w.li = level_info<3>(sc, offsets, w.level, gridtype, w.align_corners);
    w.P = (w.li.hashmap_size + PART - 1) >> PART_SHIFT;
    if (w.P > BK_MAX) return;                              // handled by the generic atomic kernel
    w.NC = (w.P <= BK_MAX / 8 && w.li.resolution >= COARSE_RES) ? 8u : 1u;
    if constexpr (FILL) walk_fill_unit<T>(w, sc, gradT + (size_t)w.level * B * 2, inputs, plan, qvals, qkeys);
    else walk_count_unit(w, sc, inputs, plan, touched_, level_full);
}

// per partition: exclusive scan over the units' counts (in place) and the partition total.  One wavefront per (level, partition).
__global__ __launch_bounds__(256) void k_bwd_scan_units(const int32_t* __restrict__ offsets, uint32_t L, uint32_t U, BwdPlan plan) {
    const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= L * BK_MAX) return;
    const uint32_t level = t / BK_MAX, k = t % BK_MAX;
    const uint32_t size = (uint32_t)(offsets[level + 1] - offsets[level]);
    const uint32_t P = (size + PART - 1) >> PART_SHIFT;
    const int lane = threadIdx.x & 63;
    if (P > BK_MAX || k >= P) { if (lane == 0) plan.totals[t] = 0; return; }
    uint32_t* p = plan.part_cnt + (size_t)t * U;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < U; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t v = c < U ? p[c] : 0u;
        const uint32_t inc = lae::wave_incl_scan(v);
        if (c < U) p[c] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) plan.totals[t] = carry;
}

// partition totals -> first queue slot of every partition.  One block.
__global__ __launch_bounds__(1024) void k_bwd_scan_parts(uint32_t n, BwdPlan plan) {
    __shared__ uint32_t lds[17];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n ? plan.totals[i] : 0;
        uint32_t total;
        const uint32_t ex = lae::block_excl_scan<16>(v, &total, lds);
        if (i < n) plan.offs[i] = carry + ex;
        carry += total;
    }
}

// ---------------------------------------------------------------- stages of k_bwd_acc
// fp16 bits -> value * 2^24 as a signed integer (exact: finite fp16 values are multiples of 2^-24, |v| * 2^24 < 2^40)
__device__ __forceinline__ long long half_to_fix24(uint32_t u) {
    // branch-free, sign applied to the 11-bit mantissa in 32 bits: (+-mantissa) << (max(e, 1) - 1), subnormals have no hidden bit
    const uint32_t e = (u >> 10) & 31u;
    const int32_t smask = (int32_t)(u << 16) >> 31;
    const uint32_t mant = (u & 1023u) | (min(e, 1u) << 10);
    const int32_t sm = (int32_t)(mant ^ (uint32_t)smask) - smask;
    return (long long)sm << (max(e, 1u) - 1u);
}
// the same for |value| < 128 (exponent field < 22): value * 2^24 fits int32, and the float pipeline converts it exactly
// (fp16 -> fp32 is exact incl. subnormals, the scaling is a power of two, the result an integer below 2^31): 4 instructions
// instead of 10.  Both halves of a word at once.
__device__ __forceinline__ void half2_to_fix24_small(uint32_t w, long long& lo, long long& hi) {
    const half2_t h = __builtin_bit_cast(half2_t, w);
    lo = (long long)(int32_t)((float)h[0] * 16777216.0f);
    hi = (long long)(int32_t)((float)h[1] * 16777216.0f);
}
// value * 2^24 (signed integer) -> nearest fp16 (ties to even), ONE rounding; overflow -> infinity
__device__ __forceinline__ uint32_t fix24_to_half(long long t) {
    const uint32_t sign = t < 0 ? 0x8000u : 0u;
    const unsigned long long mag = t < 0 ? (unsigned long long)(-t) : (unsigned long long)t;
    if (mag < 1024ull) return sign | (uint32_t)mag;              // zero / subnormal: exact
    const int msb = 63 - __builtin_clzll(mag);                   // >= 10
    const int shift = msb - 10;
    unsigned long long q = mag >> shift;                         // 11 bits, leading one included
    if (shift > 0) {
        const unsigned long long rem = mag & ((1ull << shift) - 1ull), halfway = 1ull << (shift - 1);
        if (rem > halfway || (rem == halfway && (q & 1ull))) q++;
    }
    int e = msb - 9;                                             // biased exponent
    if (q == 2048ull) { q = 1024ull; e++; }
    if (e >= 31) return sign | 0x7c00u;
    return sign | ((uint32_t)e << 10) | ((uint32_t)q & 1023u);
}
__device__ __forceinline__ bool half_nonfinite(uint32_t u) { return (u & 0x7c00u) == 0x7c00u; }

// the workgroup's accumulator of one partition, in LDS.  fp16 grads: int64 acc0[PART] | acc1[PART] (channel 0 / 1, SoA: fewer
// bank conflicts than interleaved) and a bit per entry that got a non-finite contribution; fp32: float[2 * PART] in the same words
struct AccBins { unsigned long long* acc64; uint32_t* poison; };

// ---- tickets.  Ticket t in [s_first[l], s_first[l] + P * SUB) is (partition, sub-range) number t - s_first[l] of level l, the
// coarse levels first: their sub-ranges + merge are the longest chains.  -> the number of partition tasks
__device__ __forceinline__ uint32_t build_ticket_table(const int32_t* __restrict__ offsets, uint32_t L, uint32_t bk_target, uint32_t* s_cnt,
                                                       uint32_t* s_sub, uint32_t* s_first, uint32_t* s_total) {
    const uint32_t tid = threadIdx.x;
    if (tid < L) {
        const LevelBins lb = level_bins_of((uint32_t)(offsets[tid + 1] - offsets[tid]), bk_target);
        s_cnt[tid] = lb.P <= BK_MAX ? lb.P * lb.SUB : 0u;
        s_sub[tid] = lb.SUB;
    }
    __syncthreads();
    if (tid == 0) { uint32_t run = 0; for (uint32_t l = 0; l < L; l++) { s_first[l] = run; run += s_cnt[l]; } *s_total = run; }
    __syncthreads();
    const uint32_t total = *s_total;
    __syncthreads();
    return total;
}
struct AccTask { uint32_t level, p, sub, SUB; };             // sub-range `sub` of SUB of partition p of `level`: all wave-uniform
__device__ __forceinline__ AccTask decode_ticket(uint32_t t, uint32_t L, const uint32_t* s_first, const uint32_t* s_sub) {
    AccTask k; uint32_t level = 0;
    while (level + 1 < L && t >= s_first[level + 1]) level++;
    k.level = __builtin_amdgcn_readfirstlane(level);
    const uint32_t bk = t - __builtin_amdgcn_readfirstlane(s_first[k.level]);
    k.SUB = __builtin_amdgcn_readfirstlane(s_sub[k.level]);
    k.p = bk / k.SUB; k.sub = bk % k.SUB;
    return k;
}

// ---- per-task set-up
// the partition's items in the queue (n of them from slot q0) and whether the accumulator holds old values: wave-uniform
struct AccRange { uint32_t n, q0; bool dirty; };
__device__ __forceinline__ AccRange partition_range(const BwdPlan& plan, uint32_t level, uint32_t p) {
    // (the dirty snapshot travels with the two plan words: three loads in flight, one wait)
    const uint32_t n_raw = plan.totals[level * BK_MAX + p], q0_raw = plan.offs[level * BK_MAX + p], dirty_raw = *plan_dirty_snapshot(plan);
    return AccRange{(uint32_t)__builtin_amdgcn_readfirstlane(n_raw), (uint32_t)__builtin_amdgcn_readfirstlane(q0_raw), __builtin_amdgcn_readfirstlane(dirty_raw) != 0u};
}
// the old values of the lane's table entries (fp16; d2 = the partition's entries as words, n_old of them are read) are requested
// now, all in flight together, and consumed after the items: their latency hides behind the partition's whole accumulate phase (a
// load per touched entry inside the flush loop made every round wait for its own memory latency).  A clean accumulator (training:
// the optimizer zeroes it in every step) holds zeros: n_old = 0, nothing is read (16 KB per task), and RN(0 + sum) in the flush is
// what the read would have given.  Then the bins are zeroed.  Every thread calls it (one barrier at the end).
template <typename T>
__device__ __forceinline__ void open_partition(const AccBins& bins, const uint32_t* __restrict__ d2, uint32_t n_old, uint32_t (&oldv)[PART / ACC_THREADS]) {
    const uint32_t tid = threadIdx.x;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int it = 0; it < (int)(PART / ACC_THREADS); it++) { const uint32_t e = tid + it * ACC_THREADS; oldv[it] = e < n_old ? d2[e] : 0u; }
    }
    for (uint32_t i = tid; i < (sizeof(T) == 2 ? 2 * PART : PART); i += ACC_THREADS) bins.acc64[i] = 0ull;
    if (tid < PART / 32) bins.poison[tid] = 0u;
    __syncthreads();
}

// ---- adding items
// The fp16 item rule.  An item's two words {corner x, corner x+1} are added to four exact 2^-24 fixed-point sums; a word with a
// non-finite half marks its corner instead (bad0 / bad1), and commit() then poisons the corner's entry and adds nothing to it.
struct HalfSums { long long s00 = 0, s01 = 0, s10 = 0, s11 = 0; bool bad0 = false, bad1 = false; };
__device__ __forceinline__ void half_item_add(HalfSums& s, uint32_t w0, uint32_t w1) {
    // one test for the item's four halves: adding 10 to an exponent field carries out of it iff the field is >= 22,
    // i.e. |value| >= 128 or non-finite; below that the cheap conversion is exact (gradients that large are rare)
    const uint32_t carry = (((w0 & 0x7c007c00u) + 0x28002800u) | ((w1 & 0x7c007c00u) + 0x28002800u)) & 0x80008000u;
    if (carry == 0) {
        long long a, b;
        half2_to_fix24_small(w0, a, b); s.s00 += a; s.s01 += b;
        half2_to_fix24_small(w1, a, b); s.s10 += a; s.s11 += b;
    } else {
        if (half_nonfinite(w0) || half_nonfinite(w0 >> 16)) s.bad0 = true;
        else { s.s00 += half_to_fix24(w0 & 0xffffu); s.s01 += half_to_fix24(w0 >> 16); }
        if (half_nonfinite(w1) || half_nonfinite(w1 >> 16)) s.bad1 = true;
        else { s.s10 += half_to_fix24(w1 & 0xffffu); s.s11 += half_to_fix24(w1 >> 16); }
    }
}
// the sums of the items of one key -> the bins
__device__ __forceinline__ void half_sums_commit(const HalfSums& s, uint32_t key, const AccBins& bins) {
    const uint32_t e0 = key & (PART - 1), code = key >> 12, e1 = e0 ^ ((2u << code) - 1u);
    unsigned long long* acc64 = bins.acc64;
    if (!(s.bad0 || s.bad1)) {
        // branch-free: a single-corner item (1 in ~4096) carries zeros in its second word, which are added to e0 again
        const uint32_t e1s = code != KEY_SINGLE ? e1 : e0;
        atomicAdd(&acc64[e0], (unsigned long long)s.s00);
        atomicAdd(&acc64[PART + e0], (unsigned long long)s.s01);
        atomicAdd(&acc64[e1s], (unsigned long long)s.s10);
        atomicAdd(&acc64[PART + e1s], (unsigned long long)s.s11);
    } else {
        if (s.bad0) atomicOr(&bins.poison[e0 >> 5], 1u << (e0 & 31));
        else { atomicAdd(&acc64[e0], (unsigned long long)s.s00); atomicAdd(&acc64[PART + e0], (unsigned long long)s.s01); }
        if (code != KEY_SINGLE) {
            if (s.bad1) atomicOr(&bins.poison[e1 >> 5], 1u << (e1 & 31));
            else { atomicAdd(&acc64[e1], (unsigned long long)s.s10); atomicAdd(&acc64[PART + e1], (unsigned long long)s.s11); }
        }
    }
}
// one item on its own
template <typename T>
__device__ __forceinline__ void add_item(const AccBins& bins, uint32_t key, const typename BVal<T>::type& v) {
    if constexpr (sizeof(T) == 2) {
        HalfSums s;
        half_item_add(s, v.x, v.y);
        half_sums_commit(s, key, bins);
    } else {
        const uint32_t e0 = key & (PART - 1), code = key >> 12, e1 = e0 ^ ((2u << code) - 1u);
        float* af = reinterpret_cast<float*>(bins.acc64);
        atomicAdd(af + e0, v.x); atomicAdd(af + PART + e0, v.y);
        if (code != KEY_SINGLE) { atomicAdd(af + e1, v.z); atomicAdd(af + PART + e1, v.w); }
    }
}
// fp32 items [lo, hi) of a finer level: neighbouring items are unrelated
__device__ __forceinline__ void add_items_float_fine(const AccBins& bins, const float4* __restrict__ pv, const uint16_t* __restrict__ pk, uint32_t lo, uint32_t hi) {
    uint32_t i = lo + threadIdx.x;
    for (; i + 3 * ACC_THREADS < hi; i += 4 * ACC_THREADS) {              // four loads in flight per lane
        float4 v[4]; uint32_t k[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { v[j] = pv[i + j * ACC_THREADS]; k[j] = pk[i + j * ACC_THREADS]; }
#pragma unroll
        for (int j = 0; j < 4; j++) add_item<float>(bins, k[j], v[j]);
    }
    for (; i < hi; i += ACC_THREADS) { const float4 v = pv[i]; const uint32_t k = pk[i]; add_item<float>(bins, k, v); }
}
// fp32 items [lo, hi) of a coarse level: 8 consecutive items per lane
__device__ __forceinline__ void add_items_float_coarse(const AccBins& bins, const float4* __restrict__ pv, const uint16_t* __restrict__ pk, uint32_t lo, uint32_t hi) {
    for (uint32_t c = lo + threadIdx.x * 8u; c < hi; c += ACC_THREADS * 8u) {
        float4 v[8]; uint32_t k[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { const uint32_t ii = min(c + (uint32_t)j, hi - 1u); v[j] = pv[ii]; k[j] = pk[ii]; }
        const uint32_t cnt = min(8u, hi - c);
#pragma unroll
        for (int j = 0; j < 8; j++) if ((uint32_t)j < cnt) add_item<float>(bins, k[j], v[j]);
    }
}
// fp16 items [abs_lo, abs_hi) of the queue.
// coarse level: a cell holds many samples of a ray and many rays, so consecutive queue items repeat the same
// key, and same-address LDS atomics of ONE instruction serialise (level 0: 16 workgroups x 70 k atomics at ~2
// cycles each = the whole pass).  Each lane takes 8 CONSECUTIVE items and sums them in registers while the key
// repeats: one atomic group per run, neighbouring lanes 8 items apart.
__device__ __forceinline__ void add_items_half(const AccBins& bins, const uint2* __restrict__ qvals, const uint16_t* __restrict__ qkeys,
                                               uint32_t abs_lo, uint32_t abs_hi, bool coarse) {
    // groups of 8 items on ABSOLUTE 8-item boundaries of the queue: a lane reads one 64-byte line of values and
    // 16 bytes of keys with five 16-byte buffer loads (a partition of a fine level is one round of loads);
    // items of the neighbouring sub-range in the first / last group are masked.  On the coarse levels
    // neighbouring LANES take groups 128 items apart (another ray, usually another cell): lanes 8 items apart sit
    // in the same cell and their atomics to the same 8 entries serialise.
    using u4 = __attribute__((__vector_size__(16))) uint32_t;
    const uint32_t tid = threadIdx.x;
    const uint32_t A0 = abs_lo & ~7u;
    const uint32_t n_groups = (abs_hi - A0 + 7u) >> 3;
    // whole groups are always inside the queue (its capacity is a multiple of 8 items); the range check of a
    // 16-byte buffer load is all-or-nothing, so the records cover whole groups
    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint2*>(qvals + A0), 0, (int)(n_groups * 64u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(qkeys + A0), 0, (int)(n_groups * 16u), 0x00020000);
    for (uint32_t gq = coarse ? (tid & 63u) * (ACC_THREADS / 64) + (tid >> 6) : tid; gq < n_groups; gq += ACC_THREADS) {
        const u4 va = __builtin_amdgcn_raw_buffer_load_b128(rs_v, (int)(gq * 64u), 0, 0);
        const u4 vb = __builtin_amdgcn_raw_buffer_load_b128(rs_v, (int)(gq * 64u + 16u), 0, 0);
        const u4 vc = __builtin_amdgcn_raw_buffer_load_b128(rs_v, (int)(gq * 64u + 32u), 0, 0);
        const u4 vd = __builtin_amdgcn_raw_buffer_load_b128(rs_v, (int)(gq * 64u + 48u), 0, 0);
        const u4 kk = __builtin_amdgcn_raw_buffer_load_b128(rs_k, (int)(gq * 16u), 0, 0);
        const uint32_t w[16] = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3], vc[0], vc[1], vc[2], vc[3], vd[0], vd[1], vd[2], vd[3]};
        const uint32_t a0 = A0 + gq * 8u;
        const uint32_t first = a0 < abs_lo ? abs_lo - a0 : 0u, last = min(8u, abs_hi - a0);
        if (!coarse) {             // finer levels: neighbouring items are unrelated, one atomic group per item
#pragma unroll
            for (int j = 0; j < 8; j++)
                if ((uint32_t)j >= first && (uint32_t)j < last) { uint2 v; v.x = w[2 * j]; v.y = w[2 * j + 1]; add_item<half_t>(bins, (kk[j >> 1] >> (16 * (j & 1))) & 0xffffu, v); }
            continue;
        }
        uint32_t ckey = 0;
        HalfSums s;
        bool started = false;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if ((uint32_t)j >= first && (uint32_t)j < last) {
                const uint32_t kj = (kk[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                if (!started || kj != ckey) {
                    if (started) half_sums_commit(s, ckey, bins);
                    ckey = kj; s = HalfSums{}; started = true;
                }
                half_item_add(s, w[2 * j], w[2 * j + 1]);
            }
        }
        if (started) half_sums_commit(s, ckey, bins);
    }
}

// ---- sub-ranges of one partition: every one ADDS its exact partial sums (int64: the adds commute, so the
// result has the same bits whatever the order) into the partition's merge record with device-scope atomics;
// the last to arrive (told by the value its counter add returned) takes the sums out with atomic exchanges,
// which also leaves the record zero for the next launch.  Every access to the record is an atomic, so no
// fence and no cache maintenance is needed (an agent-scope release here writes back ALL dirty lines of the
// XCD's L2 -- tens of MB of queue right after the fill pass: 40 us per level measured; storing 64 KB partials
// write-through and letting the last arriver add SUB of them: 16 us on its critical path).
// -> true in the workgroup that arrived last: its bins now hold the partition's sums.  Every thread calls it (barriers inside).
template <typename T>
__device__ __forceinline__ bool merge_sub_ranges(const AccBins& bins, unsigned long long* __restrict__ rec, uint32_t* arrivals, uint32_t SUB, uint32_t* s_arr) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr uint32_t ACCW = HALF ? 2 * PART : PART;
    const uint32_t tid = threadIdx.x;
    unsigned long long* acc64 = bins.acc64; uint32_t* poison = bins.poison;
    uint32_t* __restrict__ rec_poison = reinterpret_cast<uint32_t*>(rec + ACCW);
    if constexpr (HALF) {
        for (uint32_t i = tid; i < ACCW; i += ACC_THREADS) { const unsigned long long v = acc64[i]; if (v) atomicAdd(rec + i, v); }
    } else {
        const float* af = reinterpret_cast<const float*>(acc64);
        float* rf = reinterpret_cast<float*>(rec);
        for (uint32_t i = tid; i < 2 * PART; i += ACC_THREADS) { const float v = af[i]; if (v != 0.0f) atomicAdd(rf + i, v); }
    }
    if (tid < PART / 32 && poison[tid]) atomicOr(rec_poison + tid, poison[tid]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *s_arr = atomicAdd(arrivals, 1u);
    __syncthreads();
    if (*s_arr != SUB - 1) return false;
    for (uint32_t i = tid; i < ACCW; i += ACC_THREADS) acc64[i] = atomicExch(rec + i, 0ull);
    if (tid < PART / 32) poison[tid] = atomicExch(rec_poison + tid, 0u);
    __syncthreads();
    return true;
}

// ---- the flushes: the partition's sums -> its n_ent table entries at d
// fp16: old + exact sum, rounded ONCE (this workgroup is the only writer of this table slice); oldv = the lane's old entries
__device__ __forceinline__ void flush_half(const AccBins& bins, uint32_t* __restrict__ d2, const uint32_t (&oldv)[PART / ACC_THREADS], uint32_t n_ent,
                                           int32_t* __restrict__ nf_flag) {
    const uint32_t tid = threadIdx.x;
    bool wrote_nonfinite = false;
#pragma unroll
    for (int it = 0; it < (int)(PART / ACC_THREADS); it++) {
        const uint32_t e = tid + it * ACC_THREADS;
        if (e >= n_ent) break;
        const long long i0 = (long long)bins.acc64[e], i1 = (long long)bins.acc64[PART + e];
        // e >> 5 = (tid >> 5) + 32 * it, e & 31 = tid & 31: one address register for the four words, not four
        const bool bad = (bins.poison[(tid >> 5) + it * (ACC_THREADS / 32)] >> (tid & 31)) & 1u;
        if (i0 == 0 && i1 == 0 && !bad) continue;
        const uint32_t o = oldv[it];
        uint32_t r0, r1;
        if (bad) { r0 = 0x7e00u; r1 = 0x7e00u; }
        else {
            r0 = half_nonfinite(o) ? (o & 0xffffu) : fix24_to_half(i0 + half_to_fix24(o & 0xffffu));
            r1 = half_nonfinite(o >> 16) ? (o >> 16) : fix24_to_half(i1 + half_to_fix24(o >> 16));
        }
        d2[e] = r0 | (r1 << 16);
        wrote_nonfinite |= half_nonfinite(r0) || half_nonfinite(r1);
    }
    // every non-finite value in the table gradient was stored by a flush like this one: the caller's flag (the
    // optimizer's found_inf word) makes a scan of the 12 M-entry gradient for non-finite values unnecessary
    if (nf_flag && wrote_nonfinite) atomicOr(nf_flag, 1);
}
__device__ __forceinline__ void flush_float(const AccBins& bins, float2* __restrict__ d2, uint32_t n_ent, int32_t* __restrict__ nf_flag) {
    const float* af = reinterpret_cast<const float*>(bins.acc64);
    for (uint32_t e = threadIdx.x; e < n_ent; e += ACC_THREADS) {
        const float v0 = af[e], v1 = af[PART + e];
        if (v0 == 0.0f && v1 == 0.0f) continue;
        float2 o = d2[e]; o.x += v0; o.y += v1; d2[e] = o;
        if (nf_flag && !(isfinite(o.x) && isfinite(o.y))) atomicOr(nf_flag, 1);
    }
}

template <typename T>
__global__ __launch_bounds__(ACC_THREADS, 8) void k_bwd_acc(
    const int32_t* __restrict__ offsets, T* __restrict__ grad_grid, uint32_t L, LevelScales sc, uint32_t gridtype,
    bool align_corners, BwdPlan plan, const typename BVal<T>::type* __restrict__ qvals, const uint16_t* __restrict__ qkeys,
    unsigned long long* __restrict__ partials, int32_t* __restrict__ nf_flag, uint32_t bk_target) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr uint32_t ACCW = HALF ? 2 * PART : PART;
    __shared__ unsigned long long acc64[ACCW];
    __shared__ uint32_t poison[PART / 32];
    __shared__ uint32_t s_cnt[MAX_LEVELS], s_sub[MAX_LEVELS], s_first[MAX_LEVELS];
    __shared__ uint32_t s_ticket, s_arr;
    const uint32_t tid = threadIdx.x;
    const AccBins bins = {acc64, poison};
    const uint32_t total_buckets = build_ticket_table(offsets, L, bk_target, s_cnt, s_sub, s_first, &s_arr);

    // the first task of every workgroup is its own index (gridDim.x same-address atomics at launch would queue up behind one
    // another); later tasks are drawn from the ticket counter, which therefore counts from gridDim.x
    bool first_task = true;
    uint32_t tail_task;                                         // first ticket behind the partition tasks
    [[maybe_unused]] uint32_t stamp_task = 0;
    GRID_STAMP(4096 + blockIdx.x, 0);
    for (;;) {
        if (tid == 0) s_ticket = first_task ? blockIdx.x : atomicAdd(&plan.tickets[0], 1u) + gridDim.x;
        first_task = false;
        __syncthreads();
        const uint32_t t = __builtin_amdgcn_readfirstlane(s_ticket);       // scalar: everything derived from it is wave-uniform
        GRID_STAMP(4096 + blockIdx.x, 1 + stamp_task * 6);                   // ticket in hand
        if (t >= total_buckets) { tail_task = t - total_buckets; break; }
        GRID_NOTE(4096 + blockIdx.x, 2 + stamp_task * 6, t);
        const AccTask k = decode_ticket(t, L, s_first, s_sub);
        const uint32_t level = k.level, p = k.p;
        const uint32_t table_off = (uint32_t)offsets[level], hashmap_size = (uint32_t)offsets[level + 1] - table_off;
        const AccRange r = partition_range(plan, level, p);
        const uint32_t n = r.n, q0 = r.q0;
        const uint32_t lo = (uint32_t)(((uint64_t)n * k.sub) / k.SUB), hi = (uint32_t)(((uint64_t)n * (k.sub + 1)) / k.SUB);
        if (n == 0) { __syncthreads(); continue; }              // uniform per (level, partition): no sub-range has work
        const uint32_t part_lo = p << PART_SHIFT;
        const uint32_t n_ent = min(PART, hashmap_size - part_lo);
        T* __restrict__ dst = grad_grid + ((size_t)table_off + part_lo) * 2;
        uint32_t oldv[PART / ACC_THREADS];
        open_partition<T>(bins, reinterpret_cast<const uint32_t*>(dst), r.dirty ? n_ent : 0u, oldv);
        GRID_STAMP(4096 + blockIdx.x, 3 + stamp_task * 6);                   // zeroed
        const bool coarse = (uint32_t)ceilf(sc.scale[level]) + 1 < COARSE_RES;
        if constexpr (HALF) add_items_half(bins, qvals, qkeys, q0 + lo, q0 + hi, coarse);
        else if (!coarse) add_items_float_fine(bins, qvals + q0, qkeys + q0, lo, hi);
        else add_items_float_coarse(bins, qvals + q0, qkeys + q0, lo, hi);
        GRID_STAMP(4096 + blockIdx.x, 4 + stamp_task * 6);                   // thread 0 out of the items
        __syncthreads();
        GRID_STAMP(4096 + blockIdx.x, 5 + stamp_task * 6);                   // every wave out of the items
        if (k.SUB > 1) {
            unsigned long long* __restrict__ rec = partials + (size_t)(level * SUB_RECS + p) * sub_rec_words<T>();
            if (!merge_sub_ranges<T>(bins, rec, &plan.tickets[TICKET_ARRIVALS + level * SUB_RECS + p], k.SUB, &s_arr)) {
                GRID_STAMP(4096 + blockIdx.x, 6 + stamp_task * 6); stamp_task++; __syncthreads(); continue;
            }
        }
        if constexpr (HALF) flush_half(bins, reinterpret_cast<uint32_t*>(dst), oldv, n_ent, nf_flag);
        else flush_float(bins, reinterpret_cast<float2*>(dst), n_ent, nf_flag);
        GRID_STAMP(4096 + blockIdx.x, 6 + stamp_task * 6);                   // flushed
        stamp_task++;
        __syncthreads();
    }
    // tail tasks (fused field backward): the tickets behind the partition tasks reduce the MLP weight-gradient slabs and finish the
    // deferred loss, one block of k_dw_reduce2 each, where workgroups are running out of partitions.  Tickets only grow, so a
    // workgroup that has drawn one of them draws no partition task any more: a loop of its own, in which nothing of the loop
    // above is live (inside it the tail's addresses cost scalar registers the pass does not have).  The LDS scratch aliases
    // acc64; the job was left in the plan by the fill pass (n_tasks == 0: none).
    static_assert(sizeof(acc64) >= lae_dw::DWR_LDS_FLOATS * sizeof(float) && ACC_THREADS == (int)lae_dw::DWR_THREADS, "tail tasks run in this workgroup");
    const lae_dw::DwTailJob& tail = *plan_tail_job(plan);
    const uint32_t n_tail = __builtin_amdgcn_readfirstlane(tail.n_tasks);
    while (tail_task < n_tail) {
        lae_dw::dw_tail_task(tail, tail_task, reinterpret_cast<float*>(acc64));     // one barrier inside: every wave has read s_ticket
        if (tid == 0) s_ticket = atomicAdd(&plan.tickets[0], 1u) + gridDim.x;
        __syncthreads();
        tail_task = __builtin_amdgcn_readfirstlane(s_ticket) - total_buckets;
    }
}

// [B][L][2] -> [L][B][2] through an LDS tile (256 samples x L levels), coalesced on both sides
template <typename T>
__global__ __launch_bounds__(256) void k_grad_transpose(const T* __restrict__ in, T* __restrict__ out, uint32_t B, uint32_t L) {
    using V = typename std::conditional<sizeof(T) == 2, uint32_t, uint2>::type;     // one (c0, c1) pair
    __shared__ V tile[256 * 33];
    const uint32_t b0 = blockIdx.x * 256;
    const uint32_t nb = min(256u, B - b0);
    const V* src = reinterpret_cast<const V*>(in) + (size_t)b0 * L;
    for (uint32_t e = threadIdx.x; e < nb * L; e += 256) tile[(e / L) * (L + 1) + (e % L)] = src[e];
    __syncthreads();
    V* dstv = reinterpret_cast<V*>(out);
    for (uint32_t e = threadIdx.x; e < nb * L; e += 256) {
        const uint32_t l = e / nb, b = e % nb;
        dstv[(size_t)l * B + b0 + b] = tile[b * (L + 1) + l];
    }
}

// ---------------------------------------------------------------- K15
// gridencoder.cu:343-369
template <typename T>
__global__ void k_grid_input_bwd(const T* __restrict__ grad, const T* __restrict__ dy_dx, T* __restrict__ grad_inputs,
                                 uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint64_t gs_b, uint64_t gs_l) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    const T* dd = dy_dx + (size_t)b * L * D * C;
    T r = (T)0.0f;
    for (uint32_t l = 0; l < L; l++)
        for (uint32_t ch = 0; ch < C; ch++) {
            const T gv = grad[(size_t)b * gs_b + (size_t)l * gs_l + ch];
            const T dv = dd[(size_t)l * D * C + d * C + ch];
            if constexpr (sizeof(T) == 2) r = (half_t)((float)r + (float)(half_t)((float)gv * (float)dv));
            else r = fmaf(gv, dv, r);
        }
    grad_inputs[t] = r;
}

// ---------------------------------------------------------------- host dispatch
struct BwdArgs {
    const void* grad; const float* inputs; const int32_t* offsets; void* gemb; uint32_t B, L; LevelScales sc;
    uint32_t gridtype; bool align; uint32_t interp; uint64_t gs_b, gs_l; hipStream_t stream;
    const int32_t* offsets_host = nullptr;
    int32_t* nf_flag = nullptr;                                 // set to 1 when a non-finite table gradient is stored (binned path)
    uint32_t* touched = nullptr;                                // bit per 8 table entries (one 64-byte line of fp32 pairs): set by the count pass
    uint32_t* touched_full = nullptr;                           // MAX_LEVELS words behind the bitmap: level l is fully marked
    uint32_t* dirty = nullptr;                                  // the accumulator's "dirty" word (include/laenerf.h), or NULL
    const lae_dw::DwTailJob* tail = nullptr;                    // binned fp16 path only: tasks the accumulate pass takes along
};
template <typename T, int D, int C>
static void launch_bwd(const BwdArgs& a) {
    const uint32_t nb = lae::cdiv(a.B, GRID_BLOCK);
    const bool xcd = (a.L % 8) == 0;
    k_grid_bwd<T, D, C><<<nb * a.L, GRID_BLOCK, 0, a.stream>>>((const T*)a.grad, a.inputs, a.offsets, (T*)a.gemb, a.B, a.L, a.sc, a.gridtype, a.align,
                                                                a.interp, nb, xcd, a.gs_b, a.gs_l, false, a.dirty);
}
template <typename T, int D>
static int dispatch_bwd_c(const BwdArgs& a, uint32_t C) {
    switch (C) {
        case 1: if constexpr (sizeof(T) == 4) { launch_bwd<T, D, 1>(a); return LAE_OK; } return LAE_EINVAL;   // odd C in fp16 is rejected, grid.py:42-44 never produces it
        case 2: launch_bwd<T, D, 2>(a); return LAE_OK;
        case 4: launch_bwd<T, D, 4>(a); return LAE_OK;
        case 8: launch_bwd<T, D, 8>(a); return LAE_OK;
        default: return LAE_EINVAL;
    }
}
template <typename T>
static int dispatch_bwd_d(const BwdArgs& a, uint32_t D, uint32_t C) {
    switch (D) {
        case 2: return dispatch_bwd_c<T, 2>(a, C);
        case 3: return dispatch_bwd_c<T, 3>(a, C);
        case 4: return dispatch_bwd_c<T, 4>(a, C);
        case 5: return dispatch_bwd_c<T, 5>(a, C);
        default: return LAE_EINVAL;
    }
}

// 0 = binned LDS pipeline where available (default), 1 = always the generic global-atomic kernel
static int g_force_atomic_bwd = 0;

// the shapes the binned pipeline is built for, and whether it runs for them (lae_grid_set_backward_mode(1) switches it off)
static inline bool binned_shape(uint32_t D, uint32_t C, uint32_t L, uint32_t B) { return D == 3 && C == 2 && L <= 32 && B <= BWD_MAX_SAMPLES; }
static inline bool binned_path_runs(uint32_t D, uint32_t C, uint32_t L, uint32_t B) { return binned_shape(D, C, L, B) && !g_force_atomic_bwd; }
// every level of the caller's host copy of the level offsets goes through the binned pipeline (none is left to k_grid_bwd)
static inline bool all_levels_binned(const int32_t* offsets_host, uint32_t L) {
    for (uint32_t l = 0; l < L; l++)
        if (!level_is_binned((uint32_t)(offsets_host[l + 1] - offsets_host[l]))) return false;
    return true;
}
static inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// words of the "ever touched" bitmap proper (one bit per 8 entries, + 2 words of slack); MAX_LEVELS words of per-level
// "fully marked" flags follow it (include/laenerf.h)
static inline size_t touched_words(const int32_t* offsets_host, uint32_t L) { return ((size_t)offsets_host[L] >> 3 >> 5) + 2; }

// What a backward request may not ask for (-> LAE_EINVAL), and the launch arguments of one that may run.  Shared by
// lae_grid_encode_backward_plan (plan_pass: positions only), grid_backward and lae_nerf_field_backward, which refuses before its first launch.
static int bwd_args(BwdArgs& a, const void* grad, const float* inputs, const int32_t* offsets, void* gemb, uint32_t B, uint32_t D, uint32_t C,
                    uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, bool blc,
                    float in_shift, float in_scale, const int32_t* offsets_host, const void* plan, int32_t* nf_flag, uint32_t* touched,
                    uint32_t* dirty, const lae_dw::DwTailJob* tail, void* stream, bool plan_pass = false) {
    if (gridtype > 1 || interp > 1 || (dtype != LAE_F32 && dtype != LAE_F16)) return LAE_EINVAL;
    if (plan_pass && !binned_shape(D, C, L, B)) return LAE_EINVAL;
    const bool binned = binned_path_runs(D, C, L, B);
    // tail tasks ride in the accumulate pass of the binned fp16 pipeline and nowhere else
    if (tail && !(binned && dtype == LAE_F16)) return LAE_EINVAL;
    if (plan && !(binned && !blc)) return LAE_EINVAL;
    if (touched && dtype != LAE_F16) return LAE_EINVAL;
    // only the binned pipeline knows what it stores (the generic kernel's float atomics do not): every level must go
    // through it, which the host copy of the level sizes proves
    if ((nf_flag || touched) && !(binned && offsets_host && all_levels_binned(offsets_host, L))) return LAE_EINVAL;
    a.grad = grad; a.inputs = inputs; a.offsets = offsets; a.gemb = gemb; a.B = B; a.L = L;
    if (const int rc = fill_scales(a.sc, L, S, H)) return rc;
    a.sc.in_shift = in_shift; a.sc.in_scale = in_scale;
    a.gridtype = gridtype; a.align = align_corners != 0; a.interp = interp;
    a.gs_b = blc ? (uint64_t)L * C : C;
    a.gs_l = blc ? C : (uint64_t)B * C;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    a.offsets_host = offsets_host; a.nf_flag = nf_flag; a.dirty = dirty; a.tail = tail;
    a.touched = touched; a.touched_full = touched ? touched + touched_words(offsets_host, L) : nullptr;
    return LAE_OK;
}

// The binned backward in two halves.  PLAN (count pass + scans) reads the sample positions only and fills {tickets |
// partition totals | partition offsets | per-unit counter rows | per-partition unit table}; EXEC (fill + accumulate) needs the
// gradients.  A caller may run PLAN early -- e.g. right after the march, on another stream beside the forward pass
// (lae_grid_encode_backward_plan) -- the default entry points run both back to back with the plan in the library workspace.
// Library workspace of EXEC: {partial sums of sub-ranges | queue: values, keys}; the queue is sized for the worst case of 8
// items per (sample, level) -- hashed levels produce 4 -- and only its front is ever touched.
struct PlanLayout { size_t totals_off, offs_off, cnt_off, part_off, bytes; };
static inline uint32_t bwd_units(uint32_t B) { return lae::cdiv(B, UNIT_SAMPLES); }
static inline PlanLayout plan_layout(uint32_t B, uint32_t L) {
    const size_t U = bwd_units(B);
    PlanLayout w;
    w.totals_off = up256((size_t)TICKET_WORDS * 4 + sizeof(lae_dw::DwTailJob) + 4);
    w.offs_off = w.totals_off + up256((size_t)L * BK_MAX * 4);
    w.cnt_off = w.offs_off + up256((size_t)L * BK_MAX * 4);
    w.part_off = w.cnt_off + up256((size_t)L * U * BK_MAX * 2);
    w.bytes = w.part_off + up256((size_t)L * BK_MAX * U * 4);
    return w;
}
static inline BwdPlan plan_at(void* buf, uint32_t B, uint32_t L) {
    const PlanLayout lay = plan_layout(B, L);
    uint8_t* p = reinterpret_cast<uint8_t*>(buf);
    return BwdPlan{reinterpret_cast<uint16_t*>(p + lay.cnt_off), reinterpret_cast<uint32_t*>(p + lay.part_off), reinterpret_cast<uint32_t*>(p + lay.totals_off),
                   reinterpret_cast<uint32_t*>(p + lay.offs_off), reinterpret_cast<uint32_t*>(p)};      // {cnt, part_cnt, totals, offs, tickets}
}
// merge records of split partitions: at the START of the workspace, sized for MAX_LEVELS whatever the call (their place
// must not move with B or L: they are zeroed once per buffer and every launch leaves them zero)
static inline size_t merge_bytes() { return up256((size_t)MAX_LEVELS * SUB_RECS * sub_rec_words<half_t>() * 8); }
// items the queue holds: the worst case of 8 per (sample, level)
static inline size_t queue_items(uint32_t B, uint32_t L) { return (size_t)L * bwd_units(B) * UNIT_SAMPLES * 8; }
template <typename T>
static inline size_t bwd_exec_ws_bytes(uint32_t B, uint32_t L) {
    return merge_bytes() + up256(queue_items(B, L) * sizeof(typename BVal<T>::type)) + up256(queue_items(B, L) * 2);
}

// one walk pass: the PLAIN instantiation for the shipped configuration, U * L blocks
template <typename T, bool FILL>
static void launch_walk(const BwdArgs& a, size_t lds_bytes, const T* g, const BwdPlan& plan, typename BVal<T>::type* qvals, uint16_t* qkeys, uint32_t* touched,
                        uint32_t* level_full, uint32_t* dirty, const lae_dw::DwTailJob& tail) {
    const uint32_t U = bwd_units(a.B);
    const auto walk = (a.gridtype == 0 && !a.align && a.interp == 0) ? k_bwd_walk<T, FILL, true> : k_bwd_walk<T, FILL, false>;
    walk<<<U * a.L, FILL_THREADS, lds_bytes, a.stream>>>(g, a.inputs, a.offsets, a.B, a.L, a.sc, a.gridtype, a.align, a.interp, U, plan, qvals, qkeys, touched, level_full, dirty, tail);
}

template <typename T>
static void bwd_plan(const BwdArgs& a, const BwdPlan& plan) {
    const uint32_t B = a.B, L = a.L, U = bwd_units(B);
    // the count pass keeps the line bits of its level in LDS when the caller wants its "ever touched" bitmap maintained:
    // room for the largest level (a.touched implies a.offsets_host and every level <= 2^21 entries, checked by bwd_args)
    size_t line_lds = 0;
    if (a.touched) {
        uint32_t words = 1;
        for (uint32_t l = 0; l < L; l++) {
            const uint32_t off = (uint32_t)a.offsets_host[l], size = (uint32_t)(a.offsets_host[l + 1] - a.offsets_host[l]);
            words = std::max(words, ((((off >> 3) & 31u) + ((size + 7u) >> 3) + 31u) >> 5));
        }
        line_lds = (size_t)words * 4;
    }
    launch_walk<T, false>(a, line_lds, nullptr, plan, nullptr, nullptr, a.touched, a.touched_full, nullptr, lae_dw::DwTailJob{});
    k_bwd_scan_units<<<lae::cdiv((size_t)L * BK_MAX, 4), 256, 0, a.stream>>>(a.offsets, L, U, plan);
    k_bwd_scan_parts<<<1, 1024, 0, a.stream>>>(L * BK_MAX, plan);
}

// gT: the gradients, level-major [L, B, 2]
template <typename T>
static int launch_bwd_fast(const void* gT, const BwdArgs& a, const void* caller_plan = nullptr) {
    using V = typename BVal<T>::type;
    const uint32_t B = a.B, L = a.L;
    const size_t plan_bytes = caller_plan ? 0 : plan_layout(B, L).bytes;
    uint8_t* ws = reinterpret_cast<uint8_t*>(lae::workspace(lae::WS_GRID_BINS, plan_bytes + bwd_exec_ws_bytes<T>(B, L), a.stream));
    if (!ws) return LAE_ELAUNCH;
    unsigned long long* partials = reinterpret_cast<unsigned long long*>(ws);
    {   // the merge records must start at zero (afterwards every launch leaves them zero): once per buffer
        static std::mutex mtx;
        static std::vector<void*> zeroed;
        static uint64_t epoch = 0;
        std::lock_guard<std::mutex> lk(mtx);
        if (epoch != lae::workspace_epoch()) { zeroed.clear(); epoch = lae::workspace_epoch(); }
        if (std::find(zeroed.begin(), zeroed.end(), (void*)ws) == zeroed.end()) {
            if (hipMemsetAsync(ws, 0, merge_bytes(), a.stream) != hipSuccess) {
                (void)hipGetLastError();
                lae::set_last_error_str("grid backward: could not zero the merge records (first call inside a capture? warm up eagerly)");
                return LAE_ELAUNCH;
            }
            if (zeroed.size() > 64) zeroed.clear();
            zeroed.push_back((void*)ws);
        }
    }
    const BwdPlan plan = plan_at(caller_plan ? const_cast<void*>(caller_plan) : ws + merge_bytes(), B, L);
    uint8_t* ex = ws + merge_bytes() + plan_bytes;
    V* qvals = reinterpret_cast<V*>(ex);
    uint16_t* qkeys = reinterpret_cast<uint16_t*>(ex + up256(queue_items(B, L) * sizeof(V)));
    const T* g = (const T*)gT;
    T* ge = (T*)a.gemb;
    if (!caller_plan) bwd_plan<T>(a, plan);
    const lae_dw::DwTailJob tail_job = a.tail ? *a.tail : lae_dw::DwTailJob{};
    launch_walk<T, true>(a, 0, g, plan, qvals, qkeys, nullptr, nullptr, a.dirty, tail_job);
    // workgroups per level: 32 up to ~400 k samples, 64 beyond (same-box A/B in round 4: lego, 258 k samples, 0.3508 / 0.3547 ms per
    // step at 32 / 64; flower, 658 k, 0.666 / 0.647) -- the smallest levels' few cells take every sample's LDS atomics
    // a split level (P < bk_target) owns one merge record per partition and its arrival tickets are indexed with SUB_RECS: the
    // choice made here may never exceed it.  The records are sized for MAX_LEVELS x SUB_RECS whatever the call
    // (135 MB, zeroed once per buffer: their place must not move with B or L) -- 0.05 % of the card's HBM, a conscious choice.
    static_assert(BK_TARGET <= SUB_RECS && 64u <= SUB_RECS, "bk_target choices must fit the merge records");
    const uint32_t bk_target = std::min(B >= 400000u ? 64u : BK_TARGET, SUB_RECS);
    k_bwd_acc<T><<<(uint32_t)lae::num_cus() * 2, ACC_THREADS, 0, a.stream>>>(a.offsets, ge, L, a.sc, a.gridtype, a.align, plan, qvals, qkeys, partials, a.nf_flag, bk_target);
    // levels with more partitions than a directory row holds (more than 2^21 entries): generic atomic kernel.  With the
    // caller's host copy of the level sizes the launch is skipped when no level needs it; without one it is always made
    // (its blocks return at once for the levels the binned path has handled).
    if (!a.offsets_host || !all_levels_binned(a.offsets_host, L)) {
        const uint32_t nbg = lae::cdiv(B, GRID_BLOCK);
        k_grid_bwd<T, 3, 2><<<nbg * L, GRID_BLOCK, 0, a.stream>>>(g, a.inputs, a.offsets, ge, B, L, a.sc, a.gridtype, a.align, a.interp, nbg,
                                                                  (L % 8) == 0, 2, (uint64_t)B * 2, true);
    }
    return LAE_OK;
}

static int grid_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                         void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                         const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners, uint32_t interp,
                         int dtype, bool blc, void* stream, float in_shift = 0.0f, float in_scale = 1.0f,
                         const int32_t* offsets_host = nullptr, const void* plan = nullptr, int32_t* nf_flag = nullptr,
                         uint32_t* touched = nullptr, uint32_t* dirty = nullptr, const lae_dw::DwTailJob* tail = nullptr) {
    (void)embeddings;
    if (B == 0) return LAE_OK;
    if (!grad || !inputs || !offsets || !grad_embeddings) return LAE_ENULL;
    BwdArgs a;
    int rc = bwd_args(a, grad, inputs, offsets, grad_embeddings, B, D, C, L, S, H, gridtype, align_corners, interp, dtype, blc, in_shift,
                      in_scale, offsets_host, plan, nf_flag, touched, dirty, tail, stream);
    if (rc) return rc;
    if (binned_path_runs(D, C, L, B)) {
        // binned path (k_bwd_walk / k_bwd_acc); [B, L*2] grads are transposed into the workspace first
        const size_t esz = dtype == LAE_F16 ? 2 : 4;
        const void* gT = grad;
        if (blc) {
            void* ws = lae::workspace(lae::WS_GRID_GRAD_T, (size_t)B * L * 2 * esz, a.stream);
            if (!ws) return LAE_ELAUNCH;
            if (dtype == LAE_F16) k_grad_transpose<half_t><<<lae::cdiv(B, 256), 256, 0, a.stream>>>((const half_t*)grad, (half_t*)ws, B, L);
            else k_grad_transpose<float><<<lae::cdiv(B, 256), 256, 0, a.stream>>>((const float*)grad, (float*)ws, B, L);
            gT = ws;
        }
        rc = (dtype == LAE_F16) ? launch_bwd_fast<half_t>(gT, a, plan) : launch_bwd_fast<float>(gT, a, plan);
    } else if (dtype == LAE_F32) rc = dispatch_bwd_d<float>(a, D, C);
    else rc = dispatch_bwd_d<half_t>(a, D, C);
    if (rc) return rc;
    if (dy_dx && grad_inputs) {                           // :410 kernel_input_backward
        const uint32_t n = B * D;
        if (dtype == LAE_F32) k_grid_input_bwd<float><<<lae::cdiv(n, 256), 256, 0, a.stream>>>((const float*)grad, (const float*)dy_dx, (float*)grad_inputs, B, D, C, L, a.gs_b, a.gs_l);
        else k_grid_input_bwd<half_t><<<lae::cdiv(n, 256), 256, 0, a.stream>>>((const half_t*)grad, (const half_t*)dy_dx, (half_t*)grad_inputs, B, D, C, L, a.gs_b, a.gs_l);
    }
    return lae::check_launch("grid_encode_backward");
}

}  // namespace

extern "C" {

int lae_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                             void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             const void* dy_dx, void* grad_inputs, uint32_t gridtype, int align_corners,
                             uint32_t interp, int dtype, void* stream) {
    return grid_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs,
                         gridtype, align_corners, interp, dtype, false, stream);
}

int lae_grid_encode_backward_ex(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype,
                                int align_corners, uint32_t interp, int dtype, int blc, float in_shift, float in_scale,
                                const int32_t* offsets_host, int32_t* nonfinite_flag, uint32_t* touched_lines, uint32_t* grad_dirty,
                                void* stream) {
    return grid_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs,
                         gridtype, align_corners, interp, dtype, blc != 0, stream, in_shift, in_scale, offsets_host, nullptr,
                         nonfinite_flag, touched_lines, grad_dirty);
}

uint64_t lae_grid_backward_workspace_bytes(uint32_t B, uint32_t L, int dtype) {
    return plan_layout(B, L).bytes + (dtype == LAE_F16 ? bwd_exec_ws_bytes<half_t>(B, L) : bwd_exec_ws_bytes<float>(B, L));
}

uint64_t lae_grid_backward_plan_bytes(uint32_t B, uint32_t L) { return plan_layout(B, L).bytes; }

uint64_t lae_grid_touched_lines_words(uint64_t n_entries) { return (n_entries >> 3 >> 5) + 2 + MAX_LEVELS; }

int lae_grid_encode_backward_plan(const float* inputs, const int32_t* offsets, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                  uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, float in_shift,
                                  float in_scale, const int32_t* offsets_host, void* plan, uint32_t* touched_lines, void* stream) {
    if (B == 0) return LAE_OK;
    if (!inputs || !offsets || !plan) return LAE_ENULL;
    BwdArgs a;                                             // (touched_lines: every level must go through this pass, see lae_grid_encode_backward_ex)
    if (const int rc = bwd_args(a, nullptr, inputs, offsets, nullptr, B, D, C, L, S, H, gridtype, align_corners, interp, dtype, false, in_shift,
                                in_scale, offsets_host, nullptr, nullptr, touched_lines, nullptr, nullptr, stream, true)) return rc;
    if (dtype == LAE_F16) bwd_plan<half_t>(a, plan_at(plan, B, L));
    else bwd_plan<float>(a, plan_at(plan, B, L));
    return lae::check_launch("grid_encode_backward_plan");
}

int lae_grid_encode_backward_planned(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t B,
                                     uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                     uint32_t interp, int dtype, float in_shift, float in_scale, const int32_t* offsets_host,
                                     const void* plan, int32_t* nonfinite_flag, uint32_t* grad_dirty, void* stream) {
    if (!plan) return LAE_ENULL;
    return grid_backward(grad, inputs, nullptr, offsets, grad_embeddings, B, D, C, L, S, H, nullptr, nullptr, gridtype, align_corners,
                         interp, dtype, false, stream, in_shift, in_scale, offsets_host, plan, nonfinite_flag, nullptr, grad_dirty);
}

// Fused field backward: colour-net backward, sigma-net backward, fill pass, accumulate pass -- lae_nerf_head_backward (level-major
// encoder features) followed by lae_grid_encode_backward_ex / _planned (D = 3, C = 2, fp16, level-major gradients) in one call, so
// that the reduction of the MLP weight-gradient slabs and the deferred loss value need no launch of their own: they ride as tail
// tasks in the accumulate pass (k_bwd_acc), behind its partition tasks.  Same bits as the two calls.  Where the binned pipeline
// does not run (more than 32 levels or 2^24 samples, lae_grid_set_backward_mode(1)) and under LAE_FIELD_NO_RIDE_ALONG=1 (A/B
// switch, read at every call) the two calls are made as they are.
int lae_nerf_field_backward(const float* grad_sigmas, const float* grad_rgbs, const void* enc, const float* dirs, const void* h,
                            const float* rgbs, const void* sigma_weights, const void* color_weights, uint32_t M, float density_scale,
                            void* grad_h, void* grad_enc, void* grad_sigma_weights, void* grad_color_weights,
                            int accumulate_weight_grads, int32_t* weights_nonfinite_flag, const float* loss_partials,
                            uint32_t loss_n_part, uint32_t loss_n_elem, const float* loss_scale, float* loss_out,
                            const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t L, float S, uint32_t H,
                            uint32_t gridtype, int align_corners, uint32_t interp, float in_shift, float in_scale,
                            const int32_t* offsets_host, const void* plan, int32_t* table_nonfinite_flag, uint32_t* touched_lines,
                            uint32_t* grad_dirty, void* stream) {
    // everything either half would refuse is refused here, before the first launch
    if (!grad_sigma_weights || !grad_color_weights) return LAE_ENULL;
    if (loss_out && (!loss_partials || loss_n_elem == 0)) return LAE_EINVAL;
    if (M > 0) {
        if (!grad_sigmas || !grad_rgbs || !enc || !dirs || !h || !rgbs || !sigma_weights || !color_weights || !grad_h || !grad_enc ||
            !inputs || !offsets || !grad_embeddings) return LAE_ENULL;
        if (M % 16 != 0) return LAE_EINVAL;
        BwdArgs a;
        if (const int rc = bwd_args(a, grad_enc, inputs, offsets, grad_embeddings, M, 3, 2, L, S, H, gridtype, align_corners, interp, LAE_F16,
                                    false, in_shift, in_scale, offsets_host, plan, table_nonfinite_flag, touched_lines, grad_dirty, nullptr,
                                    stream)) return rc;
    }
    const char* off = getenv("LAE_FIELD_NO_RIDE_ALONG");
    const bool ride = M > 0 && binned_path_runs(3, 2, L, M) && !(off && off[0] == '1');
    lae_dw::DwTailJob tail{};
    int rc = lae::nerf_head_backward(grad_sigmas, grad_rgbs, enc, dirs, h, rgbs, sigma_weights, color_weights, M, density_scale, grad_h,
                                     grad_enc, grad_sigma_weights, grad_color_weights, accumulate_weight_grads, 1, weights_nonfinite_flag,
                                     loss_partials, loss_n_part, loss_n_elem, loss_scale, loss_out, stream, ride ? &tail : nullptr);
    if (rc != LAE_OK) return rc;
    // with a plan the bitmap was maintained by lae_grid_encode_backward_plan
    return grid_backward(grad_enc, inputs, nullptr, offsets, grad_embeddings, M, 3, 2, L, S, H, nullptr, nullptr, gridtype, align_corners,
                         interp, LAE_F16, false, stream, in_shift, in_scale, offsets_host, plan, table_nonfinite_flag,
                         plan ? nullptr : touched_lines, grad_dirty, ride ? &tail : nullptr);
}

int lae_grid_set_backward_mode(int mode) {
    if (mode != 0 && mode != 1) return LAE_EINVAL;
    g_force_atomic_bwd = mode;
    return LAE_OK;
}

}  // extern "C"

#ifdef LAE_GRID_STAMPS
GRID_STAMPS_READER(lae_debug_grid_bwd_stamps)
#endif
