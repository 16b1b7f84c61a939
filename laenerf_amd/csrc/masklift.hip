// masklift.hip -- lift 2D masks of a few posed views into the edit grid's selection bitfield.
//
// The reference starts a selection from mouse clicks in its GUI (nerf/gui.py -> Trainer.project_points -> EditGrid.new_from_points);
// there is no GUI here, and what a headless user has are 2D masks (metrics.load_masks).  This is a project-and-vote pass over
// (occupied cells x views).
//
// THE RULE.  Per view v: a camera-to-world pose [R | o], one set of intrinsics (fx, fy, cx, cy), and per pixel the raw `sum w t`
// (depth) and `weights_sum` (opacity) of render_eval(scale_depth=False) -- t is the Euclidean distance along the unit ray -- and a
// mask byte (nonzero = selected).
//   surface    t_surf = depth / opacity if opacity >= min_opacity, else +inf (a transparent pixel has nothing in front).  The pack
//              kernel stores |t_surf| with the sign bit set iff the mask is set: one fp32 per pixel, one gather per (cell, view).
//   cell       (cascade c, coordinates (x, y, z) in G^3); centre w = (((coord + 0.5) / G) * 2 - 1) * mip_bound, mip_bound =
//              min(2^c, bound): the inverse of the marcher's cell lookup.  Its bit sits where density_bitfield keeps it (Morton order,
//              cascade-major).  Only cells whose density_bitfield bit is set take part; cells of a coarser cascade inside a finer
//              cascade's box are NOT skipped (the marcher samples them when dt_gamma > 0).
//   projection d = w - o, q = R^T d.  q.z <= 0: no vote.  u = fx q.x / q.z + cx, v = fy q.y / q.z + cy (pixel centres at +0.5, as
//              pinhole_ray); outside [0, W) x [0, H): no vote.  The pixel is (floor u, floor v), t_cell = |d|.
//   visibility t_cell <= t_surf + depth_margin * side, side = 2 mip_bound / G.  Not visible (occluded): no vote.  A NaN t_surf
//              never votes.  Visible with the mask set: in += 1; visible with the mask clear: out += 1.
//   decision   selected iff occupied and in >= min_views and float(in) >= min_share * float(in + out) (one fp32 multiply, one
//              compare).  Integer votes: the result is the same bits from run to run.
// There is no visual-hull fill of cells hidden in every view (masks mark visible surface, not silhouettes through occluders);
// depth_margin sets how many cells deep the selected shell is.
//
// Every fp32 statement below is one rounding (the library is built with -ffp-contract=off; divisions and the root are the
// correctly rounded ones), and editing/mask_lift.py's mask_lift_numpy(dtype=float32) writes the same statements in the same order.
#include "lae_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

__device__ __forceinline__ uint32_t morton_compact(uint32_t x) {  // raymarching.cu:73-81
    x &= 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

constexpr int ML_THREADS = 256, ML_WAVES = ML_THREADS / 64, ML_POSE_CHUNK = LAE_MASK_LIFT_POSE_CHUNK;

__global__ __launch_bounds__(256) void k_mask_lift_pack(const float* __restrict__ depth, const float* __restrict__ opacity,
                                                        const uint8_t* __restrict__ mask, uint32_t n, float min_opacity,
                                                        float* __restrict__ packed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float a = opacity[i];
    const float t = a >= min_opacity ? __fdiv_rn(depth[i], a) : __builtin_inff();
    const uint32_t b = (__builtin_bit_cast(uint32_t, t) & 0x7fffffffu) | (mask[i] ? 0x80000000u : 0u);
    packed[i] = __builtin_bit_cast(float, b);
}

// One workgroup per ML_THREADS consecutive cells of the cascade-major Morton order; thread <-> cell for the occupancy read, the
// decision and the stores (a wave's 64 decisions are 8 bitfield bytes through a ballot).  In between, the occupied cells of the
// workgroup (n of them, typically none or most: occupancy clusters in Morton order) are compacted into slots, and the threads are
// re-dealt as (slot, slice): slice s of S = ML_THREADS / next_pow2(n) takes the views s, s + S, ... of its cell, so a workgroup with
// few occupied cells spreads the views of each over its waves instead of idling.  Consecutive lanes keep consecutive occupied cells
// of one view: they gather neighbouring pixels, and they read the same pose from LDS (a broadcast).  The partial votes meet in LDS
// by plain stores and an owner's sum: no atomics.
__global__ __launch_bounds__(ML_THREADS) void k_mask_lift(const float* __restrict__ packed, const float* __restrict__ poses, uint32_t V,
                                                          float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                                          const uint8_t* __restrict__ bits, uint32_t total, uint32_t cshift, float rG,
                                                          float bound, float depth_margin, uint32_t min_views, float min_share,
                                                          uint8_t* __restrict__ grid_out, uint16_t* __restrict__ votes_out) {
    __shared__ float P[ML_POSE_CHUNK * 12];
    __shared__ uint32_t part[ML_THREADS];              // in | out << 16 of thread (slice, slot)
    __shared__ uint16_t slot_tid[ML_THREADS];          // slot -> thread (cell) of the workgroup
    __shared__ uint32_t wave_cnt[ML_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t base = blockIdx.x * ML_THREADS, gi = base + tid;
    const bool live = gi < total;
    const bool occ = live && ((bits[gi >> 3] >> (gi & 7u)) & 1u);
    const unsigned long long om = __ballot(occ);
    if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(om);
    __syncthreads();
    uint32_t n = 0, before = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)ML_WAVES; k++) {
        const uint32_t c = wave_cnt[k];
        before += k < wv ? c : 0u;
        n += c;
    }
    const uint32_t rank = before + (uint32_t)__popcll(om & ((1ull << lane) - 1ull));
    uint32_t mine = 0;                                 // in | out << 16; in + out <= V <= 65535, so neither half carries
    if (n) {                                           // uniform over the workgroup
        if (occ) slot_tid[rank] = (uint16_t)tid;
        __syncthreads();
        const uint32_t sh = n > 1u ? 32u - (uint32_t)__clz((int)(n - 1u)) : 0u;           // next_pow2(n) = 1 << sh, <= ML_THREADS
        const uint32_t S = min((uint32_t)ML_THREADS >> sh, (uint32_t)ML_POSE_CHUNK);      // a chunk has no more views than that
        const uint32_t slot = tid & ((1u << sh) - 1u), slice = tid >> sh;
        const bool active = slot < n && slice < S;
        const uint32_t cgi = base + slot_tid[active ? slot : 0u];
        const uint32_t cas = cgi >> cshift, m = cgi & ((1u << cshift) - 1u);
        const float mip_bound = fminf(scalbnf(1.0f, (int)cas), bound);
        const float wx = ((((float)morton_compact(m) + 0.5f) * rG) * 2.0f - 1.0f) * mip_bound;
        const float wy = ((((float)morton_compact(m >> 1) + 0.5f) * rG) * 2.0f - 1.0f) * mip_bound;
        const float wz = ((((float)morton_compact(m >> 2) + 0.5f) * rG) * 2.0f - 1.0f) * mip_bound;
        const float slack = depth_margin * ((2.0f * mip_bound) * rG);
        const float Wf = (float)W, Hf = (float)H;
        const size_t HW = (size_t)H * W;
        uint32_t votes = 0;
        for (uint32_t b0 = 0; b0 < V; b0 += ML_POSE_CHUNK) {
            const uint32_t nb = min((uint32_t)ML_POSE_CHUNK, V - b0);
            __syncthreads();
            for (uint32_t e = tid; e < nb * 12u; e += ML_THREADS) P[e] = poses[(size_t)(b0 + e / 12u) * 16u + (e % 12u)];
            __syncthreads();
            if (!active) continue;
            for (uint32_t b = slice; b < nb; b += S) {
                const float* Q = P + b * 12u;                          // rows 0..2 of [R | o]
                const float dx = wx - Q[3], dy = wy - Q[7], dz = wz - Q[11];
                const float qz = (dx * Q[2] + dy * Q[6]) + dz * Q[10];
                if (!(qz > 0.0f)) continue;
                const float qx = (dx * Q[0] + dy * Q[4]) + dz * Q[8];
                const float qy = (dx * Q[1] + dy * Q[5]) + dz * Q[9];
                const float u = __fdiv_rn(fx * qx, qz) + cx, v = __fdiv_rn(fy * qy, qz) + cy;
                if (!(u >= 0.0f && u < Wf && v >= 0.0f && v < Hf)) continue;
                // 0 <= u < W: truncation is floor; the min() only matters where (float)W rounded up (W > 2^24)
                const uint32_t px = min((uint32_t)u, W - 1u), py = min((uint32_t)v, H - 1u);
                const float p = packed[(size_t)(b0 + b) * HW + (size_t)py * W + px];
                const float t_cell = __fsqrt_rn((dx * dx + dy * dy) + dz * dz);
                if (t_cell <= fabsf(p) + slack) votes += (__builtin_bit_cast(uint32_t, p) >> 31) ? 1u : 0x10000u;
            }
        }
        part[tid] = votes;                                             // thread (slice, slot) is thread (slice << sh) + slot
        __syncthreads();
        if (occ)
            for (uint32_t s = 0; s < S; s++) mine += part[(s << sh) + rank];
    }
    const uint32_t in = mine & 0xffffu, out = mine >> 16;
    const bool sel = occ && in >= min_views && (float)in >= min_share * (float)(in + out);
    const unsigned long long sm = __ballot(sel);
    if (votes_out && live) reinterpret_cast<uint32_t*>(votes_out)[gi] = mine;              // (in, out) as two uint16
    const uint32_t byte = ((base + wv * 64u) >> 3) + lane;
    if (lane < 8u && byte < (total >> 3)) grid_out[byte] = (uint8_t)(sm >> (8u * lane));
}

}  // namespace

extern "C" {

int lae_mask_lift_pack(const float* depth, const float* opacity, const uint8_t* mask, uint32_t HW, float min_opacity, float* packed,
                       void* stream) {
    if (!depth || !opacity || !mask || !packed) return LAE_ENULL;
    if (HW == 0 || HW >= 0x80000000u || !(min_opacity > 0.0f)) return LAE_EINVAL;
    k_mask_lift_pack<<<lae::cdiv(HW, 256u), 256, 0, STREAM(stream)>>>(depth, opacity, mask, HW, min_opacity, packed);
    return lae::check_launch("mask_lift_pack");
}

int lae_mask_lift(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                  const uint8_t* density_bitfield, uint32_t C, uint32_t G, float bound, float depth_margin, uint32_t min_views,
                  float min_share, uint8_t* grid_out, uint16_t* votes_out, void* stream) {
    if (!packed || !poses || !density_bitfield || !grid_out) return LAE_ENULL;
    if (G < 2 || G > 128 || (G & (G - 1)) != 0 || C == 0 || C > 16 || V == 0 || V > 65535u || H < 1 || W < 1 ||
        (uint64_t)H * W >= 0x80000000ull || !(fx > 0.0f) || !(fy > 0.0f) || !(cx == cx) || !(cy == cy) || !(bound > 0.0f) ||
        !(depth_margin >= 0.0f) || !(min_share >= 0.0f && min_share <= 1.0f))
        return LAE_EINVAL;
    uint32_t lg = 0;
    while ((1u << lg) < G) lg++;
    const uint32_t cshift = 3 * lg, total = C << cshift;                         // <= 16 * 2^21 cells
    k_mask_lift<<<lae::cdiv(total, (uint32_t)ML_THREADS), ML_THREADS, 0, STREAM(stream)>>>(
        packed, poses, V, fx, fy, cx, cy, H, W, density_bitfield, total, cshift, 1.0f / (float)G, bound, depth_margin, min_views,
        min_share, grid_out, votes_out);
    return lae::check_launch("mask_lift");
}

}  // extern "C"
