// raymarching.hip -- occupancy-grid ray marching + alpha compositing for gfx950.
//
// Replaces raymarching/src/raymarching.cu of the reference (cited per kernel).
// Written for wave64: ray compaction uses wavefront scans instead of the
// reference's two global atomicAdd reservations, which also makes the sample
// layout deterministic (ray-id order).
//
// Arithmetic contract (shared with oracle/lae_oracle.c): compiled with
// -ffp-contract=off; the a*b+c shapes that nvcc contracts in the reference are
// explicit fmaf() here, everything else is separate IEEE ops, so t-sequences,
// voxel indices, sample counts and positions are bit-identical to the oracle.
#include <string.h>
#include <algorithm>
#include <climits>
#include <cstddef>
#include <type_traits>
#include <hip/hip_fp16.h>
#include "lae_common.h"
#include "raymarch_common.h"

namespace {

// ---------------------------------------------------------------- K2
// raymarching.cu:162-198
__global__ void k_sph_from_ray(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                               float radius, uint32_t N, float* __restrict__ coords) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float RPI = 0.3183098861837907f;
    const float ox = rays_o[3 * (size_t)n], oy = rays_o[3 * (size_t)n + 1], oz = rays_o[3 * (size_t)n + 2];
    const float dx = rays_d[3 * (size_t)n], dy = rays_d[3 * (size_t)n + 1], dz = rays_d[3 * (size_t)n + 2];
    const float A = dx * dx + dy * dy + dz * dz;
    const float Bh = ox * dx + oy * dy + oz * dz;
    const float Cc = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-Bh + sqrtf(Bh * Bh - A * Cc)) / A;
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    coords[2 * (size_t)n] = 2 * atan2f(sqrtf(x * x + z * z), y) * RPI - 1;
    coords[2 * (size_t)n + 1] = atan2f(z, x) * RPI;
}

// ---------------------------------------------------------------- get_rays (nerf/utils.py:61-153)
// Pinhole rays of B cam2world poses for N pixel indices each (inds == NULL: every pixel in row-major order), optionally
// with the ray/box interval of K1 in the same pass (aabb != NULL).  The reference builds two H*W meshgrids, gathers them,
// stacks, normalises and runs a [N,3] x [3,3] matmul per call (~15 launches); pixel centre = index + 0.5 (:82-83).
__global__ void k_get_rays(const float* __restrict__ poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t W,
                           const int64_t* __restrict__ inds, uint64_t inds_stride, uint32_t N, float off_x, float off_y,
                           int perturb, float* __restrict__ rays_o, float* __restrict__ rays_d,
                           const float* __restrict__ aabb, float min_near, float* __restrict__ nears,
                           float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (n >= N) return;
    const float* __restrict__ P = poses + 16 * (size_t)b;
    const int64_t pix = inds ? inds[(size_t)b * inds_stride + n] : (int64_t)n;
    float o[3], d[3];
    pinhole_ray(P, fx, fy, cx, cy, W, pix, perturb, off_x, off_y, o, d);
    const size_t r = (size_t)b * N + n;
#pragma unroll
    for (int k = 0; k < 3; k++) { rays_o[3 * r + k] = o[k]; rays_d[3 * r + k] = d[k]; }
    if (!aabb) return;
    ray_box(o, d, aabb, min_near, nears + r, fars + r);
}

// ---------------------------------------------------------------- K3 / K4 / K5
__global__ void k_morton3D(const int32_t* __restrict__ coords, uint32_t N, int32_t* __restrict__ indices) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    indices[n] = (int32_t)morton_encode((uint32_t)coords[3 * (size_t)n], (uint32_t)coords[3 * (size_t)n + 1],
                                        (uint32_t)coords[3 * (size_t)n + 2]);
}
__global__ void k_morton3D_invert(const int32_t* __restrict__ indices, uint32_t N, int32_t* __restrict__ coords) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int32_t ind = indices[n];
    coords[3 * (size_t)n + 0] = (int32_t)morton_compact((uint32_t)(ind >> 0));
    coords[3 * (size_t)n + 1] = (int32_t)morton_compact((uint32_t)(ind >> 1));
    coords[3 * (size_t)n + 2] = (int32_t)morton_compact((uint32_t)(ind >> 2));
}
// raymarching.cu:267-289; one thread per output byte, two 16-byte loads
__global__ void k_packbits(const float* __restrict__ grid, uint32_t N, float thresh, uint8_t* __restrict__ bitfield) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float4 a = reinterpret_cast<const float4*>(grid)[2 * (size_t)n];
    const float4 b = reinterpret_cast<const float4*>(grid)[2 * (size_t)n + 1];
    uint32_t bits = (a.x > thresh) | ((a.y > thresh) << 1) | ((a.z > thresh) << 2) | ((a.w > thresh) << 3) |
                    ((b.x > thresh) << 4) | ((b.y > thresh) << 5) | ((b.z > thresh) << 6) | ((b.w > thresh) << 7);
    bitfield[n] = (uint8_t)bits;
}

// ---------------------------------------------------------------- K6 (training march)
// raymarching.cu:311-480.  MI355X form: ONE WAVEFRONT PER RAY.
//
// The reference walks a ray with one thread: probe the bitfield (a dependent 1-byte load), then either emit a
// sample and advance by dt, or skip to the voxel exit with `do t += dt while (t < tt)`.  Either way t only ever
// moves along the fixed sequence T_{k+1} = T_k + clamp(T_k * dt_gamma, dt_min, dt_max): occupancy decides
// which T_k are VISITED, never their values.  So a wave evaluates 64 consecutive candidates at once
//   1. lanes build T_k..T_k+63 with the exact serial fp32 recurrence (pure VALU, no memory),
//   2. every lane probes its candidate (64 bitfield loads in flight instead of 1),
//   3. the visited chain is resolved on the scalar unit from two ballots: runs of occupied candidates are
//      taken whole, an empty candidate jumps to the first T_j >= tt (ballot + ctz),
//   4. emitted samples are ranked with popcounts of the emit mask -> consecutive lanes write consecutive rows.
// Counts, offsets and every emitted float are bit-identical to the serial walk (same probe_at / same sums).
// cooperative zero fill of sample rows [rows_end, M): wave n of N takes the n-th slice
__device__ __forceinline__ void zero_tail_rows(uint32_t rows_end, uint32_t M, uint32_t n, uint32_t N, int lane, float* __restrict__ buf,
                                               uint32_t floats_per_row) {
    if (rows_end >= M) return;
    const uint32_t tail = M - rows_end, chunk = (tail + N - 1) / N;
    const uint32_t lo = rows_end + min(tail, n * chunk), hi = rows_end + min(tail, (n + 1) * chunk);
    for (size_t e = (size_t)lo * floats_per_row + lane; e < (size_t)hi * floats_per_row; e += 64) buf[e] = 0.0f;
}

constexpr int MARCH_WAVES = 4;                 // rays per 256-thread block
constexpr int MARCH_BLOCK = 64 * MARCH_WAVES;


// The count pass leaves one record per candidate chunk that emitted samples: where the chunk starts and which lanes
// emit.  The emit pass replays the records (no bitfield probes, no chain resolution): it only rebuilds the candidate
// times and writes rows.  A ray with more than MARCH_REC_MAX such chunks is flagged and walked again instead.
constexpr uint32_t MARCH_REC_MAX = 24;
constexpr uint32_t MARCH_REC_OVERFLOW = 0xffffffffu;
struct MarchRec { float t_base; uint32_t lo, hi; };
struct MarchRecs { uint32_t* nrec; MarchRec* rec; };      // nrec[N], rec[N * MARCH_REC_MAX]; both NULL = feature off

// EMIT == false: count the samples of ray n.  EMIT == true: write them at `offset` (num_steps known).
template <bool EMIT>
__global__ __launch_bounds__(MARCH_BLOCK) void k_march_train_wave(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const uint8_t* __restrict__ grid, MarchCfg cfg,
    uint32_t max_steps, uint32_t N, uint32_t M, const uint32_t* __restrict__ m_limit, const float* __restrict__ nears,
    const float* __restrict__ fars, const float* __restrict__ noises, uint32_t* __restrict__ counts, const uint32_t* __restrict__ prefix,
    float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas, int32_t* __restrict__ rays, MarchRecs recs) {
    const uint32_t n = blockIdx.x * MARCH_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // one ray per wave: scalar
    if (n >= N) return;                                   // whole wave
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n_rec = 0;

    uint32_t limit = max_steps, offset = 0;
    if (EMIT) {
        const uint32_t rows_end = prefix[N + 2];
        zero_tail_rows(rows_end, M, n, N, lane, xyzs, 3);
        zero_tail_rows(rows_end, M, n, N, lane, dirs, 3);
        zero_tail_rows(rows_end, M, n, N, lane, deltas, 2);
        limit = counts[n];
        offset = prefix[N] + prefix[n];                   // prefix[N] = counter value before this call (:405)
        if (lane == 0) {
            const uint32_t row = prefix[N + 1] + n;       // :406 (ray-id order)
            rays[3 * (size_t)row + 0] = (int32_t)n;
            rays[3 * (size_t)row + 1] = (int32_t)offset;
            rays[3 * (size_t)row + 2] = (int32_t)limit;
        }
        const uint32_t M_trunc = m_limit ? min(*m_limit, M) : M;   // lae_march_rays_train_limit: threshold from device memory
        if (limit == 0 || offset + limit > M_trunc) return;     // :415-416 (overflowing rays write nothing)
    }
    const Ray r = load_ray(rays_o, rays_d, n);
    const float far = fars[n];
    float t_base = nears[n];
    t_base = fmaf(step_of(cfg, t_base), noises[n], t_base);                   // :351
    float last_t = t_base;                                // post-step t of the previous emitted sample
    uint32_t emitted = 0;
    bool pending = false;                                 // walker is skipping towards pending_tt
    float pending_tt = 0.f;

    if (EMIT && recs.nrec && recs.nrec[n] != MARCH_REC_OVERFLOW) {
        // replay: same candidate times, same emit masks, same row arithmetic as the walk below
        const uint32_t nr = recs.nrec[n];
        const MarchRec* __restrict__ rr = recs.rec + (size_t)n * MARCH_REC_MAX;
        for (uint32_t k = 0; k < nr; k++) {
            const MarchRec rc = rr[k];
            const unsigned long long emit = (unsigned long long)rc.lo | ((unsigned long long)rc.hi << 32);
            const float t = candidate_t(cfg, rc.t_base, lane);
            const float dt = step_of(cfg, t);
            const float t_next = t + dt;
            const unsigned long long pm = emit & below;
            const int prev_lane = pm ? 63 - __builtin_clzll(pm) : 0;
            const float prev_next = __shfl(t_next, prev_lane, 64);
            if ((emit >> lane) & 1ull) {
                const size_t row = (size_t)offset + emitted + (uint32_t)__builtin_popcountll(pm);
                float* px = xyzs + 3 * row; float* pd = dirs + 3 * row; float* pl = deltas + 2 * row;
                px[0] = clampf(fmaf(t, r.dx, r.ox), -cfg.bound, cfg.bound);
                px[1] = clampf(fmaf(t, r.dy, r.oy), -cfg.bound, cfg.bound);
                px[2] = clampf(fmaf(t, r.dz, r.oz), -cfg.bound, cfg.bound);
                pd[0] = r.dx; pd[1] = r.dy; pd[2] = r.dz;
                pl[0] = dt;
                pl[1] = t_next - (pm ? prev_next : last_t);                   // :461
            }
            const int top = 63 - __builtin_clzll(emit);
            last_t = __shfl(t_next, top, 64);
            emitted += (uint32_t)__builtin_popcountll(emit);
        }
        return;
    }

    while (t_base < far && emitted < limit) {
        // 1. candidates: lane i gets T_{base+i} by i serial steps (identical rounding to the serial walk)
        const float t = candidate_t(cfg, t_base, lane);
        const float dt = step_of(cfg, t);
        const float t_next = t + dt;                      // == T_{base+i+1}
        const bool valid = t < far;
        // 2. probe
        Probe p;
        p.occ = false; p.tt = t; p.x = p.y = p.z = 0.f; p.dt = dt; p.index = 0;
        if (valid) p = probe_at(r, cfg, grid, t);
        const unsigned long long valid_mask = __ballot(valid);
        const unsigned long long occ_mask = __ballot(valid && p.occ);
        // 3. visited chain (all scalar)
        unsigned long long emit = 0ull;
        int k = 0;
        if (pending) {
            const unsigned long long m = __ballot(valid && t >= pending_tt);
            if (m) { k = __builtin_ctzll(m); pending = false; } else k = 64;
        }
        while (k < 64 && ((valid_mask >> k) & 1ull)) {
            if ((occ_mask >> k) & 1ull) {
                const unsigned long long inv = (~occ_mask) >> k;
                const int run = inv ? __builtin_ctzll(inv) : 64 - k;          // bits beyond `valid` are 0 in occ_mask
                emit |= ((run >= 64) ? ~0ull : ((1ull << run) - 1ull)) << k;
                k += run;
            } else {
                const float tt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p.tt), k));
                unsigned long long m = __ballot(valid && t >= tt);
                m &= (k >= 63) ? 0ull : ~((2ull << k) - 1ull);                // at least one step (:396-398)
                if (m) k = __builtin_ctzll(m);
                else { pending = true; pending_tt = tt; k = 64; }
            }
        }
        // cap at `limit` samples (:359 / :427)
        uint32_t cnt = (uint32_t)__builtin_popcountll(emit);
        bool done = false;
        if (emitted + cnt > limit) {
            const uint32_t keep = limit - emitted;
            const bool mine = ((emit >> lane) & 1ull) && (uint32_t)__builtin_popcountll(emit & below) < keep;
            emit = __ballot(mine);
            cnt = keep;
            done = true;
        }
        if (!EMIT && recs.nrec && emit) {                 // leave a record for the emit pass
            if (n_rec < MARCH_REC_MAX) {
                if (lane == 0) recs.rec[(size_t)n * MARCH_REC_MAX + n_rec] = MarchRec{t_base, (uint32_t)emit, (uint32_t)(emit >> 32)};
                n_rec++;
            } else n_rec = MARCH_REC_OVERFLOW;
        }
        // 4. emit
        if (EMIT && emit) {
            const unsigned long long pm = emit & below;
            const int prev_lane = pm ? 63 - __builtin_clzll(pm) : 0;
            const float prev_next = __shfl(t_next, prev_lane, 64);
            if ((emit >> lane) & 1ull) {
                const size_t row = (size_t)offset + emitted + (uint32_t)__builtin_popcountll(pm);
                float* px = xyzs + 3 * row; float* pd = dirs + 3 * row; float* pl = deltas + 2 * row;
                px[0] = p.x; px[1] = p.y; px[2] = p.z;
                pd[0] = r.dx; pd[1] = r.dy; pd[2] = r.dz;
                pl[0] = dt;
                pl[1] = t_next - (pm ? prev_next : last_t);                   // :461
            }
            const int top = 63 - __builtin_clzll(emit);
            last_t = __shfl(t_next, top, 64);
        }
        emitted += cnt;
        if (done || valid_mask != ~0ull) break;           // cap reached, or the ray left [near, far) in this chunk
        t_base = __shfl(t_next, 63, 64);
    }
    if (!EMIT && lane == 0) {
        counts[n] = emitted;
        if (recs.nrec) recs.nrec[n] = n_rec;
    }
}

// exclusive scan of the per-ray counts (single block) + counter update (:405-406).
// prefix[0..N) = exclusive prefix, prefix[N] / prefix[N+1] = counter values before this call.
// prefix[N + 2] = rows_end: first sample row not written by this call (end of the last ray that fits into M);
// the emit pass zero-fills [rows_end, M) so callers need not pre-zero xyzs / dirs / deltas.
__global__ __launch_bounds__(1024) void k_scan_counts(const uint32_t* __restrict__ counts, uint32_t N, uint32_t M_cap,
                                                       const uint32_t* __restrict__ m_limit, uint32_t* __restrict__ prefix,
                                                       int32_t* __restrict__ counter, uint32_t* __restrict__ rows_end_out) {
    const uint32_t M = m_limit ? min(*m_limit, M_cap) : M_cap;
    __shared__ uint32_t lds[17];
    __shared__ uint32_t s_end, s_base;
    if (threadIdx.x == 0) { s_end = 0; s_base = counter ? (uint32_t)counter[0] : 0u; }
    __syncthreads();
    const uint32_t b0u = s_base;
    uint32_t carry = 0, my_end = 0;
    for (uint32_t base = 0; base < N; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < N ? counts[i] : 0;
        uint32_t total;
        const uint32_t ex = lae::block_excl_scan<16>(v, &total, lds);
        if (i < N) {
            prefix[i] = carry + ex;
            const unsigned long long end = (unsigned long long)b0u + carry + ex + v;
            if (v != 0 && end <= (unsigned long long)M) my_end = max(my_end, carry + ex + v);
        }
        carry += total;
    }
    atomicMax(&s_end, my_end);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t b0 = 0, b1 = 0;
        if (counter) {
            b0 = atomicAdd(counter, (int32_t)carry);
            b1 = atomicAdd(counter + 1, (int32_t)N);
        }
        prefix[N] = (uint32_t)b0;
        prefix[N + 1] = (uint32_t)b1;
        prefix[N + 2] = min(M, (uint32_t)b0 + s_end);
        if (rows_end_out) rows_end_out[0] = prefix[N + 2];
    }
}


// ---------------------------------------------------------------- K7 / K8 (training composite)
// raymarching.cu:500-577 / :601-682.  MI355X form: one wavefront per ray, 64 samples per pass.
// Transmittance T_k = prod_{j<k} (1 - alpha_j) is a wave-level multiplicative scan, the running colour /
// depth sums are additive scans, the early stop `T < T_thresh` is a ballot + ctz.  Sample reads and gradient
// writes are lane-consecutive (coalesced); the reference's one-thread-per-ray loop strides by ray.
// Scan association differs from the serial loop -> results agree to fp32 rounding (tests: 2e-6).
// Wave-level scans on the DPP data path (row shifts 1, 2, 4, 8 inside the 16-lane rows, then row_bcast:15 / :31 across
// them -- GFX9 controls, present on gfx950): six dependent VALU operations per scan.  Written with __shfl_up the compiler
// emits ds_bpermute_b32, an LDS round trip per step: 74 of them in the training compositing kernel, whose duration is the
// dependent chain of its longest rays (several passes of 64 samples, forward and backward).  Lanes that a shift leaves
// without a source take the operation's identity (`old` operand), so no per-step select is needed.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float identity, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity), __builtin_bit_cast(int, v), CTRL,
                                                                 ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_scan_add(float v, int) {
    v += dpp_f<0x111, 0xf>(0.0f, v); v += dpp_f<0x112, 0xf>(0.0f, v); v += dpp_f<0x114, 0xf>(0.0f, v); v += dpp_f<0x118, 0xf>(0.0f, v);
    v += dpp_f<0x142, 0xa>(0.0f, v);        // row_bcast:15 -> rows 1 and 3
    v += dpp_f<0x143, 0xc>(0.0f, v);        // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ float wave_scan_mul(float v, int) {
    v *= dpp_f<0x111, 0xf>(1.0f, v); v *= dpp_f<0x112, 0xf>(1.0f, v); v *= dpp_f<0x114, 0xf>(1.0f, v); v *= dpp_f<0x118, 0xf>(1.0f, v);
    v *= dpp_f<0x142, 0xa>(1.0f, v);
    v *= dpp_f<0x143, 0xc>(1.0f, v);
    return v;
}
__device__ __forceinline__ float wave_last(float v) {        // value of lane 63 in every lane
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_prev(float v, float first) {   // value of the lane below; `first` in lane 0 (wave_shr:1)
    return dpp_f<0x138, 0xf>(first, v);
}
__device__ __forceinline__ float wave_sum(float v) { return wave_last(wave_scan_add(v, 0)); }

constexpr int COMP_WAVES = 4;
constexpr int COMP_BLOCK = 64 * COMP_WAVES;

// BLEND: additionally the post-ops of run_cuda (renderer.py:321, 325) in the epilogue:
//   image_out = image + (1 - weights_sum) * bg,  depth_out = clamp(depth - near, min=0) / (far - near);
// `image` keeps the un-blended colour the backward needs.
struct Blend { const float* nears; const float* fars; const float* bg_rays; float bg[3]; float* image_out; float* depth_out; };

// DENSE: (a) the gradient of the BLEND epilogue is folded in: grad_ws_eff = grad_ws - sum_c grad_image_c * bg_c;
// (b) EVERY row of grad_sigmas / grad_rgbs in [0, M) is written (zeros for samples after the early stop and for the
// rows [rows_end, M) no ray owns), so the caller allocates them uninitialised.  Needs the contiguous ray-id-order
// layout lae_march_rays_train produces.
struct Dense { const float* bg_rays; float bg[3]; const uint32_t* rows_end; const float* grad_scale; };   // grad_scale: device scalar or NULL

// DEPTH: additionally the gradient of the raw depth D = sum_k w_k t_k (t_k = running sum of deltas[.,1], as the forward), which
// the reference's backward drops (raymarching.py:273-275): with D_k the running sum including sample k,
//   dD / dsigma_k = delta0_k * (T_post_k * t_k - (D - D_k))
// -- the colour rule with t in place of the colour -- enters the bracket of grad_sigmas times grad_depth[ray]; grad_rgbs does
// not change.  Two more scans per pass (t, w * t).  A ray whose grad_depth is zero takes the path without them (one ray is one
// wave: the branch is uniform), so its gradients are the bits of the flavour without DEPTH.  The DEPTH = false instantiations are
// the kernels they were: every addition is behind `if constexpr`.
struct DepthGrad { const float* grad_depth; const float* depth; };

// per-ray state of the DEPTH flavours: g_D, the ray's D, the squared residual; `on` = g_D != 0 (uniform over the wave: one ray is
// one wave).  Empty without DEPTH.  The running t and D_k live in BwdRun: the DIST flavours carry the same two.
template <bool DEPTH> struct DepthState { float gD = 0.0f, df = 0.0f, dq = 0.0f; bool on = false; };
template <> struct DepthState<false> {};
struct NoArg {};                                          // a trailing kernel argument of the flavours without DEPTH / DIST

// DIST: the mip-NeRF-360 distortion of the ray's weights in its O(n) form (the reference's loss.py:29-76, eff_distloss(w, t, delta0),
// which its CUDA-ray path never calls), over the samples the forward uses, lengths in the march's own units (not divided by
// far - near: m = t_k, interval = deltas[k,0], what that function would be handed here):
//   l_ray = (1/3) sum_k delta0_k w_k^2 + 2 sum_k w_k (t_k W_<k - WT_<k),   W_<k = sum_{j<k} w_j,  WT_<k = sum_{j<k} w_j t_j
// Forward: the two sums of the pass (w, w * t) become scans, whose lane below gives the exclusive prefixes, and one more sum.
// Backward, with W = weights_sum, D = the raw depth and W_k, WT_k the prefixes including sample k:
//   q_k = dl / dw_k = (2/3) delta0_k w_k + 2 (t_k (W_<k - (W - W_k)) + ((D - WT_k) - WT_<k))
//   grad_sigmas_k += delta0_k * g * (T_post_k * q_k - (Q - Q_k)),   Q_k = sum_{j<=k} q_j w_j,   g = d loss / d l_ray
// -- the colour rule with q in place of the colour; grad_rgbs does not change.  l is homogeneous of degree 2 in w, so Q = 2 l: the
// backward needs W, D and l of the forward and nothing else.  Scans per pass: t and w * t (shared with DEPTH), w, q * w.  A ray whose
// g is zero takes the path without them (uniform over its wave) and has the bits of the flavour without DIST; the DIST = false
// instantiations are the kernels they were.
struct DistGrad { const float* grad_dist; const float* dist; const float* depth; };
// per-ray state of the DIST backward: g, Q = 2 l, W, D, the running W_k and Q_k; `on` = g != 0.  Empty without DIST.
template <bool DIST> struct DistState { float g = 0.0f, qf = 0.0f, wf = 0.0f, df = 0.0f, w = 0.0f, q = 0.0f; bool on = false; };
template <> struct DistState<false> {};
template <bool DIST> struct DistAcc { float l = 0.0f; };  // the forward's l_ray
template <> struct DistAcc<false> {};

// ---- the pieces every training compositing kernel is made of.  The kernels keep their loops and decide when a pass is loaded (the
// step kernel requests the next pass before it scans the current one); the per-pass arithmetic exists once, here.

// row n of `rays`; `has` is false for a ray that is dropped: no samples, or samples that do not fit into M (:521 / :624)
struct RayHead { uint32_t index, offset, num_steps; bool has; };
__device__ __forceinline__ RayHead load_ray_head(const int32_t* __restrict__ rays, uint32_t n, uint32_t M) {
    RayHead h;
    h.index = (uint32_t)rays[3 * (size_t)n]; h.offset = (uint32_t)rays[3 * (size_t)n + 1]; h.num_steps = (uint32_t)rays[3 * (size_t)n + 2];
    h.has = !(h.num_steps == 0 || h.offset + h.num_steps > M);
    return h;
}
__device__ __forceinline__ const float* ray_bg(const float* bg_rays, const float* bg, uint32_t index) {
    return bg_rays ? bg_rays + 3 * (size_t)index : bg;
}

// operands of sample k of a ray (one lane of a pass of 64): all zero past the ray's end; d1 is read only where t_k is wanted
struct Sample { float sg, d0, d1, c0, c1, c2; };
__device__ __forceinline__ Sample load_sample(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                              const float* __restrict__ deltas, const RayHead& h, uint32_t k, bool with_t) {
    Sample s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k < h.num_steps) {
        const size_t i = (size_t)h.offset + k;
        s.sg = sigmas[i]; s.d0 = deltas[2 * i];
        if (with_t) s.d1 = deltas[2 * i + 1];
        s.c0 = rgbs[3 * i]; s.c1 = rgbs[3 * i + 1]; s.c2 = rgbs[3 * i + 2];
    }
    return s;
}

// alpha, the transmittance scan and the early stop of one pass, common to forward and backward.  T: transmittance before the pass.
// `valid` comes in as "inside the ray" and leaves as "inside the ray and not after the stop"; w is zero elsewhere.
struct PassW { float w, T_post, incl; bool done; };
__device__ __forceinline__ PassW pass_weights(const Sample& s, bool& valid, float T, float T_thresh, int lane) {
    const float alpha = valid ? 1.0f - __expf(-s.sg * s.d0) : 0.0f;
    PassW p;
    p.incl = wave_scan_mul(1.0f - alpha, lane);                             // prod_{j<=k} within the pass
    const float excl = wave_prev(p.incl, 1.0f);
    p.T_post = T * p.incl;
    const unsigned long long stop = __ballot(valid && p.T_post < T_thresh); // :557 (sample included)
    p.done = false;
    if (stop) { const int last = __builtin_ctzll(stop); valid = valid && lane <= last; p.done = true; }
    p.w = valid ? alpha * (T * excl) : 0.0f;
    return p;
}

// one forward pass: adds the pass to the ray's sums, carries T and t; -> the ray stopped in this pass
struct FwdAcc { float r, g, b, d, ws; };
template <bool DIST>
__device__ __forceinline__ bool composite_fwd_pass(const Sample& s, bool valid, float T_thresh, int lane, float& T, float& t, FwdAcc& a,
                                                   DistAcc<DIST>& xa) {
    const PassW p = pass_weights(s, valid, T, T_thresh, lane);
    const float tk = t + wave_scan_add(s.d1, lane);
    a.r += wave_sum(p.w * s.c0); a.g += wave_sum(p.w * s.c1); a.b += wave_sum(p.w * s.c2);
    if constexpr (DIST) {                                                   // the two sums below as scans: same bits in lane 63
        const float dk = wave_scan_add(p.w * tk, lane), wk = wave_scan_add(p.w, lane);
        const float d_lt = a.d + wave_prev(dk, 0.0f), w_lt = a.ws + wave_prev(wk, 0.0f);     // WT_<k, W_<k
        xa.l += wave_sum(p.w * ((1.0f / 3.0f) * s.d0 * p.w + 2.0f * (tk * w_lt - d_lt)));
        a.d += wave_last(dk); a.ws += wave_last(wk);
    } else {
        a.d += wave_sum(p.w * tk); a.ws += wave_sum(p.w);
    }
    if (p.done) return true;
    T *= wave_last(p.incl);
    t = wave_last(tk);
    return false;
}

// lane 0 of a forward wave: the ray's sums, the blended colour o, the BLEND outputs
__device__ __forceinline__ void store_ray(float* __restrict__ weights_sum, float* __restrict__ depth, float* __restrict__ image,
                                          uint32_t index, const FwdAcc& a) {
    weights_sum[index] = a.ws; depth[index] = a.d;
    image[3 * (size_t)index] = a.r; image[3 * (size_t)index + 1] = a.g; image[3 * (size_t)index + 2] = a.b;
}
__device__ __forceinline__ void blend_colour(const float* bg, const FwdAcc& a, float o[3]) {
    const float rest = 1.0f - a.ws;
    o[0] = a.r + rest * bg[0]; o[1] = a.g + rest * bg[1]; o[2] = a.b + rest * bg[2];
}
__device__ __forceinline__ void store_blend(const Blend& bl, uint32_t index, const float o[3], float d) {
    bl.image_out[3 * (size_t)index] = o[0]; bl.image_out[3 * (size_t)index + 1] = o[1]; bl.image_out[3 * (size_t)index + 2] = o[2];
    const float nr = bl.nears[index];
    bl.depth_out[index] = fmaxf(d - nr, 0.0f) / (bl.fars[index] - nr);
}

// what the backward of a ray holds fixed over its passes (the colour gradient, the ray's colour, the weights_sum term of the
// bracket) and what it carries from pass to pass
struct BwdRay { float g0, g1, g2, rf, gf, bf, tail; };
struct BwdRun { float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, t = 0.0f, d = 0.0f; };    // t, d (= D_k): DEPTH / DIST rays only
__device__ __forceinline__ void zero_grad_row(float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs, size_t i) {
    grad_rgbs[3 * i] = 0.f; grad_rgbs[3 * i + 1] = 0.f; grad_rgbs[3 * i + 2] = 0.f; grad_sigmas[i] = 0.f;
}

// one backward pass: writes the gradient rows of the pass (row i in this lane), carries T and the running sums; -> the ray stopped
// in this pass.  With DEPTH and ds.on, or DIST and xs.on, s.d1 must be loaded.
template <bool DENSE, bool DEPTH, bool DIST>
__device__ __forceinline__ bool composite_bwd_pass(const Sample& s, bool valid, size_t i, const BwdRay& c, float T_thresh, int lane,
                                                   BwdRun& st, DepthState<DEPTH>& ds, DistState<DIST>& xs,
                                                   float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs) {
    const bool in_ray = valid;
    const PassW p = pass_weights(s, valid, st.T, T_thresh, lane);
    const float rk = st.r + wave_scan_add(p.w * s.c0, lane);                // running sums INCLUDING this sample
    const float gk = st.g + wave_scan_add(p.w * s.c1, lane);
    const float bk = st.b + wave_scan_add(p.w * s.c2, lane);
    [[maybe_unused]] float tk = 0.0f, dk = 0.0f, wk = 0.0f, qk = 0.0f, Qk = 0.0f;
    [[maybe_unused]] bool with_t = false;
    if constexpr (DEPTH) with_t = ds.on;
    if constexpr (DIST) with_t = with_t || xs.on;
    if constexpr (DEPTH || DIST) {
        if (with_t) {
            tk = st.t + wave_scan_add(s.d1, lane);                          // t_k, as the forward
            dk = st.d + wave_scan_add(p.w * tk, lane);                      // D_k, including this sample
        }
    }
    if constexpr (DIST) {
        if (xs.on) {
            wk = xs.w + wave_scan_add(p.w, lane);                           // W_k, including this sample
            const float w_lt = wave_prev(wk, xs.w), d_lt = wave_prev(dk, st.d);
            qk = (2.0f / 3.0f) * s.d0 * p.w + 2.0f * (tk * (w_lt - (xs.wf - wk)) + ((xs.df - dk) - d_lt));
            Qk = xs.q + wave_scan_add(qk * p.w, lane);
        }
    }
    if (valid) {
        grad_rgbs[3 * i] = c.g0 * p.w; grad_rgbs[3 * i + 1] = c.g1 * p.w; grad_rgbs[3 * i + 2] = c.g2 * p.w;      // :657-659
        float br = c.g0 * (p.T_post * s.c0 - (c.rf - rk)) + c.g1 * (p.T_post * s.c1 - (c.gf - gk)) +
                   c.g2 * (p.T_post * s.c2 - (c.bf - bk)) + c.tail;                                               // :662-667
        if constexpr (DEPTH) {
            if (ds.on) br = br + ds.gD * (p.T_post * tk - (ds.df - dk));
        }
        if constexpr (DIST) {
            if (xs.on) br = br + xs.g * (p.T_post * qk - (xs.qf - Qk));
        }
        grad_sigmas[i] = s.d0 * br;
    } else if (DENSE && in_ray) {
        zero_grad_row(grad_sigmas, grad_rgbs, i);
    }
    if (p.done) return true;
    st.T *= wave_last(p.incl);
    st.r = wave_last(rk); st.g = wave_last(gk); st.b = wave_last(bk);
    if constexpr (DEPTH || DIST) {
        if (with_t) { st.t = wave_last(tk); st.d = wave_last(dk); }
    }
    if constexpr (DIST) {
        if (xs.on) { xs.w = wave_last(wk); xs.q = wave_last(Qk); }
    }
    return false;
}

template <bool BLEND, bool DIST = false>
__global__ __launch_bounds__(COMP_BLOCK) void k_composite_train_fwd(
    const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const int32_t* __restrict__ rays, uint32_t M, uint32_t N, float T_thresh, float* __restrict__ weights_sum,
    float* __restrict__ depth, float* __restrict__ image, Blend bl, std::conditional_t<DIST, float*, NoArg> dist) {
    const uint32_t n = blockIdx.x * COMP_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // one ray per wave: scalar
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    const RayHead h = load_ray_head(rays, n, M);
    FwdAcc a{0.f, 0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] DistAcc<DIST> xa;
    if (h.has) {
        float T = 1.0f, t = 0.0f;
        for (uint32_t base = 0; base < h.num_steps; base += 64) {
            const uint32_t k = base + lane;
            const Sample s = load_sample(sigmas, rgbs, deltas, h, k, true);
            if (composite_fwd_pass<DIST>(s, k < h.num_steps, T_thresh, lane, T, t, a, xa)) break;
        }
    }
    if (lane == 0) {
        store_ray(weights_sum, depth, image, h.index, a);
        if constexpr (DIST) dist[h.index] = xa.l;
        if constexpr (BLEND) {
            float o[3];
            blend_colour(ray_bg(bl.bg_rays, bl.bg, h.index), a, o);
            store_blend(bl, h.index, o, a.d);
        }
    }
}

template <bool DENSE, bool DEPTH = false, bool DIST = false>
__global__ __launch_bounds__(COMP_BLOCK) void k_composite_train_bwd(
    const float* __restrict__ grad_ws, const float* __restrict__ grad_image, const float* __restrict__ sigmas,
    const float* __restrict__ rgbs, const float* __restrict__ deltas, const int32_t* __restrict__ rays,
    const float* __restrict__ weights_sum, const float* __restrict__ image, uint32_t M, uint32_t N, float T_thresh,
    float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs, Dense dn, std::conditional_t<DEPTH, DepthGrad, NoArg> dg,
    std::conditional_t<DIST, DistGrad, NoArg> xg) {
    const uint32_t n = blockIdx.x * COMP_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // one ray per wave: scalar
    if (n >= N) return;
    const int lane = threadIdx.x & 63;
    if constexpr (DENSE) {
        const uint32_t rows_end = dn.rows_end[0];
        zero_tail_rows(rows_end, M, n, N, lane, grad_sigmas, 1);
        zero_tail_rows(rows_end, M, n, N, lane, grad_rgbs, 3);
    }
    const RayHead h = load_ray_head(rays, n, M);
    if (!h.has) return;
    const uint32_t index = h.index;
    float gws = grad_ws ? grad_ws[index] : 0.0f;
    float g0 = grad_image[3 * (size_t)index], g1 = grad_image[3 * (size_t)index + 1], g2 = grad_image[3 * (size_t)index + 2];
    [[maybe_unused]] DepthState<DEPTH> ds;
    if constexpr (DEPTH) { ds.gD = dg.grad_depth[index]; ds.df = dg.depth[index]; }
    [[maybe_unused]] DistState<DIST> xs;
    if constexpr (DIST) { xs.g = xg.grad_dist[index]; xs.qf = 2.0f * xg.dist[index]; xs.wf = weights_sum[index]; xs.df = xg.depth[index]; }
    if constexpr (DENSE) {
        if (dn.grad_scale) {                               // fused criterion: upstream d(loss) arrives as a device scalar
            const float gs = dn.grad_scale[0];
            g0 *= gs; g1 *= gs; g2 *= gs; gws *= gs;
            if constexpr (DEPTH) ds.gD *= gs;
            if constexpr (DIST) xs.g *= gs;
        }
        const float* bg = ray_bg(dn.bg_rays, dn.bg, index);
        gws = gws - ((g0 * bg[0] + g1 * bg[1]) + g2 * bg[2]);
    }
    const BwdRay c{g0, g1, g2, image[3 * (size_t)index], image[3 * (size_t)index + 1], image[3 * (size_t)index + 2],
                   gws * (1 - weights_sum[index])};
    bool with_t = false;
    if constexpr (DEPTH) with_t = ds.on = ds.gD != 0.0f;
    if constexpr (DIST) { xs.on = xs.g != 0.0f; with_t = with_t || xs.on; }
    BwdRun st;
    bool stopped = false;
    for (uint32_t base = 0; base < h.num_steps; base += 64) {
        const uint32_t k = base + lane;
        const size_t i = (size_t)h.offset + k;
        if (DENSE && stopped) {                                             // samples after the early stop: zero gradient
            if (k < h.num_steps) zero_grad_row(grad_sigmas, grad_rgbs, i);
            continue;
        }
        const Sample s = load_sample(sigmas, rgbs, deltas, h, k, with_t);
        if (composite_bwd_pass<DENSE, DEPTH, DIST>(s, k < h.num_steps, i, c, T_thresh, lane, st, ds, xs, grad_sigmas, grad_rgbs)) {
            if (!DENSE) break;
            stopped = true;
        }
    }
}

// ---------------------------------------------------------------- K7 + criterion + K8 in one launch (training step)
// composite_rays_train forward with the BLEND epilogue, the trainer's MSE criterion (d loss / d pixel needs this ray's
// pixel only) and composite_rays_train backward (DENSE), one wavefront per ray: the three launches of the step's middle
// (11.8 + 5.6 + 11 us and two kernel boundaries) become one.  Arithmetic is that of k_composite_train_fwd<true>,
// k_mse_fwd and k_composite_train_bwd<true> (grad_scale = 1): the passes are the same two functions.  The loss VALUE needs
// all rays: every workgroup leaves the sum of its rays' squared errors in partials[blockIdx.x], k_loss_finish adds them in a
// fixed order (deterministic).
struct StepLoss { const float* target; const float* scale; float* grad_image; float* partials; float* poison_loss; };

// The four terms below are the C ABI's own structs (include/laenerf.h): the kernel takes what the caller filled in, the layout is
// written once.
// DEPTH: a second criterion on the raw depth D of the ray, the reference's depth supervision (nerf/utils.py:585-589, 634-635):
//   z = src[inds ? inds[index] : index] (fp32 or fp16),  m = z > 0 && nears[index] < fars[index],  res = m * (D - (z - nears[index])),
//   loss += lambda * mean(res^2),  g_D = ((res * (2 * lambda / N)) * scale) -> grad_depth[index]
// and the backward carries g_D as k_composite_train_bwd<true, true> does (the reference's backward drops it; value_only restores that:
// the value is computed, g_D is forced to zero).  A ray with g_D == 0 runs the statements of the flavour without DEPTH.
// partials[] receive sum(sq + 3 * lambda * res^2): the finishers, which divide by 3 N, yield MSE + lambda * mean(res^2) as they are;
// DepthLoss::partials receive sum(res^2) (lae_loss_finish with n_elem = N gives the depth term alone).
using DepthLoss = lae_depth_term;

// DIST: a further criterion, the distortion l_ray of the ray's weights (see DistGrad): loss += lambda * mean over ALL N rays of l_ray (a
// ray without samples has l = 0), g = ((lambda / N) * scale) -> grad_dist[index] for every ray, carried through the backward as
// k_composite_train_bwd<true, ., true> does; value_only forces g = 0.  With g == 0 (lambda == 0 or value_only: every ray of the launch)
// the backward runs the statements of the flavour without DIST.  partials[] additionally receive 3 * lambda * sum(l_ray), partials of
// the term alone go to DistLoss::partials (lae_loss_finish with n_elem = N gives L_dist).
using DistLoss = lae_dist_term;

// CRIT: the colour criterion is chosen by `kind` (lae::colour_elem_loss; LAE_LOSS_MSE runs the statements above), and with
// opac != NULL the opacity entropy of the ray's weights_sum W joins the loss: o = clamp(W, 1e-5, 1 - 1e-5),
// h = -(o log2 o + (1 - o) log2(1 - o)), loss += opac_lambda * mean over ALL N rays of h, grad_ws[index] = ((opac_lambda / N) *
// (log2(1 - o) - log2 o)) * scale where W lies in [1e-5, 1 - 1e-5] (torch.clamp's gradient) and 0 outside or with opac_value_only.  The backward takes
// it where k_composite_train_bwd<true> takes grad_weights_sum -- the ray's constant of the bracket, nothing per sample.  partials[]
// additionally receive 3 * opac_lambda * sum(h), CritLoss::opac_partials sum(h).  The CRIT = false instantiations are the kernels they were.
using CritLoss = lae_crit_term;

// WGT (with CRIT, LAE_LOSS_MSE only): a per-pixel weight w on the colour residual and a second colour target t with its own weight,
// the reference's train_step_npr (nerf/utils.py:523-526).  Both are gathered at inds[index] (or index) BEFORE the forward scan -- two
// wave-uniform requests whose latency the scan hides -- and enter the criterion after it, per ray, nothing per sample:
//   u = 1 - 0.5 w,  a_c = w * (o_c - gt_c),  v1 = fmaf(a2, a2, fmaf(a1, a1, a0 * a0)),  b_c = u * (t_c - o_c),  v2 = (b0 b0 + b1 b1) + b2 b2
//   sq = v1 + lambda * v2,   grad_image_c = (((w * a_c) - lambda * (u * b_c)) * (2 / (3 N))) * scale
// (with a second target the bracket of grad_image is evaluated in double and rounded once: its two parts cancel, see below)
// t is blended over the ray's own background when it has an alpha (rgb * a + bg * (1 - a), three roundings, the sampler's blend of gt).
// With w == 1 and no second target the statements reduce to those above bit for bit (1 * x is exact).  partials[] receive sq,
// WeightLoss::partials sum(v2) (lae_loss_finish with n_elem = 3 N gives the second term alone).  The WGT = false instantiations are
// the kernels they were.
using WeightLoss = lae_weight_term;
// a header edit that moves a field fails the build here: the kernels' argument bytes are these layouts
static_assert(sizeof(DepthLoss) == 48 && offsetof(DepthLoss, src) == 0 && offsetof(DepthLoss, dtype) == 8 && offsetof(DepthLoss, inds) == 16 &&
              offsetof(DepthLoss, lambda) == 24 && offsetof(DepthLoss, value_only) == 28 && offsetof(DepthLoss, grad_depth) == 32 &&
              offsetof(DepthLoss, partials) == 40, "lae_depth_term");
static_assert(sizeof(DistLoss) == 32 && offsetof(DistLoss, lambda) == 0 && offsetof(DistLoss, value_only) == 4 && offsetof(DistLoss, dist) == 8 &&
              offsetof(DistLoss, grad_dist) == 16 && offsetof(DistLoss, partials) == 24, "lae_dist_term");
static_assert(sizeof(CritLoss) == 40 && offsetof(CritLoss, kind) == 0 && offsetof(CritLoss, param) == 4 && offsetof(CritLoss, opac_lambda) == 8 &&
              offsetof(CritLoss, opac_value_only) == 12 && offsetof(CritLoss, opac) == 16 && offsetof(CritLoss, grad_ws) == 24 &&
              offsetof(CritLoss, opac_partials) == 32, "lae_crit_term");
static_assert(sizeof(WeightLoss) == 56 && offsetof(WeightLoss, w_src) == 0 && offsetof(WeightLoss, w_dtype) == 8 && offsetof(WeightLoss, t2_src) == 16 &&
              offsetof(WeightLoss, t2_dtype) == 24 && offsetof(WeightLoss, t2_channels) == 28 && offsetof(WeightLoss, inds) == 32 &&
              offsetof(WeightLoss, lambda) == 40 && offsetof(WeightLoss, partials) == 48, "lae_weight_term");
__device__ __forceinline__ float load_plane(const void* src, int dtype, size_t i) {
    return dtype == LAE_IMG_F16 ? __half2float(((const __half*)src)[i]) : ((const float*)src)[i];
}

template <bool DEPTH, bool DIST, bool CRIT = false, bool WGT = false>
__global__ __launch_bounds__(COMP_BLOCK) void k_composite_train_step(
    const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const int32_t* __restrict__ rays, uint32_t M, uint32_t N, float T_thresh, float* __restrict__ weights_sum,
    float* __restrict__ depth, float* __restrict__ image, Blend bl, StepLoss sl, const uint32_t* __restrict__ rows_end_p,
    float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs, std::conditional_t<DEPTH, DepthLoss, NoArg> dl,
    std::conditional_t<DIST, DistLoss, NoArg> xl, std::conditional_t<CRIT, CritLoss, NoArg> cl,
    std::conditional_t<WGT, WeightLoss, NoArg> wl) {
    static_assert(CRIT || !WGT, "the weighted flavours are built on the CRIT ones");
    __shared__ float s_sq[COMP_WAVES];
    [[maybe_unused]] __shared__ float s_dq[COMP_WAVES];
    [[maybe_unused]] __shared__ float s_xq[COMP_WAVES];
    [[maybe_unused]] __shared__ float s_oq[COMP_WAVES];
    [[maybe_unused]] __shared__ float s_tq[COMP_WAVES];
    [[maybe_unused]] float oq = 0.0f, gws_in = 0.0f;                        // CRIT: the ray's entropy h and its grad_ws
    [[maybe_unused]] float pw = 1.0f, t2[4] = {0.0f, 0.0f, 0.0f, 1.0f}, tq = 0.0f;   // WGT: the weight, the second target (alpha 1 without one), v2
    [[maybe_unused]] DepthState<DEPTH> ds;
    [[maybe_unused]] DistState<DIST> xs;
    [[maybe_unused]] DistAcc<DIST> xa;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t n = blockIdx.x * COMP_WAVES + wv;                      // one ray per wave: scalar
    const int lane = threadIdx.x & 63;
    float sq = 0.0f;
    if (n < N) {
        const uint32_t rows_end = rows_end_p[0];
        zero_tail_rows(rows_end, M, n, N, lane, grad_sigmas, 1);
        zero_tail_rows(rows_end, M, n, N, lane, grad_rgbs, 3);
        const RayHead h = load_ray_head(rays, n, M);
        const uint32_t index = h.index;
        if constexpr (WGT) {                                                    // requested here, used after the forward scan
            const size_t pi = wl.inds ? (size_t)wl.inds[index] : (size_t)index;
            if (wl.w_src) pw = load_plane(wl.w_src, wl.w_dtype, pi);
            if (wl.t2_src) {
                const size_t ti = (size_t)wl.t2_channels * pi;
                t2[0] = load_plane(wl.t2_src, wl.t2_dtype, ti); t2[1] = load_plane(wl.t2_src, wl.t2_dtype, ti + 1);
                t2[2] = load_plane(wl.t2_src, wl.t2_dtype, ti + 2);
                if (wl.t2_channels == 4) t2[3] = load_plane(wl.t2_src, wl.t2_dtype, ti + 3);
            }
        }
        // ---- forward.  The next pass of 64 samples is requested before the current one is scanned: the kernel's time is that of
        // its longest rays (several passes, forward and backward), one memory latency per pass otherwise
        FwdAcc a{0.f, 0.f, 0.f, 0.f, 0.f};
        if (h.has) {
            float T = 1.0f, t = 0.0f;
            Sample nxt = load_sample(sigmas, rgbs, deltas, h, lane, true);
            for (uint32_t base = 0; base < h.num_steps; base += 64) {
                const Sample cur = nxt;
                if (base + 64 < h.num_steps) nxt = load_sample(sigmas, rgbs, deltas, h, base + 64 + lane, true);
                if (composite_fwd_pass<DIST>(cur, base + lane < h.num_steps, T_thresh, lane, T, t, a, xa)) break;
            }
        }
        const float* bg = ray_bg(bl.bg_rays, bl.bg, index);
        float o[3];
        blend_colour(bg, a, o);
        // ---- criterion (k_mse_fwd): grad = ((pred - target) * 2 / n_elements) * scale
        const float s = sl.scale ? sl.scale[0] : 1.0f;
        const float gk = 2.0f / (float)(3u * N);
        const float e0 = o[0] - sl.target[3 * (size_t)index], e1 = o[1] - sl.target[3 * (size_t)index + 1],
                    e2 = o[2] - sl.target[3 * (size_t)index + 2];
        sq = fmaf(e2, e2, fmaf(e1, e1, e0 * e0));
        float g0 = (e0 * gk) * s, g1 = (e1 * gk) * s, g2 = (e2 * gk) * s;
        if constexpr (WGT) {                                                    // LAE_LOSS_MSE only (checked on the host)
            const float a0 = pw * e0, a1 = pw * e1, a2 = pw * e2;
            sq = fmaf(a2, a2, fmaf(a1, a1, a0 * a0));
            if (wl.t2_src) {                                                    // uniform over the launch
                const float u = 1.0f - 0.5f * pw;
                float tc[3] = {t2[0], t2[1], t2[2]};
                if (wl.t2_channels == 4) {
                    const float rest = __fsub_rn(1.0f, t2[3]);
                    for (int c = 0; c < 3; c++) tc[c] = __fadd_rn(__fmul_rn(t2[c], t2[3]), __fmul_rn(bg[c], rest));
                }
                const float b0 = u * (tc[0] - o[0]), b1 = u * (tc[1] - o[1]), b2 = u * (tc[2] - o[2]);
                tq = (b0 * b0 + b1 * b1) + b2 * b2;
                sq = sq + wl.lambda * tq;
                // grad_image = (((w * a) - lambda * (u * b)) * (2 / (3 N))) * scale.  The two parts cancel where the pixel lies between its
                // two targets -- where the training converges --, and rounded to fp32 one by one they would leave the difference with an
                // unbounded relative error.  Three values per ray: the bracket is evaluated in double on the fp32 operands (w, o, gt, t,
                // scale) and rounded once, so grad_image keeps the relative bound of the step without a second target everywhere
                const double wd = pw, ud = 1.0 - 0.5 * wd, ld = wl.lambda, kd = (2.0 / (double)(3u * N)) * (double)s;
                const float* gt = sl.target + 3 * (size_t)index;
                g0 = (float)(((wd * (wd * ((double)o[0] - (double)gt[0]))) - ld * (ud * (ud * ((double)tc[0] - (double)o[0])))) * kd);
                g1 = (float)(((wd * (wd * ((double)o[1] - (double)gt[1]))) - ld * (ud * (ud * ((double)tc[1] - (double)o[1])))) * kd);
                g2 = (float)(((wd * (wd * ((double)o[2] - (double)gt[2]))) - ld * (ud * (ud * ((double)tc[2] - (double)o[2])))) * kd);
            } else {
                g0 = ((pw * a0) * gk) * s; g1 = ((pw * a1) * gk) * s; g2 = ((pw * a2) * gk) * s;
            }
        }
        if constexpr (CRIT) {
            if (cl.kind != LAE_LOSS_MSE) {                                  // uniform over the launch
                const float g1n = 1.0f / (float)(3u * N);
                const lae::ElemLoss l0 = lae::colour_elem_loss(cl.kind, cl.param, e0, sl.target[3 * (size_t)index]),
                                    l1 = lae::colour_elem_loss(cl.kind, cl.param, e1, sl.target[3 * (size_t)index + 1]),
                                    l2 = lae::colour_elem_loss(cl.kind, cl.param, e2, sl.target[3 * (size_t)index + 2]);
                sq = (l0.v + l1.v) + l2.v;
                g0 = (l0.dv * g1n) * s; g1 = (l1.dv * g1n) * s; g2 = (l2.dv * g1n) * s;
            }
            if (cl.opac) {
                const float hi = 1.0f - 1e-5f;
                const float oc = fminf(fmaxf(a.ws, 1e-5f), hi);
                const float la = log2f(oc), lb = log2f(1.0f - oc);
                oq = -(oc * la + (1.0f - oc) * lb);
                sq = sq + (3.0f * cl.opac_lambda) * oq;
                const bool inside = a.ws >= 1e-5f && a.ws <= hi;
                gws_in = cl.opac_value_only || !inside ? 0.0f : ((cl.opac_lambda / (float)N) * (lb - la)) * s;
                if (lane == 0) { cl.opac[index] = oq; cl.grad_ws[index] = gws_in; }
            }
        }
        if constexpr (DEPTH) {
            const size_t zi = dl.inds ? (size_t)dl.inds[index] : (size_t)index;
            const float z = dl.dtype == LAE_IMG_F16 ? __half2float(((const __half*)dl.src)[zi]) : ((const float*)dl.src)[zi];
            // a ray that misses the bounding box carries the sentinel interval near == far == FLT_MAX: it has no near to measure from
            // and is left unsupervised like a pixel with z == 0 (its residual would be ~FLT_MAX and the loss value infinite)
            const float nr = bl.nears[index];
            const float res = (z > 0.0f && nr < bl.fars[index] ? 1.0f : 0.0f) * (a.d - (z - nr));
            ds.dq = res * res;
            sq = sq + (3.0f * dl.lambda) * ds.dq;
            ds.gD = dl.value_only ? 0.0f : (res * (2.0f * dl.lambda / (float)N)) * s;
            ds.df = a.d;
            ds.on = ds.gD != 0.0f;
            if (lane == 0) dl.grad_depth[index] = ds.gD;
        }
        if constexpr (DIST) {
            sq = sq + (3.0f * xl.lambda) * xa.l;
            xs.g = xl.value_only ? 0.0f : (xl.lambda / (float)N) * s;
            xs.qf = 2.0f * xa.l; xs.wf = a.ws; xs.df = a.d;
            xs.on = xs.g != 0.0f;
            if (lane == 0) { xl.dist[index] = xa.l; xl.grad_dist[index] = xs.g; }
        }
        if (lane == 0) {
            store_ray(weights_sum, depth, image, index, a);
            store_blend(bl, index, o, a.d);
            sl.grad_image[3 * (size_t)index] = g0; sl.grad_image[3 * (size_t)index + 1] = g1; sl.grad_image[3 * (size_t)index + 2] = g2;
        }
        // ---- backward (DENSE, grad_weights_sum = 0, grad_scale = 1)
        if (h.has) {
            float gws = 0.0f - ((g0 * bg[0] + g1 * bg[1]) + g2 * bg[2]);
            if constexpr (CRIT) gws = gws_in - ((g0 * bg[0] + g1 * bg[1]) + g2 * bg[2]);      // grad_ws enters where the blend's term does
            const BwdRay c{g0, g1, g2, a.r, a.g, a.b, gws * (1 - a.ws)};
            BwdRun st;
            bool stopped = false;
            Sample nxt = load_sample(sigmas, rgbs, deltas, h, lane, true);
            for (uint32_t base = 0; base < h.num_steps; base += 64) {
                const uint32_t k = base + lane;
                const size_t i = (size_t)h.offset + k;
                const Sample cur = nxt;
                if (!stopped && base + 64 < h.num_steps) nxt = load_sample(sigmas, rgbs, deltas, h, base + 64 + lane, true);
                if (stopped) {                                                      // samples after the early stop: zero gradient
                    if (k < h.num_steps) zero_grad_row(grad_sigmas, grad_rgbs, i);
                    continue;
                }
                if (composite_bwd_pass<true, DEPTH, DIST>(cur, k < h.num_steps, i, c, T_thresh, lane, st, ds, xs, grad_sigmas, grad_rgbs)) stopped = true;
            }
        }
    }
    if (lane == 0) s_sq[wv] = sq;
    if constexpr (DEPTH) { if (lane == 0) s_dq[wv] = ds.dq; }
    if constexpr (DIST) { if (lane == 0) s_xq[wv] = xa.l; }
    if constexpr (CRIT) { if (lane == 0) s_oq[wv] = oq; }
    if constexpr (WGT) { if (lane == 0) s_tq[wv] = tq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < COMP_WAVES; w++) t += s_sq[w];
        sl.partials[blockIdx.x] = t;
        if constexpr (DEPTH) {
            float u = 0.0f;
#pragma unroll
            for (int w = 0; w < COMP_WAVES; w++) u += s_dq[w];
            dl.partials[blockIdx.x] = u;
        }
        if constexpr (DIST) {
            float u = 0.0f;
#pragma unroll
            for (int w = 0; w < COMP_WAVES; w++) u += s_xq[w];
            xl.partials[blockIdx.x] = u;
        }
        if constexpr (CRIT) {
            if (cl.opac) {
                float u = 0.0f;
#pragma unroll
                for (int w = 0; w < COMP_WAVES; w++) u += s_oq[w];
                cl.opac_partials[blockIdx.x] = u;
            }
        }
        if constexpr (WGT) {
            if (wl.t2_src) {
                float u = 0.0f;
#pragma unroll
                for (int w = 0; w < COMP_WAVES; w++) u += s_tq[w];
                wl.partials[blockIdx.x] = u;
            }
        }
        // deferred loss value (lae_composite_rays_train_step with poison_loss): whoever reads it before the finishing
        // launch (lae_loss_finish, or the extra block of lae_nerf_head_backward) sees NaN, not a stale number
        if (blockIdx.x == 0 && sl.poison_loss) { sl.poison_loss[0] = __builtin_nanf(""); sl.poison_loss[1] = __builtin_nanf(""); }
    }
}

// sum of the workgroups' squared-error sums in a fixed order -> loss_out[0] = mean * scale, loss_out[1] = mean
__global__ __launch_bounds__(1024) void k_loss_finish(const float* __restrict__ partials, uint32_t n_part, uint32_t n_elem,
                                                       const float* __restrict__ scale, float* __restrict__ loss_out) {
    __shared__ float part[16];
    float acc = 0.0f;
    for (uint32_t i = threadIdx.x; i < n_part; i += 1024) acc += partials[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; w++) t += part[w];
        const float loss = t / (float)n_elem;
        loss_out[0] = loss * (scale ? scale[0] : 1.0f);
        loss_out[1] = loss;
    }
}

// ---------------------------------------------------------------- K9 / K10 (inference march)
// raymarching.cu:700-805 and :811-926 (EDIT = distill variant)
template <bool EDIT>
__global__ void k_march_infer(uint32_t n_alive, uint32_t n_step, const int32_t* __restrict__ rays_alive,
                              const float* __restrict__ rays_t, const float* __restrict__ rays_o,
                              const float* __restrict__ rays_d, MarchCfg cfg, const uint8_t* __restrict__ grid,
                              const uint8_t* __restrict__ edit_grid, const float* __restrict__ fars,
                              float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas,
                              uint8_t* __restrict__ edit_occ, const float* __restrict__ noises) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int32_t index = rays_alive[n];
    const Ray r = load_ray(rays_o, rays_d, (uint32_t)index);
    float* px = xyzs + 3 * (size_t)n * n_step;
    float* pd = dirs + 3 * (size_t)n * n_step;
    float* pl = deltas + 2 * (size_t)n * n_step;
    uint8_t* pe = EDIT ? edit_occ + (size_t)n * n_step : nullptr;
    float t = rays_t[index];
    const float far = fars[index];
    t = fmaf(clampf(t * cfg.dt_gamma, cfg.dt_min, cfg.dt_max), noises[n], t);     // :746
    float last_t = t;
    uint32_t step = 0;
    while (t < far && step < n_step) {
        const Probe p = probe_at(r, cfg, grid, t);
        if (p.occ) {
            px[0] = p.x; px[1] = p.y; px[2] = p.z;
            pd[0] = r.dx; pd[1] = r.dy; pd[2] = r.dz;
            t += p.dt;
            pl[0] = p.dt; pl[1] = t - last_t; last_t = t;
            if (EDIT) {
                if ((edit_grid[p.index >> 3] >> (p.index & 7u)) & 1u) *pe = 1;
                pe++;
            }
            px += 3; pd += 3; pl += 2; step++;
        } else t = skip_to(cfg, t, p.tt);
    }
}

// ---------------------------------------------------------------- K11 / K12 (inference composite)
// raymarching.cu:948-1035 and :1037-1142.  Its own: the fetch from the global arrays and the write-back; the loop body is
// lae::composite_infer_sample.
template <bool EDIT>
__global__ void k_composite_infer(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* __restrict__ rays_alive,
                                  float* __restrict__ rays_t, const float* __restrict__ sigmas,
                                  const float* __restrict__ rgbs, const float* __restrict__ deltas,
                                  float* __restrict__ weights_sum, float* __restrict__ weights_edit_sum,
                                  float* __restrict__ depth, float* __restrict__ depth_edit,
                                  const uint8_t* __restrict__ edit_occ, float* __restrict__ image) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int32_t index = rays_alive[n];
    const float* s = sigmas + (size_t)n * n_step;
    const float* c = rgbs + 3 * (size_t)n * n_step;
    const float* dl = deltas + 2 * (size_t)n * n_step;
    const uint8_t* eo = EDIT ? edit_occ + (size_t)n * n_step : nullptr;
    lae::RayAcc a{weights_sum[index], depth[index], image[3 * (size_t)index], image[3 * (size_t)index + 1], image[3 * (size_t)index + 2],
                  rays_t[index], 0.f, 0.f};
    if (EDIT) { a.wse = weights_edit_sum[index]; a.de = depth_edit[index]; }
    uint32_t step = 0;
    while (step < n_step) {
        const float d0 = dl[2 * step];
        if (d0 == 0) break;
        if (lae::composite_infer_sample<EDIT>(a, s[step], d0, dl[2 * step + 1], c[3 * step], c[3 * step + 1], c[3 * step + 2],
                                              EDIT && eo[step], T_thresh)) break;           // (lae_common.h, shared with k_frame_head)
        step++;
    }
    if (step < n_step) rays_alive[n] = -1; else rays_t[index] = a.t;
    weights_sum[index] = a.ws; depth[index] = a.depth;
    if (EDIT) { weights_edit_sum[index] = a.wse; depth_edit[index] = a.de; }
    image[3 * (size_t)index] = a.r; image[3 * (size_t)index + 1] = a.g; image[3 * (size_t)index + 2] = a.b;
}

// ---------------------------------------------------------------- alive-list compaction
constexpr int COMPACT_BLOCK = 256;
__global__ __launch_bounds__(COMPACT_BLOCK) void k_compact_count(const int32_t* __restrict__ rays_alive, uint32_t n,
                                                                  uint32_t* __restrict__ local_prefix,
                                                                  uint32_t* __restrict__ block_totals) {
    __shared__ uint32_t lds[COMPACT_BLOCK / 64 + 1];
    const uint32_t i = blockIdx.x * COMPACT_BLOCK + threadIdx.x;
    const uint32_t keep = (i < n && rays_alive[i] >= 0) ? 1u : 0u;
    uint32_t total;
    const uint32_t ex = lae::block_excl_scan<COMPACT_BLOCK / 64>(keep, &total, lds);
    if (i < n) local_prefix[i] = ex;
    if (threadIdx.x == 0) block_totals[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_compact_scan(uint32_t* __restrict__ totals, uint32_t nblk,
                                                        int32_t* __restrict__ n_out) {
    __shared__ uint32_t lds[17];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblk; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblk ? totals[i] : 0;
        uint32_t total;
        const uint32_t ex = lae::block_excl_scan<16>(v, &total, lds);
        if (i < nblk) totals[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_out = (int32_t)carry;
}
__global__ __launch_bounds__(COMPACT_BLOCK) void k_compact_scatter(const int32_t* __restrict__ rays_alive, uint32_t n,
                                                                    const uint32_t* __restrict__ local_prefix,
                                                                    const uint32_t* __restrict__ block_prefix,
                                                                    int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * COMPACT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t v = rays_alive[i];
    if (v >= 0) out[block_prefix[blockIdx.x] + local_prefix[i]] = v;
}

// ---------------------------------------------------------------- host side of K7 / K8: one body per C entry
// the kernel argument of a term: its struct where the flavour has the term, NoArg where it does not
template <bool ON, class T>
std::conditional_t<ON, T, NoArg> term_arg(const T* p) {
    if constexpr (ON) return *p;
    else return NoArg{};
}

// lae_composite_rays_train_step.  A NULL term is absent.  The term-only arguments are checked first (weight, criterion, depth,
// distortion), before the N == 0 return; then the pointers.
int composite_train_step_impl(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M, uint32_t N,
                              float T_thresh, const Blend& bl, const uint32_t* rows_end, const StepLoss& sl, float* weights_sum, float* depth,
                              float* image, float* grad_sigmas, float* grad_rgbs, float* loss_out, int defer_loss, const DepthLoss* dl,
                              const DistLoss* xl, const CritLoss* crit, const WeightLoss* wl, void* stream) {
    // a weight term without a criterion struct is MSE without the entropy term; one without a plane is the CRIT call without WGT
    const CritLoss mse{LAE_LOSS_MSE, 0.0f, 0.0f, 0, nullptr, nullptr, nullptr};
    const CritLoss* cl = crit ? crit : wl ? &mse : nullptr;
    const bool wgt = wl && (wl->w_src || wl->t2_src);
    if (wgt) {
        if (cl->kind != LAE_LOSS_MSE) return LAE_EINVAL;                    // the reference has no weighted L1 / Huber / MAPE
        if (wl->w_src && wl->w_dtype != LAE_IMG_F16 && wl->w_dtype != LAE_IMG_F32) return LAE_EINVAL;
        if (wl->t2_src) {
            if (wl->t2_dtype != LAE_IMG_F16 && wl->t2_dtype != LAE_IMG_F32) return LAE_EINVAL;
            if (wl->t2_channels != 3 && wl->t2_channels != 4) return LAE_EINVAL;
            if (!(wl->lambda >= 0.0f) || !(wl->lambda <= 3.0e38f)) return LAE_EINVAL;
        }
    }
    if (cl) {
        if (!lae::colour_loss_kind_ok(cl->kind, cl->param)) return LAE_EINVAL;
        if (cl->opac && (!(cl->opac_lambda >= 0.0f) || !(cl->opac_lambda <= 3.0e38f))) return LAE_EINVAL;
    }
    if (dl) {
        if (dl->dtype != LAE_IMG_F16 && dl->dtype != LAE_IMG_F32) return LAE_EINVAL;
        if (!(dl->lambda >= 0.0f) || !(dl->lambda <= 3.0e38f)) return LAE_EINVAL;    // NaN, negative and infinite weights
    }
    if (xl && (!(xl->lambda >= 0.0f) || !(xl->lambda <= 3.0e38f))) return LAE_EINVAL;
    if (N == 0) return LAE_OK;
    if (!rays || !weights_sum || !depth || !image || !bl.nears || !bl.fars || !bl.depth_out || !bl.image_out || !rows_end || !sl.target ||
        !sl.grad_image || !loss_out || !sl.partials)
        return LAE_ENULL;
    if (dl && (!dl->src || !dl->grad_depth || !dl->partials)) return LAE_ENULL;      // dl->inds may be NULL (src holds one value per ray)
    if (xl && (!xl->dist || !xl->grad_dist || !xl->partials)) return LAE_ENULL;
    if (cl && cl->opac && (!cl->grad_ws || !cl->opac_partials)) return LAE_ENULL;
    if (wgt && wl->t2_src && !wl->partials) return LAE_ENULL;                        // wl->inds may be NULL (the planes hold one value per ray)
    if (M > 0 && (!sigmas || !rgbs || !deltas || !grad_sigmas || !grad_rgbs)) return LAE_ENULL;
    const uint32_t nb = lae::cdiv(N, COMP_WAVES);
    auto launch = [&](auto with_depth, auto with_dist, auto with_crit, auto with_wgt) {
        constexpr bool DEPTH = decltype(with_depth)::value, DIST = decltype(with_dist)::value, CRIT = decltype(with_crit)::value,
                       WGT = decltype(with_wgt)::value;
        k_composite_train_step<DEPTH, DIST, CRIT, WGT><<<nb, COMP_BLOCK, 0, STREAM(stream)>>>(
            sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image, bl, sl, rows_end, grad_sigmas, grad_rgbs, term_arg<DEPTH>(dl),
            term_arg<DIST>(xl), term_arg<CRIT>(cl), term_arg<WGT>(wl));
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    // twelve flavours: depth and distortion on or off, times no criterion struct (the CRIT = false kernels) / CRIT / CRIT with WGT
    auto colour = [&](auto with_depth, auto with_dist) {
        if (wgt) launch(with_depth, with_dist, yes, yes);
        else if (cl) launch(with_depth, with_dist, yes, no);
        else launch(with_depth, with_dist, no, no);
    };
    if (dl) xl ? colour(yes, yes) : colour(yes, no);
    else xl ? colour(no, yes) : colour(no, no);
    // defer_loss: the one-block sum of the partials (5.5 us + a kernel boundary on the step's critical path for a number that
    // feeds nothing on the device) is left to lae_loss_finish or to a later launch that takes it along
    // (lae_nerf_head_backward); loss_out holds NaN until then
    if (!defer_loss) k_loss_finish<<<1, 1024, 0, STREAM(stream)>>>(sl.partials, nb, 3u * N, sl.scale, loss_out);
    return lae::check_launch("composite_rays_train_step");
}

// lae_composite_rays_train_backward_blend_ex: DEPTH = grad_depth != NULL, DIST = grad_dist != NULL; `depth` is the D of both
int composite_train_backward_blend_impl(const float* grad_weights_sum, const float* grad_image, const float* sigmas, const float* rgbs,
                                        const float* deltas, const int32_t* rays, const float* weights_sum, const float* image, uint32_t M,
                                        uint32_t N, float T_thresh, const Dense& dn, float* grad_sigmas, float* grad_rgbs,
                                        const float* grad_depth, const float* depth, const float* grad_dist, const float* dist, void* stream) {
    if (N == 0 || M == 0) return LAE_OK;
    if (!grad_image || !sigmas || !rgbs || !deltas || !rays || !weights_sum || !image || !grad_sigmas || !grad_rgbs || !dn.rows_end)
        return LAE_ENULL;                                   // grad_weights_sum may be NULL (= zero)
    if ((grad_depth || grad_dist) && !depth) return LAE_ENULL;
    if (grad_dist && !dist) return LAE_ENULL;
    const DepthGrad dg{grad_depth, depth};
    const DistGrad xg{grad_dist, dist, depth};
    auto launch = [&](auto with_depth, auto with_dist) {
        constexpr bool DEPTH = decltype(with_depth)::value, DIST = decltype(with_dist)::value;
        k_composite_train_bwd<true, DEPTH, DIST><<<lae::cdiv(N, COMP_WAVES), COMP_BLOCK, 0, STREAM(stream)>>>(
            grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs, dn,
            term_arg<DEPTH>(&dg), term_arg<DIST>(&xg));
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (grad_depth) grad_dist ? launch(yes, yes) : launch(yes, no);
    else grad_dist ? launch(no, yes) : launch(no, no);
    return lae::check_launch("composite_rays_train_backward_blend");
}


}  // namespace

// =====================================================================
// C ABI
// =====================================================================

extern "C" {

int lae_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near,
                           float* nears, float* fars, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays_o || !rays_d || !aabb || !nears || !fars) return LAE_ENULL;
    k_near_far<<<lae::cdiv(N, 256), 256, 0, STREAM(stream)>>>(rays_o, rays_d, aabb, N, min_near, nears, fars);
    return lae::check_launch("near_far_from_aabb");
}

int lae_get_rays(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                 const int64_t* inds, uint64_t inds_batch_stride, uint32_t N, int perturb, float off_x, float off_y,
                 float* rays_o, float* rays_d, const float* aabb, float min_near, float* nears, float* fars, void* stream) {
    if (N == 0 || B == 0) return LAE_OK;
    if (!poses || !rays_o || !rays_d) return LAE_ENULL;
    if (aabb && (!nears || !fars)) return LAE_ENULL;
    if (H == 0 || W == 0 || B > 65535u || (!inds && (uint64_t)N != (uint64_t)H * W)) return LAE_EINVAL;
    k_get_rays<<<dim3(lae::cdiv(N, 256), B), 256, 0, STREAM(stream)>>>(poses, B, fx, fy, cx, cy, W, inds, inds_batch_stride, N, off_x,
                                                                       off_y, perturb, rays_o, rays_d, aabb, min_near, nears, fars);
    return lae::check_launch("get_rays");
}

int lae_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays_o || !rays_d || !coords) return LAE_ENULL;
    k_sph_from_ray<<<lae::cdiv(N, 256), 256, 0, STREAM(stream)>>>(rays_o, rays_d, radius, N, coords);
    return lae::check_launch("sph_from_ray");
}

int lae_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, void* stream) {
    if (N == 0) return LAE_OK;
    if (!coords || !indices) return LAE_ENULL;
    k_morton3D<<<lae::cdiv(N, 256), 256, 0, STREAM(stream)>>>(coords, N, indices);
    return lae::check_launch("morton3D");
}

int lae_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, void* stream) {
    if (N == 0) return LAE_OK;
    if (!coords || !indices) return LAE_ENULL;
    k_morton3D_invert<<<lae::cdiv(N, 256), 256, 0, STREAM(stream)>>>(indices, N, coords);
    return lae::check_launch("morton3D_invert");
}

int lae_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, void* stream) {
    if (N == 0) return LAE_OK;
    if (!grid || !bitfield) return LAE_ENULL;
    k_packbits<<<lae::cdiv(N, 256), 256, 0, STREAM(stream)>>>(grid, N, density_thresh, bitfield);
    return lae::check_launch("packbits");
}

constexpr uint32_t MARCH_REC_RAYS_MAX = 1u << 18;         // replay records only for batches up to 256 k rays (73 MB of scratch)
static inline uint64_t march_base_bytes(uint32_t N) { return ((4ull * (2ull * N + 3) + 60) + 15) / 16 * 16; }
uint64_t lae_march_rays_train_scratch_bytes(uint32_t N) {
    // counts[N] | prefix[N + 2] | rows_end | (N <= 2^18:) nrec[N] | records[N * 24]
    return march_base_bytes(N) + (N <= MARCH_REC_RAYS_MAX ? ((4ull * N + 15) / 16 * 16) + (uint64_t)N * MARCH_REC_MAX * sizeof(MarchRec) : 0ull);
}

static int march_rays_train_impl(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                                 uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const uint32_t* m_limit,
                                 const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays,
                                 int32_t* counter, const float* noises, void* scratch, uint32_t* rows_end_out, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays_o || !rays_d || !grid || !nears || !fars || !xyzs || !dirs || !deltas || !rays || !noises || !scratch)
        return LAE_ENULL;
    if (C == 0 || C > 8 || H == 0 || H > 1024 || max_steps == 0) return LAE_EINVAL;
    const MarchCfg cfg = make_cfg(bound, dt_gamma, max_steps, C, H);
    const uint32_t nblk = lae::cdiv(N, MARCH_WAVES);
    uint32_t* counts = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* prefix = counts + N;
    hipStream_t s = STREAM(stream);
    MarchRecs recs{nullptr, nullptr};
    if (N <= MARCH_REC_RAYS_MAX) {
        uint8_t* base = reinterpret_cast<uint8_t*>(scratch) + march_base_bytes(N);
        recs.nrec = reinterpret_cast<uint32_t*>(base);
        recs.rec = reinterpret_cast<MarchRec*>(base + (4ull * N + 15) / 16 * 16);
    }
    k_march_train_wave<false><<<nblk, MARCH_BLOCK, 0, s>>>(rays_o, rays_d, grid, cfg, max_steps, N, M, m_limit, nears, fars, noises,
                                                           counts, nullptr, nullptr, nullptr, nullptr, nullptr, recs);
    k_scan_counts<<<1, 1024, 0, s>>>(counts, N, M, m_limit, prefix, counter, rows_end_out);
    k_march_train_wave<true><<<nblk, MARCH_BLOCK, 0, s>>>(rays_o, rays_d, grid, cfg, max_steps, N, M, m_limit, nears, fars, noises,
                                                          counts, prefix, xyzs, dirs, deltas, rays, recs);
    return lae::check_launch("march_rays_train");
}

int lae_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                         const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                         const float* noises, void* scratch, uint32_t* rows_end_out, void* stream) {
    return march_rays_train_impl(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nullptr, nears, fars, xyzs, dirs,
                                 deltas, rays, counter, noises, scratch, rows_end_out, stream);
}

int lae_march_rays_train_limit(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, float dt_gamma,
                               uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M_cap, const uint32_t* m_limit,
                               const float* nears, const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays,
                               int32_t* counter, const float* noises, void* scratch, uint32_t* rows_end_out, void* stream) {
    if (N != 0 && !m_limit) return LAE_ENULL;
    return march_rays_train_impl(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M_cap, m_limit, nears, fars, xyzs,
                                 dirs, deltas, rays, counter, noises, scratch, rows_end_out, stream);
}

int lae_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                     uint32_t M, uint32_t N, float T_thresh, float* weights_sum, float* depth,
                                     float* image, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays || !weights_sum || !depth || !image) return LAE_ENULL;
    if (M > 0 && (!sigmas || !rgbs || !deltas)) return LAE_ENULL;
    k_composite_train_fwd<false><<<lae::cdiv(N, COMP_WAVES), COMP_BLOCK, 0, STREAM(stream)>>>(sigmas, rgbs, deltas, rays, M, N,
                                                                                               T_thresh, weights_sum, depth, image, Blend{}, NoArg{});
    return lae::check_launch("composite_rays_train_forward");
}

int lae_composite_rays_train_forward_blend(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                           uint32_t M, uint32_t N, float T_thresh, const float* nears, const float* fars,
                                           const float* bg_rays, float bg_r, float bg_g, float bg_b, float* weights_sum,
                                           float* depth, float* image, float* depth_out, float* image_out, float* dist, void* stream) {
    if (N == 0) return LAE_OK;
    if (!rays || !weights_sum || !depth || !image || !nears || !fars || !depth_out || !image_out) return LAE_ENULL;
    if (M > 0 && (!sigmas || !rgbs || !deltas)) return LAE_ENULL;
    const Blend bl{nears, fars, bg_rays, {bg_r, bg_g, bg_b}, image_out, depth_out};
    const uint32_t nb = lae::cdiv(N, COMP_WAVES);
    if (dist)
        k_composite_train_fwd<true, true><<<nb, COMP_BLOCK, 0, STREAM(stream)>>>(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth,
                                                                                 image, bl, dist);
    else
        k_composite_train_fwd<true><<<nb, COMP_BLOCK, 0, STREAM(stream)>>>(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image,
                                                                           bl, NoArg{});
    return lae::check_launch("composite_rays_train_forward_blend");
}

int lae_composite_rays_train_step(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M,
                                  uint32_t N, float T_thresh, const float* nears, const float* fars, const float* bg_rays, float bg_r,
                                  float bg_g, float bg_b, const uint32_t* rows_end, const float* target, const float* scale,
                                  float* weights_sum, float* depth, float* image, float* depth_out, float* image_out,
                                  float* grad_image, float* grad_sigmas, float* grad_rgbs, float* loss_out, float* partials,
                                  int defer_loss, const lae_depth_term* depth_term, const lae_dist_term* dist_term,
                                  const lae_crit_term* crit_term, const lae_weight_term* weight_term, void* stream) {
    return composite_train_step_impl(sigmas, rgbs, deltas, rays, M, N, T_thresh, Blend{nears, fars, bg_rays, {bg_r, bg_g, bg_b}, image_out, depth_out},
                                     rows_end, StepLoss{target, scale, grad_image, partials, defer_loss ? loss_out : nullptr}, weights_sum, depth,
                                     image, grad_sigmas, grad_rgbs, loss_out, defer_loss, depth_term, dist_term, crit_term, weight_term, stream);
}

int lae_loss_finish(const float* partials, uint32_t n_part, uint32_t n_elem, const float* scale, float* loss_out, void* stream) {
    if (!partials || !loss_out) return LAE_ENULL;
    if (n_elem == 0) return LAE_EINVAL;
    k_loss_finish<<<1, 1024, 0, STREAM(stream)>>>(partials, n_part, n_elem, scale, loss_out);
    return lae::check_launch("loss_finish");
}

int lae_composite_rays_train_backward_blend_ex(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                               const float* rgbs, const float* deltas, const int32_t* rays,
                                               const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                               float T_thresh, const float* bg_rays, float bg_r, float bg_g, float bg_b,
                                               const uint32_t* rows_end, const float* grad_scale, float* grad_sigmas,
                                               float* grad_rgbs, const float* grad_depth, const float* depth, const float* grad_dist,
                                               const float* dist, void* stream) {
    return composite_train_backward_blend_impl(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh,
                                               Dense{bg_rays, {bg_r, bg_g, bg_b}, rows_end, grad_scale}, grad_sigmas, grad_rgbs, grad_depth, depth,
                                               grad_dist, dist, stream);
}

int lae_composite_rays_train_backward_blend(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                            const float* rgbs, const float* deltas, const int32_t* rays,
                                            const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                            float T_thresh, const float* bg_rays, float bg_r, float bg_g, float bg_b,
                                            const uint32_t* rows_end, float* grad_sigmas, float* grad_rgbs, void* stream) {
    if (N == 0 || M == 0) return LAE_OK;
    if (!grad_weights_sum) return LAE_ENULL;
    return lae_composite_rays_train_backward_blend_ex(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N,
                                                      T_thresh, bg_rays, bg_r, bg_g, bg_b, rows_end, nullptr, grad_sigmas, grad_rgbs, nullptr, nullptr,
                                                      nullptr, nullptr, stream);
}

int lae_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                      const float* rgbs, const float* deltas, const int32_t* rays,
                                      const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                      float T_thresh, float* grad_sigmas, float* grad_rgbs, void* stream) {
    if (N == 0 || M == 0) return LAE_OK;
    if (!grad_weights_sum || !grad_image || !sigmas || !rgbs || !deltas || !rays || !weights_sum || !image ||
        !grad_sigmas || !grad_rgbs)
        return LAE_ENULL;
    k_composite_train_bwd<false><<<lae::cdiv(N, COMP_WAVES), COMP_BLOCK, 0, STREAM(stream)>>>(
        grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas,
        grad_rgbs, Dense{}, NoArg{}, NoArg{});
    return lae::check_launch("composite_rays_train_backward");
}

int lae_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                   const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                   uint32_t C, uint32_t H, const uint8_t* grid, const float* nears, const float* fars, float* xyzs,
                   float* dirs, float* deltas, const float* noises, void* stream) {
    (void)nears;
    if (n_alive == 0 || n_step == 0) return LAE_OK;
    if (!rays_alive || !rays_t || !rays_o || !rays_d || !grid || !fars || !xyzs || !dirs || !deltas || !noises)
        return LAE_ENULL;
    if (C == 0 || C > 8 || H == 0 || H > 1024 || max_steps == 0) return LAE_EINVAL;
    const MarchCfg cfg = make_cfg(bound, dt_gamma, max_steps, C, H);
    k_march_infer<false><<<lae::cdiv(n_alive, 128), 128, 0, STREAM(stream)>>>(
        n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, cfg, grid, nullptr, fars, xyzs, dirs, deltas, nullptr,
        noises);
    return lae::check_launch("march_rays");
}

int lae_march_rays_distill(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t,
                           const float* rays_o, const float* rays_d, float bound, float dt_gamma, uint32_t max_steps,
                           uint32_t C, uint32_t H, const uint8_t* grid, const uint8_t* edit_grid, const float* nears,
                           const float* fars, float* xyzs, float* dirs, float* deltas, uint8_t* edit_occ,
                           const float* noises, void* stream) {
    (void)nears;
    if (n_alive == 0 || n_step == 0) return LAE_OK;
    if (!rays_alive || !rays_t || !rays_o || !rays_d || !grid || !edit_grid || !fars || !xyzs || !dirs || !deltas ||
        !edit_occ || !noises)
        return LAE_ENULL;
    if (C == 0 || C > 8 || H == 0 || H > 1024 || max_steps == 0) return LAE_EINVAL;
    const MarchCfg cfg = make_cfg(bound, dt_gamma, max_steps, C, H);
    k_march_infer<true><<<lae::cdiv(n_alive, 128), 128, 0, STREAM(stream)>>>(
        n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, cfg, grid, edit_grid, fars, xyzs, dirs, deltas, edit_occ,
        noises);
    return lae::check_launch("march_rays_distill");
}

int lae_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, float* rays_t,
                       const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum, float* depth,
                       float* image, void* stream) {
    if (n_alive == 0) return LAE_OK;
    if (!rays_alive || !rays_t || !sigmas || !rgbs || !deltas || !weights_sum || !depth || !image) return LAE_ENULL;
    k_composite_infer<false><<<lae::cdiv(n_alive, 128), 128, 0, STREAM(stream)>>>(
        n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, nullptr, depth, nullptr,
        nullptr, image);
    return lae::check_launch("composite_rays");
}

int lae_composite_rays_distill(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t* rays_alive, float* rays_t,
                               const float* sigmas, const float* rgbs, const float* deltas, float* weights_sum,
                               float* weights_edit_sum, float* depth, float* depth_edit, const uint8_t* edit_occ,
                               float* image, void* stream) {
    if (n_alive == 0) return LAE_OK;
    if (!rays_alive || !rays_t || !sigmas || !rgbs || !deltas || !weights_sum || !weights_edit_sum || !depth ||
        !depth_edit || !edit_occ || !image)
        return LAE_ENULL;
    k_composite_infer<true><<<lae::cdiv(n_alive, 128), 128, 0, STREAM(stream)>>>(
        n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, weights_edit_sum, depth,
        depth_edit, edit_occ, image);
    return lae::check_launch("composite_rays_distill");
}

uint64_t lae_compact_scratch_bytes(uint32_t n_alive) {
    return 4ull * ((uint64_t)n_alive + lae::cdiv(n_alive, COMPACT_BLOCK)) + 64;
}

int lae_compact_rays_alive(const int32_t* rays_alive, uint32_t n_alive, int32_t* out_alive, int32_t* n_out_dev,
                           void* scratch, void* stream) {
    if (!n_out_dev) return LAE_ENULL;
    hipStream_t s = STREAM(stream);
    if (n_alive == 0) return hipMemsetAsync(n_out_dev, 0, 4, s) == hipSuccess ? LAE_OK : LAE_ELAUNCH;
    if (!rays_alive || !out_alive || !scratch) return LAE_ENULL;
    const uint32_t nblk = lae::cdiv(n_alive, COMPACT_BLOCK);
    uint32_t* local_prefix = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* totals = local_prefix + n_alive;
    k_compact_count<<<nblk, COMPACT_BLOCK, 0, s>>>(rays_alive, n_alive, local_prefix, totals);
    k_compact_scan<<<1, 1024, 0, s>>>(totals, nblk, n_out_dev);
    k_compact_scatter<<<nblk, COMPACT_BLOCK, 0, s>>>(rays_alive, n_alive, local_prefix, totals, out_alive);
    return lae::check_launch("compact_rays_alive");
}


}  // extern "C"
