// nerfhead.hip -- the fused NeRF head forward (k_nerf_head_fwd5) and the frame loop's head + compositing kernel (k_frame_head).
// Weight layout and MFMA mapping: head of ffmlp.hip; fragment helpers: mlp_frags.h; the head's backward: mlpbackward.hip.
#include <string>
#include <algorithm>
#include "lae_common.h"
#include "mlp_frags.h"

namespace {

// ---------------------------------------------------------------- fused NeRF head (network_ff.py:51-81 in one kernel)
// sigma net (32 -> 64 -> 64 -> 16) -> sigma = density_scale * exp(h[0]) ; colour-net input = [SH_4(dir) | h[1..15] | 0]
// -> colour net (32 -> 64 -> 64 -> 64 -> 16) -> rgb = sigmoid(out[0..2]).  One wave owns a 16-row tile and chains
// every activation through registers in the MFMA C/D layout (lane = row, 4 regs = 4 consecutive features):
//   * h[1 + m] -> colour feature 16 + m is a shift by one feature: three in-lane register moves and one
//     16-lane shuffle;
//   * the 16 SH values of a row are evaluated per lane and the lane keeps components 4g..4g+3 (its K-slice);
//   * weights of both nets sit row-major in LDS (ds_read_b64 fragments).
// Saved for the backward: h [M,16] fp16 (32 B/row) and rgb; nothing else touches HBM.

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Head4Scratch { half_t sh[64][16]; float q[64][4]; };             // per wave: SH block and logits on their way between row-per-lane and fragment layout

// ---------------------------------------------------------------- fused NeRF head, the kernel that ships
// (round 1-2: one 16-row tile per wave iteration, weights row-major in LDS; round 3 first form: fragments in 144 registers,
// one wave per SIMD -- both removed in round 4, their measurements are in DESIGN.md appendix A.)
//  * a wave owns FOUR tiles (64 rows) per iteration and every layer is issued for all four before its activations are
//    needed: four independent MFMA -> cvt / relu -> MFMA chains per wave instead of one;
//  * per-row scalar work (SH polynomials, exp, three sigmoids with an IEEE division each) is done by lane L for row L once,
//    not by the four lane groups of a 16-row tile; the values reach / leave the MFMA fragment layout through a wave-private
//    3 KB LDS scratch (2 wide stores + 4 fragment reads for the SH block; one masked store per tile + one read for the
//    density logit and the colour logits).  sigma / rgb leave as one coalesced row-per-lane store;
//  * the A fragments are re-read from a pre-swizzled LDS image (one conflict-free ds_read_b128 per fragment PAIR and four
//    tiles) instead of being held in registers: in-kernel stamps (tools/ubench/mlp_probe.hip) showed that 1024 waves each
//    pulling 37 KB of fragments from L2 take 7.5 us before the first row is touched, and that one wave alone on a SIMD
//    issues an instruction every ~5 cycles whatever it is -- the rate of this kernel is instructions per row x issue
//    interval, and the issue interval halves with a second wave on the SIMD.
// LDS image of a [16 MT, 32 KP] weight matrix: fragment pair (mt, p) of lane l = 16 bytes at ((mt * KP + p) * 64 + l) * 16:
// halves 0-3 = W[16 mt + c][32 p + 4 g ..], halves 4-7 = W[16 mt + c][32 p + 16 + 4 g ..] (the two operands of one K = 32 MFMA).
template <int MT, int KP, int NTH>
__device__ __forceinline__ void stage_swizzled_issue(const half_t* __restrict__ W, uint4 (&buf)[(MT * KP * 64 + NTH - 1) / NTH]) {
    constexpr int CHUNKS = MT * 16 * KP * 32 / 8;                        // 16-byte chunks of the row-major matrix
#pragma unroll
    for (int i = 0; i < (MT * KP * 64 + NTH - 1) / NTH; i++) {
        const int e = (int)threadIdx.x + i * NTH;
        if (e < CHUNKS) buf[i] = *reinterpret_cast<const uint4*>(W + (size_t)e * 8);
    }
}
template <int MT, int KP, int NTH>
__device__ __forceinline__ void stage_swizzled_store(half_t* img, const uint4 (&buf)[(MT * KP * 64 + NTH - 1) / NTH]) {
    constexpr int CHUNKS = MT * 16 * KP * 32 / 8, K = KP * 32;
#pragma unroll
    for (int i = 0; i < (MT * KP * 64 + NTH - 1) / NTH; i++) {
        const int e = (int)threadIdx.x + i * NTH;
        if (e < CHUNKS) {
            const int row = (e * 8) / K, k = (e * 8) % K;                // halves k .. k + 7 of row `row`
            const int mt = row >> 4, cc = row & 15;
#pragma unroll
            for (int piece = 0; piece < 2; piece++) {
                const int kk = k + 4 * piece, p = kk >> 5, hh = (kk >> 4) & 1, gg = (kk >> 2) & 3;
                const uint2 v = piece ? uint2{buf[i].z, buf[i].w} : uint2{buf[i].x, buf[i].y};
                *reinterpret_cast<uint2*>(img + ((size_t)((mt * KP + p) * 64 + gg * 16 + cc)) * 8 + hh * 4) = v;
            }
        }
    }
}
struct Head5Img {                                                       // halves
    static constexpr int S0 = 0, S1 = S0 + 64 * 32, SO = S1 + 64 * 64, C0 = SO + 16 * 64, C1 = C0 + 64 * 32, C2 = C1 + 64 * 64,
                         CO = C2 + 64 * 64, END = CO + 16 * 64;
};
// 64-wide layer on NT tiles, A fragment pairs from the swizzled image
template <int KP, int NT>
__device__ __forceinline__ void layer64s(const half_t* img, int lane, const h4 (&in)[NT][2 * KP], h4 (&out)[NT][4]) {
    f4 acc[NT][4];
#pragma unroll
    for (int p = 0; p < KP; p++)
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const h8 a = *reinterpret_cast<const h8*>(img + ((size_t)((mt * KP + p) * 64 + lane)) * 8);
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const h8 b = __builtin_shufflevector(in[t][2 * p], in[t][2 * p + 1], 0, 1, 2, 3, 4, 5, 6, 7);
                acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, p == 0 ? f4{0, 0, 0, 0} : acc[t][mt], 0, 0, 0);
            }
        }
#pragma unroll
    for (int t = 0; t < NT; t++) relu4(acc[t], out[t]);
}
template <int NT>
__device__ __forceinline__ void out16s(const half_t* img, int lane, const h4 (&in)[NT][4], f4 (&o)[NT]) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const h8 a = *reinterpret_cast<const h8*>(img + ((size_t)(p * 64 + lane)) * 8);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const h8 b = __builtin_shufflevector(in[t][2 * p], in[t][2 * p + 1], 0, 1, 2, 3, 4, 5, 6, 7);
            o[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, p == 0 ? f4{0, 0, 0, 0} : o[t], 0, 0, 0);
        }
    }
}

template <bool COLOR, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_nerf_head_fwd5(
    const half_t* __restrict__ enc, const float* __restrict__ dirs, const half_t* __restrict__ Ws, const half_t* __restrict__ Wc,
    uint32_t n_tiles, float density_scale, half_t* __restrict__ h_out, float* __restrict__ sigmas, float* __restrict__ rgbs,
    int level_major, const uint32_t* __restrict__ n_rows_dev, uint32_t lm_rows) {
    constexpr int NT = 4, NTH = 64 * WAVES;
    using I = Head5Img;
    if (n_rows_dev) n_tiles = min(n_tiles, (*n_rows_dev + 15u) / 16u);
    if (n_tiles == 0) return;
    extern __shared__ __attribute__((aligned(16))) half_t lds[];
    half_t* img = lds;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    Head4Scratch* sc = reinterpret_cast<Head4Scratch*>(lds + (COLOR ? I::END : I::C0)) + w;
    MLP_STAMP(blockIdx.x * WAVES + w, 0);
    // ---- weights -> swizzled LDS image: every global load of the workgroup in flight before the first LDS store
    {
        constexpr int N1 = (4 * 1 * 64 + NTH - 1) / NTH, N2 = (4 * 2 * 64 + NTH - 1) / NTH, NO = (1 * 2 * 64 + NTH - 1) / NTH;
        uint4 b0[N1], b1[N2], b2[NO];
        stage_swizzled_issue<4, 1, NTH>(Ws, b0);
        stage_swizzled_issue<4, 2, NTH>(Ws + 64 * 32, b1);
        stage_swizzled_issue<1, 2, NTH>(Ws + 64 * 32 + 4096, b2);
        if constexpr (COLOR) {
            uint4 c0[N1], c1[N2], c2[N2], c3[NO];
            stage_swizzled_issue<4, 1, NTH>(Wc, c0);
            stage_swizzled_issue<4, 2, NTH>(Wc + 64 * 32, c1);
            stage_swizzled_issue<4, 2, NTH>(Wc + 64 * 32 + 4096, c2);
            stage_swizzled_issue<1, 2, NTH>(Wc + 64 * 32 + 8192, c3);
            stage_swizzled_store<4, 1, NTH>(img + I::C0, c0);
            stage_swizzled_store<4, 2, NTH>(img + I::C1, c1);
            stage_swizzled_store<4, 2, NTH>(img + I::C2, c2);
            stage_swizzled_store<1, 2, NTH>(img + I::CO, c3);
        }
        stage_swizzled_store<4, 1, NTH>(img + I::S0, b0);
        stage_swizzled_store<4, 2, NTH>(img + I::S1, b1);
        stage_swizzled_store<1, 2, NTH>(img + I::SO, b2);
    }
    const uint32_t n_groups = (n_tiles + NT - 1) / NT;
    const uint32_t wave0 = blockIdx.x * WAVES + (uint32_t)w, nwaves = gridDim.x * WAVES;
    const uint32_t n_rows = n_tiles * 16u;
    h4 xf_n[NT][2] = {};
    float d_n[3] = {0.f, 0.f, 0.f};
    // inputs through buffer descriptors: one 32-bit lane offset per group, the tile / k-step / level strides ride in the
    // instruction's immediate and scalar offsets (the 64-bit address arithmetic of 16 + 3 plain loads was ~90 instructions
    // per group), and the hardware range check returns zeros past the end instead of branches around the loads.  Level-major
    // features: a row past the live rows of plane l reads plane l + 1 (memory of the same buffer; its results are never stored).
    const __amdgpu_buffer_rsrc_t rs_enc = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(enc), 0,
                                                                            (int)((level_major ? lm_rows : n_rows) * 64u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dir = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(COLOR ? dirs : sigmas), 0, (int)(n_rows * 12u), 0x00020000);
    const uint32_t plane = lm_rows * 4u;                               // bytes per level plane
    auto request = [&](uint32_t grp) {
        const uint32_t row0 = grp * 64u;
        if (level_major) {
            const uint32_t vo = ((uint32_t)(2 * g) * lm_rows + row0 + (uint32_t)c) * 4u;
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int kt = 0; kt < 2; kt++) {
                    const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(rs_enc, (int)(vo + t * 64u), (int)((8u * kt) * plane), 0);
                    const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(rs_enc, (int)(vo + t * 64u), (int)((8u * kt + 1u) * plane), 0);
                    xf_n[t][kt] = __builtin_bit_cast(h4, uint2{lo, hi});
                }
        } else {
            const uint32_t vo = (row0 + (uint32_t)c) * 64u + 8u * (uint32_t)g;
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int kt = 0; kt < 2; kt++) {
                    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
                    const u2v v = __builtin_amdgcn_raw_buffer_load_b64(rs_enc, (int)(vo + t * 1024u + kt * 32u), 0, 0);
                    xf_n[t][kt] = __builtin_bit_cast(h4, v);
                }
        }
        if constexpr (COLOR) {
            const uint32_t vo = (row0 + (uint32_t)lane) * 12u;
#pragma unroll
            for (int k = 0; k < 3; k++) d_n[k] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_dir, (int)(vo + 4u * k), 0, 0));
        }
    };
    if (wave0 < n_groups) request(wave0);
    __syncthreads();                                                     // the image is complete
    [[maybe_unused]] int stamp_i = 1;
    for (uint32_t grp = wave0; grp < n_groups; grp += nwaves) {
        MLP_STAMP(blockIdx.x * WAVES + w, stamp_i); stamp_i++;
        h4 xf[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++) { xf[t][0] = xf_n[t][0]; xf[t][1] = xf_n[t][1]; }
        const float dx = d_n[0], dy = d_n[1], dz = d_n[2];
        if (grp + nwaves < n_groups) request(grp + nwaves);
        const uint32_t row_l = grp * 64u + (uint32_t)lane;
        if constexpr (COLOR) {
            float o[16], gx[1], gy[1], gz[1];
            sh_eval<4, false>(dx, dy, dz, o, gx, gy, gz);
            h8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; j++) { lo[j] = (half_t)o[j]; hi[j] = (half_t)o[8 + j]; }
            *reinterpret_cast<h8*>(&sc->sh[lane][0]) = lo;
            *reinterpret_cast<h8*>(&sc->sh[lane][8]) = hi;
        }
        h4 a0[NT][4], a1[NT][4];
        layer64s<1, NT>(img + I::S0, lane, xf, a0);
        layer64s<2, NT>(img + I::S1, lane, a0, a1);
        f4 so[NT];
        out16s<NT>(img + I::SO, lane, a1, so);
        h4 hq[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++) hq[t][r] = (half_t)so[t][r];
            const uint32_t tile = grp * NT + t;
            if (h_out && tile < n_tiles) *reinterpret_cast<h4*>(h_out + ((size_t)tile * 16 + c) * 16 + 4 * g) = hq[t];
            if (g == 0) sc->q[t * 16 + c][0] = (float)hq[t][0];
        }
        wave_lds_fence();
        if (row_l < n_rows) sigmas[row_l] = density_scale * expf(sc->q[lane][0]);        // trunc_exp forward (activation.py:9)
        if constexpr (!COLOR) { wave_lds_fence(); continue; }
        h4 cin[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            cin[t][0] = *reinterpret_cast<const h4*>(&sc->sh[t * 16 + c][4 * g]);
            const half_t nxt = __builtin_bit_cast(half_t, (uint16_t)__shfl_down((int)__builtin_bit_cast(uint16_t, hq[t][0]), 16, 64));
            cin[t][1][0] = hq[t][1]; cin[t][1][1] = hq[t][2]; cin[t][1][2] = hq[t][3];
            cin[t][1][3] = g == 3 ? (half_t)0.0f : nxt;
        }
        layer64s<1, NT>(img + I::C0, lane, cin, a0);
        layer64s<2, NT>(img + I::C1, lane, a0, a1);
        layer64s<2, NT>(img + I::C2, lane, a1, a0);
        f4 co[NT];
        out16s<NT>(img + I::CO, lane, a0, co);
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < NT; t++)
            if (g == 0) *reinterpret_cast<f4*>(&sc->q[t * 16 + c][0]) = co[t];
        wave_lds_fence();
        if (row_l < n_rows) {
            const f4 v = *reinterpret_cast<const f4*>(&sc->q[lane][0]);
            struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };
            F3 out;
            out.x = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[0])));
            out.y = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[1])));
            out.z = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[2])));
            *reinterpret_cast<F3*>(rgbs + (size_t)row_l * 3) = out;
        }
        wave_lds_fence();
    }
    MLP_STAMP(blockIdx.x * WAVES + w, 15);
}

// ---------------------------------------------------------------- frame loop: head + composite_rays in one launch
// k_nerf_head_fwd5<true> followed, inside the wave, by composite_rays / composite_rays_distill (raymarching.cu:948-1035 /
// :1037-1142) for the rays whose rows the wave just shaded.  Rows are ray-major in 64-row groups of whole rays
// (lae_common.h FrameCtrl), lane L of a wave does the per-row work of row L of its group, so the sigma / rgb of a ray's
// n_step rows sit in n_step consecutive lanes: they go through the wave's LDS scratch to the lane of the ray's first row,
// which runs the reference's serial loop (lae::composite_infer_sample, the body k_composite_infer runs: the image is the same
// bits as the two-kernel form's) on the ray's 32-byte accumulator record.  sigmas / rgbs never reach memory (16 B written + 16 B read per row) and
// the compositing launch with its 40-56 B per ray of scattered accumulator traffic is gone: 9 / 29 us per iteration of the
// 800x800 / 1080p frame (profiles/r4_*).
// Work is dealt in CONTIGUOUS runs of groups, one run per wave (unit u = blockIdx.x * WAVES + wave), and a wave appends the
// rays that go on to its own survivor segment [u * R, ...) + count (+ the workgroup's sum of counts): the next iteration's
// per-ray kernels walk the segments in unit order (frame.hip frame_locate), so the alive list keeps its order -- stable
// compaction, no atomics, the same list every run.  (Compacting inside this launch -- every workgroup publishing its count
// and waiting for the counts of the workgroups before it -- was built and measured in round 4: 12.65 against 12.26 ms per
// 800x800 frame, and two processes sharing one GPU crawl when spinning workgroups keep each other's predecessors out.)
struct FrameHeadScratch { float dl[64][2]; uint32_t eo[64]; };         // per wave, behind its Head4Scratch

template <bool EDIT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_frame_head(
    const half_t* __restrict__ enc, const float* __restrict__ dirs, const half_t* __restrict__ Ws, const half_t* __restrict__ Wc,
    float density_scale, uint32_t lm_rows, lae::FrameHeadArgs fa) {
    constexpr int NT = 4, NTH = 64 * WAVES;
    using I = Head5Img;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t unit = blockIdx.x * WAVES + (uint32_t)w, n_units = gridDim.x * WAVES;
    const lae::FrameCtrl ctl = *fa.cur;
    const uint32_t n_alive = ctl.n_alive, n_step = max(ctl.n_step, 1u);
    const uint32_t rpg = lae::frame_rays_per_group(n_step);
    const uint32_t n_groups = (n_alive + rpg - 1) / rpg;
    const uint32_t per_unit = (n_groups + n_units - 1) / n_units;
    // the block's first unit decides whether the block has any work (units are dealt in order)
    if (min(n_groups, blockIdx.x * WAVES * per_unit) >= n_groups) {
        if (lane == 0) fa.seg_counts_next[unit] = 0u;
        if (threadIdx.x == 0) fa.blk_counts_next[blockIdx.x] = 0u;
        return;
    }
    __shared__ uint32_t wave_kept[WAVES];
    uint32_t kept = 0;                                                   // survivors this wave has appended (uniform)
    int32_t* seg = fa.seg_next + (size_t)unit * fa.R;
    const uint32_t g_lo = min(n_groups, unit * per_unit), g_hi = min(n_groups, g_lo + per_unit);
    extern __shared__ __attribute__((aligned(16))) half_t lds[];
    half_t* img = lds;
    Head4Scratch* sc = reinterpret_cast<Head4Scratch*>(lds + I::END) + w;
    FrameHeadScratch* fs = reinterpret_cast<FrameHeadScratch*>(reinterpret_cast<Head4Scratch*>(lds + I::END) + WAVES) + w;
    {   // weights -> swizzled LDS image.  The head below is k_nerf_head_fwd5<true>'s, written out a second time ON PURPOSE: shared
        // pieces cost that kernel 1.5-3.5 % ("shared bodies"); a change to the head is made in both
        constexpr int N1 = (4 * 1 * 64 + NTH - 1) / NTH, N2 = (4 * 2 * 64 + NTH - 1) / NTH, NO = (1 * 2 * 64 + NTH - 1) / NTH;
        uint4 b0[N1], b1[N2], b2[NO], c0[N1], c1[N2], c2[N2], c3[NO];
        stage_swizzled_issue<4, 1, NTH>(Ws, b0);
        stage_swizzled_issue<4, 2, NTH>(Ws + 64 * 32, b1);
        stage_swizzled_issue<1, 2, NTH>(Ws + 64 * 32 + 4096, b2);
        stage_swizzled_issue<4, 1, NTH>(Wc, c0);
        stage_swizzled_issue<4, 2, NTH>(Wc + 64 * 32, c1);
        stage_swizzled_issue<4, 2, NTH>(Wc + 64 * 32 + 4096, c2);
        stage_swizzled_issue<1, 2, NTH>(Wc + 64 * 32 + 8192, c3);
        stage_swizzled_store<4, 1, NTH>(img + I::C0, c0);
        stage_swizzled_store<4, 2, NTH>(img + I::C1, c1);
        stage_swizzled_store<4, 2, NTH>(img + I::C2, c2);
        stage_swizzled_store<1, 2, NTH>(img + I::CO, c3);
        stage_swizzled_store<4, 1, NTH>(img + I::S0, b0);
        stage_swizzled_store<4, 2, NTH>(img + I::S1, b1);
        stage_swizzled_store<1, 2, NTH>(img + I::SO, b2);
    }
    const uint32_t n_rows = (ctl.n_rows + 15u) & ~15u;                 // rows the emit kernel wrote (pad rows of the last tile are zeros)
    const __amdgpu_buffer_rsrc_t rs_enc = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(enc), 0, (int)(lm_rows * 64u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dir = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dirs), 0, (int)(n_rows * 12u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_dl = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(fa.deltas), 0, (int)(n_rows * 8u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_eo = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(EDIT ? fa.edit_occ : reinterpret_cast<const uint8_t*>(fa.deltas)), 0, (int)n_rows, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_alive = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(fa.alive), 0, (int)(n_alive * 4u), 0x00020000);
    const uint32_t plane = lm_rows * 4u;
    // the lane of a ray's first row owns the ray
    const uint32_t slot = (uint32_t)lane / n_step;
    const bool own = slot * n_step == (uint32_t)lane && slot < rpg;
    h4 xf_n[NT][2] = {};
    float d_n[3] = {0.f, 0.f, 0.f}, dl_n[2] = {0.f, 0.f};
    uint32_t eo_n = 0, idx_n = 0;
    auto request = [&](uint32_t grp) {
        const uint32_t row0 = grp * 64u;
        const uint32_t vo = ((uint32_t)(2 * g) * lm_rows + row0 + (uint32_t)c) * 4u;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int kt = 0; kt < 2; kt++) {
                const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(rs_enc, (int)(vo + t * 64u), (int)((8u * kt) * plane), 0);
                const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(rs_enc, (int)(vo + t * 64u), (int)((8u * kt + 1u) * plane), 0);
                xf_n[t][kt] = __builtin_bit_cast(h4, uint2{lo, hi});
            }
        const uint32_t r = row0 + (uint32_t)lane;
#pragma unroll
        for (int k = 0; k < 3; k++) d_n[k] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_dir, (int)(r * 12u + 4u * k), 0, 0));
#pragma unroll
        for (int k = 0; k < 2; k++) dl_n[k] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_dl, (int)(r * 8u + 4u * k), 0, 0));
        if (EDIT) eo_n = (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs_eo, (int)r, 0, 0);
        idx_n = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_alive, (int)((grp * rpg + slot) * 4u), 0, 0);   // 0 past the list
    };
    if (g_lo < g_hi) request(g_lo);
    __syncthreads();                                                     // the image is complete
    for (uint32_t grp = g_lo; grp < g_hi; grp++) {
        h4 xf[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++) { xf[t][0] = xf_n[t][0]; xf[t][1] = xf_n[t][1]; }
        const float dx = d_n[0], dy = d_n[1], dz = d_n[2], d0 = dl_n[0], d1 = dl_n[1];
        const uint32_t eo = eo_n, idx = idx_n;
        if (grp + 1 < g_hi) request(grp + 1);
        const bool valid = own && grp * rpg + slot < n_alive;
        // the ray's accumulators: requested now, needed after the two networks
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        lae::RayAcc* ap = fa.acc + idx;
        if (valid) { a0 = reinterpret_cast<const float4*>(ap)[0]; a1 = reinterpret_cast<const float4*>(ap)[1]; }
        {
            float o[16], gx[1], gy[1], gz[1];
            sh_eval<4, false>(dx, dy, dz, o, gx, gy, gz);
            h8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; j++) { lo[j] = (half_t)o[j]; hi[j] = (half_t)o[8 + j]; }
            *reinterpret_cast<h8*>(&sc->sh[lane][0]) = lo;
            *reinterpret_cast<h8*>(&sc->sh[lane][8]) = hi;
        }
        h4 a0h[NT][4], a1h[NT][4];
        layer64s<1, NT>(img + I::S0, lane, xf, a0h);
        layer64s<2, NT>(img + I::S1, lane, a0h, a1h);
        f4 so[NT];
        out16s<NT>(img + I::SO, lane, a1h, so);
        h4 hq[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int r = 0; r < 4; r++) hq[t][r] = (half_t)so[t][r];
            if (g == 0) sc->q[t * 16 + c][0] = (float)hq[t][0];
        }
        wave_lds_fence();
        const float sig = density_scale * expf(sc->q[lane][0]);          // trunc_exp forward (activation.py:9), renderer.py:370
        h4 cin[NT][2];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            cin[t][0] = *reinterpret_cast<const h4*>(&sc->sh[t * 16 + c][4 * g]);
            const half_t nxt = __builtin_bit_cast(half_t, (uint16_t)__shfl_down((int)__builtin_bit_cast(uint16_t, hq[t][0]), 16, 64));
            cin[t][1][0] = hq[t][1]; cin[t][1][1] = hq[t][2]; cin[t][1][2] = hq[t][3];
            cin[t][1][3] = g == 3 ? (half_t)0.0f : nxt;
        }
        layer64s<1, NT>(img + I::C0, lane, cin, a0h);
        layer64s<2, NT>(img + I::C1, lane, a0h, a1h);
        layer64s<2, NT>(img + I::C2, lane, a1h, a0h);
        f4 co[NT];
        out16s<NT>(img + I::CO, lane, a0h, co);
        wave_lds_fence();
#pragma unroll
        for (int t = 0; t < NT; t++)
            if (g == 0) *reinterpret_cast<f4*>(&sc->q[t * 16 + c][0]) = co[t];
        wave_lds_fence();
        {
            const f4 v = *reinterpret_cast<const f4*>(&sc->q[lane][0]);
            const float cr = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[0])));
            const float cg = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[1])));
            const float cb = (float)(half_t)(1.0f / (1.0f + expf(-(float)(half_t)v[2])));
            wave_lds_fence();                                            // every lane has read its logits
            *reinterpret_cast<f4*>(&sc->q[lane][0]) = f4{sig, cr, cg, cb};
            fs->dl[lane][0] = d0; fs->dl[lane][1] = d1;
            if (EDIT) fs->eo[lane] = eo;
        }
        wave_lds_fence();
        // ---- composite_rays of the group's rays (raymarching.cu:948-1035; k_frame_composite of round 1-3, same statements)
        bool keep = false;
        if (valid) {
            lae::RayAcc a{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            uint32_t step = 0;
            while (step < n_step) {
                const float e0 = fs->dl[lane + step][0];
                if (e0 == 0) break;
                const f4 v = *reinterpret_cast<const f4*>(&sc->q[lane + step][0]);         // sigma, rgb
                if (lae::composite_infer_sample<EDIT>(a, v[0], e0, fs->dl[lane + step][1], v[1], v[2], v[3],
                                                      EDIT && fs->eo[lane + step], fa.T_thresh)) break;
                step++;
            }
            keep = step == n_step;
            reinterpret_cast<float4*>(ap)[0] = make_float4(a.ws, a.depth, a.r, a.g);
            reinterpret_cast<float4*>(ap)[1] = make_float4(a.b, keep ? a.t : a1.y, a.wse, a.de);   // rays_t moves only for rays that go on
        }
        const unsigned long long km = __ballot(keep);
        if (keep) seg[kept + (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull))] = (int32_t)idx;
        kept += (uint32_t)__builtin_popcountll(km);
        wave_lds_fence();                                                // scratch is rewritten by the next group
    }
    if (lane == 0) { fa.seg_counts_next[unit] = kept; wave_kept[w] = kept; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int i = 0; i < WAVES; i++) tot += wave_kept[i];
        fa.blk_counts_next[blockIdx.x] = tot;
    }
}

}  // namespace

static uint32_t head_blocks_per_cu() {
    static const int v = lae::env_int("LAE_HEAD_BLOCKS_PER_CU", 1, {1, 2, 3, 4});
    return (uint32_t)v;
}
static int head5_waves() {
    static const int v = lae::env_int("LAE_HEAD5_WAVES", 8, {4, 8, 16});
    return v;
}
template <bool COLOR, int WAVES>
static int launch_head_fwd5_w(const half_t* enc, const float* dirs, const half_t* Ws, const half_t* Wc, uint32_t n_tiles, uint32_t launch_tiles,
                              float density_scale, half_t* h_out, float* sigmas, float* rgbs, int level_major,
                              const uint32_t* n_rows_dev, uint32_t lm_rows, hipStream_t s) {
    const size_t lds_bytes = (size_t)(COLOR ? Head5Img::END : Head5Img::C0) * 2 + (size_t)WAVES * sizeof(Head4Scratch);
    static bool lds_allowed = false;
    if (const int rc = lae::allow_dynamic_lds(lds_allowed, reinterpret_cast<const void*>(&k_nerf_head_fwd5<COLOR, WAVES>), lds_bytes)) return rc;
    const uint32_t n_groups = lae::cdiv(launch_tiles, 4);
    const uint32_t blocks = std::max(1u, std::min(lae::cdiv(n_groups, WAVES), (uint32_t)lae::num_cus() * head_blocks_per_cu()));
    k_nerf_head_fwd5<COLOR, WAVES><<<blocks, 64 * WAVES, lds_bytes, s>>>(enc, dirs, Ws, Wc, n_tiles, density_scale, h_out, sigmas, rgbs,
                                                                        level_major, n_rows_dev, lm_rows);
    return LAE_OK;
}
template <bool COLOR>
static int launch_head_fwd5(const half_t* enc, const float* dirs, const half_t* Ws, const half_t* Wc, uint32_t n_tiles, uint32_t launch_tiles,
                            float density_scale, half_t* h_out, float* sigmas, float* rgbs, int level_major,
                            const uint32_t* n_rows_dev, uint32_t lm_rows, hipStream_t s) {
    switch (head5_waves()) {
        case 4: return launch_head_fwd5_w<COLOR, 4>(enc, dirs, Ws, Wc, n_tiles, launch_tiles, density_scale, h_out, sigmas, rgbs, level_major, n_rows_dev, lm_rows, s);
        case 16: return launch_head_fwd5_w<COLOR, 16>(enc, dirs, Ws, Wc, n_tiles, launch_tiles, density_scale, h_out, sigmas, rgbs, level_major, n_rows_dev, lm_rows, s);
        default: return launch_head_fwd5_w<COLOR, 8>(enc, dirs, Ws, Wc, n_tiles, launch_tiles, density_scale, h_out, sigmas, rgbs, level_major, n_rows_dev, lm_rows, s);
    }
}
// k_nerf_head_fwd5 stages the weights with 16-byte loads and addresses rows through buffer descriptors with 32-bit byte
// offsets (row * 64, lm_rows * 64, row * 12): both are preconditions of every entry point below
static int head_args_ok(const void* ws, const void* wc, uint64_t rows, const char* who) {
    if (((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(wc)) & 15) != 0) {
        lae::set_last_error_str((std::string(who) + ": the weight pointers must be 16-byte aligned").c_str());
        return LAE_EINVAL;
    }
    if (rows * 64ull > 0xffffffffull) {
        lae::set_last_error_str((std::string(who) + ": more than 2^26 - 1 rows per call (32-bit row offsets); split the batch").c_str());
        return LAE_EINVAL;
    }
    return LAE_OK;
}

// frame loop (frame.hip lae_render_frame): level-major features [16, M_cap, 2], loop state in device memory
uint32_t lae::frame_head_max_blocks() { return (uint32_t)lae::num_cus() * head_blocks_per_cu(); }

template <bool EDIT, int WAVES>
static int launch_frame_head(const half_t* enc, const float* dirs, const half_t* Ws, const half_t* Wc, uint32_t lm_rows, uint32_t blocks,
                             float density_scale, const lae::FrameHeadArgs& fa, hipStream_t s) {
    const size_t lds_bytes = (size_t)Head5Img::END * 2 + (size_t)WAVES * (sizeof(Head4Scratch) + sizeof(FrameHeadScratch));
    static bool lds_allowed = false;
    if (const int rc = lae::allow_dynamic_lds(lds_allowed, reinterpret_cast<const void*>(&k_frame_head<EDIT, WAVES>), lds_bytes)) return rc;
    k_frame_head<EDIT, WAVES><<<blocks, 64 * WAVES, lds_bytes, s>>>(enc, dirs, Ws, Wc, density_scale, lm_rows, fa);
    return LAE_OK;
}

int lae::nerf_head_composite_frame(const void* enc, const float* dirs, const void* sigma_weights, const void* color_weights,
                                   uint32_t M_cap, float density_scale, const FrameHeadArgs& fa, bool edit, uint32_t n_blocks,
                                   hipStream_t stream) {
    if (M_cap % 64 != 0 || n_blocks == 0) return LAE_EINVAL;
    if (const int rc = head_args_ok(sigma_weights, color_weights, M_cap, "render_frame(head)")) return rc;
    const half_t *e = (const half_t*)enc, *ws = (const half_t*)sigma_weights, *wc = (const half_t*)color_weights;
    return edit ? launch_frame_head<true, FRAME_HEAD_WAVES>(e, dirs, ws, wc, M_cap, n_blocks, density_scale, fa, stream)
                : launch_frame_head<false, FRAME_HEAD_WAVES>(e, dirs, ws, wc, M_cap, n_blocks, density_scale, fa, stream);
}

extern "C" {

int lae_nerf_head_forward(const void* enc, const float* dirs, const void* sigma_weights, const void* color_weights,
                          uint32_t M, float density_scale, void* h_out, float* sigmas, float* rgbs, int enc_level_major,
                          void* stream) {
    if (M == 0) return LAE_OK;
    if (!enc || !dirs || !sigma_weights || !color_weights || !h_out || !sigmas || !rgbs) return LAE_ENULL;
    if (M % 16 != 0) return LAE_EINVAL;
    if (const int rc = head_args_ok(sigma_weights, color_weights, M, "nerf_head_forward")) return rc;
    const int rc = launch_head_fwd5<true>((const half_t*)enc, dirs, (const half_t*)sigma_weights, (const half_t*)color_weights, M / 16, M / 16,
                                          density_scale, (half_t*)h_out, sigmas, rgbs, enc_level_major, nullptr, M,
                                          reinterpret_cast<hipStream_t>(stream));
    return rc != LAE_OK ? rc : lae::check_launch("nerf_head_forward");
}

int lae_nerf_density_forward(const void* enc, const void* sigma_weights, uint32_t M, float density_scale, void* h_out,
                             float* sigmas, int enc_level_major, void* stream) {
    if (M == 0) return LAE_OK;
    if (!enc || !sigma_weights || !sigmas) return LAE_ENULL;
    if (M % 16 != 0) return LAE_EINVAL;
    if (const int rc = head_args_ok(sigma_weights, sigma_weights, M, "nerf_density_forward")) return rc;
    const int rc = launch_head_fwd5<false>((const half_t*)enc, nullptr, (const half_t*)sigma_weights, nullptr, M / 16, M / 16, density_scale,
                                           (half_t*)h_out, sigmas, nullptr, enc_level_major, nullptr, M, reinterpret_cast<hipStream_t>(stream));
    return rc != LAE_OK ? rc : lae::check_launch("nerf_density_forward");
}

}  // extern "C"
