// mlpbackward.hip -- the fused recompute backward of the 64-wide ReLU MLPs: the FFMLP operator's fused path
// (lae::ffmlp_backward_fused, called by lae_ffmlp_backward_ex in ffmlp.hip) and the fused NeRF head's backward
// (lae::nerf_head_backward / lae_nerf_head_backward).  Weight layout and MFMA mapping: head of ffmlp.hip; fragment helpers:
// mlp_frags.h.  Two kernels do the same mathematics, k_mlp_bwd_wave (ships) and k_mlp_bwd_coop (its A/B predecessor); the steps
// they share are written once, ahead of them.
#include <algorithm>
#include <type_traits>
#include "lae_common.h"
#include "dw_reduce.h"
#include "mlp_frags.h"

namespace {

using lae_dw::DWR_GROUPS;
using lae_dw::LossFinish;

// colour-net input fragments of a tile: k-step 0 = SH components 4g..4g+3 of the row's direction,
// k-step 1 = features 16 + 4g + j = h[1 + 4g + j] (h = fp16 sigma-net output in C/D layout), feature 31 = 0
__device__ __forceinline__ void color_inputs(float dx, float dy, float dz, const h4& hq, int g, h4 (&cin)[2]);
__device__ __forceinline__ void color_inputs(const float* __restrict__ dirs, size_t row, const h4& hq, int g, h4 (&cin)[2]) {
    color_inputs(dirs[3 * row], dirs[3 * row + 1], dirs[3 * row + 2], hq, g, cin);
}
__device__ __forceinline__ void color_inputs(float dx, float dy, float dz, const h4& hq, int g, h4 (&cin)[2]) {
    float o[16], gx[1], gy[1], gz[1];
    sh_eval<4, false>(dx, dy, dz, o, gx, gy, gz);
    // the lane keeps components 4g .. 4g + 3.  Every lane evaluates all 16 (~40 instructions) and picks with bit masks:
    // written as `g == 0 ? o[j] : g == 1 ? ...` the compiler sinks the polynomials into four divergent branches, which a
    // wave (all four g groups) then runs one after the other -- ~190 of the ~600 instructions per 16-row tile
    const uint32_t m0 = g == 0 ? 0xffffffffu : 0u, m1 = g == 1 ? 0xffffffffu : 0u, m2 = g == 2 ? 0xffffffffu : 0u,
                   m3 = g == 3 ? 0xffffffffu : 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t bits = (__builtin_bit_cast(uint32_t, o[j]) & m0) | (__builtin_bit_cast(uint32_t, o[4 + j]) & m1) |
                              (__builtin_bit_cast(uint32_t, o[8 + j]) & m2) | (__builtin_bit_cast(uint32_t, o[12 + j]) & m3);
        cin[0][j] = (half_t)__builtin_bit_cast(float, bits);
    }
    const half_t nxt = __builtin_bit_cast(half_t, (uint16_t)__shfl_down((int)__builtin_bit_cast(uint16_t, hq[0]), 16, 64));
    cin[1][0] = hq[1]; cin[1][1] = hq[2]; cin[1][2] = hq[3];
    cin[1][3] = g == 3 ? (half_t)0.0f : nxt;
}

// ---------------------------------------------------------------- fused backward (WIDTH = 64, ReLU)
// One kernel for everything the reference does in kernel_mlp_fused_backward + (num_layers+1) split-K CUTLASS
// GEMMs (ffmlp.cu:410-518, 800-877), WITHOUT the forward/backward buffers: the hidden activations are
// recomputed from the 64-byte input row (cheap on the matrix cores; the buffers cost ~3.5 KB/sample of HBM
// traffic), dL/dH is chained through the layers in registers exactly like k_mlp_bwd, and every wave accumulates
// its own dW = dY^T A for all weight tiles over its 16-row tiles:
//   * the dY / A tiles are written row-major into a WAVE-PRIVATE LDS region with ds_write_b64 straight from the
//     MFMA C/D layout and read back transposed with ds_read_b64_tr_b16 -- that IS the A / B operand layout for a
//     product that sums over the batch (lane) index; no barrier, waves never share tiles;
//   * weights live row-major in LDS (padded rows): forward fragments are plain ds_read_b64, the transposed
//     fragments of the backward chain are ds_read_b64_tr_b16 of the same image;
//   * the 4 waves' dW accumulators are summed through LDS once at the end (fixed order) and stored as one fp32
//     slab per workgroup; k_dw_reduce adds the slabs in order -> deterministic gradients.
typedef __fp16 hraw4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ h4 lds_tr_read(const half_t* p) {
    const hraw4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hraw4*)(p));
    return __builtin_bit_cast(h4, r);
}

// B fragments of a 32-wide encoder row.  Row-major [M,32]: features 16kt + 4g .. +3 are one 8-byte load.  Level-major
// [16][M][2] (the grid kernels' native layout): the same four features are the channel pairs of levels 8kt + 2g and
// 8kt + 2g + 1 -- two 4-byte loads, 64 contiguous bytes per level for the 16 rows of a tile.
__device__ __forceinline__ void load_enc_frags(const half_t* __restrict__ enc, size_t row, size_t M, int g, int level_major, h4 (&xf)[2]) {
#pragma unroll
    for (int kt = 0; kt < 2; kt++) {
        if (level_major) {
            const uint32_t lo = *reinterpret_cast<const uint32_t*>(enc + ((size_t)(8 * kt + 2 * g) * M + row) * 2);
            const uint32_t hi = *reinterpret_cast<const uint32_t*>(enc + ((size_t)(8 * kt + 2 * g + 1) * M + row) * 2);
            const uint2 v{lo, hi};
            xf[kt] = __builtin_bit_cast(h4, v);
        } else {
            xf[kt] = *reinterpret_cast<const h4*>(enc + row * 32 + kt * 16 + 4 * g);
        }
    }
}

// MODE 1 = colour net of the fused NeRF head: the input rows are built on the fly from (h, dirs) exactly like
// k_nerf_head_fwd, dL/dout comes from (grad_rgb, rgb) through the sigmoid, and instead of dL/dX the kernel writes
// dL/dh [M,16] = [ grad_sigma * density_scale * exp(clamp(h0, -15, 15)) | dX[16..30] ] (trunc_exp backward,
// activation.py:14-17, and the inverse of the one-feature shift) -- the sigma net's backward reads that directly.
struct HeadBwdArgs {
    const float* dirs; const float* rgbs; const float* grad_rgbs; const float* grad_sigmas; float density_scale;
    int level_major;        // MODE 0, IN = 32: x and grad_in are [16][B][2] (the grid kernels' layout) instead of [B,32]
};

// ---------------------------------------------------------------- steps both backward kernels take (lane = (c, g), row = tile * 16 + c)
// MODE 0 inputs of a row: the B fragments of x and the dL/dout fragment.  Bn = rows of the batch (level-major stride).
template <int IN>
__device__ __forceinline__ void load_inputs(const half_t* __restrict__ x, const half_t* __restrict__ grad, size_t row, size_t Bn, int g,
                                            int level_major, h4 (&xf)[IN / 16], h4& gf) {
    if constexpr (IN == 32) load_enc_frags(x, row, Bn, g, level_major, xf);
    else {
#pragma unroll
        for (int kt = 0; kt < IN / 16; kt++) xf[kt] = *reinterpret_cast<const h4*>(x + row * IN + kt * 16 + 4 * g);
    }
    gf = *reinterpret_cast<const h4*>(grad + row * 16 + 4 * g);
}
// MODE 1 upstream gradient: dL/dlogit of one colour channel from dL/drgb and rgb = sigmoid(logit)
__device__ __forceinline__ half_t rgb_logit_grad(float grad_rgb, float y) { return (half_t)(grad_rgb * y * (1.0f - y)); }
// MODE 1 dL/dh fragment of a row from acc = dX features 16 + 4g .. 16 + 4g + 3: the inverse of the one-feature shift of
// color_inputs (h[4g] comes from lane group g - 1), and in lane group 0 the trunc_exp backward of the density logit h[0]
__device__ __forceinline__ h4 head_grad_h(const f4& acc, const float* grad_sigma, float density_scale, half_t h0, int g) {
    const half_t v3 = (half_t)acc[3];
    const half_t prev = __builtin_bit_cast(half_t, (uint16_t)__shfl_up((int)__builtin_bit_cast(uint16_t, v3), 16, 64));
    h4 v;
    v[0] = prev;
    if (g == 0) v[0] = (half_t)(*grad_sigma * density_scale * expf(lae::clampf((float)h0, -15.0f, 15.0f)));
    v[1] = (half_t)acc[0]; v[2] = (half_t)acc[1]; v[3] = (half_t)acc[2];
    return v;
}
// MODE 0 dX store: features 16 it + 4g .. + 3 of a row, row-major [Bn, IN] or (IN = 32) level-major [16][Bn][2]
template <int IN>
__device__ __forceinline__ void store_dx(half_t* __restrict__ grad_in, size_t row, size_t Bn, int it, int g, int level_major, const h4& v) {
    if (IN == 32 && level_major) {
        const uint2 u = __builtin_bit_cast(uint2, v);
        *reinterpret_cast<uint32_t*>(grad_in + ((size_t)(8 * it + 2 * g) * Bn + row) * 2) = u.x;
        *reinterpret_cast<uint32_t*>(grad_in + ((size_t)(8 * it + 2 * g + 1) * Bn + row) * 2) = u.y;
    } else
        *reinterpret_cast<h4*>(grad_in + row * IN + it * 16 + 4 * g) = v;
}
// where a 16 x 16 dW tile lives in the slab, which has the weights' layout: tile (mt, nt) of matrix mat, 0 = W0 [64, IN],
// 1 .. NH = hidden [64, 64], NH + 1 = Wout [16, 64] (mt = 0) -> offset of its element [0][0] and the row stride
struct DwSlot { size_t base; uint32_t ld; };
template <int IN>
__device__ __forceinline__ DwSlot dw_slot(uint32_t mat, uint32_t mt, uint32_t nt) {
    if (mat == 0) return {(size_t)(mt * 16) * IN + nt * 16, IN};
    return {(size_t)64 * IN + (size_t)(mat - 1) * 4096 + (size_t)(mt * 16) * 64 + nt * 16, 64};
}
// a dW tile in the C/D layout (lane (c, g), reg r = element [4g + r][c]) -> its slot
__device__ __forceinline__ void store_dw_tile(float* __restrict__ slab, const DwSlot& s, int c, int g, const f4& v) {
#pragma unroll
    for (int r = 0; r < 4; r++) slab[s.base + (size_t)(4 * g + r) * s.ld + c] = v[r];
}

// ---------------------------------------------------------------- fused backward, workgroup-cooperative dW
// Same mathematics as k_mlp_bwd_fused, different ownership of the weight-gradient tiles.  There every wave accumulates
// ALL dW tiles of the net over its own rows (176 accumulator registers for the colour net -> 2 waves/SIMD with spills,
// and a cross-wave reduction at the end).  Here a workgroup of WAVES waves shares one [16*WAVES rows] tile of X, H, D, G
// in LDS: each wave still runs the forward recompute and the dL/dH chain for its own 16 rows in registers, but after a
// barrier the dW tiles are DIVIDED among the waves, each contracted over all 16*WAVES rows with K = 32 MFMAs.  Per wave
// that is 6 accumulator tiles instead of 44, half as many dW MFMAs, no final reduction, and 4 waves/SIMD.
template <int IN, int NH, int WAVES>
struct CoopCfg {
    static constexpr int KT0 = IN / 16;
    static constexpr int R = 16 * WAVES;                   // rows per workgroup iteration
    static constexpr int LDX = IN + 8, LDH = 72, LDG = 24;
    static constexpr int W0_OFF = 0;
    static constexpr int WH_OFF = 64 * LDX;
    static constexpr int WO_OFF = WH_OFF + NH * 64 * LDH;
    static constexpr int W_HALVES = WO_OFF + 16 * LDH;
    static constexpr int X_OFF = W_HALVES;
    static constexpr int H_OFF = X_OFF + R * LDX;
    static constexpr int D_OFF = H_OFF + R * LDH;
    static constexpr int G_OFF = D_OFF + R * LDH;
    static constexpr int LDS_HALVES = G_OFF + R * LDG;
    static constexpr int TH = 16 / WAVES > 0 ? 16 / WAVES : 1;                      // hidden-layer dW tiles per wave
    static constexpr int T0 = (4 * KT0 + WAVES - 1) / WAVES;                        // input-layer dW tiles per wave
};

template <int IN, int NH, int MODE, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_mlp_bwd_coop(
    const half_t* __restrict__ grad, const half_t* __restrict__ x, const half_t* __restrict__ W, uint32_t n_tiles,
    half_t* __restrict__ grad_in, float* __restrict__ slabs, uint32_t nW, HeadBwdArgs ha) {
    using C = CoopCfg<IN, NH, WAVES>;
    constexpr int KT0 = C::KT0, R = C::R;
    static_assert(16 % WAVES == 0 && WAVES >= 4, "dW tiles are dealt round-robin to 4, 8 or 16 waves");
    extern __shared__ __attribute__((aligned(16))) half_t lds[];
    half_t* Wl = lds;
    half_t* Xs = lds + C::X_OFF; half_t* Hs = lds + C::H_OFF; half_t* Ds = lds + C::D_OFF; half_t* Gs = lds + C::G_OFF;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    // wave index as a SCALAR: the per-wave branches below (`w < 4`, `t < 4 * KT0`) must be uniform branches.  As a vector
    // value they compile to EXEC-masked regions; with IN = 48 (the only shape where waves 4-7 skip a dW0 tile) one 16-row
    // tile of dX / dW came out wrong in ~25 % of the launches (tests/test_gpu_ffmlp.py [1152-48-64-2]).
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tq = (lane & 15) >> 2, tp = lane & 3;
    const int r0 = 16 * w;                                   // this wave's rows inside the shared tiles
    const size_t Bn = (size_t)n_tiles * 16;

    stage_rows<64 * WAVES>(Wl + C::W0_OFF, C::LDX, W, 64, IN);
    stage_rows<64 * WAVES>(Wl + C::WH_OFF, C::LDH, W + 64 * IN, NH * 64, 64);                   // the hidden matrices are one [NH * 64, 64] image
    stage_rows<64 * WAVES>(Wl + C::WO_OFF, C::LDH, W + 64 * IN + (size_t)NH * 4096, 16, 64);

    f4 aO = f4{0, 0, 0, 0};
    f4 aH[NH][C::TH], a0[C::T0];
#pragma unroll
    for (int m = 0; m < NH; m++)
#pragma unroll
        for (int i = 0; i < C::TH; i++) aH[m][i] = f4{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < C::T0; i++) a0[i] = f4{0, 0, 0, 0};

    // dW tile (mt, nt) += A^T B over the R shared rows: A block mt of tile `At` (ld lda), B block nt of tile `Bt` (ld ldb)
    auto dw_tile = [&](const half_t* At, int lda, int mt, const half_t* Bt, int ldb, int nt, f4 acc) {
#pragma unroll
        for (int ks = 0; ks < R / 32; ks++) {
            const half_t* ar = At + (32 * ks + 4 * g + tq) * lda + mt * 16 + 4 * tp;
            const half_t* br = Bt + (32 * ks + 4 * g + tq) * ldb + nt * 16 + 4 * tp;
            acc = mfma32(lds_tr_read(ar), lds_tr_read(ar + 16 * lda), lds_tr_read(br), lds_tr_read(br + 16 * ldb), acc);
        }
        return acc;
    };

    const uint32_t n_groups = (n_tiles + WAVES - 1) / WAVES;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint32_t tile = grp * WAVES + w;
        const bool active = tile < n_tiles;
        const size_t row = (size_t)(active ? tile : 0) * 16 + c;
        const h4 zero4 = h4{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f};
        // ---- inputs of this wave's 16 rows
        h4 xf[KT0];
        h4 gf = zero4, hq = zero4;
        if constexpr (MODE == 1) {
            hq = *reinterpret_cast<const h4*>(x + row * 16 + 4 * g);
            color_inputs(ha.dirs, row, hq, g, xf);
            if (g == 0) {
#pragma unroll
                for (int r = 0; r < 3; r++) gf[r] = rgb_logit_grad(ha.grad_rgbs[row * 3 + r], ha.rgbs[row * 3 + r]);
            }
        } else {
            load_inputs<IN>(x, grad, row, Bn, g, ha.level_major, xf, gf);
        }
        if (!active) {                                       // rows past the batch contribute nothing
#pragma unroll
            for (int kt = 0; kt < KT0; kt++) xf[kt] = zero4;
            gf = zero4;
        }
        __syncthreads();                                     // S0: readers of X / G / H / D of the previous group are done
#pragma unroll
        for (int kt = 0; kt < KT0; kt++) *reinterpret_cast<h4*>(Xs + (r0 + c) * C::LDX + kt * 16 + 4 * g) = xf[kt];
        *reinterpret_cast<h4*>(Gs + (r0 + c) * C::LDG + 4 * g) = gf;
        // ---- recompute the hidden activations of the own rows (registers)
        h4 h[NH + 1][4];
        {
            f4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
                acc[mt] = mfma_ksteps<KT0>([&](int kt) { return *reinterpret_cast<const h4*>(Wl + C::W0_OFF + (mt * 16 + c) * C::LDX + kt * 16 + 4 * g); },
                                           xf, f4{0, 0, 0, 0});
            relu4(acc, h[0]);
#pragma unroll
            for (int l = 0; l < NH; l++) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
                    acc[mt] = mfma_ksteps<4>([&](int kt) { return *reinterpret_cast<const h4*>(Wl + C::WH_OFF + (l * 64 + mt * 16 + c) * C::LDH + kt * 16 + 4 * g); },
                                             h[l], f4{0, 0, 0, 0});
                relu4(acc, h[l + 1]);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++) *reinterpret_cast<h4*>(Hs + (r0 + c) * C::LDH + mt * 16 + 4 * g) = h[NH][mt];
        __syncthreads();                                     // S1: G and H_NH of all rows are in LDS
        // ---- output layer: dWout tile nt = w (waves 0..3) ; own rows: dH_NH = (Wout^T G) * relu'
        if (w < 4) aO = dw_tile(Gs, C::LDG, 0, Hs, C::LDH, w, aO);
        h4 d[4];
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const h4 a = lds_tr_read(Wl + C::WO_OFF + (4 * g + tq) * C::LDH + mt * 16 + 4 * tp);             // A[f][o] = Wout[o][f]
            const f4 acc = mfma16(a, gf, f4{0, 0, 0, 0});
#pragma unroll
            for (int r = 0; r < 4; r++) d[mt][r] = ((float)h[NH][mt][r] > 0.0f) ? (half_t)acc[r] : (half_t)0.0f;
        }
        // ---- hidden layers, last to first
#pragma unroll
        for (int l = NH; l >= 1; l--) {
            __syncthreads();                                 // S2: readers of H and D are done
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                *reinterpret_cast<h4*>(Ds + (r0 + c) * C::LDH + mt * 16 + 4 * g) = d[mt];
                *reinterpret_cast<h4*>(Hs + (r0 + c) * C::LDH + mt * 16 + 4 * g) = h[l - 1][mt];
            }
            __syncthreads();                                 // S3: D_l and H_{l-1} of all rows are in LDS
#pragma unroll
            for (int i = 0; i < C::TH; i++) {
                const int t = w + i * WAVES;                 // tile (mt, nt) = (t / 4, t % 4)
                aH[l - 1][i] = dw_tile(Ds, C::LDH, t / 4, Hs, C::LDH, t % 4, aH[l - 1][i]);
            }
            h4 dn[4];
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                const f4 acc = mfma_ksteps<4>([&](int kt) { return lds_tr_read(Wl + C::WH_OFF + ((l - 1) * 64 + kt * 16 + 4 * g + tq) * C::LDH + mt * 16 + 4 * tp); },   // W_l^T
                                              d, f4{0, 0, 0, 0});
#pragma unroll
                for (int r = 0; r < 4; r++) dn[mt][r] = ((float)h[l - 1][mt][r] > 0.0f) ? (half_t)acc[r] : (half_t)0.0f;
            }
#pragma unroll
            for (int mt = 0; mt < 4; mt++) d[mt] = dn[mt];
        }
        // ---- input layer: dW0 tiles dealt to the waves ; own rows: dX = W0^T dH_0
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 4; mt++) *reinterpret_cast<h4*>(Ds + (r0 + c) * C::LDH + mt * 16 + 4 * g) = d[mt];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C::T0; i++) {
            const int t = w + i * WAVES;                     // tile (mt, nt) = (t / KT0, t % KT0)
            if (t < 4 * KT0) a0[i] = dw_tile(Ds, C::LDH, t / KT0, Xs, C::LDX, t % KT0, a0[i]);
        }
        if constexpr (MODE == 1) {
            const f4 acc = mfma_ksteps<4>([&](int kt) { return lds_tr_read(Wl + C::W0_OFF + (kt * 16 + 4 * g + tq) * C::LDX + 16 + 4 * tp); },   // W0^T, features 16..31
                                          d, f4{0, 0, 0, 0});
            const h4 v = head_grad_h(acc, ha.grad_sigmas + row, ha.density_scale, hq[0], g);
            if (active) *reinterpret_cast<h4*>(grad_in + row * 16 + 4 * g) = v;
        } else if (grad_in) {
#pragma unroll
            for (int it = 0; it < KT0; it++) {
                const f4 acc = mfma_ksteps<4>([&](int kt) { return lds_tr_read(Wl + C::W0_OFF + (kt * 16 + 4 * g + tq) * C::LDX + it * 16 + 4 * tp); },   // W0^T
                                              d, f4{0, 0, 0, 0});
                h4 v;
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = (half_t)acc[r];
                if (active) store_dx<IN>(grad_in, row, Bn, it, g, ha.level_major, v);
            }
        }
    }

    // ---- every wave owns its tiles: straight to this workgroup's slab
    float* slab = slabs + (size_t)blockIdx.x * nW;
#pragma unroll
    for (int i = 0; i < C::T0; i++) {
        const int t = w + i * WAVES;
        if (t < 4 * KT0) store_dw_tile(slab, dw_slot<IN>(0, t / KT0, t % KT0), c, g, a0[i]);
    }
#pragma unroll
    for (int m = 0; m < NH; m++)
#pragma unroll
        for (int i = 0; i < C::TH; i++) {
            const int t = w + i * WAVES;
            store_dw_tile(slab, dw_slot<IN>(1 + m, t / 4, t % 4), c, g, aH[m][i]);
        }
    if (w < 4) store_dw_tile(slab, dw_slot<IN>(NH + 1, 0, w), c, g, aO);
}

// ---------------------------------------------------------------- fused backward, round-3 form: no activation ever touches LDS
// k_mlp_bwd_coop shares X / H / D / G tiles of 128 rows among 8 waves: 7 workgroup barriers per 128 rows and every
// activation written row-major to LDS and read back transposed (66 % of its wave cycles parked at waitcnt / barrier, 10 % of
// the MFMA rate).  What the weight gradient needs is the TRANSPOSE of tiles that the chain already holds in registers:
//   chain layout (C/D of W x act^T):  lane (c, g) holds feats 4g .. 4g+3 of batch row c
//   dW operand layout              :  lane (c, g) holds batch rows 4g .. 4g+3 of feature c     (A = D^T and B = H of dW = D^T H)
// and a 16 x 16 transpose IS one MFMA: with the chain-layout registers as the A operand and the identity as B,
// C[m][n] = sum_k A[m][k] I[k][n] = A[m][n] comes out in the C/D layout = lane (n = feature, rows 4g..) -- exact (products
// with 0 / 1, fp32 accumulate, values are halves).  So a wave keeps its own two 16-row tiles in registers through recompute,
// dL/dH chain and transposes, accumulates ALL dW tiles of the net itself with K = 32 MFMAs over the 32 rows (tile A rows in
// the low k-slots, tile B rows in the high ones, the same permutation in both operands), and never synchronises with another
// wave until the final fixed-order reduction of the four waves' dW through LDS.  Only the weights are read from LDS.
// MFMAs per 16 rows (colour net): recompute 20, chain 22, transposes 27, dW 22 = 91 (coop: 66) -- the matrix pipe was never
// the limit.
template <int IN, int NH>
struct WaveCfg {
    static constexpr int KT0 = IN / 16;
    static constexpr int LDX = IN + 8, LDH = 72;
    static constexpr int W0_OFF = 0, WH_OFF = 64 * LDX, WO_OFF = WH_OFF + NH * 64 * LDH, W_HALVES = WO_OFF + 16 * LDH;
    static constexpr int N_TILES = 4 * KT0 + NH * 16 + 4;                 // 16x16 dW tiles: W0 | hidden | Wout
    static constexpr size_t LDS_BYTES = (size_t)W_HALVES * 2 + (size_t)N_TILES * 2048;      // weight image + two dW images (final reduction)
};

// dL/dH of a ReLU layer: acc where the (post-ReLU, hence >= +0) activation is positive, else 0; packed halves.  -h as int16
// is negative exactly when h > 0; its sign bit smeared over the half is the mask.  (Written with vector types the compiler
// turns this back into four compares and selects per pair.)
__device__ __forceinline__ h4 relu_bwd4(const f4& acc, const h4& h) {
    h2 lo = {(half_t)acc[0], (half_t)acc[1]}, hi = {(half_t)acc[2], (half_t)acc[3]};
    const uint2 hb = __builtin_bit_cast(uint2, h);
    uint32_t d0 = __builtin_bit_cast(uint32_t, lo), d1 = __builtin_bit_cast(uint32_t, hi), m0, m1;
    const uint32_t fifteen = 0x000f000fu;
    asm("v_pk_sub_i16 %0, 0, %1\n\tv_pk_ashrrev_i16 %0, %2, %0" : "=&v"(m0) : "v"(hb.x), "v"(fifteen));
    asm("v_pk_sub_i16 %0, 0, %1\n\tv_pk_ashrrev_i16 %0, %2, %0" : "=&v"(m1) : "v"(hb.y), "v"(fifteen));
    d0 &= m0; d1 &= m1;
    return __builtin_bit_cast(h4, uint2{d0, d1});
}

// four 16 x 16 transposes at once: the MFMAs first, the conversions after (a conversion right behind its MFMA waits for it)
template <int N>
__device__ __forceinline__ void mfma_transpose_n(const h4 (&x)[N], const h4& ident, h4 (&o)[N]) {
    f4 r[N];
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = mfma16(x[i], ident, f4{0, 0, 0, 0});
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) o[i][j] = (half_t)r[i][j];
}

// WPE = waves per SIMD the kernel is compiled for: 1 (up to 512 registers: the colour net's 176 accumulator registers + two tiles
// of working state) or 2 (256 registers: nets with one hidden GEMM; the inputs are then not requested ahead -- the partner wave
// covers the latency -- which frees the registers of the second request)
template <int IN, int NH, int MODE, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_mlp_bwd_wave(
    const half_t* __restrict__ grad, const half_t* __restrict__ x, const half_t* __restrict__ W, uint32_t n_tiles,
    half_t* __restrict__ grad_in, float* __restrict__ slabs, uint32_t nW, HeadBwdArgs ha) {
    using C = WaveCfg<IN, NH>;
    constexpr int KT0 = C::KT0;
    extern __shared__ __attribute__((aligned(16))) half_t lds[];
    half_t* Wl = lds;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tq = (lane & 15) >> 2, tp = lane & 3;           // transposed-read lane address (ds_read_tr16_b64)
    const h4 zero4 = h4{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f};
    MLP_STAMP(blockIdx.x * 4 + w, 0);

    const uint32_t n_pairs = (n_tiles + 1) / 2;
    const uint32_t wave0 = blockIdx.x * 4 + (uint32_t)w, nwaves = gridDim.x * 4;
    const size_t Bn = (size_t)n_tiles * 16;
    // ---- inputs, requested one pair ahead (one wave per SIMD: nothing else hides a memory latency per pair)
    struct Req { h4 xf[2][KT0]; h4 gf[2]; h4 hq[2]; float dir[2][3], y[2][3], gy[2][3], gs[2]; };
    constexpr bool AHEAD = WPE == 1;
    Req nx = {};                                                         // (copied whole below: no member may be indeterminate)
    auto request = [&](uint32_t pair) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint32_t tile = min(2 * pair + t, n_tiles - 1);          // a tile past the batch re-reads the last one; its operands are zeroed below
            const size_t row = (size_t)tile * 16 + c;
            if constexpr (MODE == 1) {
                nx.hq[t] = *reinterpret_cast<const h4*>(x + row * 16 + 4 * g);
#pragma unroll
                for (int r = 0; r < 3; r++) nx.dir[t][r] = ha.dirs[3 * row + r];
                if (g == 0) {
#pragma unroll
                    for (int r = 0; r < 3; r++) { nx.y[t][r] = ha.rgbs[row * 3 + r]; nx.gy[t][r] = ha.grad_rgbs[row * 3 + r]; }
                    nx.gs[t] = ha.grad_sigmas[row];
                }
            } else {
                load_inputs<IN>(x, grad, row, Bn, g, ha.level_major, nx.xf[t], nx.gf[t]);
            }
        }
    };
    if (AHEAD && wave0 < n_pairs) request(wave0);

    // ---- weights -> LDS (row-major, padded): every 16-byte global load of the workgroup in flight before the first store
    {
        constexpr int CH0 = 64 * IN / 8, CHH = NH * 64 * 64 / 8, CHO = 16 * 64 / 8;
        constexpr int N0 = (CH0 + 255) / 256, N1 = (CHH + 255) / 256, N2 = (CHO + 255) / 256;
        uint4 b0[N0], b1[N1], b2[N2];
#pragma unroll
        for (int i = 0; i < N0; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CH0) b0[i] = *reinterpret_cast<const uint4*>(W + (size_t)e * 8); }
#pragma unroll
        for (int i = 0; i < N1; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CHH) b1[i] = *reinterpret_cast<const uint4*>(W + 64 * IN + (size_t)e * 8); }
#pragma unroll
        for (int i = 0; i < N2; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CHO) b2[i] = *reinterpret_cast<const uint4*>(W + 64 * IN + NH * 4096 + (size_t)e * 8); }
#pragma unroll
        for (int i = 0; i < N0; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CH0) { const int r = (e * 8) / IN, k = (e * 8) % IN; *reinterpret_cast<uint4*>(Wl + C::W0_OFF + r * C::LDX + k) = b0[i]; } }
#pragma unroll
        for (int i = 0; i < N1; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CHH) { const int r = (e * 8) / 64, k = (e * 8) % 64; *reinterpret_cast<uint4*>(Wl + C::WH_OFF + r * C::LDH + k) = b1[i]; } }
#pragma unroll
        for (int i = 0; i < N2; i++) { const int e = (int)threadIdx.x + 256 * i; if (e < CHO) { const int r = (e * 8) / 64, k = (e * 8) % 64; *reinterpret_cast<uint4*>(Wl + C::WO_OFF + r * C::LDH + k) = b2[i]; } }
    }
    __syncthreads();

    h4 ident;
#pragma unroll
    for (int j = 0; j < 4; j++) ident[j] = (4 * g + j == c) ? (half_t)1.0f : (half_t)0.0f;

    f4 dW0[4][KT0], dWh[NH][4][4], dWo[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < KT0; j++) dW0[i][j] = f4{0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < NH; m++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) dWh[m][i][j] = f4{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; j++) dWo[j] = f4{0, 0, 0, 0};

    [[maybe_unused]] int stamp_i = 1;
    for (uint32_t pair = wave0; pair < n_pairs; pair += nwaves) {
        MLP_STAMP(blockIdx.x * 4 + w, stamp_i); stamp_i++;
        // ---- this pair's inputs (chain layout) from the request issued one iteration ago; then the next request
        if (!AHEAD) request(pair);
        const Req cur = nx;
        if (AHEAD && pair + nwaves < n_pairs) request(pair + nwaves);
        h4 xf[2][KT0], gf[2], hq[2];
        bool act[2];
        size_t row[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const uint32_t tile = 2 * pair + t;
            act[t] = tile < n_tiles;                                     // wave-uniform
            row[t] = (size_t)(act[t] ? tile : 0) * 16 + c;
            gf[t] = zero4; hq[t] = cur.hq[t];
            if constexpr (MODE == 1) {
                static_assert(MODE == 0 || KT0 == 2, "head colour net has a 32-wide input");
                color_inputs(cur.dir[t][0], cur.dir[t][1], cur.dir[t][2], hq[t], g, xf[t]);
                if (g == 0) {
#pragma unroll
                    for (int r = 0; r < 3; r++) gf[t][r] = rgb_logit_grad(cur.gy[t][r], cur.y[t][r]);
                }
            } else {
#pragma unroll
                for (int kt = 0; kt < KT0; kt++) xf[t][kt] = cur.xf[t][kt];
                gf[t] = cur.gf[t];
            }
            // a tile past the batch (odd tile count) re-reads the last tile and contributes nothing: with dL/dout = 0 every dL/dH
            // and so every dW term of the tile is zero; its dX is not stored
            if (!act[t]) gf[t] = zero4;
        }
        MLP_PHASE(blockIdx.x * 4 + w, 0);
        // ---- recompute the hidden activations (post-ReLU) of both tiles; one fragment read serves both.  The fragments of a
        // layer are requested one layer AHEAD (with one wave per SIMD nothing else covers an LDS latency: 42 % of the wave's
        // cycles were s_waitcnt, profiles/r3a_sq_stall_breakdown.txt) and pinned there with a scheduling barrier.
        h4 h[2][NH + 1][4];
        {
            auto load_w0 = [&](h4 (&a)[4][KT0]) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int kt = 0; kt < KT0; kt++) a[mt][kt] = *reinterpret_cast<const h4*>(Wl + C::W0_OFF + (mt * 16 + c) * C::LDX + kt * 16 + 4 * g);
            };
            auto load_wh = [&](int l, h4 (&a)[4][4]) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int kt = 0; kt < 4; kt++) a[mt][kt] = *reinterpret_cast<const h4*>(Wl + C::WH_OFF + (l * 64 + mt * 16 + c) * C::LDH + kt * 16 + 4 * g);
            };
            f4 acc[2][4];
            h4 a0[4][KT0], a1[4][4], a2[4][4];
            load_w0(a0);
            load_wh(0, a1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int t = 0; t < 2; t++) acc[t][mt] = mfma_ksteps<KT0>([&](int kt) { return a0[mt][kt]; }, xf[t], f4{0, 0, 0, 0});
            if constexpr (NH > 1) load_wh(1, a2);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 2; t++) relu4(acc[t], h[t][0]);
#pragma unroll
            for (int l = 0; l < NH; l++) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int t = 0; t < 2; t++)
                        acc[t][mt] = mfma_ksteps<4>([&](int kt) { return (l & 1) ? a2[mt][kt] : a1[mt][kt]; }, h[t][l], f4{0, 0, 0, 0});
                static_assert(NH <= 2, "fragment double buffer: two hidden GEMMs at most");
#pragma unroll
                for (int t = 0; t < 2; t++) relu4(acc[t], h[t][l + 1]);
            }
        }
        MLP_PHASE(blockIdx.x * 4 + w, 1);
        // transposed weight fragments (A[f][o] = W[o][f]) of the chain, likewise requested one step ahead
        auto load_wt = [&](int l, h4 (&a)[4][4]) {               // W_l^T of hidden GEMM l (1-based)
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int kt = 0; kt < 4; kt++) a[mt][kt] = lds_tr_read(Wl + C::WH_OFF + ((l - 1) * 64 + kt * 16 + 4 * g + tq) * C::LDH + mt * 16 + 4 * tp);
        };
        h4 wt[2][4][4];                                         // double buffer: hidden layer l uses wt[l & 1]
        h4 wo[4];
#pragma unroll
        for (int mt = 0; mt < 4; mt++) wo[mt] = lds_tr_read(Wl + C::WO_OFF + (4 * g + tq) * C::LDH + mt * 16 + 4 * tp);            // A[f][o] = Wout[o][f]
        load_wt(NH, wt[NH & 1]);
        __builtin_amdgcn_sched_barrier(0);
        // ---- output layer: dWout += G^T H_NH over the 32 rows ; dH_NH = (Wout^T G) * relu'
        h4 d[2][4];
        {
            h4 TG[2], TH[2][4];
            { const h4 gg[2] = {gf[0], gf[1]}; mfma_transpose_n<2>(gg, ident, TG); }
#pragma unroll
            for (int t = 0; t < 2; t++) mfma_transpose_n<4>(h[t][NH], ident, TH[t]);
            f4 da[2][4];
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int t = 0; t < 2; t++) da[t][mt] = mfma16(wo[mt], gf[t], f4{0, 0, 0, 0});
#pragma unroll
            for (int nt = 0; nt < 4; nt++) dWo[nt] = mfma32(TG[0], TG[1], TH[0][nt], TH[1][nt], dWo[nt]);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++) d[t][mt] = relu_bwd4(da[t][mt], h[t][NH][mt]);
        }
        MLP_PHASE(blockIdx.x * 4 + w, 2);
        // ---- hidden layers, last to first: dW_l += D_l^T H_{l-1} ; dH_{l-1} = (W_l^T dH_l) * relu'
        h4 wx[MODE == 1 ? 1 : KT0][4];                          // W0^T fragments of the dX product (MODE 1: features 16..31 only)
#pragma unroll
        for (int l = NH; l >= 1; l--) {
            if (l > 1) load_wt(l - 1, wt[(l - 1) & 1]);          // next step's fragments
            else {
#pragma unroll
                for (int it = 0; it < (MODE == 1 ? 1 : KT0); it++)
#pragma unroll
                    for (int kt = 0; kt < 4; kt++)
                        wx[it][kt] = lds_tr_read(Wl + C::W0_OFF + (kt * 16 + 4 * g + tq) * C::LDX + (MODE == 1 ? 16 : it * 16) + 4 * tp);   // W0^T
            }
            __builtin_amdgcn_sched_barrier(0);
            h4 TD[2][4], TH[2][4];
#pragma unroll
            for (int t = 0; t < 2; t++) { mfma_transpose_n<4>(d[t], ident, TD[t]); mfma_transpose_n<4>(h[t][l - 1], ident, TH[t]); }
            f4 da[2][4];
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int t = 0; t < 2; t++) da[t][mt] = mfma_ksteps<4>([&](int kt) { return wt[l & 1][mt][kt]; }, d[t], f4{0, 0, 0, 0});
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < 4; nt++) dWh[l - 1][mt][nt] = mfma32(TD[0][mt], TD[1][mt], TH[0][nt], TH[1][nt], dWh[l - 1][mt][nt]);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++) d[t][mt] = relu_bwd4(da[t][mt], h[t][l - 1][mt]);
        }
        MLP_PHASE(blockIdx.x * 4 + w, 3);
        // ---- input layer: dW0 += D_0^T X ; dX = W0^T dH_0
        {
            h4 TD[2][4], TX[2][KT0];
#pragma unroll
            for (int t = 0; t < 2; t++) { mfma_transpose_n<4>(d[t], ident, TD[t]); mfma_transpose_n<KT0>(xf[t], ident, TX[t]); }
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < KT0; nt++) dW0[mt][nt] = mfma32(TD[0][mt], TD[1][mt], TX[0][nt], TX[1][nt], dW0[mt][nt]);
        }
        if constexpr (MODE == 1) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const f4 acc = mfma_ksteps<4>([&](int kt) { return wx[0][kt]; }, d[t], f4{0, 0, 0, 0});
                const h4 v = head_grad_h(acc, &cur.gs[t], ha.density_scale, hq[t][0], g);
                if (act[t]) *reinterpret_cast<h4*>(grad_in + row[t] * 16 + 4 * g) = v;
            }
        } else if (grad_in) {
#pragma unroll
            for (int it = 0; it < KT0; it++) {
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const f4 acc = mfma_ksteps<4>([&](int kt) { return wx[MODE == 1 ? 0 : it][kt]; }, d[t], f4{0, 0, 0, 0});
                    h4 v;
#pragma unroll
                    for (int r = 0; r < 4; r++) v[r] = (half_t)acc[r];
                    if (act[t]) store_dx<IN>(grad_in, row[t], Bn, it, g, ha.level_major, v);
                }
            }
        }
        MLP_PHASE(blockIdx.x * 4 + w, 4);
    }

    // ---- the 4 waves' dW tiles -> one fp32 slab per workgroup, in a fixed order: (w0 + w2) + (w1 + w3).  Tiles travel in
    // the C/D register layout (one 16-byte LDS access per tile and lane); the slab store undoes it.
    MLP_STAMP(blockIdx.x * 4 + w, 14);
    f4* red = reinterpret_cast<f4*>(lds + C::W_HALVES);                  // [2][N_TILES][64] f4
    auto for_tiles = [&](auto&& fn) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < KT0; j++) fn(t++, dW0[i][j]);
#pragma unroll
        for (int m = 0; m < NH; m++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) fn(t++, dWh[m][i][j]);
#pragma unroll
        for (int j = 0; j < 4; j++) fn(t++, dWo[j]);
    };
    if (w < 2) for_tiles([&](int t, const f4& v) { red[((size_t)w * C::N_TILES + t) * 64 + lane] = v; });
    __syncthreads();
    if (w >= 2) for_tiles([&](int t, const f4& v) { f4& r = red[((size_t)(w - 2) * C::N_TILES + t) * 64 + lane]; r = r + v; });
    __syncthreads();
    float* slab = slabs + (size_t)blockIdx.x * nW;
    for (uint32_t e = threadIdx.x; e < (uint32_t)C::N_TILES * 64; e += 256) {
        const uint32_t t = e >> 6, ln = e & 63, cc = ln & 15, gg = ln >> 4;        // tiles in for_tiles order: W0 | hidden | Wout
        const f4 v = red[e] + red[(size_t)C::N_TILES * 64 + e];
        DwSlot slot;
        if (t < 4u * KT0) slot = dw_slot<IN>(0, t / KT0, t % KT0);
        else if (t < 4u * KT0 + NH * 16u) {
            const uint32_t u = t - 4 * KT0;
            slot = dw_slot<IN>(1 + u / 16, (u % 16) / 4, u % 4);
        } else slot = dw_slot<IN>(NH + 1, 0, t - 4 * KT0 - NH * 16);
        store_dw_tile(slab, slot, cc, gg, v);
    }
    MLP_STAMP(blockIdx.x * 4 + w, 15);
}

// the reduction of two networks' slabs in one launch (blocks [0, nb_a) reduce A, the rest B): one graph node less per step.
// One block more than the reduction needs takes the deferred loss value along (lae_composite_rays_train_step with
// defer_loss), without a launch of its own on the step's critical path.  Device bodies: dw_reduce.h.
__global__ __launch_bounds__(64 * DWR_GROUPS) void k_dw_reduce2(lae_dw::DwTailJob job) {
    __shared__ float part[lae_dw::DWR_LDS_FLOATS];
    lae_dw::dw_tail_task(job, blockIdx.x, part);
}

// 2 = wave-private dW with MFMA transposes (k_mlp_bwd_wave, default), 0 = workgroup-cooperative dW (k_mlp_bwd_coop, round 2), 3 = wave-private
// for one hidden GEMM and cooperative for two; A/B switch, see lae_ffmlp_set_mode.  -1: LAE_MLP_BWD_VARIANT not read yet.
int g_bwd_fused_variant = -1;
int bwd_fused_variant() {
    if (g_bwd_fused_variant < 0) g_bwd_fused_variant = lae::env_int("LAE_MLP_BWD_VARIANT", 2, {0, 2, 3});
    return g_bwd_fused_variant;
}

template <int IN, int NH, int MODE = 0>
int launch_bwd_fused(const half_t* grad, const half_t* x, const half_t* W, uint32_t B, half_t* grad_in, half_t* gw, hipStream_t s,
                     HeadBwdArgs ha = HeadBwdArgs{}, int accumulate = 0, float* slabs = nullptr, uint32_t* n_slices_out = nullptr,
                     int32_t* nf_flag = nullptr) {
    // slabs != nullptr: the partial slabs go to the caller's region (room for 2 * num_cus slices) and the reduction is
    // left to the caller (lae_nerf_head_backward reduces both networks in one launch)
    const uint32_t nW = 64 * (IN + 64 * NH + 16);
    const uint32_t n_tiles = B / 16, cus = (uint32_t)lae::num_cus();
    const int variant = bwd_fused_variant();
    const bool wave = variant == 2 || (variant == 3 && NH == 1);       // 3: wave-private for one hidden GEMM, cooperative for two
    // wave-private: one wave per SIMD (2 measured on the sigma net, 26 spilled registers: 3.1 us per pair and SIMD against 2.4);
    // cooperative: the round-2 kernel, kept as the A/B predecessor
    constexpr int WPE = 1, COOP_WAVES = 8;
    void (*const kernel)(const half_t*, const half_t*, const half_t*, uint32_t, half_t*, float*, uint32_t, HeadBwdArgs) =
        wave ? &k_mlp_bwd_wave<IN, NH, MODE, WPE> : &k_mlp_bwd_coop<IN, NH, MODE, COOP_WAVES>;
    const uint32_t threads = wave ? 256 : 64 * COOP_WAVES;
    const size_t lds_bytes = wave ? WaveCfg<IN, NH>::LDS_BYTES : (size_t)CoopCfg<IN, NH, COOP_WAVES>::LDS_HALVES * 2;
    const uint32_t blocks = std::max(1u, wave ? std::min(lae::cdiv(lae::cdiv(n_tiles, 2), 4), cus * WPE) : std::min(lae::cdiv(n_tiles, COOP_WAVES), cus * 2));
    static bool lds_allowed[2] = {false, false};
    if (const int rc = lae::allow_dynamic_lds(lds_allowed[wave], reinterpret_cast<const void*>(kernel), lds_bytes)) return rc;
    float* ws = slabs ? slabs : reinterpret_cast<float*>(lae::workspace(lae::WS_FFMLP_SLABS, (size_t)blocks * nW * sizeof(float), s));
    if (!ws) return LAE_ELAUNCH;
    kernel<<<blocks, threads, lds_bytes, s>>>(grad, x, W, n_tiles, grad_in, ws, nW, ha);
    if (n_slices_out) *n_slices_out = blocks;
    if (!slabs) lae::dw_reduce_launch(ws, blocks, nW, gw, accumulate, nf_flag, s);
    return LAE_OK;
}

// (IN, NH) of the served shapes as compile-time constants: f(integral_constant<IN>, integral_constant<NH>), LAE_EINVAL otherwise
template <typename F>
int dispatch_in_nh(uint32_t in_dim, uint32_t n_hidden, F&& f) {
    using std::integral_constant;
    auto with_nh = [&](auto in) {
        return n_hidden == 1 ? f(in, integral_constant<int, 1>{}) : n_hidden == 2 ? f(in, integral_constant<int, 2>{}) : (int)LAE_EINVAL;
    };
    switch (in_dim) {
        case 32: return with_nh(integral_constant<int, 32>{});
        case 48: return with_nh(integral_constant<int, 48>{});
        case 64: return with_nh(integral_constant<int, 64>{});
        default: return LAE_EINVAL;
    }
}

}  // namespace

void lae::set_mlp_bwd_variant(int variant) { g_bwd_fused_variant = variant; }

int lae::ffmlp_backward_fused(uint32_t in_dim, uint32_t n_hidden, const void* grad, const void* x, const void* W, uint32_t B,
                              void* grad_in, void* gw, int accumulate, int32_t* nf_flag, hipStream_t s) {
    return dispatch_in_nh(in_dim, n_hidden, [&](auto in, auto nh) {
        return launch_bwd_fused<decltype(in)::value, decltype(nh)::value>((const half_t*)grad, (const half_t*)x, (const half_t*)W, B, (half_t*)grad_in,
                                                                          (half_t*)gw, s, HeadBwdArgs{}, accumulate, nullptr, nullptr, nf_flag);
    });
}

// tail != nullptr (lae_nerf_field_backward, M > 0): the reduction of the two networks' slabs and the deferred loss value are not
// launched but handed back as a job; the caller's next launch on the stream (the grid backward's accumulate pass) runs it
int lae::nerf_head_backward(const float* grad_sigmas, const float* grad_rgbs, const void* enc, const float* dirs, const void* h,
                            const float* rgbs, const void* sigma_weights, const void* color_weights, uint32_t M,
                            float density_scale, void* grad_h, void* grad_enc, void* grad_sigma_weights,
                            void* grad_color_weights, int accumulate_weight_grads, int enc_level_major, int32_t* nonfinite_flag,
                            const float* loss_partials, uint32_t loss_n_part, uint32_t loss_n_elem, const float* loss_scale,
                            float* loss_out, void* stream, lae_dw::DwTailJob* tail) {
    if (tail) tail->n_tasks = 0;
    if (!grad_sigma_weights || !grad_color_weights) return LAE_ENULL;
    if (loss_out && (!loss_partials || loss_n_elem == 0)) return LAE_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (M == 0) {                                        // no samples: zero weight gradients (like the reference's GEMMs on empty batches)
        if (loss_out) {
            const int rc = lae_loss_finish(loss_partials, loss_n_part, loss_n_elem, loss_scale, loss_out, stream);
            if (rc != LAE_OK) return rc;
        }
        if (accumulate_weight_grads) return LAE_OK;
        if (hipMemsetAsync(grad_sigma_weights, 0, 64 * (32 + 64 + 16) * 2, s) != hipSuccess) return LAE_ELAUNCH;
        if (hipMemsetAsync(grad_color_weights, 0, 64 * (32 + 128 + 16) * 2, s) != hipSuccess) return LAE_ELAUNCH;
        return LAE_OK;
    }
    if (!grad_sigmas || !grad_rgbs || !enc || !dirs || !h || !rgbs || !sigma_weights || !color_weights || !grad_h) return LAE_ENULL;
    if (M % 16 != 0) return LAE_EINVAL;
    HeadBwdArgs ha{dirs, rgbs, grad_rgbs, grad_sigmas, density_scale, 0};
    HeadBwdArgs hs{};
    hs.level_major = enc_level_major;
    // partial slabs of both networks side by side in the workspace, reduced by ONE launch after the second backward kernel
    const uint32_t nW_c = 64 * (32 + 128 + 16), nW_s = 64 * (32 + 64 + 16);
    const size_t cap = (size_t)lae::num_cus() * 2;
    float* ws = reinterpret_cast<float*>(lae::workspace(lae::WS_FFMLP_SLABS, cap * (nW_c + nW_s) * sizeof(float), s));
    if (!ws) return LAE_ELAUNCH;
    float* ws_s = ws + cap * nW_c;
    uint32_t n_c = 0, n_s = 0;
    int rc = launch_bwd_fused<32, 2, 1>(nullptr, (const half_t*)h, (const half_t*)color_weights, M, (half_t*)grad_h,
                                        (half_t*)grad_color_weights, s, ha, accumulate_weight_grads, ws, &n_c);
    if (rc != LAE_OK) return rc;
    rc = launch_bwd_fused<32, 1, 0>((const half_t*)grad_h, (const half_t*)enc, (const half_t*)sigma_weights, M, (half_t*)grad_enc,
                                    (half_t*)grad_sigma_weights, s, hs, accumulate_weight_grads, ws_s, &n_s);
    if (rc != LAE_OK) return rc;
    const uint32_t nb_c = lae::cdiv(nW_c, 64u), nb_s = lae::cdiv(nW_s, 64u);
    const LossFinish lf{loss_partials, loss_n_part, loss_n_elem, loss_scale, loss_out};
    const lae_dw::DwTailJob job{ws, n_c, nW_c, (half_t*)grad_color_weights, ws_s, n_s, nW_s, (half_t*)grad_sigma_weights, nb_c, nb_s,
                                accumulate_weight_grads, nonfinite_flag, lf, nb_c + nb_s + (loss_out ? 1u : 0u)};
    if (tail) *tail = job;
    else k_dw_reduce2<<<job.n_tasks, 64 * DWR_GROUPS, 0, s>>>(job);
    return lae::check_launch("nerf_head_backward");
}

extern "C" {

int lae_nerf_head_backward(const float* grad_sigmas, const float* grad_rgbs, const void* enc, const float* dirs, const void* h,
                           const float* rgbs, const void* sigma_weights, const void* color_weights, uint32_t M,
                           float density_scale, void* grad_h, void* grad_enc, void* grad_sigma_weights,
                           void* grad_color_weights, int accumulate_weight_grads, int enc_level_major, int32_t* nonfinite_flag,
                           const float* loss_partials, uint32_t loss_n_part, uint32_t loss_n_elem, const float* loss_scale,
                           float* loss_out, void* stream) {
    return lae::nerf_head_backward(grad_sigmas, grad_rgbs, enc, dirs, h, rgbs, sigma_weights, color_weights, M, density_scale, grad_h,
                                   grad_enc, grad_sigma_weights, grad_color_weights, accumulate_weight_grads, enc_level_major,
                                   nonfinite_flag, loss_partials, loss_n_part, loss_n_elem, loss_scale, loss_out, stream, nullptr);
}

}  // extern "C"
