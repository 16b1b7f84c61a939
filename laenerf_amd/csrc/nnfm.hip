// nnfm.hip -- nearest-neighbour feature matching (ARF / Ref-NPR; the reference's editing/semantic_encoder.py:83-164
// nn_feat_replace / argmin_cos_distance / cos_loss and editing/ref_loss.py NNFMLoss) without the Na x Nb distance matrix.
//
// All features are fp32 and channel-major [n, C, N] (what StyleNetwork.features returns, flattened); n independent problems.
//   pack:    per position v / (sqrt(sum v^2 + 1e-8) + 1e-8) (the matching normalization), rounded to fp16 and written
//            position-major [n, N_pad, C_pad] (channel contiguous, N_pad a multiple of 64, C_pad of 32, padding zero-filled here)
//   match:   cosines by v_mfma_f32_16x16x32_f16 with fp32 accumulation.  A workgroup of four waves owns 64 content rows and one
//            chunk of NNFM_CHUNK = 256 style columns; a wave owns the 64 rows against 64 of the columns, 4 x 4 accumulator tiles
//            (eight 16-byte fragment loads per sixteen MFMAs; the four waves read the same A rows, which the L1 serves).
//            Both operands are position-major, so a lane's fragment (row or column lane & 15, k-slots 8 * (lane >> 4) .. + 7) is
//            one 16-byte load; A and B share the k permutation, so the contraction does not depend on it.  In the C/D layout
//            col = lane & 15 is the style column and row = 4 * (lane >> 4) + reg the content row: after the K loop every lane
//            compares its tiles' columns in rising order (a strict > keeps the lowest index), the 16 column lanes are reduced,
//            and one partial per (chunk, wave) and row is stored.  A second launch combines the partials in a fixed order: the
//            largest cosine wins, among equal cosines the lowest index -- the rule is order independent, so the result does not
//            depend on the schedule.  Padded style columns are excluded by index (a zero column has cosine 0 and would beat
//            every negative cosine).
//   loss:    cos_loss(x, gather(s, z)) on the fp32 features: per position a.t, |a|, |t| (four channel slices per position,
//            summed in a fixed order), the mean by one block in a fixed order (fp64 sum).  The statistics are kept for the
//            backward, which is then elementwise over [C, Na] and coalesced along the positions.
#include "lae_common.h"

namespace {

typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr uint32_t NNFM_ROWS = 64;        // content rows per workgroup = the padding unit of N
constexpr uint32_t NNFM_CHUNK = 256;      // style columns per workgroup (grid.y = ceil(Nb / NNFM_CHUNK))
constexpr uint32_t NNFM_KPAD = 32;        // one K = 32 MFMA step
constexpr int NNFM_THREADS = 256;
constexpr uint32_t NNFM_MAX_N = 1u << 23;      // chunks fit gridDim.y
constexpr uint32_t NNFM_MAX_C = 1u << 16;

__host__ __device__ __forceinline__ uint32_t pad_to(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }
__host__ __device__ __forceinline__ uint32_t n_chunks(uint32_t Nb) { return (Nb + NNFM_CHUNK - 1) / NNFM_CHUNK; }

struct Best { float v; int32_t j; };
// the order-independent rule: the larger cosine wins; among equal cosines the lower index
__device__ __forceinline__ bool better(float v, int32_t j, float bv, int32_t bj) { return v > bv || (v == bv && j < bj); }

// ---------------------------------------------------------------------------------------------------------------- pack
// block = 64 positions x 4 channel slices.  Reads are coalesced along the positions; 64 x 32 tiles go through LDS so that the
// fp16 rows are written 16 bytes per thread along the channels.
constexpr int PACK_PITCH = 40;            // halves per LDS row: 32 + 8 (keeps the 16-byte reads aligned, spreads the banks)
__global__ void __launch_bounds__(NNFM_THREADS) k_nnfm_pack(const float* __restrict__ feats, uint32_t C, uint32_t N, uint32_t N_pad,
                                                            uint32_t C_pad, half_t* __restrict__ packed) {
    __shared__ float ss[4][64];
    __shared__ __attribute__((aligned(16))) half_t tile[64 * PACK_PITCH];
    const uint32_t p = blockIdx.y;
    const uint32_t pos = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 64 + pos;
    const bool live = i < N;
    const float* src = feats + (size_t)p * C * N + i;
    float s = 0.0f;
    if (live)
        for (uint32_t c = sl; c < C; c += 4) { const float v = src[(size_t)c * N]; s = fmaf(v, v, s); }
    ss[sl][pos] = s;
    __syncthreads();
    const float tot = ((ss[0][pos] + ss[1][pos]) + ss[2][pos]) + ss[3][pos];
    const float inv = 1.0f / (sqrtf(tot + 1e-8f) + 1e-8f);
    const uint32_t wpos = threadIdx.x >> 2, wch = threadIdx.x & 3;       // writer: 4 threads x 8 halves per position
    half_t* dst = packed + ((size_t)p * N_pad + blockIdx.x * 64 + wpos) * C_pad + wch * 8;
    for (uint32_t c0 = 0; c0 < C_pad; c0 += 32) {
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            const uint32_t c = c0 + sl + 4 * q;
            const float v = (live && c < C) ? src[(size_t)c * N] * inv : 0.0f;
            tile[pos * PACK_PITCH + sl + 4 * q] = (half_t)v;
        }
        __syncthreads();
        *reinterpret_cast<uint4*>(dst + c0) = *reinterpret_cast<const uint4*>(&tile[wpos * PACK_PITCH + wch * 8]);
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------- match
__device__ __forceinline__ h8 load_frag(const half_t* p) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    return __builtin_bit_cast(h8, q);
}

// grid (Na_pad / 64, chunks, n).  partial [n, 4 * chunks, Na_pad] of (cosine, index): wave w of a workgroup owns the 64 content rows
// against columns 64 w .. 64 w + 63 of the chunk, a 4 x 4 grid of accumulator tiles (the four waves read the same A rows)
__global__ void __launch_bounds__(NNFM_THREADS) k_nnfm_match(const half_t* __restrict__ A, const half_t* __restrict__ B, uint32_t Na_pad,
                                                             uint32_t Nb, uint32_t Nb_pad, uint32_t C_pad, Best* __restrict__ partial) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 15, g = lane >> 4;
    const uint32_t p = blockIdx.z;
    const uint32_t row0 = blockIdx.x * NNFM_ROWS;
    const uint32_t cw = blockIdx.y * NNFM_CHUNK + wave * 64;
    float bv[4][4];
    int32_t bj[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int q = 0; q < 4; q++) { bv[mt][q] = -INFINITY; bj[mt][q] = 0x7fffffff; }

    if (cw < Nb) {                                                          // else: only padding (or nothing) in this wave's columns
        const half_t* a = A + ((size_t)p * Na_pad + row0 + r) * C_pad + 8 * g;
        const half_t* b = B + ((size_t)p * Nb_pad + cw + r) * C_pad + 8 * g;
        const size_t t16 = (size_t)16 * C_pad;
        f4 acc[4][4];
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) acc[mt][nt] = f4{0, 0, 0, 0};
        // the next K step's fragments are in flight while this one's sixteen MFMAs issue
        h8 fa[4], fb[4];
#pragma unroll
        for (int t = 0; t < 4; t++) { fa[t] = load_frag(a + t * t16); fb[t] = load_frag(b + t * t16); }
        for (uint32_t k = NNFM_KPAD; k < C_pad; k += NNFM_KPAD) {
            h8 na[4], nb[4];
#pragma unroll
            for (int t = 0; t < 4; t++) { na[t] = load_frag(a + t * t16 + k); nb[t] = load_frag(b + t * t16 + k); }
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < 4; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 4; t++) { fa[t] = na[t]; fb[t] = nb[t]; }
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {                                    // columns in rising order: a strict > keeps the lowest index
            const uint32_t j = cw + nt * 16 + r;
            if (j < Nb) {                                                   // padded columns are excluded by index
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (acc[mt][nt][q] > bv[mt][q]) { bv[mt][q] = acc[mt][nt][q]; bj[mt][q] = (int32_t)j; }
            }
        }
        // over the 16 column lanes (lanes that share lane >> 4 hold the same content rows)
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float v = bv[mt][q];
                int32_t j = bj[mt][q];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) {
                    const float ov = __shfl_xor(v, m, 64);
                    const int32_t oj = __shfl_xor(j, m, 64);
                    if (better(ov, oj, v, j)) { v = ov; j = oj; }
                }
                bv[mt][q] = v; bj[mt][q] = j;
            }
    }
    if (r == 0) {
        Best* out = partial + ((size_t)p * (4 * gridDim.y) + 4 * blockIdx.y + wave) * Na_pad + row0 + 4 * g;
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                Best o; o.v = bv[mt][q]; o.j = bj[mt][q];
                out[mt * 16 + q] = o;
            }
    }
}

__global__ void __launch_bounds__(NNFM_THREADS) k_nnfm_combine(const Best* __restrict__ partial, uint32_t n_part, uint32_t Na, uint32_t Na_pad,
                                                               uint32_t Nb, int32_t* __restrict__ z, float* __restrict__ d_best) {
    const uint32_t i = blockIdx.x * NNFM_THREADS + threadIdx.x, p = blockIdx.y;
    if (i >= Na) return;
    const Best* src = partial + (size_t)p * n_part * Na_pad + i;
    float v = -INFINITY;
    int32_t j = 0x7fffffff;
    for (uint32_t k = 0; k < n_part; k++) {
        const Best b = src[(size_t)k * Na_pad];
        if (better(b.v, b.j, v, j)) { v = b.v; j = b.j; }
    }
    if ((uint32_t)j >= Nb) { j = 0; v = NAN; }                             // nothing comparable (non-finite features): a valid index
    z[(size_t)p * Na + i] = j;
    if (d_best) d_best[(size_t)p * Na + i] = 1.0f - v;
}

// ---------------------------------------------------------------------------------------------------------------- loss
// stats [4, n * Na]: a . t^ (t^ = t / (|t| + 1e-8)), |a|, |t|, the position's term 1 - a^ . t^
__global__ void __launch_bounds__(NNFM_THREADS) k_nnfm_stats(const float* __restrict__ x, const float* __restrict__ s, const int32_t* __restrict__ z,
                                                             uint32_t C, uint32_t Na, uint32_t Nb, size_t P, float* __restrict__ stats) {
    __shared__ float sh[3][4][64];
    const uint32_t p = blockIdx.y;
    const uint32_t pos = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 64 + pos;
    float dot = 0.0f, aa = 0.0f, tt = 0.0f;
    if (i < Na) {
        uint32_t zi = (uint32_t)z[(size_t)p * Na + i];
        if (zi >= Nb) zi = Nb - 1;                                         // never a read outside s
        const float* xa = x + (size_t)p * C * Na + i;
        const float* st = s + (size_t)p * C * Nb + zi;
        for (uint32_t c = sl; c < C; c += 4) {
            const float a = xa[(size_t)c * Na], t = st[(size_t)c * Nb];
            dot = fmaf(a, t, dot); aa = fmaf(a, a, aa); tt = fmaf(t, t, tt);
        }
    }
    sh[0][sl][pos] = dot; sh[1][sl][pos] = aa; sh[2][sl][pos] = tt;
    __syncthreads();
    if (sl == 0 && i < Na) {
        const float d = ((sh[0][0][pos] + sh[0][1][pos]) + sh[0][2][pos]) + sh[0][3][pos];
        const float na = sqrtf(((sh[1][0][pos] + sh[1][1][pos]) + sh[1][2][pos]) + sh[1][3][pos]);
        const float nt = sqrtf(((sh[2][0][pos] + sh[2][1][pos]) + sh[2][2][pos]) + sh[2][3][pos]);
        const float dh = d / (nt + 1e-8f);
        const size_t o = (size_t)p * Na + i;
        stats[o] = dh;
        stats[P + o] = na;
        stats[2 * P + o] = nt;
        stats[3 * P + o] = 1.0f - dh / (na + 1e-8f);
    }
}

// one block: the mean of the P terms, thread-strided partial sums then a tree, all in fp64 and in a fixed order
__global__ void __launch_bounds__(1024) k_nnfm_mean(const float* __restrict__ terms, size_t P, float* __restrict__ loss) {
    __shared__ double sh[1024];
    double acc = 0.0;
    for (size_t k = threadIdx.x; k < P; k += 1024) acc += (double)terms[k];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sh[0] / (double)P);
}

// dx[c, i] = -(g / P) * (t^ / s_a - (a . t^) a / (|a| s_a^2)), s_a = |a| + 1e-8; 0 where a is the zero vector
__global__ void __launch_bounds__(NNFM_THREADS) k_nnfm_bwd(const float* __restrict__ x, const float* __restrict__ s, const int32_t* __restrict__ z,
                                                           const float* __restrict__ stats, const float* __restrict__ g_loss, uint32_t C,
                                                           uint32_t Na, uint32_t Nb, size_t P, float* __restrict__ dx) {
    const uint32_t p = blockIdx.z;
    const uint32_t i = blockIdx.x * NNFM_THREADS + threadIdx.x;
    if (i >= Na) return;
    const size_t o = (size_t)p * Na + i;
    uint32_t zi = (uint32_t)z[o];
    if (zi >= Nb) zi = Nb - 1;
    const float dh = stats[o], na = stats[P + o], nt = stats[2 * P + o];
    const float sa = na + 1e-8f;
    const float k = -g_loss[0] / (float)P;
    const float ct = na > 0.0f ? k / ((nt + 1e-8f) * sa) : 0.0f;
    const float ca = na > 0.0f ? k * dh / (na * sa * sa) : 0.0f;
    const uint32_t c_end = min(C, (blockIdx.y + 1) * 32u);
    for (uint32_t c = blockIdx.y * 32u; c < c_end; c++) {
        const size_t xo = ((size_t)p * C + c) * Na + i;
        const float a = x[xo], t = s[((size_t)p * C + c) * Nb + zi];
        dx[xo] = ct * t - ca * a;
    }
}

int check_dims(uint32_t n, uint32_t C, uint32_t Na, uint32_t Nb) {
    if (n < 1 || n > 65535 || C < 1 || C > NNFM_MAX_C || Nb < 1 || Nb > NNFM_MAX_N || Na > NNFM_MAX_N) return LAE_EINVAL;
    return LAE_OK;
}

}  // namespace

extern "C" {

uint64_t lae_nnfm_packed_bytes(uint32_t n, uint32_t C, uint32_t N) {
    return (uint64_t)n * pad_to(N, NNFM_ROWS) * pad_to(C, NNFM_KPAD) * sizeof(half_t);
}

uint64_t lae_nnfm_match_bytes(uint32_t n, uint32_t Na, uint32_t Nb) {
    return (uint64_t)n * 4 * n_chunks(Nb) * pad_to(Na, NNFM_ROWS) * sizeof(Best);
}

uint64_t lae_nnfm_workspace_bytes(uint32_t n, uint32_t C, uint32_t Na, uint32_t Nb) {
    const uint64_t part = (lae_nnfm_match_bytes(n, Na, Nb) + 255) & ~(uint64_t)255;
    return part + lae_nnfm_packed_bytes(n, C, Na);
}

int lae_nnfm_pack(const float* feats, uint32_t n, uint32_t C, uint32_t N, void* packed, void* stream) {
    if (n < 1 || n > 65535 || C < 1 || C > NNFM_MAX_C || N > NNFM_MAX_N) return LAE_EINVAL;
    if (N == 0) return LAE_OK;
    if (!feats || !packed) return LAE_ENULL;
    if ((uintptr_t)packed & 15) return LAE_EINVAL;
    const uint32_t N_pad = pad_to(N, NNFM_ROWS), C_pad = pad_to(C, NNFM_KPAD);
    hipLaunchKernelGGL(k_nnfm_pack, dim3(N_pad / 64, n), dim3(NNFM_THREADS), 0, (hipStream_t)stream, feats, C, N, N_pad, C_pad,
                       (half_t*)packed);
    return lae::check_launch("nnfm_pack");
}

int lae_nnfm_match(const void* a_packed, const void* b_packed, uint32_t n, uint32_t Na, uint32_t Nb, uint32_t C, int32_t* z, float* d_best,
                   void* workspace, void* stream) {
    const int rc = check_dims(n, C, Na, Nb);
    if (rc != LAE_OK) return rc;
    if (Na == 0) return LAE_OK;
    if (!a_packed || !b_packed || !z || !workspace) return LAE_ENULL;
    if (((uintptr_t)a_packed | (uintptr_t)b_packed) & 15 || (uintptr_t)workspace & 7) return LAE_EINVAL;
    const uint32_t Na_pad = pad_to(Na, NNFM_ROWS), Nb_pad = pad_to(Nb, NNFM_ROWS), C_pad = pad_to(C, NNFM_KPAD);
    const uint32_t chunks = n_chunks(Nb);
    hipLaunchKernelGGL(k_nnfm_match, dim3(Na_pad / NNFM_ROWS, chunks, n), dim3(NNFM_THREADS), 0, (hipStream_t)stream, (const half_t*)a_packed,
                       (const half_t*)b_packed, Na_pad, Nb, Nb_pad, C_pad, (Best*)workspace);
    int e = lae::check_launch("nnfm_match");
    if (e != LAE_OK) return e;
    hipLaunchKernelGGL(k_nnfm_combine, dim3(lae::cdiv(Na, NNFM_THREADS), n), dim3(NNFM_THREADS), 0, (hipStream_t)stream, (const Best*)workspace,
                       4 * chunks, Na, Na_pad, Nb, z, d_best);
    return lae::check_launch("nnfm_combine");
}

int lae_nnfm_loss_forward(const float* x, const float* s, const int32_t* z, uint32_t n, uint32_t C, uint32_t Na, uint32_t Nb, float* loss,
                          float* stats, void* stream) {
    const int rc = check_dims(n, C, Na, Nb);
    if (rc != LAE_OK) return rc;
    if (Na == 0) return LAE_OK;
    if (!x || !s || !z || !loss || !stats) return LAE_ENULL;
    const size_t P = (size_t)n * Na;
    hipLaunchKernelGGL(k_nnfm_stats, dim3(lae::cdiv(Na, 64), n), dim3(NNFM_THREADS), 0, (hipStream_t)stream, x, s, z, C, Na, Nb, P, stats);
    int e = lae::check_launch("nnfm_stats");
    if (e != LAE_OK) return e;
    hipLaunchKernelGGL(k_nnfm_mean, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)(stats + 3 * P), P, loss);
    return lae::check_launch("nnfm_mean");
}

int lae_nnfm_loss_backward(const float* x, const float* s, const int32_t* z, const float* stats, const float* g_loss_dev, uint32_t n, uint32_t C,
                           uint32_t Na, uint32_t Nb, float* dx, void* stream) {
    const int rc = check_dims(n, C, Na, Nb);
    if (rc != LAE_OK) return rc;
    if (Na == 0) return LAE_OK;
    if (!x || !s || !z || !stats || !g_loss_dev || !dx) return LAE_ENULL;
    const size_t P = (size_t)n * Na;
    hipLaunchKernelGGL(k_nnfm_bwd, dim3(lae::cdiv(Na, NNFM_THREADS), lae::cdiv(C, 32), n), dim3(NNFM_THREADS), 0, (hipStream_t)stream, x, s, z,
                       stats, g_loss_dev, C, Na, Nb, P, dx);
    return lae::check_launch("nnfm_loss_backward");
}

}  // extern "C"
