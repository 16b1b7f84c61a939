// tsdf.hip -- fuse rendered depth (and colour) views into a truncated signed distance field on a lattice, and colour the
// marching-cubes vertices of that field from the fused colours ("TSDF export").
//
// The reference exports a mesh from a level set of the raw density (nerf/utils.py:722-741); it has no counterpart of this file.
// The surface the renders show is the expected termination depth, so the views themselves are fused (KinectFusion's rule) and
// marching cubes runs at zero.  This is a project-and-gather pass over (lattice points x views), like masklift.hip.
//
// THE RULE.
//   views      packed fp32 [V, H, W], the plane lae_mask_lift_pack writes: t_surf = |packed| (the sign bit is ignored), +inf = a
//              transparent pixel, NaN = no observation.  poses fp32 [V, 4, 4] cam2world [R | o], one (fx, fy, cx, cy).
//   lattice    three fp32 axis arrays xs[nx], ys[ny], zs[nz]; voxel (i, j, k) sits at p = (xs[i], ys[j], zs[k]) and the outputs
//              are indexed (i * ny + j) * nz + k, like marching cubes' u[i, j, k].
//   frames     optional uint8 [V, H, W, 3].
//   per (voxel, view), in ascending view order -- the projection is k_mask_lift's, statement for statement:
//              d = p - o, q = R^T d.  q.z <= 0: no observation.  u = fx q.x / q.z + cx, v = fy q.y / q.z + cy; outside
//              [0, W) x [0, H): no observation.  Pixel (floor u, floor v); t_vox = |d|; s = t_surf - t_vox.  A NaN t_surf: no
//              observation.  s < -trunc: OCCLUDED, n_occ += 1.  s > trunc (a transparent pixel included): FREE, n_free += 1.
//              Otherwise NEAR: n_near += 1, S += s / trunc (an fp32 running sum), and with frames the pixel's three bytes are
//              added to three uint32 sums.
//   per voxel  n_obs = n_near + n_free;
//              tsdf = (S + float(n_free)) / float(n_obs)   if n_obs >= min_views
//                   = -1                                   else if n_occ > 0     (space is solid until seen empty)
//                   = +1                                   otherwise             (never in any frame)
//              The field written is u = -tsdf: larger inside, like a density, so marching_cubes(u, 0), the vertex attributes
//              (normals point outward) and the components filter apply unchanged.  counts uint16 [n, 4] = (near, free,
//              occluded, 0); rgb fp32 [n, 3] = float(sum) / float(n_near) / 255, zeros where n_near == 0.
// "Solid until seen empty" keeps the unobserved interior of the object from growing a second wall behind the truncation band.
// Its price: a region that some view sees only as occluded and no view sees empty stays solid (a box corner behind the
// object); the components filter (keep_largest) removes such blobs.
//
// A thread owns its voxel: no atomics, a fixed order, and two calls give the same bytes.  Every fp32 statement is one rounding
// (the library is built with -ffp-contract=off; divisions are __fdiv_rn; the root is sqrtf, which the compiler rounds correctly by
// default -- this toolchain lowers __fsqrt_rn to the bare v_sqrt_f32, which is good to one ulp only), and tsdf.py's
// tsdf_numpy(dtype=float32) writes the same statements in the same order.
//
// VERTEX COLOURS (second kernel).  A marching-cubes vertex lies on a lattice edge; (base, axis, t) are located exactly as
// lae_mesh_vertex_attrs does.  Both endpoints have n_near > 0: c = c_a + t (c_b - c_a); one has: that endpoint's colour; neither:
// grey 0.5, and the vertex is counted in *n_grey.
#include <stdlib.h>

#include "lae_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

// A workgroup takes a brick of TS_BI x TS_BJ x TS_BK voxels, k fastest across lanes: a wave is one i-slab of 4 x 16 voxels, its
// stores are 64-byte runs and its gathers land in a small pixel patch of each view.
constexpr int TS_BI = 4, TS_BJ = 4, TS_BK = 16, TS_THREADS = TS_BI * TS_BJ * TS_BK, TS_CHUNK = LAE_TSDF_POSE_CHUNK;
static_assert(TS_THREADS == 256 && TS_CHUNK == 64, "the cull is one wave testing one view per lane");
constexpr uint32_t TS_MAX_SIDE = 512;                  // marching cubes' own shape limit (mesh.hip check_dims)
// The cull's margin, relative to the magnitude of the tested sum's terms.  The voxel loop's q and u carry a few fp32 roundings
// (relative 2^-22 of those terms); a view is skipped only where every voxel of the brick misses the threshold by 2^-10 of them.
constexpr float TS_CULL_MARGIN = 0x1p-10f;

__device__ __forceinline__ float len3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// true when no point within `rad` of c can project to the tested side's inside: m . (p - o) stays below zero by the margin for
// m = a * column ka of R + b * column 2 (u < 0 when q.z > 0), term = the magnitude bound of the sum's terms, L >= |p - o|
__device__ __forceinline__ bool plane_culls(const float* Q, int ka, float a, float b, float dx, float dy, float dz, float rad, float term,
                                            float L) {
    const float mx = a * Q[ka] + b * Q[2], my = a * Q[4 + ka] + b * Q[6], mz = a * Q[8 + ka] + b * Q[10];
    return (mx * dx + my * dy + mz * dz) + rad * len3(mx, my, mz) + TS_CULL_MARGIN * term * L < 0.0f;
}

template <bool FRAMES>
__global__ __launch_bounds__(TS_THREADS) void k_tsdf_fuse(const float* __restrict__ packed, const float* __restrict__ poses, uint32_t V,
                                                          float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                                          const float* __restrict__ xs, const float* __restrict__ ys,
                                                          const float* __restrict__ zs, uint32_t nx, uint32_t ny, uint32_t nz,
                                                          const uint8_t* __restrict__ frames, float trunc, uint32_t min_views,
                                                          int cull, float* __restrict__ u_out, uint2* __restrict__ counts_out,
                                                          float* __restrict__ rgb_out) {
    __shared__ float P[TS_CHUNK * 12];
    __shared__ uint32_t surv[TS_CHUNK];                // the chunk's surviving views, ascending
    __shared__ uint32_t n_surv;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t i0 = blockIdx.z * TS_BI, j0 = blockIdx.y * TS_BJ, k0 = blockIdx.x * TS_BK;
    const uint32_t i = i0 + (tid >> 6), j = j0 + ((tid >> 4) & 3u), k = k0 + (tid & 15u);
    const bool live = i < nx && j < ny && k < nz;
    const float wx = live ? xs[i] : 0.0f, wy = live ? ys[j] : 0.0f, wz = live ? zs[k] : 0.0f;

    // the brick's bounding sphere, from the axis values it covers (the grid has no empty brick: i0 < nx, j0 < ny, k0 < nz)
    float ccx = 0.0f, ccy = 0.0f, ccz = 0.0f, rad = 0.0f;
    if (cull && tid < 64u) {
        float lo[3], hi[3];
        const float* ax[3] = {xs, ys, zs};
        const uint32_t a0[3] = {i0, j0, k0}, a1[3] = {min(i0 + TS_BI, nx), min(j0 + TS_BJ, ny), min(k0 + TS_BK, nz)};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = hi[a] = ax[a][a0[a]];
            for (uint32_t e = a0[a] + 1u; e < a1[a]; e++) { lo[a] = fminf(lo[a], ax[a][e]); hi[a] = fmaxf(hi[a], ax[a][e]); }
        }
        ccx = 0.5f * (lo[0] + hi[0]); ccy = 0.5f * (lo[1] + hi[1]); ccz = 0.5f * (lo[2] + hi[2]);
        // half the box's diagonal, widened by 2^-10 for the roundings of the centre and of this line
        rad = (0.5f * len3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])) * (1.0f + TS_CULL_MARGIN);
    }

    const float Wf = (float)W, Hf = (float)H;
    const size_t HW = (size_t)H * W;
    uint32_t nf = 0, n_occ = 0;                        // n_near | n_free << 16; V <= 65535, so neither half carries
    uint32_t sum_r = 0, sum_g = 0, sum_b = 0;          // <= 65535 * 255
    float S = 0.0f;
    for (uint32_t b0 = 0; b0 < V; b0 += TS_CHUNK) {
        const uint32_t nb = min((uint32_t)TS_CHUNK, V - b0);
        __syncthreads();
        for (uint32_t e = tid; e < nb * 12u; e += TS_THREADS) P[e] = poses[(size_t)(b0 + e / 12u) * 16u + (e % 12u)];
        __syncthreads();
        if (tid < 64u) {                               // wave 0: one view per lane
            bool keep = lane < nb;
            if (cull && keep) {
                const float* Q = P + lane * 12u;
                const float dx = ccx - Q[3], dy = ccy - Q[7], dz = ccz - Q[11];
                const float L = len3(dx, dy, dz) + rad;
                const float n0 = len3(Q[0], Q[4], Q[8]), n1 = len3(Q[1], Q[5], Q[9]), n2 = len3(Q[2], Q[6], Q[10]);
                // behind the camera: q.z <= col2 . d + rad |col2| for every voxel of the brick
                const bool behind = ((Q[2] * dx + Q[6] * dy) + Q[10] * dz) + rad * n2 + TS_CULL_MARGIN * n2 * L < 0.0f;
                // the four frame planes: u < 0 <=> (fx col0 + cx col2) . d < 0 where q.z > 0; u >= W <=> (-fx col0 + (W - cx) col2) . d <= 0
                const bool left = plane_culls(Q, 0, fx, cx, dx, dy, dz, rad, fx * n0 + fabsf(cx) * n2, L);
                const bool right = plane_culls(Q, 0, -fx, Wf - cx, dx, dy, dz, rad, fx * n0 + fabsf(Wf - cx) * n2, L);
                const bool top = plane_culls(Q, 1, fy, cy, dx, dy, dz, rad, fy * n1 + fabsf(cy) * n2, L);
                const bool bottom = plane_culls(Q, 1, -fy, Hf - cy, dx, dy, dz, rad, fy * n1 + fabsf(Hf - cy) * n2, L);
                keep = !(behind || left || right || top || bottom);      // a NaN anywhere compares false: the view is kept
            }
            const unsigned long long km = __ballot(keep);
            if (keep) surv[__popcll(km & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0u) n_surv = (uint32_t)__popcll(km);
        }
        __syncthreads();
        if (!live) continue;
        const uint32_t ns = n_surv;
        for (uint32_t s_i = 0; s_i < ns; s_i++) {
            const uint32_t b = surv[s_i];
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
            const size_t pix = (size_t)(b0 + b) * HW + (size_t)py * W + px;
            const float t_surf = fabsf(packed[pix]);
            if (t_surf != t_surf) continue;
            const float t_vox = len3(dx, dy, dz);
            const float s = t_surf - t_vox;
            if (s < -trunc) {
                n_occ += 1u;
            } else if (s > trunc) {
                nf += 0x10000u;
            } else {
                nf += 1u;
                S = S + __fdiv_rn(s, trunc);
                if (FRAMES) {
                    const uint8_t* c = frames + pix * 3u;
                    sum_r += c[0]; sum_g += c[1]; sum_b += c[2];
                }
            }
        }
    }
    if (!live) return;
    const uint32_t n_near = nf & 0xffffu, n_free = nf >> 16, n_obs = n_near + n_free;
    const float tsdf = n_obs >= min_views ? __fdiv_rn(S + (float)n_free, (float)n_obs) : (n_occ > 0u ? -1.0f : 1.0f);
    const uint32_t at = (i * ny + j) * nz + k;                     // < 512^3
    u_out[at] = -tsdf;
    if (counts_out) counts_out[at] = make_uint2(nf, n_occ);        // (near, free, occluded, 0) as four uint16
    if (FRAMES && rgb_out) {
        const float fn = (float)n_near;
        rgb_out[3u * at + 0u] = n_near ? __fdiv_rn(__fdiv_rn((float)sum_r, fn), 255.0f) : 0.0f;
        rgb_out[3u * at + 1u] = n_near ? __fdiv_rn(__fdiv_rn((float)sum_g, fn), 255.0f) : 0.0f;
        rgb_out[3u * at + 2u] = n_near ? __fdiv_rn(__fdiv_rn((float)sum_b, fn), 255.0f) : 0.0f;
    }
}

constexpr int VC_THREADS = 256;

// one thread per vertex; (base, axis, t) as k_mesh_vertex_attrs finds them
__global__ __launch_bounds__(VC_THREADS) void k_tsdf_vertex_colors(const float* __restrict__ rgb, const uint16_t* __restrict__ counts,
                                                                   uint32_t nx, uint32_t ny, uint32_t nz, const float* __restrict__ verts,
                                                                   uint32_t V, float* __restrict__ colors, uint32_t* __restrict__ n_grey) {
    const uint32_t idx = blockIdx.x * VC_THREADS + threadIdx.x;
    bool grey = false;
    if (idx < V) {
        const int n[3] = {(int)nx, (int)ny, (int)nz};
        int base[3], q[3];
        float t = 0.0f;
        int axis = -1;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            float v = verts[3 * (uint64_t)idx + a];
            if (!__builtin_isfinite(v)) v = 0.0f;
            const float b = fminf(fmaxf(floorf(v), 0.0f), (float)(n[a] - 1));     // clamped as a float: the conversion cannot overflow
            base[a] = q[a] = (int)b;
            const float frac = __fsub_rn(v, b);
            if (axis < 0 && frac > 0.0f) { axis = a; t = frac; }
        }
        if (axis >= 0) q[axis] = min(base[axis] + 1, n[axis] - 1);
        const uint32_t pa = ((uint32_t)base[0] * ny + (uint32_t)base[1]) * nz + (uint32_t)base[2];
        const uint32_t pb = ((uint32_t)q[0] * ny + (uint32_t)q[1]) * nz + (uint32_t)q[2];
        const bool ha = counts[4u * pa] > 0, hb = counts[4u * pb] > 0;
        grey = !ha && !hb;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float ca = rgb[3u * pa + c], cb = rgb[3u * pb + c];
            colors[3 * (uint64_t)idx + c] = ha && hb ? __fadd_rn(ca, __fmul_rn(t, __fsub_rn(cb, ca))) : (ha ? ca : (hb ? cb : 0.5f));
        }
    }
    if (n_grey) {                                                  // integer adds: the count is the same whatever their order
        const unsigned long long gm = __ballot(grey);
        if ((threadIdx.x & 63u) == 0u && gm) atomicAdd(n_grey, (uint32_t)__popcll(gm));
    }
}

bool dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= TS_MAX_SIDE && ny <= TS_MAX_SIDE && nz <= TS_MAX_SIDE;
}

}  // namespace

extern "C" {

int lae_tsdf_fuse(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                  const float* xs, const float* ys, const float* zs, uint32_t nx, uint32_t ny, uint32_t nz, const uint8_t* frames,
                  float trunc, uint32_t min_views, float* u, uint16_t* counts, float* rgb, void* stream) {
    if (!packed || !poses || !xs || !ys || !zs || !u) return LAE_ENULL;
    if (rgb && !frames) return LAE_ENULL;
    if (V == 0 || V > 65535u || H < 1 || W < 1 || (uint64_t)H * W >= 0x80000000ull || !dims_ok(nx, ny, nz) || !(fx > 0.0f) ||
        !(fy > 0.0f) || !(cx == cx) || !(cy == cy) || !(trunc > 0.0f) || !(trunc <= 3.0e38f) || min_views == 0 ||
        (reinterpret_cast<uintptr_t>(counts) & 7u))
        return LAE_EINVAL;
    const char* e = getenv("LAE_TSDF_CULL");                       // 0: every view is walked for every brick (A/B; the same bytes)
    const int cull = !e || atoi(e) != 0;
    const dim3 grid(lae::cdiv(nz, TS_BK), lae::cdiv(ny, TS_BJ), lae::cdiv(nx, TS_BI));
    uint2* c2 = reinterpret_cast<uint2*>(counts);
    if (frames)
        k_tsdf_fuse<true><<<grid, TS_THREADS, 0, STREAM(stream)>>>(packed, poses, V, fx, fy, cx, cy, H, W, xs, ys, zs, nx, ny, nz, frames,
                                                                   trunc, min_views, cull, u, c2, rgb);
    else
        k_tsdf_fuse<false><<<grid, TS_THREADS, 0, STREAM(stream)>>>(packed, poses, V, fx, fy, cx, cy, H, W, xs, ys, zs, nx, ny, nz, nullptr,
                                                                    trunc, min_views, cull, u, c2, nullptr);
    return lae::check_launch("tsdf_fuse");
}

int lae_tsdf_vertex_colors(const float* rgb, const uint16_t* counts, uint32_t nx, uint32_t ny, uint32_t nz, const float* verts, uint32_t V,
                           float* colors, uint32_t* n_grey, void* stream) {
    if (!dims_ok(nx, ny, nz)) return LAE_EINVAL;
    if (n_grey) {
        hipError_t err = hipMemsetAsync(n_grey, 0, sizeof(uint32_t), STREAM(stream));
        if (err != hipSuccess) { lae::set_last_error("tsdf_vertex_colors/memset", err); return LAE_ELAUNCH; }
    }
    if (V == 0) return LAE_OK;
    if (!rgb || !counts || !verts || !colors) return LAE_ENULL;
    k_tsdf_vertex_colors<<<lae::cdiv(V, VC_THREADS), VC_THREADS, 0, STREAM(stream)>>>(rgb, counts, nx, ny, nz, verts, V, colors, n_grey);
    return lae::check_launch("tsdf_vertex_colors");
}

}  // extern "C"
