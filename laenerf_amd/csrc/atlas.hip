// atlas.hip -- a per-triangle texture atlas baked on the device: the texels of a closed-form layout placed on their triangles, the
// colours of rendered or edited views fused into them, and the atlas packed as an image ("Textured export";
// atlas.py restates the three kernels in numpy).  The reference exports geometry only (nerf/utils.py:722-741).
//
// THE LAYOUT.  Triangles are packed two to a square cell of n x n texels (n = cell >= 4): cells = ceil(T / 2), cpr = ceil(sqrt(cells))
// cells per row, the image is S x S with S = cpr * n; triangle t lives in cell t / 2, half t & 1; cell c has its origin at texel
// ((c % cpr) * n, (c / cpr) * n).  Texels are numbered CELL-MAJOR: id = c * n * n + j * n + i for texel (i, j) of cell c, so a
// wavefront's texels share one or two triangles (n = 8: exactly one cell).  With m = n - 3, in texel-centre coordinates of the cell:
//   half 0 owns i + j <= n - 1, UV corners (0, 0), (m, 0), (0, m);       a = i,         b = j
//   half 1 owns i + j >= n,     UV corners are the point mirror;        a = n - 1 - i, b = n - 1 - j
// A bilinear lookup at a point with x + y <= m touches texels with i + j <= m + 1 = n - 2 only, so the halves never read each
// other's texels; every owned texel, gutter included, is placed by the AFFINE EXTENSION of the half's UV -> triangle map.
//
// lae_atlas_texels, per texel of triangle t = (i0, i1, i2), v = the vertices, every statement one fp32 rounding (the library is
// built with -ffp-contract=off; divisions are __fdiv_rn, roots sqrtf):
//   b1 = float(a) / float(m), b2 = float(b) / float(m); e1 = v[i1] - v[i0], e2 = v[i2] - v[i0];
//   pos = (v[i0] + b1 * e1) + b2 * e2                                    (per component)
//   c   = e1 x e2: c.x = e1.y * e2.z - e1.z * e2.y, c.y = e1.z * e2.x - e1.x * e2.z, c.z = e1.x * e2.y - e1.y * e2.x
//   len = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);  nrm = c / len if len > 0 and finite, else 0 (a zero-area triangle: its texels
//         are flagged by the zero normal -- no view counts for them in lae_atlas_fuse_views, they come out grey)
//   g   = (vn[i0] + b1 * (vn[i1] - vn[i0])) + b2 * (vn[i2] - vn[i0]), gl = its length as above;
//   dirs = -(g / gl) if gl > 0 and finite (and vertex normals are given), else -nrm, else (0, 0, 1) where nrm is 0 too
//   owner = t.  Texels of the unused half of an odd T's last cell: owner -1, the rest 0.  A triangle with a vertex index outside
//   [0, V) is treated as zero-area with pos 0 (nothing is read out of bounds).
//
// lae_atlas_fuse_views, per (texel, view) in ascending view order -- the projection is lae_tsdf_fuse's, statement for statement:
//   d = p - o, q = R^T d.  q.z <= 0: rejected.  u = fx q.x / q.z + cx, v = fy q.y / q.z + cy; outside [0, W) x [0, H): rejected.
//   Pixel (floor u, floor v); t = |d|; s = t_surf - t with t_surf = |packed|; a NaN t_surf: rejected.
//   The view counts iff |s| <= trunc and (-((nrm.x d.x + nrm.y d.y) + nrm.z d.z)) / t > min_cos; then the pixel's three bytes are
//   added to three uint32 sums and n += 1.
//   rgb = float(sum) / float(n) / 255; n == 0: 0.5, and the texel is counted in *n_grey (zeroed by the call; integer adds).
//   Unowned texels: rgb 0, count 0, not counted.
// A thread owns its texel: no atomics apart from the grey count, a fixed order, and two calls give the same bytes.
// THE CULL.  A wave holds 64 consecutive texels, i.e. at most ATLAS_MAX_TRIS triangles.  Per (wave, view) -- one view per lane, as
// in k_tsdf_fuse -- the bounding sphere of the wave's owned texel positions is tested against the camera's half-space and the four
// frame planes, and every distinct normal of the wave against min_cos with the sphere's margin; survivors are compacted by ballot,
// so the sums keep their order.  LAE_ATLAS_CULL=0 (read per call) walks every view; the bytes are the same.
//
// lae_atlas_pack: image[Y, X] of the S x S x 3 uint8 texture = the bytes of the texel at (X, Y) by lae_eval_view's rule
// (clip(x, 0, 1) * 255 truncated, NaN -> 0); unowned texels and the cells past `cells` are 0.
#include <stdlib.h>

#include "lae_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int AT_THREADS = 256, AT_WAVES = AT_THREADS / 64, AT_CHUNK = LAE_TSDF_POSE_CHUNK;
static_assert(AT_CHUNK == 64, "the cull is one view per lane");
constexpr uint32_t ATLAS_MAX_SIDE = 16384u;
constexpr int ATLAS_MAX_TRIS = 16;                     // distinct triangles in 64 consecutive texels: at most 8 (cell = 4 or 5)
constexpr float AT_CULL_MARGIN = 0x1p-10f;             // k_tsdf_fuse's: relative to the magnitude of the tested sum's terms

__device__ __forceinline__ float len3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// cells, cells per row and the image side of T triangles; false where the atlas does not fit
bool layout_of(uint32_t T, uint32_t cell, uint32_t* cells, uint32_t* cpr, uint32_t* S) {
    if (T == 0 || cell < 4u || cell > ATLAS_MAX_SIDE) return false;
    const uint32_t c = T / 2u + (T & 1u);
    uint32_t r = (uint32_t)sqrt((double)c);
    while ((uint64_t)r * r < c) r++;
    while (r > 1u && (uint64_t)(r - 1u) * (r - 1u) >= c) r--;
    if ((uint64_t)r * cell > ATLAS_MAX_SIDE) return false;
    *cells = c; *cpr = r; *S = r * cell;
    return true;
}

__global__ __launch_bounds__(AT_THREADS) void k_atlas_texels(const float* __restrict__ verts, uint32_t V, const int32_t* __restrict__ tris,
                                                              uint32_t T, const float* __restrict__ vnrm, uint32_t n, uint32_t n_texels,
                                                              float* __restrict__ pos, float* __restrict__ nrm, float* __restrict__ dirs,
                                                              int32_t* __restrict__ owner) {
    const uint32_t id = blockIdx.x * AT_THREADS + threadIdx.x;
    if (id >= n_texels) return;
    const uint32_t nn = n * n, c = id / nn, r = id - c * nn, j = r / n, i = r - j * n;
    const uint32_t half = (i + j <= n - 1u) ? 0u : 1u, t = 2u * c + half;
    float P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f}, D[3] = {0.0f, 0.0f, 0.0f};
    int32_t own = -1;
    if (t < T) {
        own = (int32_t)t;
        D[2] = 1.0f;
        const uint32_t i0 = (uint32_t)tris[3u * (size_t)t], i1 = (uint32_t)tris[3u * (size_t)t + 1u], i2 = (uint32_t)tris[3u * (size_t)t + 2u];
        if (i0 < V && i1 < V && i2 < V) {
            const float fm = (float)(n - 3u);
            const float b1 = __fdiv_rn((float)(half ? n - 1u - i : i), fm), b2 = __fdiv_rn((float)(half ? n - 1u - j : j), fm);
            float e1[3], e2[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float v0 = verts[3u * (size_t)i0 + a];
                e1[a] = verts[3u * (size_t)i1 + a] - v0;
                e2[a] = verts[3u * (size_t)i2 + a] - v0;
                P[a] = (v0 + b1 * e1[a]) + b2 * e2[a];
            }
            const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            const float len = len3(cx, cy, cz);
            const bool ok = len > 0.0f && len <= 3.0e38f;
            if (ok) { N[0] = __fdiv_rn(cx, len); N[1] = __fdiv_rn(cy, len); N[2] = __fdiv_rn(cz, len); }
            float g[3] = {0.0f, 0.0f, 0.0f};
            if (vnrm) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const float g0 = vnrm[3u * (size_t)i0 + a];
                    g[a] = (g0 + b1 * (vnrm[3u * (size_t)i1 + a] - g0)) + b2 * (vnrm[3u * (size_t)i2 + a] - g0);
                }
            }
            const float gl = len3(g[0], g[1], g[2]);
            if (gl > 0.0f && gl <= 3.0e38f) {
#pragma unroll
                for (int a = 0; a < 3; a++) D[a] = -__fdiv_rn(g[a], gl);
            } else if (ok) {
#pragma unroll
                for (int a = 0; a < 3; a++) D[a] = -N[a];
            }
            // a non-finite vertex gives non-finite positions; the normal test above leaves such a triangle zero-area
#pragma unroll
            for (int a = 0; a < 3; a++) if (!__builtin_isfinite(P[a])) P[a] = 0.0f;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        pos[3u * (size_t)id + a] = P[a];
        nrm[3u * (size_t)id + a] = N[a];
        dirs[3u * (size_t)id + a] = D[a];
    }
    owner[id] = own;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int32_t wave_min_i(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int32_t wave_max_i(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// k_tsdf_fuse's plane test: true when no point within `rad` of the centre can project to the tested side's inside
__device__ __forceinline__ bool plane_culls(const float* Q, int ka, float a, float b, float dx, float dy, float dz, float rad, float term,
                                            float L) {
    const float mx = a * Q[ka] + b * Q[2], my = a * Q[4 + ka] + b * Q[6], mz = a * Q[8 + ka] + b * Q[10];
    return (mx * dx + my * dy + mz * dz) + rad * len3(mx, my, mz) + AT_CULL_MARGIN * term * L < 0.0f;
}

__global__ __launch_bounds__(AT_THREADS) void k_atlas_fuse(const float* __restrict__ packed, const float* __restrict__ poses, uint32_t V,
                                                            float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                                            const uint8_t* __restrict__ frames, const float* __restrict__ pos,
                                                            const float* __restrict__ nrm, const int32_t* __restrict__ owner,
                                                            uint32_t n_texels, float trunc, float min_cos, int cull,
                                                            float* __restrict__ rgb_out, uint16_t* __restrict__ counts_out,
                                                            uint32_t* __restrict__ n_grey) {
    __shared__ float P[AT_CHUNK * 12];
    __shared__ uint32_t surv[AT_WAVES][AT_CHUNK];       // per wave: the chunk's surviving views, ascending
    __shared__ uint32_t n_surv[AT_WAVES];
    __shared__ float wn[AT_WAVES][ATLAS_MAX_TRIS][3];   // per wave: the normals of its triangles
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t id = blockIdx.x * AT_THREADS + tid;
    const int32_t own = id < n_texels ? owner[id] : -1;
    const bool live = own >= 0;
    float wx = 0.0f, wy = 0.0f, wz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (live) {
        wx = pos[3u * (size_t)id]; wy = pos[3u * (size_t)id + 1u]; wz = pos[3u * (size_t)id + 2u];
        nx = nrm[3u * (size_t)id]; ny = nrm[3u * (size_t)id + 1u]; nz = nrm[3u * (size_t)id + 2u];
    }

    // the wave's bounding sphere and its triangles' normals
    float ccx = 0.0f, ccy = 0.0f, ccz = 0.0f, rad = 0.0f;
    uint32_t n_tri = 0;
    bool any_live = true, cones = false;
    if (cull) {
        const float big = 3.0e38f;
        const float lox = wave_min(live ? wx : big), loy = wave_min(live ? wy : big), loz = wave_min(live ? wz : big);
        const float hix = wave_max(live ? wx : -big), hiy = wave_max(live ? wy : -big), hiz = wave_max(live ? wz : -big);
        const int32_t t_lo = wave_min_i(live ? own : 0x7fffffff), t_hi = wave_max_i(own);
        any_live = t_hi >= 0;
        if (any_live) {
            ccx = 0.5f * (lox + hix); ccy = 0.5f * (loy + hiy); ccz = 0.5f * (loz + hiz);
            const float amax = fmaxf(fmaxf(fmaxf(fabsf(lox), fabsf(hix)), fmaxf(fabsf(loy), fabsf(hiy))), fmaxf(fabsf(loz), fabsf(hiz)));
            // half the box's diagonal, widened by 2^-10 and by 2^-20 of the coordinates for the roundings of the centre and of this line
            rad = (0.5f * len3(hix - lox, hiy - loy, hiz - loz)) * (1.0f + AT_CULL_MARGIN) + 0x1p-20f * amax;
            n_tri = (uint32_t)(t_hi - t_lo) + 1u;
            cones = n_tri <= (uint32_t)ATLAS_MAX_TRIS && min_cos >= 0.0f;
            if (cones) {
                if (lane < n_tri) { wn[wv][lane][0] = 2.0f; wn[wv][lane][1] = 0.0f; wn[wv][lane][2] = 0.0f; }   // no texel of it here: skipped
            }
        }
        __syncthreads();
        if (any_live && cones && live) {                 // lanes of one triangle write the same three values
            const uint32_t slot = (uint32_t)(own - t_lo);
            wn[wv][slot][0] = nx; wn[wv][slot][1] = ny; wn[wv][slot][2] = nz;
        }
    }

    const float Wf = (float)W, Hf = (float)H;
    const size_t HW = (size_t)H * W;
    uint32_t cnt = 0, sum_r = 0, sum_g = 0, sum_b = 0;   // <= 65535 * 255
    for (uint32_t b0 = 0; b0 < V; b0 += AT_CHUNK) {
        const uint32_t nb = min((uint32_t)AT_CHUNK, V - b0);
        __syncthreads();
        for (uint32_t e = tid; e < nb * 12u; e += AT_THREADS) P[e] = poses[(size_t)(b0 + e / 12u) * 16u + (e % 12u)];
        __syncthreads();
        {                                                // every wave: one view per lane against its own sphere
            bool keep = lane < nb && any_live;
            if (cull && keep) {
                const float* Q = P + lane * 12u;
                const float dx = ccx - Q[3], dy = ccy - Q[7], dz = ccz - Q[11];
                const float dc = len3(dx, dy, dz), L = dc + rad;
                const float n0 = len3(Q[0], Q[4], Q[8]), n1 = len3(Q[1], Q[5], Q[9]), n2 = len3(Q[2], Q[6], Q[10]);
                const bool behind = ((Q[2] * dx + Q[6] * dy) + Q[10] * dz) + rad * n2 + AT_CULL_MARGIN * n2 * L < 0.0f;
                const bool left = plane_culls(Q, 0, fx, cx, dx, dy, dz, rad, fx * n0 + fabsf(cx) * n2, L);
                const bool right = plane_culls(Q, 0, -fx, Wf - cx, dx, dy, dz, rad, fx * n0 + fabsf(Wf - cx) * n2, L);
                const bool top = plane_culls(Q, 1, fy, cy, dx, dy, dz, rad, fy * n1 + fabsf(cy) * n2, L);
                const bool bottom = plane_culls(Q, 1, -fy, Hf - cy, dx, dy, dz, rad, fy * n1 + fabsf(Hf - cy) * n2, L);
                // back-facing: a texel counts only where -(N . d) > min_cos |d|.  Over the sphere -(N . d) <= -(N . dc) + rad and
                // |d| >= |dc| - rad; every triangle of the wave must miss by the margin (|N| <= 1; the unused slots hold |N| = 2)
                bool away = false;
                if (cones && dc > rad) {
                    away = true;
                    for (uint32_t k = 0; k < n_tri; k++) {
                        const float ax = wn[wv][k][0], ay = wn[wv][k][1], az = wn[wv][k][2];
                        if (ax > 1.5f) continue;                          // no texel of this triangle in the wave
                        const float facing = -((ax * dx + ay * dy) + az * dz) + rad;
                        away = away && (facing + AT_CULL_MARGIN * L < min_cos * (dc - rad));
                    }
                }
                keep = !(behind || left || right || top || bottom || away);      // a NaN anywhere compares false: the view is kept
            }
            const unsigned long long km = __ballot(keep);
            if (keep) surv[wv][__popcll(km & ((1ull << lane) - 1ull))] = lane;
            if (lane == 0u) n_surv[wv] = (uint32_t)__popcll(km);
        }
        __syncthreads();
        if (!live) continue;
        const uint32_t ns = n_surv[wv];
        for (uint32_t s_i = 0; s_i < ns; s_i++) {
            const uint32_t b = surv[wv][s_i];
            const float* Q = P + b * 12u;                          // rows 0..2 of [R | o]
            const float dx = wx - Q[3], dy = wy - Q[7], dz = wz - Q[11];
            const float qz = (dx * Q[2] + dy * Q[6]) + dz * Q[10];
            if (!(qz > 0.0f)) continue;
            const float qx = (dx * Q[0] + dy * Q[4]) + dz * Q[8];
            const float qy = (dx * Q[1] + dy * Q[5]) + dz * Q[9];
            const float u = __fdiv_rn(fx * qx, qz) + cx, v = __fdiv_rn(fy * qy, qz) + cy;
            if (!(u >= 0.0f && u < Wf && v >= 0.0f && v < Hf)) continue;
            const uint32_t px = min((uint32_t)u, W - 1u), py = min((uint32_t)v, H - 1u);
            const size_t pix = (size_t)(b0 + b) * HW + (size_t)py * W + px;
            const float t_surf = fabsf(packed[pix]);
            if (t_surf != t_surf) continue;
            const float t_tex = len3(dx, dy, dz);
            const float s = t_surf - t_tex;
            if (!(fabsf(s) <= trunc)) continue;
            const float cosv = __fdiv_rn(-((nx * dx + ny * dy) + nz * dz), t_tex);
            if (!(cosv > min_cos)) continue;
            const uint8_t* c = frames + pix * 3u;
            sum_r += c[0]; sum_g += c[1]; sum_b += c[2];
            cnt += 1u;
        }
    }
    if (id < n_texels) {
        const float fn = (float)cnt;
        rgb_out[3u * (size_t)id + 0u] = live ? (cnt ? __fdiv_rn(__fdiv_rn((float)sum_r, fn), 255.0f) : 0.5f) : 0.0f;
        rgb_out[3u * (size_t)id + 1u] = live ? (cnt ? __fdiv_rn(__fdiv_rn((float)sum_g, fn), 255.0f) : 0.5f) : 0.0f;
        rgb_out[3u * (size_t)id + 2u] = live ? (cnt ? __fdiv_rn(__fdiv_rn((float)sum_b, fn), 255.0f) : 0.5f) : 0.0f;
        if (counts_out) counts_out[id] = (uint16_t)cnt;
    }
    if (n_grey) {                                                  // integer adds: the count is the same whatever their order
        const unsigned long long gm = __ballot(live && cnt == 0u);
        if (lane == 0u && gm) atomicAdd(n_grey, (uint32_t)__popcll(gm));
    }
}

// `clip(x, 0, 1) * 255`, truncated (evaluate.hip to_u8); NaN -> 0
__device__ __forceinline__ uint8_t color_u8(float x) { return (uint8_t)(int)__fmul_rn(lae::clampf(x, 0.0f, 1.0f), 255.0f); }

// one thread per pixel of the image, X fastest: a wave writes a run of 192 bytes and reads n-texel runs of the cell rows
__global__ __launch_bounds__(AT_THREADS) void k_atlas_pack(const float* __restrict__ rgb, const int32_t* __restrict__ owner, uint32_t cells,
                                                            uint32_t n, uint32_t cpr, uint8_t* __restrict__ image) {
    const uint32_t S = cpr * n;
    const uint32_t at = blockIdx.x * AT_THREADS + threadIdx.x;     // < 2^28
    if (at >= S * S) return;
    const uint32_t Y = at / S, X = at - Y * S;
    const uint32_t c = (Y / n) * cpr + X / n;
    uint8_t r = 0, g = 0, b = 0;
    if (c < cells) {
        const uint32_t id = c * n * n + (Y % n) * n + X % n;
        if (owner[id] >= 0) { r = color_u8(rgb[3u * (size_t)id]); g = color_u8(rgb[3u * (size_t)id + 1u]); b = color_u8(rgb[3u * (size_t)id + 2u]); }
    }
    image[3u * (size_t)at] = r; image[3u * (size_t)at + 1u] = g; image[3u * (size_t)at + 2u] = b;
}

}  // namespace

extern "C" {

int lae_atlas_layout(uint32_t T, uint32_t cell, uint32_t* cells, uint32_t* cpr, uint32_t* S) {
    if (!cells || !cpr || !S) return LAE_ENULL;
    return layout_of(T, cell, cells, cpr, S) ? LAE_OK : LAE_EINVAL;
}

int lae_atlas_texels(const float* verts, uint32_t V, const int32_t* tris, uint32_t T, const float* normals, uint32_t cell, float* pos,
                     float* nrm, float* dirs, int32_t* owner, void* stream) {
    if (!verts || !tris || !pos || !nrm || !dirs || !owner) return LAE_ENULL;
    uint32_t cells, cpr, S;
    if (V == 0 || V > 0x7fffffffu || !layout_of(T, cell, &cells, &cpr, &S)) return LAE_EINVAL;
    const uint32_t n_texels = cells * cell * cell;                 // <= S * S <= 2^28
    k_atlas_texels<<<lae::cdiv(n_texels, AT_THREADS), AT_THREADS, 0, STREAM(stream)>>>(verts, V, tris, T, normals, cell, n_texels, pos, nrm,
                                                                                        dirs, owner);
    return lae::check_launch("atlas_texels");
}

int lae_atlas_fuse_views(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                         const uint8_t* frames, const float* pos, const float* nrm, const int32_t* owner, uint32_t n_texels, float trunc,
                         float min_cos, float* rgb, uint16_t* counts, uint32_t* n_grey, void* stream) {
    if (!packed || !poses || !frames || !pos || !nrm || !owner || !rgb) return LAE_ENULL;
    if (V == 0 || V > 65535u || H < 1 || W < 1 || (uint64_t)H * W >= 0x80000000ull || n_texels == 0 ||
        n_texels > ATLAS_MAX_SIDE * ATLAS_MAX_SIDE || !(fx > 0.0f) || !(fy > 0.0f) || !(cx == cx) || !(cy == cy) || !(trunc > 0.0f) ||
        !(trunc <= 3.0e38f) || !(min_cos >= 0.0f) || !(min_cos < 1.0f))
        return LAE_EINVAL;
    if (n_grey) {
        hipError_t err = hipMemsetAsync(n_grey, 0, sizeof(uint32_t), STREAM(stream));
        if (err != hipSuccess) { lae::set_last_error("atlas_fuse_views/memset", err); return LAE_ELAUNCH; }
    }
    const char* e = getenv("LAE_ATLAS_CULL");                      // 0: every view is walked for every texel (A/B; the same bytes)
    const int cull = !e || atoi(e) != 0;
    k_atlas_fuse<<<lae::cdiv(n_texels, AT_THREADS), AT_THREADS, 0, STREAM(stream)>>>(packed, poses, V, fx, fy, cx, cy, H, W, frames, pos, nrm,
                                                                                      owner, n_texels, trunc, min_cos, cull, rgb, counts,
                                                                                      n_grey);
    return lae::check_launch("atlas_fuse_views");
}

int lae_atlas_pack(const float* rgb, const int32_t* owner, uint32_t T, uint32_t cell, uint8_t* image, void* stream) {
    if (!rgb || !owner || !image) return LAE_ENULL;
    uint32_t cells, cpr, S;
    if (!layout_of(T, cell, &cells, &cpr, &S)) return LAE_EINVAL;
    k_atlas_pack<<<lae::cdiv((uint64_t)S * S, AT_THREADS), AT_THREADS, 0, STREAM(stream)>>>(rgb, owner, cells, cell, cpr, image);
    return lae::check_launch("atlas_pack");
}

}  // extern "C"
