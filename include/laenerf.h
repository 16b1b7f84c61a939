/*
 * laenerf.h -- C ABI of the MI355X-native LAENeRF / torch-ngp hot path.
 *
 * One symbol per backend function of the reference's four pybind11 modules
 * (_raymarching, _gridencoder, _shencoder, _ffmlp).  Every entry point
 *   - takes raw DEVICE pointers + sizes + scalars (no torch types),
 *   - borrows the pointers for the duration of the call only (the caller owns
 *     and pre-allocates every output / workspace, exactly like the reference's
 *     autograd.Functions do),
 *   - enqueues its kernels on `stream` (a hipStream_t passed as void*; NULL =
 *     the legacy default stream, which is what the reference launched on),
 *   - never synchronises the host and never frees or reallocates memory the caller
 *     passed in.  LIBRARY-OWNED WORKSPACES (the counterpart of the reference's
 *     process-global split-K streams + CUTLASS workspace, ffmlp.cu:711-740,
 *     cutlass_matmul.h:335-352): the fp32 dW slabs of the MLP backward, the
 *     level-major staging of the [B, L*C] grid-encoder layouts and the bin queues of
 *     the grid backward live in grow-only device buffers, one set per device.
 *     WARM-UP CONTRACT: the first call at a new largest size hipMalloc()s (a host-
 *     side, possibly blocking, call); steady state allocates nothing.  A buffer
 *     that is outgrown is retired, NOT freed -- kernels in flight and captured HIP
 *     graphs keep using the address they were given -- until lae_free_workspaces().
 *     Growth is refused (LAE_ELAUNCH, message in lae_last_error) while `stream` is
 *     being captured: run the call once eagerly at its largest size before
 *     capturing.  The library acts on the CURRENT device of the calling thread;
 *     the caller makes the device of its pointers current (hipSetDevice) first,
 *   - returns LAE_OK (0) or a negative LAE_E* code; the Python shim turns a
 *     non-zero code into RuntimeError (the reference threw c10::Error /
 *     std::runtime_error for the same conditions).
 *
 * All tensors are dense row-major ("contiguous") exactly as the reference
 * requires (CHECK_CONTIGUOUS, gridencoder.cu:455-459).
 *
 * Reference interface replaced, per symbol: see the comment above each
 * prototype (paths relative to the reference checkout).
 */
#ifndef LAENERF_H
#define LAENERF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported from liblaenerf_hip.so (the library is built with -fvisibility=hidden) */
#if defined(__GNUC__) || defined(__clang__)
#define LAE_API __attribute__((visibility("default")))
#else
#define LAE_API
#endif

#define LAE_OK 0
#define LAE_EINVAL (-1)     /* unsupported template parameter / bad argument  */
#define LAE_ELAUNCH (-2)    /* hipGetLastError() != hipSuccess after a launch */
#define LAE_ENULL (-3)      /* required pointer is NULL                       */

/* element type of the hash table / encoder outputs / encoder grads */
#define LAE_F32 0
#define LAE_F16 1

/* grid types / interpolation (gridencoder/grid.py:14-22) */
#define LAE_GRID_HASH 0
#define LAE_GRID_TILED 1
#define LAE_INTERP_LINEAR 0
#define LAE_INTERP_SMOOTHSTEP 1

/* ffmlp activations (ffmlp/ffmlp.py:89-96, ffmlp/src/utils.h:29-37) */
#define LAE_ACT_RELU 0
#define LAE_ACT_EXPONENTIAL 1
#define LAE_ACT_SINE 2
#define LAE_ACT_SIGMOID 3
#define LAE_ACT_SQUAREPLUS 4
#define LAE_ACT_SOFTPLUS 5
#define LAE_ACT_NONE 6

/* library identification: returns the static string "laenerf-hip gfx950 " LAE_ABI_TAG.  The tag changes whenever a
 * signature of this header changes incompatibly (abi2: round 2 added pointer arguments in the middle of the optimizer /
 * grid-backward / frame entry points; abi3: round 3, optimizer state words and the compositing step; abi4: round 4, lae_ffmlp_set_mode values 2 and 16-18 removed; abi5: round 5, lae_render_frame_mode, frame-loop degrade path; abi6: round 6, lae_render_frame_last_status, lae_ffmlp_forward leaves forward_buffer untouched where the backward recomputes; abi7: lae_sample_train_batch, lae_march_rays_train_limit; abi8: lae_sample_train_batch_weighted, lae_error_map_update; abi9: lae_recolor_compact, lae_recolor_compose; abi10: lae_sample_edit_view, lae_style_loss_forward_dev, lae_style_loss_backward_dev; abi11: lae_distill_compose, lae_error_map_seed; abi12: lae_marching_cubes_scratch_bytes, lae_marching_cubes_count, lae_marching_cubes_emit; abi13: lae_style_loss_backward_image_dev, lae_style_image_scratch_bytes, lae_style_image_forward, lae_style_image_backward; abi14: lae_ema_update_gated, lae_eval_view, lae_lpips_head; abi16: the depth term of the compositing step and of its backward; abi17: the distortion term of the compositing forward, backward and step; abi18: lae_mesh_vertex_attrs, lae_mesh_pack_ply; abi19: lae_nnfm_pack, lae_nnfm_match, lae_nnfm_loss_forward, lae_nnfm_loss_backward and their *_bytes helpers; abi20: lae_rayreg_build, lae_rayreg_query, lae_rayreg_supervise and their *_bytes helpers; abi21: lae_style_loss_forward_dev_w, lae_style_loss_backward_image_dev_w, lae_ref_terms_forward, lae_ref_terms_backward, lae_ref_terms_scratch_bytes; abi22: the colour criteria and the opacity entropy of the compositing step, lae_colour_loss_forward, lae_error_map_update_crit; abi23: pixel weights and a second target in the compositing step, lae_ref_distill_init, lae_ref_distill_scatter; abi24: lae_grid_input_grad, lae_pose_ray_grad, lae_pose_step; abi25: lae_sample_train_batch_gain, lae_sample_train_batch_weighted_gain, lae_exposure_step, lae_exposure_publish; abi26: lae_consistency_pair; abi27: lae_components_label, lae_components_sizes, lae_components_filter; added under abi27 without touching an existing prototype: lae_sample_train_batch_patch, lae_lpips_head_grad, lae_patch_pack, lae_patch_unpack_grad, lae_ssim_scratch_doubles, lae_ssim, lae_ssim_patch_forward, lae_ssim_patch_backward, lae_tsdf_fuse, lae_tsdf_vertex_colors, lae_undistort_map, lae_distort_map, lae_remap, lae_atlas_layout, lae_atlas_texels, lae_atlas_fuse_views, lae_atlas_pack -- a binding that needs them also checks that the library exports them; abi28: one lae_composite_rays_train_step whose loss terms are structs (lae_depth_term, lae_dist_term, lae_crit_term, lae_weight_term) in place of five cumulative entries, grad_depth / depth / grad_dist / dist on lae_composite_rays_train_backward_blend_ex and dist on lae_composite_rays_train_forward_blend in place of their _depth / _dist entries; added under abi28 without touching an existing prototype: lae_simplify_keys, lae_simplify_pairs, lae_simplify_reduce, lae_simplify_first, lae_simplify_compact, lae_region_warp, lae_region_occupancy, lae_insert_route_scratch_bytes, lae_insert_route, lae_insert_blend, lae_insert_occupancy -- a binding that needs them also checks that the library exports them).  A binding compares
 * it with the tag it was written against BEFORE the first call: a stale .so used through newer prototypes would misalign
 * arguments silently (laenerf_amd/_lib.py does, and rebuilds or raises). */
#define LAE_ABI_TAG "abi28"
LAE_API const char* lae_version(void);
/* last HIP error string recorded by a failed launch in this thread (or "") */
LAE_API const char* lae_last_error(void);

/* ------------------------------------------------------------------ */
/* _raymarching  (raymarching/src/raymarching.h:7-20, bindings.cpp:5-20) */
/* ------------------------------------------------------------------ */

/* raymarching.cu:148-156  near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars) */
LAE_API int lae_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb,
                           uint32_t N, float min_near, float* nears, float* fars, void* stream);

/* nerf/utils.py:61-153  get_rays(poses, intrinsics, H, W, N, ...): MI355X-native -- the ray generation of the data loader
 * (meshgrid + gather + stack + normalise + matmul, ~15 torch launches) as one kernel.  poses [B,4,4] cam2world, row-major;
 * inds [B,N] int64 flat pixel indices h*W+w with batch stride `inds_batch_stride` elements (0: one index row shared by all
 * poses, the reference's `inds.expand([B, N])`), or NULL for every pixel in order (then N must equal H*W).  perturb != 0
 * subtracts (off_x, off_y) from the pixel centre (`perturb_ray_dirs`, :133-136).  rays_o, rays_d [B,N,3].  aabb != NULL
 * additionally writes the near_far_from_aabb interval (raymarching.cu:91-145) of every ray to nears, fars [B,N]. */
LAE_API int lae_get_rays(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                 const int64_t* inds, uint64_t inds_batch_stride, uint32_t N, int perturb, float off_x, float off_y,
                 float* rays_o, float* rays_d, const float* aabb, float min_near, float* nears, float* fars, void* stream);

/* One training batch drawn from a device-resident image stack (the data loader of nerf/provider.py:294-343 + the
 * pixel gather and background blend of Trainer.train_step, nerf/utils.py:560-580), in one pass.
 * images [n_img, H, W, C], C in {3, 4}, dtype LAE_IMG_U8 (value / 255 through a 256-entry table), LAE_IMG_F16 or
 * LAE_IMG_F32; poses [n_img, 4, 4] cam2world; one intrinsics (fx, fy, cx, cy) for all images.
 * RNG: u(ray, word) = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *   (step & 0xffffffff, ray, word, 0), where step = *step_counter (int64, device) read at the start of the call.
 *   pixel  = (u(ray, 0) * (uint64)(H * W)) >> 32
 *   image  = (u(r, 1) * (uint64)n_img) >> 32 with r = 0xffffffff in LAE_BATCH_IMAGE mode (one image per batch,
 *            the reference's batch_size = 1 loader) and r = ray in LAE_BATCH_ALL mode (an image per ray)
 *   bg_c   = (u(ray, 2 + c) >> 8) * 2^-24, c = 0, 1, 2 (LAE_BG_RANDOM only)
 *   The reference shuffles the image order once per epoch; here the image is drawn i.i.d. per batch.
 * Rays, nears and fars are bit-identical to lae_get_rays(poses + 16 * image, ..., inds = &pixel, aabb, min_near)
 * (one shared device function).  gt = rgb (C == 3) or rgb * a + bg * (1 - a) (C == 4; three roundings, no contraction,
 * bg = 1 under LAE_BG_WHITE), after sRGB -> linear of rgb when srgb_to_linear != 0.  bg_out [N,3] (LAE_BG_RANDOM
 * only, may be NULL otherwise) receives the drawn background, inds [N] int64 = image * H * W + pixel.  A second
 * launch adds 1 to *step_counter after every ray has read it: a replayed graph draws a new batch each time. */
#define LAE_IMG_U8 0
#define LAE_IMG_F16 1
#define LAE_IMG_F32 2
#define LAE_BATCH_IMAGE 0
#define LAE_BATCH_ALL 1
#define LAE_BG_WHITE 0
#define LAE_BG_RANDOM 1
LAE_API int lae_sample_train_batch(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                           const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                           const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                           int srgb_to_linear, float* rays_o, float* rays_d, float* nears, float* fars, float* gt,
                           float* bg_out, int64_t* inds, void* stream);

/* The error-map sampler (the reference's --error_map, nerf/utils.py:112-124, and LAENeRF's --use_error_maps): the batch of
 * lae_sample_train_batch (LAE_BATCH_IMAGE mode) with the pixels drawn by a per-image map of 128 x 128 cell weights.
 * error_map [n_img, 16384] fp32 (row-major cells c = cx * 128 + cy); cells_out [N] int32; N <= 16384 (else LAE_EINVAL).
 * u(r, word) and step as above; the same step protocol (read at the start, advanced by a trailing one-thread launch).
 *   image  = (u(0xffffffff, 1) * (uint64)n_img) >> 32 (the uniform sampler's image at the same step)
 *   cells: torch.multinomial(map[image], N, replacement=False)'s algorithm, key = w / E with E ~ Exp(1), top N:
 *     v = word 0 of Philox4x32-10 with counter (step, c, 0, 1) (counter word 3 = 1: apart from the per-ray draws)
 *     u = ((v >> 8) + 0.5) * 2^-24 in (0, 1), i.e. j * 2^-25 with the odd integer j = 2 * (v >> 8) + 1
 *     E = -ln(u), computed from j, every step one fp32 rounding (no contraction), never libm:
 *       p = bit length of j; if 2 j^2 < 2^(2p): p -= 1                 (j / 2^p in [sqrt(1/2), sqrt(2)))
 *       f = float(j - 2^p) * 2^-p (exact), e = float(p - 25), z = f * f
 *       P = 7.0376836292e-2; P = P * f + c for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1,
 *           -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1)   (Cephes logf)
 *       y = f * (z * P); y = y + e * -2.12194440e-4; y = y + -0.5 * z; r = f + y; r = r + e * 0.693359375; E = -r
 *       (relative error of E <= 2^-20 against float64 for every one of the 2^24 inputs)
 *     key = w / E, correctly rounded; a weight that is negative, NaN or infinite counts as 0 (key +0)
 *     selection: the N largest keys compared as uint32 bit patterns (every key >= +0); ties at the threshold go to the
 *     lower cell index; cells_out lists the chosen cells in increasing cell order.  Deviations from torch: torch returns
 *     the cells in descending key order (within a batch the order changes only the rounding of the mean), and raises
 *     when fewer than N cells have a positive weight, where here zero-weight cells fill the rest, lowest index first.
 *   pixel of ray n in cell c: rx = (u(n, 0) >> 8) * 2^-24, ry = (u(n, 5) >> 8) * 2^-24, sx = fp32(H / 128),
 *     sy = fp32(W / 128), row = min(trunc(fp32(fp32(cx * sx) + fp32(rx * sx))), H - 1) with cx = c / 128,
 *     col = min(trunc(fp32(fp32(cy * sy) + fp32(ry * sy))), W - 1) with cy = c % 128, pixel = row * W + col
 *     (the reference's `(inds_x * sx + rand * sx).long().clamp(max=H - 1)`).
 *   background words 2..4, rays, nears, fars, gt, bg_out and inds = image * H * W + pixel as lae_sample_train_batch
 *   (one shared per-ray device function). */
LAE_API int lae_sample_train_batch_weighted(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                    const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                    const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int bg_mode,
                                    int srgb_to_linear, const float* error_map, int32_t* cells_out, float* rays_o, float* rays_d,
                                    float* nears, float* fars, float* gt, float* bg_out, int64_t* inds, void* stream);
/* The two samplers with a per-image, per-channel gain on the target colour (exposure and white balance, see lae_exposure_step):
 * gains fp32 [n_img,3] is read, fg fp32 [N,3] is one more output.  In the shared per-ray body, after the optional srgb_to_linear and
 * before the blend, every operation one fp32 rounding in this order (v_c the texel, a the alpha, bg_c the background):
 *     s_c = v_c * gains[img][c];   C == 4: fg_c = s_c * a, gt_c = fg_c + bg_c * (1 - a);   C == 3: fg_c = gt_c = s_c.
 * fg is the part of the target that scales with the gain (the background does not).  A gain of exactly 1.0f gives the gt of the entry
 * point without a gain bit for bit; rays, nears / fars, bg_out, inds, cells_out and the step protocol are those entry points'.
 * LAE_ENULL additionally: gains or fg NULL. */
LAE_API int lae_sample_train_batch_gain(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                        const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                        const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode, int bg_mode,
                                        int srgb_to_linear, const float* gains, float* rays_o, float* rays_d, float* nears, float* fars,
                                        float* gt, float* fg, float* bg_out, int64_t* inds, void* stream);
LAE_API int lae_sample_train_batch_weighted_gain(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                                 const float* poses, float fx, float fy, float cx, float cy, uint32_t N,
                                                 const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int bg_mode,
                                                 int srgb_to_linear, const float* error_map, int32_t* cells_out, const float* gains,
                                                 float* rays_o, float* rays_d, float* nears, float* fars, float* gt, float* fg,
                                                 float* bg_out, int64_t* inds, void* stream);
/* The patch sampler (the reference's --patch_size, nerf/utils.py:88-105): lae_sample_train_batch with the batch drawn as
 * n_patch = N / P^2 square patches of P x P pixels, P = patch_size.  u(ray, word) and the step protocol as there.
 *   patch q: top row  = (u(q, 5) * (uint64)(H - P)) >> 32, left column = (u(q, 6) * (uint64)(W - P)) >> 32 -- the reference's
 *            exclusive bounds, so the last image row and column are never drawn
 *   image:   (u(r, 1) * (uint64)n_img) >> 32 with r = 0xffffffff in LAE_BATCH_IMAGE mode and r = q in LAE_BATCH_ALL mode (an image
 *            per patch)
 *   ray n:   patch q = n / P^2, pixel (row + (n % P^2) / P, col + n % P) (row-major, the reference's 'ij' meshgrid),
 *            inds[n] = image * H * W + y * W + x
 * Everything per ray -- origin, direction, nears / fars, the gather, the colour space, the alpha blend, the background from words
 * 2..4 of ray n -- is what lae_sample_train_batch writes for that (image, pixel): one shared per-ray device function.
 * LAE_EINVAL before any launch: P < 2, P >= min(H, W), N == 0 or N not a multiple of P^2. */
LAE_API int lae_sample_train_batch_patch(const void* images, int dtype, uint32_t n_img, uint32_t H, uint32_t W, uint32_t C,
                                         const float* poses, float fx, float fy, float cx, float cy, uint32_t N, uint32_t patch_size,
                                         const float* aabb, float min_near, uint64_t seed, int64_t* step_counter, int mode,
                                         int bg_mode, int srgb_to_linear, float* rays_o, float* rays_d, float* nears, float* fars,
                                         float* gt, float* bg_out, int64_t* inds, void* stream);

/* The error map's EMA after a step (nerf/utils.py:609-631), one thread per ray: image = inds[n] / (H * W),
 * d = pred[n] - gt[n], err = ((d0 * d0 + d1 * d1) + d2 * d2) / 3, map[image][cells[n]] = 0.1 * old + 0.9 * err (fp32, each
 * product and the sum rounded).  The cells of one batch are distinct (lae_sample_train_batch_weighted), so there is no race;
 * a ray whose image is >= n_img or cell >= 16384 is skipped.  pred, gt [N,3] fp32. */
LAE_API int lae_error_map_update(float* error_map, uint32_t n_img, uint32_t H, uint32_t W, const int64_t* inds, const int32_t* cells,
                                 const float* pred, const float* gt, uint32_t N, void* stream);
/* lae_error_map_update for a step trained with another colour criterion: the reference's rule is error = loss.detach(), the trained
 * criterion's per-ray mean over RGB (nerf/utils.py:592, 624), so err = ((v0 + v1) + v2) / 3 with the element loss v of loss_kind
 * (LAE_LOSS_*, at lae_crit_term; e = pred - gt rounded, every operation rounded).  LAE_LOSS_MSE gives
 * lae_error_map_update's bits.  LAE_EINVAL additionally: loss_kind out of range, a Huber delta that is not finite and > 0. */
LAE_API int lae_error_map_update_crit(float* error_map, uint32_t n_img, uint32_t H, uint32_t W, const int64_t* inds, const int32_t* cells,
                                      const float* pred, const float* gt, uint32_t N, int loss_kind, float loss_param, void* stream);

/* raymarching.cu:201-209  sph_from_ray(rays_o, rays_d, radius, N, coords[N,2]) */
LAE_API int lae_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N,
                     float* coords, void* stream);

/* raymarching.cu:229-232  morton3D(coords[N,3] i32, N, indices[N] i32) */
LAE_API int lae_morton3D(const int32_t* coords, uint32_t N, int32_t* indices, void* stream);

/* raymarching.cu:257-260  morton3D_invert(indices[N], N, coords[N,3]) */
LAE_API int lae_morton3D_invert(const int32_t* indices, uint32_t N, int32_t* coords, void* stream);

/* raymarching.cu:292-300  packbits(grid[8N] f32, N bytes, thresh, bitfield[N] u8) */
LAE_API int lae_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield,
                 void* stream);

/* raymarching.cu:482-490  march_rays_train(...)
 * rays[N,3] = (ray id, offset, count).  Rows are written in RAY-ID order with
 * offsets = exclusive prefix sum of counts (the reference's atomicAdd
 * reservation order is non-deterministic; sequential execution of the
 * reference gives exactly this order).  counter[0] += sum(count),
 * counter[1] += N, like the reference's atomicAdds on a pre-zeroed counter.
 * `scratch` : caller-provided device workspace of lae_march_rays_train_scratch_bytes(N)
 * bytes (may be NULL only when N == 0): per-ray counts and offsets and, for N <= 2^18, the chunk records
 * the counting pass leaves for the emitting pass (292 B per ray).
 * Sample rows no ray owns, [rows_end, M), are zero-filled by the kernel itself (the reference relies on the caller's
 * torch.zeros, raymarching.py:207-209); rows_end is also stored to rows_end_out (device uint32, may be NULL) for
 * lae_composite_rays_train_backward_blend. */
LAE_API uint64_t lae_march_rays_train_scratch_bytes(uint32_t N);
LAE_API int lae_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid,
                         float bound, float dt_gamma, uint32_t max_steps,
                         uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float* nears, const float* fars,
                         float* xyzs, float* dirs, float* deltas,
                         int32_t* rays, int32_t* counter, const float* noises,
                         void* scratch, uint32_t* rows_end_out, void* stream);

/* lae_march_rays_train with the truncation threshold in device memory, so that one captured graph serves every
 * threshold up to its buffer size: M_cap sample rows are written (xyzs / dirs / deltas hold M_cap rows), and rays are
 * truncated where lae_march_rays_train with M = min(*m_limit, M_cap) truncates them.  rays, counter and rows_end equal
 * that call's; rows [rows_end, M_cap) are zero-filled. */
LAE_API int lae_march_rays_train_limit(const float* rays_o, const float* rays_d, const uint8_t* grid,
                               float bound, float dt_gamma, uint32_t max_steps,
                               uint32_t N, uint32_t C, uint32_t H, uint32_t M_cap, const uint32_t* m_limit,
                               const float* nears, const float* fars,
                               float* xyzs, float* dirs, float* deltas,
                               int32_t* rays, int32_t* counter, const float* noises,
                               void* scratch, uint32_t* rows_end_out, void* stream);

/* raymarching.cu:580-588 */
LAE_API int lae_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* deltas,
                                     const int32_t* rays, uint32_t M, uint32_t N, float T_thresh,
                                     float* weights_sum, float* depth, float* image, void* stream);

/* raymarching.cu:685-693 */
LAE_API int lae_composite_rays_train_backward(const float* grad_weights_sum, const float* grad_image,
                                      const float* sigmas, const float* rgbs, const float* deltas,
                                      const int32_t* rays, const float* weights_sum,
                                      const float* image, uint32_t M, uint32_t N, float T_thresh,
                                      float* grad_sigmas, float* grad_rgbs, void* stream);

/* The distortion regularizer of mip-NeRF 360 on the ray's weights, in the O(n) form of the reference's loss.py:29-76
 * (eff_distloss(w, m, interval) with m = t_k and interval = deltas[k,0]; its CUDA-ray path never calls it), inside the compositing
 * kernels.  Over the samples the forward uses (k = 0 .. the early-stop sample, included), w_k = alpha_k T_k, t_k = the running sum
 * of deltas[.,1] including sample k, lengths in the march's own units (NOT divided by far - near):
 *   l_ray = (1/3) sum_k delta0_k w_k^2 + 2 sum_k w_k (t_k W_<k - WT_<k)        W_<k = sum_{j<k} w_j,  WT_<k = sum_{j<k} w_j t_j
 *         = (1/3) sum_k delta0_k w_k^2 + sum_{i,j} w_i w_j |t_i - t_j|
 * It is an output of the forward below, an input of the backward and a term of the fused step (lae_dist_term). */

/* MI355X-native: composite + the post-ops run_cuda applies to its result (nerf/renderer.py:321, 325) in one kernel:
 *   image_out = image + (1 - weights_sum) * bg,  depth_out = clamp(depth - nears, min=0) / (fars - nears).
 * bg = bg_rays [N,3] when non-NULL, else the constant (bg_r, bg_g, bg_b).  weights_sum / depth / image receive the
 * un-blended values (saved for the backward).
 * dist [N], or NULL for none: additionally the output dist[ray] = l_ray (0 for a ray without samples); every other output has the
 * bits of the call without it. */
LAE_API int lae_composite_rays_train_forward_blend(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays,
                                           uint32_t M, uint32_t N, float T_thresh, const float* nears, const float* fars,
                                           const float* bg_rays, float bg_r, float bg_g, float bg_b, float* weights_sum,
                                           float* depth, float* image, float* depth_out, float* image_out, float* dist, void* stream);

/* Backward of the above w.r.t. (weights_sum, image_out): grad_ws_eff = grad_ws - sum_c grad_image_c * bg_c.  Writes EVERY
 * row of grad_sigmas / grad_rgbs in [0, M) (zeros after the early stop and in [rows_end, M)), so they need no
 * pre-zeroing; requires the contiguous ray-id-order sample layout of lae_march_rays_train. */
LAE_API int lae_composite_rays_train_backward_blend(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                            const float* rgbs, const float* deltas, const int32_t* rays,
                                            const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                            float T_thresh, const float* bg_rays, float bg_r, float bg_g, float bg_b,
                                            const uint32_t* rows_end, float* grad_sigmas, float* grad_rgbs, void* stream);
/* same, for a criterion fused in front of it: grad_weights_sum may be NULL (zero) and every incoming gradient is
 * multiplied by the device scalar *grad_scale when grad_scale != NULL (the upstream d(loss), so no elementwise
 * multiplication / zero-fill kernels are needed between the loss and this call).
 *
 * grad_depth [N], or NULL for none: the gradient of the RAW depth output D = sum_k w_k t_k (`depth` of the forward, not depth_out;
 * t_k = running sum of deltas[.,1]), which the reference's backward drops (raymarching.py:273-275):
 *   grad_sigmas_k += delta0_k * grad_depth * (T_post_k * t_k - (D - D_k)),  D_k = the running sum including sample k,
 * inside the same bracket as the colour terms; grad_rgbs is unchanged.  Zeros are allowed: such a ray takes the path of the call
 * without grad_depth and gives its bits.
 *
 * grad_dist [N], or NULL for none: the gradient of l_ray, with dist [N] the forward's l_ray.  With W = weights_sum, D = depth and
 * W_k, WT_k the running sums including sample k:
 *   q_k = d l_ray / d w_k = (2/3) delta0_k w_k + 2 (t_k (W_<k - (W - W_k)) + ((D - WT_k) - WT_<k))
 *   grad_sigmas_k += delta0_k * grad_dist * (T_post_k * q_k - (Q - Q_k)),   Q_k = sum_{j<=k} q_j w_j,   Q = 2 * dist
 * (l_ray is homogeneous of degree 2 in w) inside the same bracket as the colour terms; grad_rgbs is unchanged.  A ray whose
 * grad_dist is zero has the bits of the call without grad_dist (with or without grad_depth).
 *
 * depth [N], the forward's raw depth, is read with either (it is the D of both rules) and not looked at without them.  grad_scale
 * multiplies grad_depth and grad_dist as well.  LAE_ENULL: grad_depth or grad_dist without depth, grad_dist without dist. */
LAE_API int lae_composite_rays_train_backward_blend_ex(const float* grad_weights_sum, const float* grad_image, const float* sigmas,
                                               const float* rgbs, const float* deltas, const int32_t* rays,
                                               const float* weights_sum, const float* image, uint32_t M, uint32_t N,
                                               float T_thresh, const float* bg_rays, float bg_r, float bg_g, float bg_b,
                                               const uint32_t* rows_end, const float* grad_scale, float* grad_sigmas,
                                               float* grad_rgbs, const float* grad_depth, const float* depth, const float* grad_dist,
                                               const float* dist, void* stream);

/* ---- The fused training step, lae_composite_rays_train_step (prototype below its terms).
 * MI355X-native: lae_composite_rays_train_forward_blend + lae_mse_loss_forward (target [N,3], scale as there) +
 * lae_composite_rays_train_backward_blend_ex (grad_weights_sum = NULL, upstream gradient 1) as ONE launch -- d loss / d pixel of a
 * ray needs that ray's pixel only -- plus a one-block launch that adds the workgroups' squared-error sums in a fixed order into
 * loss_out[0] = MSE * scale, loss_out[1] = MSE.  Same arithmetic as the three calls.  grad_image [N,3], grad_sigmas [M],
 * grad_rgbs [M,3] are outputs (every row written); partials: cdiv(N, 4) floats of scratch.
 * defer_loss != 0 (round 3): the one-block launch is left out and loss_out[0..1] is set to NaN; the sum is done later by
 * lae_loss_finish(partials, cdiv(N, 4), 3 * N, scale, loss_out) or taken along by lae_nerf_head_backward (its loss_*
 * arguments) -- the value feeds nothing on the device, so it need not sit on the step's critical path.
 *
 * Four further loss terms join the same launch, each one struct; a NULL struct pointer means the term is absent, and the call
 * without any is the one above:
 *   loss = mean(v) [+ depth.lambda * mean(res^2)] [+ dist.lambda * L_dist] [+ crit.opac_lambda * L_op] [+ weight.lambda * mean(v2 / 3)]
 * Every term adds its part, times 3 and its weight, to partials[b], so every finisher of the base call (n_elem = 3 N) yields the
 * total loss unchanged, and leaves the partial sums of the term alone in a buffer of its own. */

/* Depth term: a second criterion on the ray's raw depth D, the reference's depth supervision
 * (nerf/utils.py:585-589, 634-635: loss += 1e-3 * mean(((depth - (gt_depth - nears)) * (gt_depth > 0))^2)):
 *   z = src[inds ? inds[ray] : ray]                     src fp32 or fp16 (dtype LAE_IMG_F32 / LAE_IMG_F16), inds
 *                                                       int64 or NULL (the `inds` of lae_sample_train_batch into a [n_img, H, W] plane)
 *   res = (z > 0 && nears[ray] < fars[ray]) * (D - (z - nears[ray]))   zero in the plane = no supervision; neither is a ray that
 *                                                       misses the bounding box (lae_near_far_from_aabb gives it near == far ==
 *                                                       FLT_MAX, the reference's rule would make the loss infinite there)
 *   grad_depth[ray] = g_D = ((res * (2 * lambda / N)) * *scale), carried through the backward as
 *   lae_composite_rays_train_backward_blend_ex carries its grad_depth; value_only != 0 computes the value and forces g_D = 0 (the
 *   reference's effective behaviour: its backward ignores the gradient of depth).  A ray with g_D == 0 gets the sample gradients
 *   of the step without the term bit for bit; a ray without samples adds its residual to the value and has no gradient.
 * The step's partials[b] = sum over the workgroup's rays of (squared colour error + 3 * lambda * res^2), so loss_out = MSE + lambda *
 * mean(res^2); the term's partials [cdiv(N, 4)] receive sum(res^2): lae_loss_finish(partials, cdiv(N, 4), N, NULL, out) gives
 * mean(res^2) alone.  grad_depth [N].
 * LAE_EINVAL: lambda not finite and >= 0, a dtype that is not LAE_IMG_F16 / LAE_IMG_F32.  LAE_ENULL: src, grad_depth or partials NULL. */
typedef struct lae_depth_term {
    const void* src;
    int dtype;
    const int64_t* inds;
    float lambda;
    int value_only;
    float* grad_depth;
    float* partials;
} lae_depth_term;

/* Distortion term (l_ray: above lae_composite_rays_train_forward_blend):
 *   loss += lambda * L_dist,   L_dist = (1/N) sum over ALL N rays of l_ray
 *   dist[ray] = l_ray (0 without samples),  grad_dist[ray] = g = (lambda / N) * *scale, carried through the backward as
 *   lae_composite_rays_train_backward_blend_ex carries its grad_dist; value_only != 0 computes the value and forces g = 0.  With
 *   g == 0 (lambda == 0 or value_only) the sample gradients are those of the step without the term bit for bit.
 * The step's partials[b] additionally receive 3 * lambda * sum(l_ray); the term's partials [cdiv(N, 4)] receive sum(l_ray):
 * lae_loss_finish(partials, cdiv(N, 4), N, NULL, out) gives L_dist alone.  dist, grad_dist [N].
 * LAE_EINVAL: lambda not finite and >= 0.  LAE_ENULL: dist, grad_dist or partials NULL. */
typedef struct lae_dist_term {
    float lambda;
    int value_only;
    float* dist;
    float* grad_dist;
    float* partials;
} lae_dist_term;

/* The colour criteria of the fused step, lae_colour_loss_forward and lae_error_map_update_crit.  Per element, with e = pred - target
 * rounded to fp32 and r = |e|, the element loss v and dv = d v / d pred (sign(0) = 0):
 *   LAE_LOSS_MSE    v = e * e                                                  dv = 2 e
 *   LAE_LOSS_L1     v = r                                                      dv = sign(e)
 *   LAE_LOSS_HUBER  v = r > delta ? r - 0.5 delta : ((0.5 / delta) * r) * r    dv = r > delta ? sign(e) : e / delta
 *                   (the reference's loss.py:18-26 huber_loss = torch's HuberLoss(delta) / delta; delta = loss_param, finite, > 0)
 *   LAE_LOSS_MAPE   v = r * k,  k = 1 / (|target| + 1e-2)                      dv = sign(e) * k     (loss.py:7-16 mape_loss)
 * the loss is the mean of v over all elements.  loss_param is read by LAE_LOSS_HUBER only. */
#define LAE_LOSS_MSE 0
#define LAE_LOSS_L1 1
#define LAE_LOSS_HUBER 2
#define LAE_LOSS_MAPE 3
/* Criterion term: the colour criterion chosen by kind (param = loss_param above) and, with opac != NULL, an opacity-entropy term on
 * weights_sum (torch-ngp's lambda_entropy):
 *   grad_image = ((e * (2 / (3 N))) * *scale) under LAE_LOSS_MSE -- the statements and the bits of the step without the term --
 *                and ((dv * (1 / (3 N))) * *scale) otherwise.
 *   o = min(max(weights_sum, 1e-5f), 1 - 1e-5f),  opac[ray] = h = -(o * log2(o) + (1 - o) * log2(1 - o)),
 *   L_op = (1/N) sum over ALL N rays of h (a ray without samples has weights_sum = 0: it adds h(1e-5) and has no gradient),
 *   grad_ws[ray] = ((opac_lambda / N) * (log2(1 - o) - log2(o))) * *scale where 1e-5f <= weights_sum <= 1 - 1e-5f and 0 outside
 *   (torch.clamp's gradient, bounds included); opac_value_only != 0 computes the value and forces grad_ws = 0.  The backward takes
 *   it where lae_composite_rays_train_backward_blend_ex takes grad_weights_sum: the fused call equals the forward plus that call
 *   with (grad_ws, grad_image).  It costs no work per sample: it joins the ray's constant of the bracket.
 * opac == NULL switches the entropy term off: opac_lambda, opac_value_only, grad_ws and opac_partials are then not looked at.  With
 * LAE_LOSS_MSE and opac == NULL every output has the bits of the step without the term (with or without the depth and distortion
 * terms); the kernels differ, so the two are not interchangeable for speed.
 * The step's partials[b] = sum over the workgroup's rays of (v0 + v1 + v2 + 3 * opac_lambda * h + the depth and distortion parts);
 * opac_partials [cdiv(N, 4)] receive sum(h): lae_loss_finish(opac_partials, cdiv(N, 4), N, NULL, out) gives L_op alone.  opac, grad_ws [N].
 * LAE_EINVAL: kind out of range, a Huber delta that is not finite and > 0, opac_lambda not finite and >= 0 (with opac != NULL).
 * LAE_ENULL: opac without grad_ws or opac_partials. */
typedef struct lae_crit_term {
    int kind;
    float param;
    float opac_lambda;
    int opac_value_only;
    float* opac;
    float* grad_ws;
    float* opac_partials;
} lae_crit_term;

/* Weight term: a per-pixel weight on the colour residual and a second colour target with its own weight -- the reference's
 * train_step_npr (nerf/utils.py:523-526: loss = mean((w (pred - gt))^2) + style_weight_d * mean(((1 - w / 2) (gt_style - pred))^2) +
 * the depth term), and mask- / confidence-weighted training in general.  LAE_LOSS_MSE only; without a criterion term the criterion
 * is LAE_LOSS_MSE without the entropy term.
 *   w_src: a weight plane, fp16 or fp32 (w_dtype = LAE_IMG_F16 / LAE_IMG_F32), gathered at inds[ray] (int64, the sampler's
 *     inds = image * H * W + pixel) or at `ray` when inds is NULL -- the rule of the depth term's inds.  NULL: no weights (w = 1),
 *     w_dtype is then not looked at.
 *   t2_src: a second target plane [.., t2_channels] (3 or 4; t2_dtype as w_dtype), gathered the same way.  NULL: no second term,
 *     t2_dtype, t2_channels, lambda and partials are then not looked at.  With 4 channels it is blended over the ray's own background
 *     as the sampler blends gt, three roundings, no contraction: t_c = s_c * s_a + bg_c * (1 - s_a); with 3, t_c = s_c.
 * Per ray, after the forward and the blend (o = image_out[ray], gt = target[ray]), every operation one fp32 rounding:
 *   u = 1 - 0.5 * w,   a_c = w * (o_c - gt_c),   v1 = fmaf(a2, a2, fmaf(a1, a1, a0 * a0)),
 *   b_c = u * (t_c - o_c),   v2 = (b0 * b0 + b1 * b1) + b2 * b2,
 *   loss = (1 / (3 N)) sum over the rays of (v1 + lambda * v2) [+ the depth, distortion and entropy terms, unchanged]
 *   grad_image_c = (((w * a_c) - lambda * (u * b_c)) * (2 / (3 N))) * *scale     (no second target: ((w * a_c) * (2 / (3 N))) * *scale)
 *   With a second target the two parts of grad_image cancel where the pixel lies between its targets (where the training converges):
 *   there the expression is evaluated in double on the fp32 operands (w, o, gt, t, *scale) and rounded to fp32 once, so that
 *   grad_image keeps the relative accuracy of the step without a second target (about 1e-7) instead of an unbounded relative error.
 *   The loss values (v1, v2) stay fp32.
 * The backward is that of the step without the term on this grad_image: nothing is added per sample.  A weight of 0 makes a_c and
 * the first term's gradient exact zeros: the pixel's colour cannot matter.
 * The step's partials[b] receive v1 + lambda * v2 (+ the other parts); the term's partials [cdiv(N, 4)] receive sum(v2):
 * lae_loss_finish(partials, cdiv(N, 4), 3 N, NULL, out) gives mean(v2 / 3), the second term alone.
 * With w_src == NULL and t2_src == NULL the call IS the one with the criterion term alone (same kernels, same bits); with a plane of
 * ones and no second target every output has those bits too (1 * x is exact).
 * LAE_EINVAL: weights or a second target with kind != LAE_LOSS_MSE (the reference has no weighted L1 / Huber / MAPE; out of scope),
 * lambda not finite and >= 0, t2_channels not 3 or 4, a dtype that is not LAE_IMG_F16 / LAE_IMG_F32.  LAE_ENULL: t2_src without partials. */
typedef struct lae_weight_term {
    const void* w_src;
    int w_dtype;
    const void* t2_src;
    int t2_dtype;
    int t2_channels;
    const int64_t* inds;
    float lambda;
    float* partials;
} lae_weight_term;

/* The step.  The terms' LAE_EINVAL conditions are checked first (weight, criterion, depth, distortion), then N == 0 returns LAE_OK,
 * then the LAE_ENULL conditions.  The structs are read during the call only. */
LAE_API int lae_composite_rays_train_step(const float* sigmas, const float* rgbs, const float* deltas, const int32_t* rays, uint32_t M,
                                  uint32_t N, float T_thresh, const float* nears, const float* fars, const float* bg_rays, float bg_r,
                                  float bg_g, float bg_b, const uint32_t* rows_end, const float* target, const float* scale,
                                  float* weights_sum, float* depth, float* image, float* depth_out, float* image_out,
                                  float* grad_image, float* grad_sigmas, float* grad_rgbs, float* loss_out, float* partials,
                                  int defer_loss, const lae_depth_term* depth_term, const lae_dist_term* dist_term,
                                  const lae_crit_term* crit_term, const lae_weight_term* weight_term, void* stream);
LAE_API int lae_loss_finish(const float* partials, uint32_t n_part, uint32_t n_elem, const float* scale, float* loss_out, void* stream);


/* raymarching.cu:929-936 */
LAE_API int lae_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive,
                   const float* rays_t, const float* rays_o, const float* rays_d,
                   float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                   const uint8_t* grid, const float* nears, const float* fars,
                   float* xyzs, float* dirs, float* deltas, const float* noises, void* stream);

/* raymarching.cu:938-945  (edit_occ is a torch.bool tensor = 1 byte / sample) */
LAE_API int lae_march_rays_distill(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive,
                           const float* rays_t, const float* rays_o, const float* rays_d,
                           float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                           const uint8_t* grid, const uint8_t* edit_grid,
                           const float* nears, const float* fars,
                           float* xyzs, float* dirs, float* deltas, uint8_t* edit_occ,
                           const float* noises, void* stream);

/* raymarching.cu:1145-1151 */
LAE_API int lae_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh,
                       int32_t* rays_alive, float* rays_t,
                       const float* sigmas, const float* rgbs, const float* deltas,
                       float* weights_sum, float* depth, float* image, void* stream);

/* raymarching.cu:1153-1159 */
LAE_API int lae_composite_rays_distill(uint32_t n_alive, uint32_t n_step, float T_thresh,
                               int32_t* rays_alive, float* rays_t,
                               const float* sigmas, const float* rgbs, const float* deltas,
                               float* weights_sum, float* weights_edit_sum,
                               float* depth, float* depth_edit,
                               const uint8_t* edit_occ, float* image, void* stream);

/* MI355X-native extension: the whole inference loop of NeRFRenderer.run_cuda (nerf/renderer.py:335-387) -- and of
 * run_cuda_distill (:394-480) when edit_grid != NULL -- as ONE call.  near_far_from_aabb, then per iteration
 * march_rays -> hash-grid encode -> fused sigma/colour head -> composite_rays -> alive-list compaction, with
 * n_alive / n_step / step kept in device memory and advanced on the device exactly like the Python
 * (`n_step = max(min(row_budget // n_alive, max_n_step), 1)`; the reference has row_budget = N (pass 0) and
 * max_n_step = 8; a larger row_budget trades buffer memory for fewer, larger iterations -- per-ray sample sequences
 * are unchanged, only the float rounding of rays_t between iterations can differ; loop ends when no ray is alive or
 * step >= max_steps), then `image + (1 - weights_sum) * bg` (blend_bg) and `clamp(depth - nears, 0) / (fars - nears)`
 * (scale_depth).  The host never waits for the device inside the loop: it sizes launches from a lagging upper bound of
 * n_alive mirrored into pinned memory.  Not stream-capturable (LAE_EINVAL while capturing).
 *   table_f16 [sum level sizes, 2] fp16, offsets [L+1] int32 (device), offsets_host = the same L+1 ints in HOST memory
 *   or NULL (only the level -> XCD balance of the encoder depends on it), L = 16, S = log2(per_level_scale), base_resolution;
 *   sigma_weights / color_weights: FFMLP flat fp16 images of the 32->64->64->16 and 32->64->64->64->16 nets;
 *   noises [N] or NULL (perturb, applied in the first iteration only, renderer.py:365); bg_rays [N,3] or NULL (then
 *   bg_r/g/b); outputs weights_sum, depth [N], image [N,3] fp32 (+ weights_edit, depth_edit [N] when edit_grid);
 *   workspace: lae_render_frame_workspace_bytes(N, L, row_budget) bytes of device memory owned by the caller;
 *   stats_out (host, may be NULL; makes the call wait for the loop's last iteration): [iterations, rows through the
 *   network, iterations launched]. */
LAE_API uint64_t lae_render_frame_workspace_bytes(uint32_t N, uint32_t L, uint64_t row_budget);
/* 1 (default) runs the lookahead marcher on a library-owned side stream beside the encoder / MLP kernels, 0 runs it
 * in-line on the caller's stream (same image bit for bit).  CONCURRENCY REQUIREMENT of the overlapped form: the two streams
 * are ordered by polled words in device memory, not by events, so they must make progress side by side.  The library probes
 * that once per caller stream (a wait kernel on the caller's stream, then a signal kernel on the side stream) and runs in
 * line by itself -- with one warning on stderr -- when they do not: both on one hardware queue (GPU_MAX_HW_QUEUES=1, many
 * live streams of one priority), serialised dispatch (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING), a counter-collecting
 * profiler.  A wait that still times out (~10 s) poisons its frame (outputs NaN, never a wrong image), the call renders
 * the frame again in line and the process stays in line from then on; LAE_ELAUNCH only if that fails too.  The reference's
 * loop has no such failure mode (nerf/renderer.py:335-387).  LAE_FRAME_OVERLAP=0 / 1 pins the mode (1 skips the probe). */
LAE_API int lae_render_frame_set_overlap(int on);
/* how the most recent frame ran: 1 = lookahead on the side stream, 0 = in line (switched off, probed as not concurrent, or
 * degraded after a time-out); before the first frame: the configured mode */
LAE_API int lae_render_frame_mode(void);
/* Round 6.  A cross-stream wait that times out while the host is still inside lae_render_frame makes the call render
 * the frame again in line.  One that gives up AFTER the call has returned (only possible without stats_out, which waits for the
 * loop's end) leaves that frame's outputs NaN -- never a wrong image -- and the call has already returned LAE_OK.  After
 * synchronising the frame's stream: 0 = the most recent frame completed, 1 = it was poisoned by such a time-out (render it again;
 * the process runs in line from the next frame on), -1 = no frame yet. */
LAE_API int lae_render_frame_last_status(void);
/* Which side stream: with the first frame of a caller stream the library times 16 hand-overs caller -> side -> caller through the
 * loop's own store / poll kernels on its highest-priority side stream (or the class LAE_FRAME_SIDE_PRIO names) and, when that
 * stream does not run beside the caller's or is slow (~50 instead of ~11 us per hand-over: which hardware queue picks a dispatch
 * up promptly depends on the streams the process already uses), on up to four streams of the caller's class created
 * on demand; the first prompt one is used, else the fastest seen.  us[0..n): the times of the most recent probe in microseconds
 * (candidate 0 first; < 0: not probed / not concurrent); returns the candidate in use, -1 before the first frame. */
LAE_API int lae_render_frame_probe_us(float* us, uint32_t n);
LAE_API int lae_render_frame(const float* rays_o, const float* rays_d, uint32_t N, const float* aabb, float min_near,
                     const uint8_t* grid, const uint8_t* edit_grid, float bound, float dt_gamma, uint32_t max_steps,
                     uint32_t C, uint32_t H, const void* table_f16, const int32_t* offsets, const int32_t* offsets_host,
                     uint32_t L, float S,
                     uint32_t base_resolution, uint32_t gridtype, int align_corners, uint32_t interp,
                     const void* sigma_weights, const void* color_weights, float density_scale, float T_thresh,
                     uint32_t max_n_step, uint64_t row_budget, const float* noises, const float* bg_rays, float bg_r, float bg_g,
                     float bg_b, int blend_bg, int scale_depth, float* weights_sum, float* depth, float* image,
                     float* weights_edit, float* depth_edit, void* workspace, uint64_t workspace_bytes, uint32_t* stats_out,
                     void* stream);

/* MI355X-native extension (no reference counterpart; replaces the host-side
 * `rays_alive = rays_alive[rays_alive >= 0]` + size sync at renderer.py:375,459):
 * order-preserving device-side compaction of the alive list.
 * out_alive[0..n_out) = entries of rays_alive that are >= 0, in order;
 * *n_out_dev (device int32) receives n_out.  scratch: lae_compact_scratch_bytes(n_alive). */
LAE_API uint64_t lae_compact_scratch_bytes(uint32_t n_alive);
LAE_API int lae_compact_rays_alive(const int32_t* rays_alive, uint32_t n_alive, int32_t* out_alive,
                           int32_t* n_out_dev, void* scratch, void* stream);

/* ------------------------------------------------------------------ */
/* _gridencoder  (gridencoder/src/gridencoder.h:12-15)                */
/* ------------------------------------------------------------------ */

/* gridencoder.cu:448-471  grid_encode_forward(inputs[B,D] f32, embeddings[sO,C],
 * offsets[L+1] i32, outputs[L,B,C], B, D, C, L, S, H, dy_dx[B,L*D*C] or NULL,
 * gridtype, align_corners, interp).  `dtype` selects the element type of
 * embeddings / outputs / dy_dx (the reference dispatches on
 * embeddings.scalar_type(), gridencoder.cu:467). */
LAE_API int lae_grid_encode_forward(const float* inputs, const void* embeddings, const int32_t* offsets,
                            void* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                            float S, uint32_t H, void* dy_dx, uint32_t gridtype,
                            int align_corners, uint32_t interp, int dtype, void* stream);

/* gridencoder.cu:473-503  grid_encode_backward(grad[L,B,C], inputs, embeddings, offsets,
 * grad_embeddings[sO,C] (pre-zeroed, accumulated into), B, D, C, L, S, H,
 * dy_dx or NULL, grad_inputs[B,D] or NULL, gridtype, align_corners, interp) */
LAE_API int lae_grid_encode_backward(const void* grad, const float* inputs, const void* embeddings,
                             const int32_t* offsets, void* grad_embeddings, uint32_t B,
                             uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             const void* dy_dx, void* grad_inputs, uint32_t gridtype,
                             int align_corners, uint32_t interp, int dtype, void* stream);

/* MI355X-native general forms.
 *   blc = 0: [L,B,C] outputs / gradients (the reference's backend layout, and what the fused field op keeps between
 *            encoder and MLP so that no transpose is needed); blc = 1: [B, L*C] directly (what grid.py:57 / grid.py:75
 *            produce with a permute + reshape copy).  Same arithmetic.
 *   in_shift / in_scale: every coordinate is read as (x + in_shift) * in_scale -- GridEncoder.forward's
 *            `(inputs + bound) / (2 * bound)` (grid.py:149) with in_shift = bound, in_scale = fp32(1 / (2 * bound)); pass
 *            0, 1 for coordinates already in [0, 1].
 *   offsets_host: the caller's HOST copy of `offsets` (L + 1 ints) or NULL.  The reference hands the backend a device
 *            tensor only; the module that built it (grid.py:118-127) has the numbers on the host, and passing them lets
 *            the library balance the forward's level -> XCD schedule and skip the launch of the generic atomic kernel
 *            when no level needs it.  It never changes a result: with NULL the forward uses the fixed level l -> XCD
 *            l mod 8 map and the backward always launches the (then idle) companion kernel.  Nothing is cached between
 *            calls (round 1 cached a device->host copy keyed on the device pointer, which a reused address could make
 *            stale). */
LAE_API int lae_grid_encode_forward_ex(const float* inputs, const void* embeddings, const int32_t* offsets, void* outputs,
                               uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, void* dy_dx,
                               uint32_t gridtype, int align_corners, uint32_t interp, int dtype, int blc, float in_shift,
                               float in_scale, const int32_t* offsets_host, void* stream);
LAE_API int lae_grid_encode_backward_ex(const void* grad, const float* inputs, const void* embeddings, const int32_t* offsets,
                                void* grad_embeddings, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                uint32_t H, const void* dy_dx, void* grad_inputs, uint32_t gridtype,
                                int align_corners, uint32_t interp, int dtype, int blc, float in_shift, float in_scale,
                                const int32_t* offsets_host, int32_t* nonfinite_flag, uint32_t* touched_lines, uint32_t* grad_dirty,
                                void* stream);
/* nonfinite_flag (may be NULL): device word that is OR-ed with 1 when this call STORES a non-finite value into
 * grad_embeddings (an overflowed sum, a non-finite contribution, or a non-finite value already there that it adds to).  A
 * caller whose gradient buffer is written by these calls only can hand the optimizer's found_inf word (state word 2 of
 * lae_adam_*) and leave the table out of lae_adam_check.  Needs the binned pipeline on every level: D = 3, C = 2,
 * offsets_host given, every level <= 2^21 entries, B <= 2^24 (LAE_EINVAL otherwise).
 * touched_lines (may be NULL; fp16 only, same conditions): bitmap with one bit per 8 table entries (bit k of word w = entries
 * 8 * (32 w + k) ... + 7, i.e. one 64-byte line of the fp32 table); the counting half of the call sets the bits of the lines
 * that hold a corner of a cell some sample lies in (a superset of the lines that receive a non-zero gradient).
 * lae_adam_apply_multi skips lines whose bit was never set (their gradient and both Adam moments are exactly zero).  With
 * the two-call form the bitmap goes to lae_grid_encode_backward_plan (the counting half), not to _planned.
 * grad_dirty (may be NULL = "may hold anything"): one device word per gradient accumulator, 0 = grad_embeddings holds nothing but
 * zeros.  The call hands the word's value to its accumulate pass and sets the word to 1 (the generic atomic kernel just sets it);
 * on 0 the binned fp16 pass does not read the old value of the entries it stores (16 KB per 4096-entry partition) and stores
 * RN(sum), which is what RN(0 + sum) gives: same bits.  lae_adam_apply_multi(grad_dirty) sets the word back to 0 for the
 * gradients it has zeroed.  Whoever else writes grad_embeddings sets the word to 1; whoever zeroes it may set it to 0. */

/* MI355X-native: the binned backward (D = 3, C = 2) in two halves.  Its first half -- the bookkeeping of a counting
 * sort: items per (level, 1024 samples, table partition), their scans -- depends on the sample positions only,
 * so a caller can run it as soon as the positions exist (e.g. right after the march, on another stream beside the
 * forward pass) and hand the result to the second half, which needs the gradients.  plan:
 * lae_grid_backward_plan_bytes(B, L) bytes of device memory owned by the caller, read-only for `_planned` except for its
 * work-queue words, which every execution resets itself (a plan serves any number of executions, one at a time).
 * grad is level-major [L, B, 2] (the layout of lae_grid_encode_backward).  B <= 2^24 samples and L <= 32 (LAE_EINVAL beyond:
 * the kernels address the batch with 32-bit byte offsets); lae_grid_encode_backward itself takes any B and falls back to its
 * global-atomic kernel above that size. */
LAE_API uint64_t lae_grid_backward_plan_bytes(uint32_t B, uint32_t L);
/* 32-bit words of a touched_lines bitmap for a table of n_entries (= offsets[L]) entries: the line bits (+ slack) followed by
 * one "every line of level l is marked" word per level, which the counting pass sets and then stops marking that level.
 * The caller zero-fills the buffer once; filling it with ones means "skip nothing". */
LAE_API uint64_t lae_grid_touched_lines_words(uint64_t n_entries);
LAE_API int lae_grid_encode_backward_plan(const float* inputs, const int32_t* offsets, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                  float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                  float in_shift, float in_scale, const int32_t* offsets_host, void* plan,
                                  uint32_t* touched_lines, void* stream);
LAE_API int lae_grid_encode_backward_planned(const void* grad, const float* inputs, const int32_t* offsets, void* grad_embeddings,
                                     uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                     int align_corners, uint32_t interp, int dtype, float in_shift, float in_scale,
                                     const int32_t* offsets_host, const void* plan, int32_t* nonfinite_flag, uint32_t* grad_dirty,
                                     void* stream);

/* Bytes of LIBRARY workspace the binned backward (D = 3, C = 2) takes for B samples and L levels when it runs both halves
 * itself: the plan + the item queue, sized for the worst case of 8 items per (sample, level) at 10 bytes each for fp16
 * gradients (hashed levels produce 4; only the front of the queue is touched) + the partial sums of split partitions.
 * Informational: the workspace is library-owned (see the header comment: warm up eagerly before capturing). */
LAE_API uint64_t lae_grid_backward_workspace_bytes(uint32_t B, uint32_t L, int dtype);

/* Host-only helper (no GPU call; used by the CPU tests): the level -> XCD schedule of the specialised forward for a table
 * with the given level offsets (HOST pointer, L + 1 ints) and `n_chunks` 256-sample chunks.  nseg_out[8]; segs_out[8][12][3] =
 * (level, first chunk, chunk count) per XCD in execution order.  Returns the largest number of workgroups any XCD owns
 * (the launch is 8 x that), or a negative error code. */
LAE_API int lae_grid_forward_schedule(const int32_t* offsets_host, uint32_t L, float S, uint32_t H, uint32_t n_chunks,
                              uint32_t* nseg_out, uint32_t* segs_out);

/* MI355X-native, A/B switch of the forward for the hot configuration (fp16 table, D = 3, C = 2, linear, hash type):
 * 0 (default) = specialised kernel with the cost-balanced level -> XCD schedule, 1 = specialised kernel with level l on
 * XCD l mod 8, 2 = the generic kernel.  Results are bit-identical in every mode. */
LAE_API int lae_grid_set_forward_mode(int mode);

/* MI355X-native: 0 (default) = binned / LDS-accumulated backward for D = 3, C = 2 (contributions routed to the owner
 * of a 4096-entry table partition, fp16 sums exact, no scattered global atomics), 1 = always the generic kernel (one
 * global atomic per corner, what the reference does). */
LAE_API int lae_grid_set_backward_mode(int mode);

/* gridencoder.cu:639-645  grad_total_variation(inputs[B,D], embeddings, grad, offsets,
 * weight, B, D, C, L, S, H, gridtype, align_corners); inputs has the table dtype. */
LAE_API int lae_grad_total_variation(const void* inputs, const void* embeddings, void* grad,
                             const int32_t* offsets, float weight, uint32_t B, uint32_t D,
                             uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                             int align_corners, int dtype, void* stream);

/* ------------------------------------------------------------------ */
/* _shencoder  (shencoder/src/shencoder.h:9-10)                       */
/* ------------------------------------------------------------------ */

/* shencoder.cu:400-417  sh_encode_forward(inputs[B,3], outputs[B,C*C], B, D=3, C=degree, dy_dx[B,3*C*C] or NULL) */
LAE_API int lae_sh_encode_forward(const float* inputs, float* outputs, uint32_t B, uint32_t D,
                          uint32_t C, float* dy_dx, void* stream);

/* shencoder.cu:419-439  sh_encode_backward(grad[B,C*C], inputs, B, D, C, dy_dx, grad_inputs[B,3] accumulated into) */
LAE_API int lae_sh_encode_backward(const float* grad, const float* inputs, uint32_t B, uint32_t D,
                           uint32_t C, const float* dy_dx, float* grad_inputs, void* stream);

/* ------------------------------------------------------------------ */
/* _ffmlp  (ffmlp/src/ffmlp.h:8-14).  All tensors fp16 (uint16 storage) */
/* ------------------------------------------------------------------ */

/* ffmlp.cu:635-671  ffmlp_forward(inputs[B,in], weights, B, input_dim, output_dim(=16 padded),
 * hidden_dim, num_layers, activation, output_activation, forward_buffer[num_layers,B,hidden], outputs[B,16]).
 * forward_buffer may be NULL.  Round 6: for the shapes the recompute backward serves (hidden 64, ReLU, linear output, 1-2 hidden
 * GEMMs, input 32 / 48 / 64) in the default mode (lae_ffmlp_set_mode(0)) the buffer is NOT written: lae_ffmlp_backward never reads
 * it there and the reference's Python only hands it on (ffmlp.py:31-35).  lae_ffmlp_set_mode(1) fills it like the reference. */
LAE_API int lae_ffmlp_forward(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                      uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                      uint32_t activation, uint32_t output_activation, void* forward_buffer,
                      void* outputs, void* stream);

/* ffmlp.cu:673-709  (inference_buffer[B,hidden] is scratch the reference never reads back) */
LAE_API int lae_ffmlp_inference(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                        uint32_t activation, uint32_t output_activation, void* inference_buffer,
                        void* outputs, void* stream);

/* ffmlp.cu:749-895  ffmlp_backward(grad[B,16], inputs, weights, forward_buffer, B, ...,
 * calc_grad_inputs, backward_buffer[num_layers,B,hidden], grad_inputs[B,in] or dummy, grad_weights) */
LAE_API int lae_ffmlp_backward(const void* grad, const void* inputs, const void* weights,
                       const void* forward_buffer, uint32_t B, uint32_t input_dim,
                       uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                       uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                       void* backward_buffer, void* grad_inputs, void* grad_weights,
                       void* stream);
/* MI355X extension (round 5): accumulate != 0 ADDS the weight gradient to grad_weights (an optimizer-owned fp16 accumulator) instead
 * of overwriting it; nonfinite_flag (device int32, may be NULL) is OR-ed with 1 when a stored weight gradient is not finite.  Both
 * are served by the fused recompute backward only (hidden 64, ReLU, 1-2 hidden GEMMs, input 32 / 48 / 64): LAE_EINVAL otherwise. */
LAE_API int lae_ffmlp_backward_ex(const void* grad, const void* inputs, const void* weights,
                          const void* forward_buffer, uint32_t B, uint32_t input_dim,
                          uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                          uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                          void* backward_buffer, void* grad_inputs, void* grad_weights,
                          int accumulate, int32_t* nonfinite_flag, void* stream);

/* MI355X-native fusion of NeRFNetwork.forward after the encoder (nerf/network_ff.py:57-79): sigma FFMLP(32,64,2 layers)
 * -> sigma = density_scale * exp(h[0]); colour input = [SH degree 4 of dirs | h[1..15] | 0] -> colour FFMLP(32,64,3 layers)
 * -> rgb = sigmoid(out[0..2]).  enc [M,32] fp16, dirs [M,3] fp32, weights in the FFMLP flat fp16 layout, M % 16 == 0.
 * Outputs: h_out [M,16] fp16 (sigma-net output, saved for the backward), sigmas [M] fp32, rgbs [M,3] fp32.
 * enc_level_major != 0: enc is the encoder's native [16, M, 2] layout (lae_grid_encode_forward) instead of [M,32]. */
LAE_API int lae_nerf_head_forward(const void* enc, const float* dirs, const void* sigma_weights, const void* color_weights,
                          uint32_t M, float density_scale, void* h_out, float* sigmas, float* rgbs, int enc_level_major,
                          void* stream);

/* The density query of NeRFNetwork.density (nerf/network_ff.py:83-96) after the encoder: sigma FFMLP -> sigma =
 * density_scale * exp(h[0]); h_out [M,16] fp16 (h[1..15] = geo_feat) may be NULL.  Used by update_extra_state. */
LAE_API int lae_nerf_density_forward(const void* enc, const void* sigma_weights, uint32_t M, float density_scale, void* h_out,
                             float* sigmas, int enc_level_major, void* stream);
/* enc_level_major (round 3): as in lae_nerf_head_forward -- the occupancy-grid maintenance queries the density of 2.1 M
 * cells per cascade and needs neither the [M,32] transpose of the features nor h. */

/* Backward of lae_nerf_head_forward: grad_sigmas [M], grad_rgbs [M,3] fp32 (as produced by
 * lae_composite_rays_train_backward) -> grad_enc [M,32] fp16 (may be NULL), grad_*_weights (fp16, flat FFMLP layout).
 * grad_h is an [M,16] fp16 scratch (receives dL/dh).  Sigmoid and trunc_exp (activation.py:14-17) backward are fused.
 * accumulate_weight_grads != 0: grad_*_weights += dW (the fused optimizer's persistent buffers) instead of = dW.
 * enc_level_major != 0: enc AND grad_enc are [16, M, 2] (what lae_grid_encode_backward consumes directly).  nonfinite_flag (may be NULL): device word OR-ed with 1 when a non-finite WEIGHT gradient is stored (see
 * lae_grid_encode_backward_ex). */
LAE_API int lae_nerf_head_backward(const float* grad_sigmas, const float* grad_rgbs, const void* enc, const float* dirs, const void* h,
                           const float* rgbs, const void* sigma_weights, const void* color_weights, uint32_t M,
                           float density_scale, void* grad_h, void* grad_enc, void* grad_sigma_weights,
                           void* grad_color_weights, int accumulate_weight_grads, int enc_level_major,
                           int32_t* nonfinite_flag, const float* loss_partials, uint32_t loss_n_part, uint32_t loss_n_elem,
                           const float* loss_scale, float* loss_out, void* stream);
/* loss_out != NULL (round 3): the launch that reduces the weight-gradient slabs carries one workgroup more, which finishes a
 * loss value deferred by lae_composite_rays_train_step(defer_loss): loss_out[0] = sum(loss_partials[0 .. loss_n_part)) /
 * loss_n_elem * (*loss_scale, or 1 when NULL), loss_out[1] = the same unscaled -- the bits lae_loss_finish would write. */

/* Backward of the whole field (hash grid D = 3, C = 2, fp16 table -> lae_nerf_head_forward with enc_level_major) in one call:
 * lae_nerf_head_backward(enc_level_major = 1) followed by lae_grid_encode_backward_ex (plan == NULL) or _planned on grad_enc
 * [L, M, 2].  The arguments are those of the two calls; weights_nonfinite_flag / table_nonfinite_flag are their nonfinite_flag
 * words (may be the same word), touched_lines is ignored with a plan (it went to lae_grid_encode_backward_plan).  Where the
 * binned pipeline runs (L <= 32, M <= 2^24, backward mode 0) the launch that reduces the weight-gradient slabs (and finishes the
 * deferred loss) is not made: its workgroups ride as tail tasks in the grid backward's accumulate pass, behind the partition
 * tasks.  Every result has the bits the two calls give.  LAE_FIELD_NO_RIDE_ALONG=1 in the environment (read at every call) makes
 * the two calls as they are: an A/B switch.  Invalid arguments of either half are refused before the first launch. */
LAE_API int lae_nerf_field_backward(const float* grad_sigmas, const float* grad_rgbs, const void* enc, const float* dirs, const void* h,
                            const float* rgbs, const void* sigma_weights, const void* color_weights, uint32_t M, float density_scale,
                            void* grad_h, void* grad_enc, void* grad_sigma_weights, void* grad_color_weights,
                            int accumulate_weight_grads, int32_t* weights_nonfinite_flag, const float* loss_partials,
                            uint32_t loss_n_part, uint32_t loss_n_elem, const float* loss_scale, float* loss_out,
                            const float* inputs, const int32_t* offsets, void* grad_embeddings, uint32_t L, float S, uint32_t H,
                            uint32_t gridtype, int align_corners, uint32_t interp, float in_shift, float in_scale,
                            const int32_t* offsets_host, const void* plan, int32_t* table_nonfinite_flag, uint32_t* touched_lines,
                            uint32_t* grad_dirty, void* stream);

/* ---- freqencoder (freqencoder/src/freqencoder.h:6-10; bindings.cpp:5-8) ----
 * outputs [B, C], C = D + 2*D*deg: the input, then per frequency f < deg the D sines and D cosines of x * 2^f.
 * backward: grad [B, C], outputs (saved forward result) -> grad_inputs [B, D] (overwritten). fp32 only. */
LAE_API int lae_freq_encode_forward(const float* inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, float* outputs,
                            void* stream);
LAE_API int lae_freq_encode_backward(const float* grad, const float* outputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                             float* grad_inputs, void* stream);

/* ---- LAENeRF palette recomposition (editing/style_encoder.py:135-158 forward_train) ----
 * w_logits, o_raw: the [M,16] fp16 outputs of the weight net (first P columns) and offset net (first 3 columns);
 * palette [P,3] fp32 (device); active_mask bit k = palette base k takes part (style_encoder.py `active_palets`).
 *   w_hat [M, popcount(mask)] fp32 = softmax over the active columns, o_hat [M,3] fp16 = tanh,
 *   pred [M,3] fp16 = clamp(w_hat @ palette[active].half() + o_hat, 0, 1).
 * backward: g_pred / g_o fp16 [M,3], g_w fp32 [M, n_active] (each may be NULL = zero) -> g_w_logits, g_o_raw [M,16] fp16
 * (zeros in padded / inactive columns), g_palette [P,3] fp32 (deterministic two-stage reduction);
 * scratch: lae_palette_backward_scratch_bytes(M). */
LAE_API int lae_palette_forward(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                        uint32_t M, void* pred, float* w_hat, void* o_hat, void* stream);
LAE_API uint64_t lae_palette_backward_scratch_bytes(uint32_t M);
LAE_API int lae_palette_backward(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                         uint32_t M, const void* g_pred, const float* g_w, const void* g_o, void* g_w_logits, void* g_o_raw,
                         float* g_palette, void* scratch, void* stream);

/* ---- recolored views of a trained palette network (nerf/utils.py:1230-1386 test_gui_styleenc / val_gui_styleenc,
 * nerf/gui.py:659-714 eval_style_predictor: torch ops and a host nonzero() in the reference) ----
 * A view is prepared once per pose (edit-grid render, compaction, the two MLPs) and recolored by one compose launch per edit:
 * what the network predicts at a pixel depends on the pose only, the palette edits only on the recomposition.
 *
 * lae_recolor_compact: depth, weights_sum [N] of an edit-grid render (scale_depth off), rays_o, rays_d [N,3] fp32.
 *   d = depth with NaN -> 0; pixel i is an edit pixel when d != 0 (d.flatten().nonzero(), utils.py:1268-1273).
 *   indices [N cap] int32: the edit pixels in ascending order; slot_map [N] int32: i's slot in that list, or -1;
 *   x_term [round_up(N,16) cap, 3] = rays_o + d * rays_d (a multiply, then an add: two roundings, torch's two elementwise
 *   kernels bit for bit); dirs [round_up(N,16) cap, 3] = rays_d; alpha [N cap] = weights_sum (the reference's pred_t);
 *   *count (device int32) = K.  Rows K .. round_up(K, 16) - 1 of x_term and dirs are zero (the MLPs take multiples of 16 rows).
 *   Stable compaction: per-block counts, a one-block scan, a scatter.  scratch: lae_recolor_compact_scratch_bytes(N).
 *
 * lae_recolor_compose: one thread per pixel.  w_logits [K_pad, >= P] fp16 (row stride w_stride) and o_raw [K_pad, >= 3] fp16
 *   (row stride o_stride): the weight / offset nets' outputs for the compacted rows (LAENeRF._logits); active_mask bit j =
 *   base j active, n_active = popcount; palette [n_active, 3], p_weights, p_bias [n_active], alpha [K], bg [3]: fp32 DEVICE
 *   arrays (no host scalar changes with an edit: a captured launch replays new values); base [N,3] the render's image.
 *   Per edit pixel (slot s): t = alpha[s], u = 1 - t; w = softmax over the active logits (e_j = exp(l_j - max): fp32
 *   difference, exp in double rounded once to fp32; sum in column order; w_j = e_j / sum); o = the first 3 columns of o_raw
 *   (raw as get_offsets returns them, style_encoder.py:98-109, or tanh(o) with LAE_RECOLOR_TANH: then identity edits give
 *   LAENeRF.forward); w @ pal summed in column order.  Every operation one fp32 rounding, no contraction.
 *   LAE_RECOLOR_PREVIEW (utils.py:1290-1302, 1310-1311): w'_j = max(p_bias_j + p_weights_j * w_j, 0), w' /= sum(w'),
 *     out = clamp(o + w' @ pal, 0, 1) + u * bg;  with LAE_RECOLOR_NO_OFFSETS (:1303-1308): clamp(w @ pal, 0, 1) + u * bg
 *     (p_weights / p_bias unused, as in the reference).  Other pixels: base.
 *   LAE_RECOLOR_WEIGHTS (:1275-1281): w_k (k-th ACTIVE base) in all three channels + u * bg.  Other pixels: base.
 *   LAE_RECOLOR_OFFSETS (:1282-1286): o * 0.5 + 0.5 + u * bg.  Other pixels: base.
 *   LAE_RECOLOR_EVAL (gui.py:708-714): clamp(w @ pal + o, 0, 1) * t + bg * u (no edit weights; NO_OFFSETS ignored).
 *     Other pixels: bg.
 *   Deviations from the reference: it computes the palette product and the sums in fp16 under autocast, here they are fp32;
 *   where sum(w') = 0 (an edit that clamps every weight away) it divides 0 / 0 and shows NaN, here the weights count as zero.
 *   out [N,3] fp32; out_u8 [N,3] (may be NULL) = torch's (out * 255).byte(): the fp32 product, truncated to int64, low byte
 *   (NaN -> 0).  k >= n_active in LAE_RECOLOR_WEIGHTS, P outside 1..16 or no active base: LAE_EINVAL. */
#define LAE_RECOLOR_PREVIEW 0
#define LAE_RECOLOR_WEIGHTS 1
#define LAE_RECOLOR_OFFSETS 2
#define LAE_RECOLOR_EVAL 3
#define LAE_RECOLOR_NO_OFFSETS 1
#define LAE_RECOLOR_TANH 2
LAE_API uint64_t lae_recolor_compact_scratch_bytes(uint32_t N);
LAE_API int lae_recolor_compact(const float* depth, const float* weights_sum, const float* rays_o, const float* rays_d, uint32_t N,
                                int32_t* indices, int32_t* slot_map, float* x_term, float* dirs, float* alpha, int32_t* count,
                                void* scratch, void* stream);
LAE_API int lae_recolor_compose(const int32_t* slot_map, uint32_t N, const void* w_logits, uint32_t w_stride, const void* o_raw,
                                uint32_t o_stride, uint32_t P, uint32_t active_mask, const float* palette, const float* p_weights,
                                const float* p_bias, const float* alpha, const float* base, const float* bg, int mode, uint32_t k,
                                int flags, float* out, uint8_t* out_u8, void* stream);

/* ---- LAENeRF's dataset rewrite before the edit is distilled into the NeRF (nerf/gui.py:357-541 distill_dataset: a per-view host
 * loop of forward_train, ~20 torch ops, a host round trip of each image and a torchvision Resize in the reference) ----
 *
 * lae_distill_compose: one thread per row over ALL views.  Rows are the extracted edit pixels, packed per view: img_idx [R] (the
 *   training image), pix [R] (pixel in scanline order), w [R] (the edit weight, weights_editgrid[indices]), pred [R,3] fp32 (the
 *   distill render's premultiplied colour at the pixel, no background), dist [R] (the smooth-transition distance weight d, 0 for rows
 *   not in indices_interp; NULL: no smooth transition).  w_logits [R_pad, >= P] / o_raw [R_pad, >= 3] fp16 with row strides as in
 *   lae_recolor_compose (LAENeRF._logits).  palette_mod / palette_og [n_active, 3], p_weights / p_bias [n_active]: fp32 DEVICE arrays
 *   (a captured launch replays a new edit); palette_og is read only with dist.
 *   Per row, in the order of gui.py:433-469 (every operation one fp32 rounding, no contraction):
 *     w_og = softmax of the active logits (lae_recolor_compose's rule), o = tanh(o_raw) (double, rounded once);
 *     w' = max(p_bias + p_weights * w_og, 0), w' /= sum(w');
 *     c = clamp(w' @ palette_mod + o, 0, 1)  (= LAE_RECOLOR_PREVIEW | LAE_RECOLOR_TANH's colour, the same device code);
 *     with dist: c = clamp((d w_og + (1 - d) w') @ (d palette_og + (1 - d) palette_mod) + o, 0, 1), the weight and palette
 *       interpolations each a multiply, a multiply and an add, the product summed in column order;
 *     s = (1 - w) * pred + w * c, or w * c with LAE_DISTILL_NO_BG;
 *     rows with w > blend_thresh write clamp(s, 0, 1) into channels 0..2 of images[img_idx, pix] (fp16: round to nearest from the
 *     fp32 value).  Every other pixel, and the alpha channel of a 4-channel image, is never touched (gui.py:464-467).
 *   images [n_img, HW, C] (C = 3 or 4), dtype 1 = fp16, 2 = fp32 (ResidentImages' codes; uint8: LAE_EINVAL), written in place.  Rows
 *   whose img_idx / pix lie outside the images are skipped.
 *   Deviations from the reference: it runs the palette product and the sums in fp16 under .half(), here they are fp32; where
 *   sum(w') = 0 (an edit that clamps every weight away) it divides 0 / 0 and writes NaN, here the weights count as zero; its
 *   ~mask * style + mask * gt lets a NaN of the render at a pixel at or below the threshold into that pixel, here such a pixel is
 *   never written.
 *
 * lae_error_map_seed: LAENeRF's --use_error_maps seed (gui.py:419-425).  dense [n_img, H*W] fp32 scratch: zeroed, then every row's w
 *   is scattered to its pixel (the dense edit-weight image of each view).  For each of the V images view_img [V] (int32, the
 *   non-occluded views), the image is resized to 128 x 128 bilinearly without antialiasing, as torch.nn.functional.interpolate(...,
 *   mode="bilinear", align_corners=False) (torchvision 0.15's Resize on a tensor): per axis scale = in / 128 (fp32),
 *   src = max(scale * (dst + 0.5) - 0.5, 0), i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), l = clamp(src - i0, 0, 1);
 *   x = (1 - ly) * ((1 - lx) x[y0][x0] + lx x[y0][x1]) + ly * ((1 - lx) x[y1][x0] + lx x[y1][x1]) (one rounding per operation);
 *   error_map[img, cell] = clamp(x + 0.15, 0, 1).  Rows of other images (the occluded views) are not touched. */
#define LAE_DISTILL_NO_BG 1
LAE_API int lae_distill_compose(uint32_t R, const int32_t* img_idx, const int32_t* pix, const float* w, const float* pred,
                                const float* dist, const void* w_logits, uint32_t w_stride, const void* o_raw, uint32_t o_stride,
                                uint32_t P, uint32_t active_mask, const float* palette_mod, const float* palette_og,
                                const float* p_weights, const float* p_bias, float blend_thresh, int flags, void* images, int dtype,
                                uint32_t n_img, uint32_t HW, uint32_t C, void* stream);
LAE_API int lae_error_map_seed(uint32_t R, const int32_t* img_idx, const int32_t* pix, const float* w, const int32_t* view_img,
                               uint32_t V, uint32_t n_img, uint32_t H, uint32_t W, float* dense, float* error_map, void* stream);

/* The data set of the Ref-NPR distillation (the reference's dataloader_nerf, editing/single_view_edit_dataset.py:447-519), built on
 * the device over all views at once.  src_images [n_img, HW, C] (C = 3 or 4; LAE_IMG_U8 / _F16 / _F32) are the training images, read
 * for their alpha only: a = src[.., 3] (uint8 as value / 255, correctly rounded), a = 1 for C == 3 (the reference reads the blue
 * channel there, a bug that is not reproduced).  Outputs, dtype LAE_IMG_F16 / LAE_IMG_F32 (values are computed in fp32, every
 * operation one rounding, and rounded to nearest even on the store): images [n_img, HW, 4], weights [n_img, HW], second
 * [n_img, HW, 4]; depths [n_img, HW] is always fp32.
 *
 * lae_ref_distill_init: the dense pass, one thread per pixel: images = (0, 0, 0, a), weights = 1 - a, second = 0, depths = 0 -- what
 *   a view skipped by the registration, or an image no view points at, keeps.
 * lae_ref_distill_scatter: one thread per packed row, after the init.
 *   registered rows (R_reg): images[reg_img, reg_pix, :3] = reg_rgb [R_reg, 3] (ref_targets),
 *                            weights[reg_img, reg_pix] = max(reg_w, 0) + (1 - a)     (target_weights; :466-469)
 *   extracted rows (R_ext):  second[ext_img, ext_pix] = (ext_rgb [R_ext, 3], a)      (the palette network's colour; :493-498)
 *                            depths[ext_img, ext_pix] = ext_depth                    (:503-504)
 *   A row whose image or pixel lies outside the planes is skipped.  Two rows of one kind that name the same pixel of one image leave
 *   an unspecified one of the two values there (the packing asserts that there are none).
 * LAE_EINVAL: C not 3 or 4, a dtype out of range. */
LAE_API int lae_ref_distill_init(const void* src_images, int src_dtype, uint32_t n_img, uint32_t HW, uint32_t C, int dtype, void* images,
                                 void* weights, void* second, float* depths, void* stream);
LAE_API int lae_ref_distill_scatter(uint32_t R_reg, const int32_t* reg_img, const int32_t* reg_pix, const float* reg_rgb, const float* reg_w,
                                    uint32_t R_ext, const int32_t* ext_img, const int32_t* ext_pix, const float* ext_rgb,
                                    const float* ext_depth, const void* src_images, int src_dtype, uint32_t n_img, uint32_t HW, uint32_t C,
                                    int dtype, void* images, void* weights, void* second, float* depths, void* stream);

/* The point-wise losses of train_LAENeRF_step (nerf/utils.py:990-996; style_encoder.py:183-205) fused behind the
 * recomposition: loss = MSE(pred, target) + w_uniform * max_j sum_i w_hat[i,j] + w_non_uniform * sum_i (1 - max_j w_hat[i,j])
 * + c_offset * sum o_hat^2 [+ the palette-only regulariser `palet_loss` (style_encoder.py:195-202) over all reg_P bases:
 * w_valid * sum floor(p) p + w_distinct * mean_ij (1 - |p_i - p_j|^2 / max), when reg_palette != NULL / (flags & LAE_STYLE_WITH_REG)].
 * forward: fin[12] (device) = {loss * scale, loss, mse, uniform, non_uniform, offset terms, arg-max column, scale, regulariser,
 * ...}; scale: device scalar or NULL (1).  backward: gradients of (upstream * fin[0]) with respect to the two MLP outputs and the
 * palette in ONE kernel (no per-point gradient tensors); upstream: device scalar.  flags: LAE_STYLE_WITH_REG (value 1: what the
 * `with_reg` argument of abi4 meant) | LAE_STYLE_ACCUMULATE_PALETTE (g_palette += instead of =: the caller hands its persistent
 * fp32 gradient buffer over and saves autograd's add launch).
 * scratch: max(lae_style_loss_scratch_bytes(M), lae_palette_backward_scratch_bytes(M)). */
#define LAE_STYLE_WITH_REG 1
#define LAE_STYLE_ACCUMULATE_PALETTE 2
LAE_API uint64_t lae_style_loss_scratch_bytes(uint32_t M);
LAE_API int lae_style_loss_forward(const void* pred, const float* target, const float* w_hat, const void* o_hat, uint32_t M,
                           uint32_t n_active, float w_uniform, float w_non_uniform, float c_offset, const float* scale, float* fin,
                           void* scratch, const float* reg_palette, uint32_t reg_P, float w_valid, float w_distinct, void* stream);
LAE_API int lae_style_loss_backward(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                            uint32_t M, const float* target, const float* fin, const float* upstream, float w_uniform,
                            float w_non_uniform, float c_offset, void* g_w_logits, void* g_o_raw, float* g_palette, void* scratch,
                            int flags, float w_valid, float w_distinct, void* stream);

/* The fused criterion with a DEVICE row count (the palette network's training on views of any size K, laenerf_amd.editing.
 * StyleTrainer): the same two launches each way, on buffers of `cap` rows (the host size every array is allocated for; a
 * multiple of 16 for the MLPs) of which the first M = min(*m_dev, cap) are live.  *m_dev >= 1 (M = 0 gives a NaN mean).
 *   - rows >= M are excluded from every sum: the MSE mean divides by 3 M, the per-column sums whose maximum is the uniform term,
 *     the non-uniform sum and the offset sum see only rows < M;
 *   - rows >= M get exactly zero g_w_logits / g_o_raw rows and add nothing to the palette gradient;
 *   - the partials of workgroups past cdiv(M, 256) are zeros, and the final reductions read only the first cdiv(M, 256) of
 *     them, in the order of the exact-size call: fin[] and g_palette are the bits of lae_style_loss_forward / _backward called
 *     with M rows on the same first M rows.
 * lae_palette_forward is called with the capacity (its rows are independent); scratch as above with M = cap. */
LAE_API int lae_style_loss_forward_dev(const void* pred, const float* target, const float* w_hat, const void* o_hat, uint32_t cap,
                               const uint32_t* m_dev, uint32_t n_active, float w_uniform, float w_non_uniform, float c_offset,
                               const float* scale, float* fin, void* scratch, const float* reg_palette, uint32_t reg_P, float w_valid,
                               float w_distinct, void* stream);
LAE_API int lae_style_loss_backward_dev(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                                uint32_t cap, const uint32_t* m_dev, const float* target, const float* fin, const float* upstream,
                                float w_uniform, float w_non_uniform, float c_offset, void* g_w_logits, void* g_o_raw, float* g_palette,
                                void* scratch, int flags, float w_valid, float w_distinct, void* stream);

/* lae_style_loss_backward_dev plus a per-row g_pred [cap,3] fp32 (device; the image terms' dL/dpred, already multiplied by the loss
 * scale): added to the criterion's dL/dpred of every live row BEFORE the clamp mask, so the step keeps one palette-backward launch.
 * g_pred == NULL: exactly lae_style_loss_backward_dev. */
LAE_API int lae_style_loss_backward_image_dev(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                                      uint32_t cap, const uint32_t* m_dev, const float* target, const float* fin, const float* upstream,
                                      float w_uniform, float w_non_uniform, float c_offset, const float* g_pred, void* g_w_logits,
                                      void* g_o_raw, float* g_palette, void* scratch, int flags, float w_valid, float w_distinct, void* stream);

/* lae_style_loss_forward_dev / lae_style_loss_backward_image_dev with the factor of the MSE as one more scalar, mse_w >= 0 (the
 * Ref-NPR second stage, whose colour term is lae_ref_terms_* below): loss = mse_w * MSE + the regularisers, and the per-point
 * gradient carries mse_w times the MSE's part.  fin[2] is the unweighted MSE against `target` in every case (a diagnostic when
 * mse_w == 0).  mse_w == 1 gives the bits of the entry points above (a multiplication by 1.0f is exact). */
LAE_API int lae_style_loss_forward_dev_w(const void* pred, const float* target, const float* w_hat, const void* o_hat, uint32_t cap,
                                 const uint32_t* m_dev, uint32_t n_active, float w_uniform, float w_non_uniform, float c_offset,
                                 float mse_w, const float* scale, float* fin, void* scratch, const float* reg_palette, uint32_t reg_P,
                                 float w_valid, float w_distinct, void* stream);
LAE_API int lae_style_loss_backward_image_dev_w(const void* w_logits, const void* o_raw, const float* palette, uint32_t P, uint32_t active_mask,
                                        uint32_t cap, const uint32_t* m_dev, const float* target, const float* fin, const float* upstream,
                                        float w_uniform, float w_non_uniform, float c_offset, float mse_w, const float* g_pred,
                                        void* g_w_logits, void* g_o_raw, float* g_palette, void* scratch, int flags, float w_valid,
                                        float w_distinct, void* stream);

/* The registered terms of the Ref-NPR second stage (the reference's train_styleenc_step_npr, nerf/utils.py:1096-1104, :1120-1122;
 * laenerf_amd.editing.ref_stage) on the step's view, everything read from device memory (capturable: no host read, no allocation;
 * one graph serves every view):
 *   v = schedule[(*step_counter - 1) mod n_sched] (the sampler advanced the counter), K = min(*m_dev, cap, counts[v]), o = row_off[v].
 * Per-row arrays of the packed set (view v's rows at row_off[v]): w8s [sum K] fp16 (the view's opacity weights), ref_target
 * [sum K, 3] fp32 and ref_weight [sum K] fp32 (the registration, dense: weight 0 = the row is not registered and its target is
 * not read), ref_count [V] int32 (R: the registered rows), row_tap [sum K] int32 (backward: the one tap that reads the row, or -1).
 * Per-view arrays of the colour patch, n_out = ph * pw outputs: tap_row [V, n_out, 4] int32 (a row of the view, -1: no tap /
 * the source pixel is off the mask), tap_w [V, n_out, 4] fp32, color_patch [V, 3, n_out] fp32.
 * forward, rows i < K:
 *   pred'[i][c] = fp16(pred[i][c] * w8s[o + i]) -- the fp32 product of two fp16 values is exact, so this is ONE rounding (the
 *     reference's in-place half multiply) -- written as fp16 predw16 [cap,3] and as the same values in fp32 predw32 [cap,3];
 *     rows >= K of both are zeros (rows >= K of pred / target are never read).
 *   terms[0], mode LAE_REF_MODE_GT:  sum_i sum_c (target[i][c] - pred'[i][c])^2 / (3 K)     (`target`: the step's [cap,3] buffer)
 *             mode LAE_REF_MODE_REF: sum_i ref_weight[o+i] sum_c (ref_target[o+i][c] - pred'[i][c])^2 / (3 R); R == 0 gives 0 and
 *             a zero gradient (DEPARTURE: the reference takes the mean of an empty tensor there, NaN).
 *   terms[1], mode LAE_REF_MODE_REF: mean over the 3 n_out values of (patch[o'][c] - color_patch[v][c][o'])^2 with
 *             patch[o'][c] = sum_t tap_w[v][o'][t] * pred'[tap_row[v][o'][t]][c] (taps with a row outside 0..K-1 add nothing);
 *             resid [n_out, 3] fp64 keeps patch - color_patch for the backward.  Mode GT: 0, nothing else is touched.
 *   Residuals, squares and sums run in fp64 in a fixed order without atomics (ref_stage.hip's header) and are rounded to fp32
 *   once: two runs give the same bits.  scratch: lae_ref_terms_scratch_bytes(cap, n_out).
 * backward: g_pred [cap,3] fp32 = w8s[o+i] * (g_predw[i][c] + g_terms[0] * d terms[0]/d pred' + g_terms[1] * d terms[1]/d pred')
 *   (the fp16 rounding is passed straight through, as autograd passes a half multiply); g_predw [cap,3] fp32 (the gradient the
 *   image block returns for predw32) may be NULL; g_terms [2] fp32 (device).  Every row is under at most one tap (the packing
 *   guarantees it for a resize scale >= 2), so the patch gradient is one gather per row.  Rows >= K get exact zeros. */
#define LAE_REF_MODE_GT 0
#define LAE_REF_MODE_REF 1
LAE_API uint64_t lae_ref_terms_scratch_bytes(uint32_t cap, uint32_t n_out);
LAE_API int lae_ref_terms_forward(const void* pred, uint32_t cap, const uint32_t* m_dev, const float* target, const int32_t* schedule,
                          uint32_t n_sched, const int64_t* step_counter, uint32_t V, const int64_t* row_off, const int32_t* counts,
                          const void* w8s, const float* ref_target, const float* ref_weight, const int32_t* ref_count,
                          const int32_t* tap_row, const float* tap_w, const float* color_patch, uint32_t n_out, int mode, void* predw16,
                          float* predw32, double* resid, void* scratch, float* terms, void* stream);
LAE_API int lae_ref_terms_backward(const void* pred, uint32_t cap, const uint32_t* m_dev, const float* target, const int32_t* schedule,
                           uint32_t n_sched, const int64_t* step_counter, uint32_t V, const int64_t* row_off, const int32_t* counts,
                           const void* w8s, const float* ref_target, const float* ref_weight, const int32_t* ref_count,
                           const int32_t* row_tap, const float* tap_w, const double* resid, uint32_t n_out, int mode, const float* g_predw,
                           const float* g_terms, float* g_pred, void* stream);

/* The image-space terms of LAENeRF's stylization step (nerf/utils.py:997-1033; editing/style_encoder.py:207-235,
 * editing/style_network.py:129-191) on the step's view, everything read from device memory (capturable; one graph serves every view):
 *   v = schedule[(*step_counter - 1) mod n_sched] (the sampler advanced the counter after its draw), K = min(*m_dev, cap).
 * The edit set's image arrays: box [V,4] int32 (x_min, x_max, y_min, y_max; crop = rows x_min..x_max-1, columns y_min..y_max-1,
 * h = x_max - x_min >= 1, w = y_max - y_min >= 1), img_off [V] int64 (first crop pixel of view v in the per-pixel arrays; crop pixel
 * (i, j) is img_off + i * w + j), pix2row [.] int32 (the view's row whose pixel that is, -1: none), cut_gt [., 3], tv_h [.] (valid for
 * i < h - 1), tv_v [.] (valid for j < w - 1), smooth [.] (cut_smooth_trans; NULL when unused), vmax [V,2] (max tv_h, max tv_v of the
 * view; 0 for an empty one).  Crop value x(i, j) = pred[pix2row] (fp16 -> fp32) if 0 <= pix2row < K, else 0.
 * forward (flags):
 *   LAE_STYLE_IMG_RESIZE: vgg_in [3,S,S] fp32 = (bilinear(x) - mean_c) / std_c, PyTorch's arithmetic for align_corners=False:
 *     src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1,
 *     val = l0y (l0x x00 + l1x x01) + l1y (l0x x10 + l1x x11); ImageNet mean / std.
 *   terms[3] fp32 = {tv, smooth, disc} (0 where the flag is off):
 *     tv  (LAE_STYLE_IMG_TV) = sum |x(i,j) - x(i+1,j)|^2 wh + sum |x(i,j) - x(i,j+1)|^2 wv, with wh = wv = 1, or with
 *         LAE_STYLE_IMG_TV_DEPTH wh = 1 - tv_h(i,j) [* (1 - smooth(i+1,j)) with LAE_STYLE_IMG_TV_SMOOTH], wv likewise;
 *     smooth (LAE_STYLE_IMG_SMOOTH) = sum |x - cut_gt|^2 smooth;
 *     disc (LAE_STYLE_IMG_DISC) = -sum |dx_h|^2 tv_h / vmax_h - sum |dx_v|^2 tv_v / vmax_v (a view whose maximum is 0 gives NaN,
 *         like the reference).
 *   The sums: n_blocks workgroups (fixed by the caller) stride over the crop, then one workgroup sums the partials in a fixed
 *   order.  scratch: lae_style_image_scratch_bytes(n_blocks).
 * backward: g_pred [cap,3] fp32 = dL/dx at each row's crop pixel (row2pix [sum K] int32: the row's crop pixel or -1, rows of view
 *   v at row_off[v]): the adjoint of resize + normalize of g_vgg [3,S,S] (LAE_STYLE_IMG_RESIZE), plus g_terms[0..2] (device) times
 *   the stencil gradients of tv / smooth / disc.  Rows >= K and rows outside the crop get exactly 0.  One thread per row gathers;
 *   no atomics (the bits do not depend on scheduling). */
#define LAE_STYLE_IMG_TV 1
#define LAE_STYLE_IMG_TV_DEPTH 2
#define LAE_STYLE_IMG_TV_SMOOTH 4
#define LAE_STYLE_IMG_SMOOTH 8
#define LAE_STYLE_IMG_DISC 16
#define LAE_STYLE_IMG_RESIZE 32
LAE_API uint64_t lae_style_image_scratch_bytes(uint32_t n_blocks);
LAE_API int lae_style_image_forward(const void* pred, uint32_t cap, const uint32_t* m_dev, const int32_t* schedule, uint32_t n_sched,
                            const int64_t* step_counter, uint32_t V, const int32_t* box, const int64_t* img_off, const int32_t* pix2row,
                            const float* cut_gt, const float* tv_h, const float* tv_v, const float* smooth, const float* vmax, uint32_t S,
                            float* vgg_in, int flags, uint32_t n_blocks, float* scratch, float* terms, void* stream);
LAE_API int lae_style_image_backward(const void* pred, uint32_t cap, const uint32_t* m_dev, const int32_t* schedule, uint32_t n_sched,
                             const int64_t* step_counter, uint32_t V, const int32_t* box, const int64_t* img_off, const int32_t* pix2row,
                             const float* cut_gt, const float* tv_h, const float* tv_v, const float* smooth, const float* vmax,
                             const int64_t* row_off, const int32_t* row2pix, uint32_t S, const float* g_vgg, const float* g_terms, int flags,
                             float* g_pred, void* stream);

/* One training view of the palette network from a device-resident edit set (EditDataset.collate, editing/edit_dataset.py:289-300,
 * laenerf_amd.editing.EditSet.sample).  The set: V views packed as x_term, dirs, targets [sum K, 3] fp32, view v's rows at
 * offsets[v] (int64) .. offsets[v] + counts[v] (int32, >= 1), depth_factor [V] fp32 (the view's (d.max() - d.min()) / num_steps).
 *   step = *step_counter (int64, device), read at the start; v = schedule[step mod n_sched] (int32, 0 <= v < V; values out of range
 *   are clamped, the caller validates); K = min(counts[v], cap); *m_dev = K (uint32).
 *   jitter of row r < K: w = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *     (step & 0xffffffff, r, 0, 2) (counter word 3 = 2: apart from lae_sample_train_batch's (.., 0) and the error map's (.., 1));
 *     u = (w >> 8) * 2^-24 (exact, in [0, 1 - 2^-24]);  t = fp32(fp32(u - 0.5) * depth_factor[v]);
 *     x[r][c] = fp32(x_term[o + r][c] + fp32(t * dirs[o + r][c]))   (o = offsets[v]; multiply then add, no contraction: the
 *     roundings of torch's `x_term + d_[..., None] * dirs`);  d[r] = dirs[o + r], target[r] = targets[o + r] (copies).
 *   rows K..cap-1: copies of row K - 1 after its jitter (the same hash-table lines; the losses skip them through m_dev).
 *   Deviation: the reference draws the jitter with torch.rand on the device (another generator): the law is the same, U[0, 1)
 *   in 2^-24 steps, the bits are not.
 * x, d, target [cap, 3] fp32, 16-byte aligned; cap a multiple of 4 (else LAE_EINVAL).  A second one-thread launch adds 1 to
 * *step_counter after the draw: a replayed graph draws the next step's view. */
LAE_API int lae_sample_edit_view(const float* x_term, const float* dirs, const float* targets, const int64_t* offsets, const int32_t* counts,
                         const float* depth_factor, uint32_t V, const int32_t* schedule, uint32_t n_sched, uint32_t cap, uint64_t seed,
                         int64_t* step_counter, float* x, float* d, float* target, uint32_t* m_dev, void* stream);

/* ---- LAENeRF input assembly (editing/style_encoder.py:135-146: encoder rows, SH(3) of the directions, cast, pad, cat -- torch ops
 * and separate launches in the reference) ----
 * forward: feats_lm [16, M, 2] fp16 (the grid kernels' level-major output) + dirs [M,3] fp32 -> feat [Mp, 32] fp16 rows and
 *   off_in [Mp, off_cols] fp16 rows = [feat | SH(degree)(dirs) | zeros]; rows M..Mp-1 zero (Mp >= M, the MLPs' multiple of 16).
 *   degree 0: no directions, off_in is not written.  degree <= 4, off_cols even, 32 + degree^2 <= off_cols <= 48.
 * backward: grad_lm [16, M, 2] fp16 = g_feat [Mp,32] + g_off [Mp,off_cols][:, :32] (fp32 add, one rounding; either may be NULL). */
LAE_API int lae_style_assemble_forward(const void* feats_lm, const float* dirs, uint32_t M, uint32_t Mp, uint32_t degree, void* feat,
                               void* off_in, uint32_t off_cols, void* stream);
LAE_API int lae_style_assemble_backward(const void* g_feat, const void* g_off, uint32_t M, uint32_t off_cols, void* grad_lm, void* stream);

/* ---- edit-grid region growing (editing/editgrid.py:274-340 EditGrid.grow_region_queue; Python + collections.deque
 * in the reference) ----
 * grid: the selection bitfield [C*H^3/8] (Morton order, like density_bitfield), modified in place; density_grid [C, H^3];
 * queue: device array of `capacity` entries x | y << 8 | z << 16 | level << 24; state (device uint32[4]): head, tail
 * (indices into queue; the caller seeds entries [head, tail)), on return also [2] = cells popped, [3] = 1 if the queue
 * would have overflowed (growth stopped early).  Pops at most grow_iterations cells in batches of max_batch (32 in the
 * reference) with the reference's FIFO order, acceptance rule (density >= thresh and not yet selected), neighbour order
 * and level rule; byte writes follow the CPU-tensor semantics of the reference's indexed assignment (last one wins). */
LAE_API int lae_grow_region(uint8_t* grid, const float* density_grid, uint32_t C, uint32_t H, float density_thresh,
                    uint32_t* queue, uint32_t capacity, uint32_t* state, uint32_t grow_iterations, uint32_t max_batch,
                    void* stream);

/* ---- EditDataset transition weights (editing/edit_dataset.py:122-146: torch.cdist in 1000-row chunks + min + clamp_max in the
 * reference) ----
 * out[i] = min(max_dist, min_j |pts[i] - set[j]|) for pts [n,3], set [m,3] fp32 (m == 0: out = max_dist), *out_max = the largest
 * out[i]; scratch: 4 n bytes of device memory.  Squared distances as dx*dx + dy*dy + dz*dz with the last two products fused. */
LAE_API int lae_min_dist_to_points(const float* pts, uint32_t n, const float* set, uint32_t m, float max_dist, float* out,
                           float* out_max, void* scratch, void* stream);

/* ---- the edit grid from 2D masks (csrc/masklift.hip, where the rule is written down in full; DESIGN.md section 4c;
 * editing/mask_lift.py restates both kernels in numpy) ----
 * lae_mask_lift_pack: one view's planes into ONE fp32 plane.  depth / opacity fp32 [HW]: the raw sum w t and the weights_sum of
 *   render_eval(scale_depth=False); mask uint8 [HW], nonzero = selected.  packed[i] = |t_surf| with the sign bit set iff mask[i],
 *   t_surf = depth / opacity (one correctly rounded division) if opacity >= min_opacity, else +inf; -0, +-inf and NaN are legal values.
 *   NULL: LAE_ENULL; HW == 0, HW >= 2^31 or min_opacity <= 0: LAE_EINVAL.
 * lae_mask_lift: the votes of V packed views [V,H,W] (poses fp32 [V,4,4] cam2world, row-major, on the device; one set of
 *   intrinsics) on the cells of density_bitfield ([C*G^3/8] uint8, Morton order, cascade-major) and the decision per cell.
 *   grid_out  uint8 [C*G^3/8], the selection in density_bitfield's layout; every byte is written, no zero fill needed
 *   votes_out optional uint16 [C*G^3, 2]: (in, out) per cell, indexed like density_grid; zeros for cells that are not occupied
 *   A cell is selected iff it is occupied, in >= min_views and float(in) >= min_share * float(in + out).  Poses go through LDS in
 *   chunks of LAE_MASK_LIFT_POSE_CHUNK views.  No atomics, no host read, no allocation: capturable, and two calls give the same
 *   bytes.  NULL packed / poses / density_bitfield / grid_out: LAE_ENULL; G not a power of two in [2, 128], C outside [1, 16],
 *   V == 0 or V > 65535, H or W < 1, H * W >= 2^31, fx or fy <= 0, bound <= 0, depth_margin < 0, min_share outside [0, 1] or a NaN
 *   among them: LAE_EINVAL; both before any launch. */
#define LAE_MASK_LIFT_POSE_CHUNK 64
LAE_API int lae_mask_lift_pack(const float* depth, const float* opacity, const uint8_t* mask, uint32_t HW, float min_opacity,
                               float* packed, void* stream);
LAE_API int lae_mask_lift(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H,
                          uint32_t W, const uint8_t* density_bitfield, uint32_t C, uint32_t G, float bound, float depth_margin,
                          uint32_t min_views, float min_share, uint8_t* grid_out, uint16_t* votes_out, void* stream);

/* ---- region transform: move, rotate, scale, copy or delete the selected region at render time (csrc/region.hip, where the rule
 * is written down in full; editing/region_transform.py restates both entries in numpy).  The reference has
 * no counterpart ----
 * The object-to-world map is x_new = s R (x - pivot) + pivot + t; the host passes (HOST pointers, read during the call) the forward
 * map M [3,4], its inverse Minv [3,4] and Rt = R^T [3,3], each formed in float64 and rounded once to fp32, rows [m0 m1 m2 | m3].
 * Grid: H a power of two in [4, 128], C = 1 or 2 (more cascades are refused: one thread walks a source cell's box at every finer
 *   cascade, unmeasured beyond 2), bound = 2^(C-1); bitfields [C*H^3/8] uint8 in density_bitfield's layout.
 * sel(q) = the selection bit of q's cell at q's OWN cascade: level = cascade_of(max |q_i|, C), coordinates
 * (int)clamp((0.5 * fma(q_i, 1 / mip_bound, 1)) * H, 0, H - 1) -- the marcher's probe with dt left out.
 * lae_region_warp: one sample row per thread, SoA loads and stores, no atomics, no host read, no allocation: capturable.  xyzs, dirs
 *   [M,3] fp32; outputs xyzs_out, dirs_out [M,3], sigma_scale [M] fp32; xyzs_out / dirs_out may be xyzs / dirs (in place).  Per row,
 *   p = Minv (x, 1) as ((m0 x + m1 y) + m2 z) + m3, one rounding per operation, never contracted:
 *     moved    mode != DELETE, |p_i| <= bound for all i, sel(p) set:  xyz = p, dir = Rt d ((r0 dx + r1 dy) + r2 dz), sigma_scale = inv_scale
 *     vacated  else, mode != COPY and sel(x) set:                      row unchanged, sigma_scale = 0
 *     kept     otherwise:                                              row unchanged, sigma_scale = 1
 *   The caller multiplies the field's density by sigma_scale before compositing.  Rows of zeros (the marcher's padding) pass through
 *   with a finite result.  inv_scale = fp32(1 / s), s in [0.5, 2].
 * lae_region_occupancy: the bitfield the marcher walks, a conservative superset of where the edited scene has density.
 *   keep   out = occ; in modes MOVE and DELETE a bit is cleared iff its selection bit is set and the cell is of its own cascade
 *          (cascade 0, or at c > 0 not all three coordinates in [H/4, 3H/4)).  No other bit is cleared.
 *   image  (MOVE, COPY) every selected, occupied source cell (own-cascade cells and, at c > 0, the layer with a coordinate equal to
 *          H/4, which a coordinate of exactly -2^(c-1) looks up) maps its 8 corners with M, takes their axis-aligned box, widens
 *          it by `margin` (0 <= margin < 0.5 / H: a rounding allowance, region_transform.py derives it) and sets the bit of every
 *          cell the box overlaps at every cascade, clipped to the cascade's domain; cell ranges by sel's coordinate statement.
 *   Bits are set with 32-bit atomicOr: the same bytes from every call.  out must not be occ or sel; every byte of out is written.
 * Both: a NULL pointer (M may be NULL with DELETE), a mode outside the three, inv_scale outside [0.5, 2], a grid the rules above
 *   or `bytes` do not fit, a non-finite matrix entry, a margin out of range, a base that is not 4-byte aligned, out aliasing an
 *   input: LAE_EINVAL before any launch (NULL included: this pair reports it as an invalid argument).  M == 0 rows: LAE_OK. */
#define LAE_REGION_MOVE 0
#define LAE_REGION_COPY 1
#define LAE_REGION_DELETE 2
LAE_API int lae_region_warp(const float* xyzs, const float* dirs, uint32_t M, const uint8_t* sel, uint64_t sel_bytes, const float* Minv,
                            const float* Rt, float inv_scale, int mode, float bound, uint32_t C, uint32_t H, float* xyzs_out,
                            float* dirs_out, float* sigma_scale, void* stream);
LAE_API int lae_region_occupancy(const uint8_t* occ, const uint8_t* sel, uint64_t bytes, const float* M, float margin, int mode,
                                 float bound, uint32_t C, uint32_t H, uint8_t* out, void* stream);

/* ---- scene insert: the selected object of one trained NeRF (the source) rendered inside another scene (the destination)
 * (csrc/insert.hip; DESIGN.md section 4c "Scene insert"; editing/scene_insert.py restates the three entries in numpy).  The reference
 * has no counterpart ----
 * The map is x_dst = s R (x_src - pivot) + position; the host passes (HOST pointers, read during the call) the forward map M [3,4],
 * its inverse Minv [3,4] and Rt = R^T [3,3], each formed in float64 and rounded once to fp32, rows [m0 m1 m2 | m3].
 * Grids: the source's (bound_s, C_s, H_s) and the destination's (bound_d, C_d, H_d), each with H a power of two in [4, 128], C = 1 or 2
 *   and bound = 2^(C-1); they may differ.  Bitfields [C*H^3/8] uint8 in density_bitfield's layout; src_sel (the selection) and src_occ
 *   (the source's occupancy) are the source grid's.
 * bit(g, q) = the bit of q's cell at q's OWN cascade in the source bitfield g: level = cascade_of(max |q_i|, C_s), coordinates
 *   (int)clamp((0.5 * fma(q_i, 1 / mip_bound, 1)) * H_s, 0, H_s - 1) -- the marcher's probe with dt left out.
 * Every operation below that decides a branch or produces an output is one rounded fp32 operation, never contracted.
 *
 * lae_insert_route: xyzs, dirs [M,3] fp32 (the destination marcher's rows), deltas [M,2] fp32 or NULL.  Per row p = Minv (x, 1) as
 *   ((m0 x + m1 y) + m2 z) + m3 and q = Rt d as (r0 dx + r1 dy) + r2 dz.  The row is INSERTED iff (deltas == NULL or deltas[2i] != 0:
 *   the marcher's padding rows are skipped) and |p_i| <= bound_s for all i and bit(src_sel, p) and bit(src_occ, p).
 *   slot [M] int32: an inserted row's rank among the inserted rows in ascending row order, -1 for every other row;
 *   xyzs_src, dirs_src [M cap, 3] fp32: row slot[i] = (p, q) of inserted row i (rows at and beyond *count are not written);
 *   *count (DEVICE uint32) = the number of inserted rows.  scratch: lae_insert_route_scratch_bytes(M) bytes of device memory.
 *   Three launches (a ballot and a prefix inside each workgroup of 1024 rows; one workgroup scans the workgroup counts, 1024 a pass
 *   with a carry; a scatter): no workgroup waits for another, no atomics, no host read, no allocation -- capturable, and two calls give
 *   the same bytes.  M == 0: *count = 0, LAE_OK.  M >= 2^31, an output overlapping an input or another output: LAE_EINVAL.
 * lae_insert_blend: sigma_d [M], rgb_d [M,3] (the destination field's), sigma_s [n_src], rgb_s [n_src,3] (the source field's on the
 *   compacted rows), each fp16 or fp32 by its own dtype code (LAE_F32 / LAE_F16); slot [M]; outputs sigma [M], rgb [M,3] fp32.
 *   slot < 0 (or >= n_src: nothing is read outside the arrays): the destination's values.  Otherwise ss = sigma_s[slot] * inv_scale and
 *     LAE_INSERT_REPLACE  sigma = ss, rgb = rgb_s[slot]                                     (the object is pasted over what stood there)
 *     LAE_INSERT_ADD      sigma = sigma_d + ss; rgb = sigma > 0 ? rgb_d + (ss / sigma) * (rgb_s - rgb_d) : rgb_d
 *                                                                              (the exact mixture of two participating media)
 *   sigma / rgb may BE sigma_d / rgb_d when those are fp32 (in place); any other overlap of an output: LAE_EINVAL.  One row per
 *   thread, streaming, capturable.  inv_scale = fp32(1 / s), s in [0.5, 2].
 * lae_insert_occupancy: the bitfield the destination's marcher walks.  out = dst_occ, plus, for every source cell that is selected,
 *   occupied and of its own cascade (cascade 0; at c > 0 not all three coordinates in (H_s/4, 3H_s/4): the layer with a coordinate
 *   equal to H_s/4 counts, as in lae_region_occupancy), the image box: the 8 corners mapped with M, their axis-aligned box widened by
 *   `margin` (0 <= margin < 0.5 / H_d: a rounding allowance, scene_insert.py derives it), and the bit of every destination cell the
 *   box overlaps at every destination cascade, clipped to the cascade's domain; cell ranges by the destination's coordinate statement.
 *   No bit is cleared.  Bits are set with 32-bit atomicOr: the same bytes from every call.  out overlaps no input; every byte of out
 *   is written.
 * All three: a NULL pointer (arrays of no rows may be NULL), a grid the rules above or the byte counts do not fit, a non-finite matrix
 *   entry, inv_scale outside [0.5, 2], a mode outside the two, a dtype code outside the two, a margin out of range, a base that is not
 *   aligned to its element (bitfields: 4 bytes), an overlapping output: LAE_EINVAL before any launch. */
#define LAE_INSERT_REPLACE 0
#define LAE_INSERT_ADD 1
LAE_API uint64_t lae_insert_route_scratch_bytes(uint32_t M);
LAE_API int lae_insert_route(const float* xyzs, const float* dirs, const float* deltas, uint32_t M, const uint8_t* src_sel,
                             const uint8_t* src_occ, uint64_t src_bytes, const float* Minv, const float* Rt, float bound_s, uint32_t C_s,
                             uint32_t H_s, int32_t* slot, float* xyzs_src, float* dirs_src, uint32_t* count, void* scratch, void* stream);
LAE_API int lae_insert_blend(const void* sigma_d, int sigma_d_dtype, const void* rgb_d, int rgb_d_dtype, const void* sigma_s,
                             int sigma_s_dtype, const void* rgb_s, int rgb_s_dtype, uint32_t n_src, const int32_t* slot, uint32_t M,
                             float inv_scale, int mode, float* sigma, float* rgb, void* stream);
LAE_API int lae_insert_occupancy(const uint8_t* dst_occ, uint64_t dst_bytes, const uint8_t* src_sel, const uint8_t* src_occ,
                                 uint64_t src_bytes, const float* M, float margin, float bound_s, uint32_t C_s, uint32_t H_s, float bound_d,
                                 uint32_t C_d, uint32_t H_d, uint8_t* out, void* stream);

/* ---- TSDF mesh export: fuse rendered depth and colour views on a lattice (csrc/tsdf.hip, where the rule is written down in
 * full; tsdf.py restates both kernels in numpy).  The reference has no counterpart ----
 * lae_tsdf_fuse: V packed views [V,H,W] (the plane lae_mask_lift_pack writes: t_surf = |packed|, the sign bit ignored, +inf = a
 *   transparent pixel, NaN = no observation; poses fp32 [V,4,4] cam2world, row-major, on the device; one set of intrinsics) on
 *   the lattice of three fp32 axis arrays xs[nx], ys[ny], zs[nz] on the device: voxel (i, j, k) sits at (xs[i], ys[j], zs[k]) and
 *   the outputs are indexed (i * ny + j) * nz + k.  frames: optional uint8 [V,H,W,3].
 *   Per (voxel, view), in ascending view order, with lae_mask_lift's projection statement for statement: d = p - o, q = R^T d;
 *   q.z <= 0 or (u, v) = (fx q.x / q.z + cx, fy q.y / q.z + cy) outside [0, W) x [0, H): no observation.  s = t_surf - |d| at
 *   pixel (floor u, floor v); a NaN t_surf: no observation; s < -trunc: occluded (n_occ += 1); s > trunc: free (n_free += 1);
 *   otherwise near: n_near += 1, S += s / trunc (an fp32 running sum), and the pixel's three bytes are added to uint32 sums.
 *   Per voxel, n_obs = n_near + n_free: tsdf = (S + float(n_free)) / float(n_obs) if n_obs >= min_views, else -1 if n_occ > 0
 *   (space is solid until seen empty), else +1 (never in any frame).
 *   u      fp32 [nx*ny*nz] = -tsdf: larger inside, like a density; marching cubes at threshold 0
 *   counts optional uint16 [nx*ny*nz, 4] = (near, free, occluded, 0); 8-byte aligned
 *   rgb    optional fp32 [nx*ny*nz, 3] = float(sum) / float(n_near) / 255, zeros where n_near == 0; needs frames
 *   Poses go through LDS in chunks of LAE_TSDF_POSE_CHUNK views; per (brick of 4 x 4 x 16 voxels, view) a conservative cull
 *   (the brick's bounding sphere against the camera's half-space and the four frame planes) skips views that contribute
 *   nothing, so the sums keep their order; LAE_TSDF_CULL=0 in the environment (read per call) turns it off, the bytes are the
 *   same.  A thread owns its voxel: no atomics, no host read, no allocation, and two calls give the same bytes.
 *   NULL packed / poses / xs / ys / zs / u, or rgb without frames: LAE_ENULL; V == 0 or V > 65535, H or W < 1, H * W >= 2^31, an
 *   axis shorter than 2 or longer than 512 (marching cubes' limit), fx or fy <= 0, trunc <= 0 or not finite, min_views == 0, a
 *   NaN among them, counts not 8-byte aligned: LAE_EINVAL; both before any launch.
 * lae_tsdf_vertex_colors: colours [V,3] fp32 for marching-cubes vertices verts [V,3] fp32 (index space) from lae_tsdf_fuse's rgb
 *   and counts.  The vertex's lattice edge (base, axis, t) is located as lae_mesh_vertex_attrs does; both endpoints have
 *   n_near > 0: c_a + t (c_b - c_a); one has: its colour; neither: 0.5.  n_grey: optional device uint32, set to the number of
 *   vertices that fell back to grey (zeroed by the call; integer adds).  V == 0: LAE_OK, nothing launched. */
#define LAE_TSDF_POSE_CHUNK 64
LAE_API int lae_tsdf_fuse(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H,
                          uint32_t W, const float* xs, const float* ys, const float* zs, uint32_t nx, uint32_t ny, uint32_t nz,
                          const uint8_t* frames, float trunc, uint32_t min_views, float* u, uint16_t* counts, float* rgb,
                          void* stream);
LAE_API int lae_tsdf_vertex_colors(const float* rgb, const uint16_t* counts, uint32_t nx, uint32_t ny, uint32_t nz, const float* verts,
                                   uint32_t V, float* colors, uint32_t* n_grey, void* stream);

/* ---- textured mesh export: a per-triangle texture atlas baked on the device (csrc/atlas.hip, where the layout and the rules
 * are written down in full; atlas.py restates the kernels in numpy).  The reference has no counterpart ----
 * The layout: triangles two to a square cell of cell x cell texels (cell >= 4), cells = ceil(T / 2), cpr = ceil(sqrt(cells)) cells
 *   per row, the image S x S with S = cpr * cell <= 16384; triangle t in cell t / 2, half t & 1; texels are numbered cell-major,
 *   id = c * cell^2 + j * cell + i.  lae_atlas_layout (host only) returns cells, cpr and S; LAE_EINVAL where T == 0, cell < 4 or
 *   S > 16384.
 * lae_atlas_texels: verts fp32 [V,3], tris int32 [T,3], optional vertex normals fp32 [V,3] -> per texel (cells * cell^2 of them)
 *   pos [.,3] (the affine extension of the half's UV -> triangle map: b1 = a / (cell - 3), b2 = b / (cell - 3),
 *   pos = (v0 + b1 (v1 - v0)) + b2 (v2 - v0)), nrm [.,3] the triangle's unit right-hand face normal (0 for a zero-area triangle or
 *   one with a vertex index outside [0, V): its texels are flagged by it and come out grey), dirs [.,3] = minus the normalised
 *   interpolated vertex normal (minus the face normal where that vanishes or no normals are given, (0, 0, 1) where both do),
 *   owner [.] int32 = t, or -1 for the unused half of an odd T's last cell.
 * lae_atlas_fuse_views: V packed views [V,H,W] and frames uint8 [V,H,W,3] fused into the texels.  Per (texel, view), in ascending
 *   view order, with lae_tsdf_fuse's projection statement for statement: d = p - o, q = R^T d; q.z <= 0 or (u, v) outside
 *   [0, W) x [0, H): rejected; s = t_surf - |d| at pixel (floor u, floor v), a NaN t_surf: rejected; the view counts iff
 *   |s| <= trunc and -(nrm . d) / |d| > min_cos: the pixel's bytes go into three uint32 sums and n += 1.
 *   rgb    fp32 [n_texels, 3] = float(sum) / float(n) / 255; 0.5 where n == 0; 0 for unowned texels
 *   counts optional uint16 [n_texels] = n
 *   n_grey optional device uint32: the owned texels with n == 0 (zeroed by the call; integer adds)
 *   Poses go through LDS LAE_TSDF_POSE_CHUNK views at a time; per (wave of 64 texels, view) a conservative cull (the bounding
 *   sphere of the wave's texels against the camera's half-space and the four frame planes, and every triangle of the wave
 *   back-facing beyond min_cos with the sphere's margin) skips views that contribute nothing; survivors are compacted by ballot,
 *   so the sums keep their order.  LAE_ATLAS_CULL=0 in the environment (read per call) turns it off, the bytes are the same.  A
 *   thread owns its texel: no atomics but the grey count, no host read, no allocation, and two calls give the same bytes.
 * lae_atlas_pack: cell-major fp32 colours -> the image uint8 [S,S,3], row 0 on top, by lae_eval_view's byte rule; unowned texels
 *   and cells past `cells` are 0.
 * NULL pointers (normals, counts and n_grey excepted): LAE_ENULL; T == 0, cell < 4, S > 16384, V == 0 (vertices), V == 0 or
 *   V > 65535 (views), H or W < 1, H * W >= 2^31, n_texels == 0 or > 16384^2, fx or fy <= 0, trunc <= 0 or not finite, min_cos
 *   outside [0, 1), a NaN among them: LAE_EINVAL; both before any launch. */
LAE_API int lae_atlas_layout(uint32_t T, uint32_t cell, uint32_t* cells, uint32_t* cpr, uint32_t* S);
LAE_API int lae_atlas_texels(const float* verts, uint32_t V, const int32_t* tris, uint32_t T, const float* normals, uint32_t cell,
                             float* pos, float* nrm, float* dirs, int32_t* owner, void* stream);
LAE_API int lae_atlas_fuse_views(const float* packed, const float* poses, uint32_t V, float fx, float fy, float cx, float cy, uint32_t H,
                                 uint32_t W, const uint8_t* frames, const float* pos, const float* nrm, const int32_t* owner,
                                 uint32_t n_texels, float trunc, float min_cos, float* rgb, uint16_t* counts, uint32_t* n_grey,
                                 void* stream);
LAE_API int lae_atlas_pack(const float* rgb, const int32_t* owner, uint32_t T, uint32_t cell, uint8_t* image, void* stream);

/* ---- mesh simplification: quadric vertex clustering (csrc/simplify.hip; simplify.py restates the
 * kernels in numpy and does the ordering between them).  The reference has no counterpart ----
 * Inputs: verts fp32 [V,3] in any frame, tris int32 [T,3], cell fp32 > 0, origin fp32 (ox, oy, oz), dims (nx, ny, nz) with
 *   nx ny nz < 4e18, optional colors fp32 [V,C] with C <= 4.
 * 1. lae_simplify_keys: the cluster of a vertex.  ijk = floor(((double)p - (double)origin) / (double)cell) per axis,
 *    keys[v] = (i ny + j) nz + k as int64.  A vertex that is not finite, below the origin or outside dims gets key -1 and ORs
 *    LAE_SIMPLIFY_BAD_VERTEX into *flag (device int32, zeroed by the caller).
 * 2. Output vertex ids (the caller's): an output vertex is the rank of its key among the non-empty clusters in ascending key
 *    order; vertex_map int32 [V] maps input to output vertices.  The caller sorts the keys stably (vorder int64 [V]: the input
 *    vertex at each sorted position, vkeys_sorted int64 [V]) and gives the segment starts vstart int64 [V_out + 1].
 * 3. lae_simplify_pairs: per triangle its up-to-three (cluster, triangle) pairs -- pair_cluster int32 [3T], slot 3 t + corner:
 *    the corner's cluster, or V_out where an earlier corner of t named that cluster already (and for a triangle with an index
 *    outside [0, V), which ORs LAE_SIMPLIFY_BAD_INDEX into *flag) -- survives uint8 [T] (1 iff the three clusters differ), and
 *    with tri_key != NULL the dedup key int64 [T]: the sorted triple packed lo << 42 | mid << 21 | hi, INT64_MAX for a triangle
 *    that does not survive (V_out <= LAE_SIMPLIFY_DEDUP_MAX, else LAE_EINVAL).  The caller sorts the slots stably by cluster
 *    (porder int64 [3T]: slot per sorted position; pstart int64 [V_out + 1]), so a cluster's triangles are in ascending order.
 * 4. lae_simplify_reduce: per cluster, all in fp64 and relative to the cell centre c = origin + (ijk + 0.5) cell.  Over the
 *    member vertices: count, mean position m, colour mean.  Over every triangle with at least one corner in the cluster, once
 *    per cluster: n = (p1 - p0) x (p2 - p0) (squared-area weighting, no division), A += n n^T, b += -(n . p0) n, N += n.
 *    Triangles that will be dropped contribute; a degenerate one contributes zero by itself.
 *    lambda = reg trace(A) / 3 + 1e-18 cell^4; (A + lambda I) x = lambda m - b (SPD 3 x 3, condition <= 1 + 3 / reg); x clamped
 *    per axis to [-cell / 2, cell / 2]; pos[c] = (float)(centre + x).  No branch: with no or only degenerate faces x = m.
 *    LAE_SIMPLIFY_MEAN skips the solve (x = m).  normals (optional) = N / |N| rounded to fp32, zero where N is zero: they point
 *    where the faces' right-hand normals point (lae_mesh_vertex_attrs' convention).  colors_out (optional) = the member mean.
 *    lanes: 1, 16 or 64 adjacent lanes share a cluster (0: LAE_SIMPLIFY_LANES in the environment, else 16 where (V + T) / V_out
 *    >= LAE_SIMPLIFY_WIDE_ITEMS and 1 below: the measured crossover); each lane sums every lanes-th item of the sorted segments
 *    and the partial sums meet in a fixed butterfly, so the bytes depend on `lanes` and on nothing else.
 * 5. lae_simplify_first (dedup): sorted_keys, order = the stable sort of tri_key -> keep uint8 [T]: 1 for the lowest input
 *    index of every vertex set among the survivors, 0 elsewhere.  Without dedup keep = survives.
 * 6. lae_simplify_compact: keep_incl int64 [T] = the inclusive running count of keep; out int32 [T_out, 3]: the kept triangles
 *    in ascending input order, corner order kept, corners through vertex_map.
 * Output vertices no triangle references stay (vertex_map is total).  Vertex clustering does not preserve manifoldness.
 * No floating-point atomics anywhere: every sum has one owner and a fixed order, two calls give the same bytes.
 * NULL pointers (colors, normals, colors_out, tri_key excepted): LAE_ENULL; cell <= 0 or not finite, a non-finite origin, a zero
 *   dim, reg <= 0, C > 4, an unknown placement or lanes, V_out > V, T_out > T: LAE_EINVAL; both before any launch.  V, T, V_out or
 *   T_out == 0: LAE_OK, nothing launched. */
#define LAE_SIMPLIFY_BAD_VERTEX 1
#define LAE_SIMPLIFY_BAD_INDEX 2
#define LAE_SIMPLIFY_QUADRIC 0
#define LAE_SIMPLIFY_MEAN 1
#define LAE_SIMPLIFY_DEDUP_MAX (1u << 21)
#define LAE_SIMPLIFY_WIDE_ITEMS 48
LAE_API int lae_simplify_keys(const float* verts, uint32_t V, float ox, float oy, float oz, float cell, uint32_t nx, uint32_t ny,
                              uint32_t nz, int64_t* keys, int32_t* flag, void* stream);
LAE_API int lae_simplify_pairs(const int32_t* tris, uint32_t T, const int32_t* vertex_map, uint32_t V, uint32_t V_out,
                               int32_t* pair_cluster, uint8_t* survives, int64_t* tri_key, int32_t* flag, void* stream);
LAE_API int lae_simplify_reduce(const float* verts, uint32_t V, const float* colors, uint32_t C, const int32_t* tris, uint32_t T,
                                const int64_t* vorder, const int64_t* vkeys_sorted, const int64_t* vstart, const int64_t* porder,
                                const int64_t* pstart, uint32_t V_out, float ox, float oy, float oz, float cell, uint32_t nx,
                                uint32_t ny, uint32_t nz, double reg, int placement, int lanes, float* pos, float* normals,
                                float* colors_out, void* stream);
LAE_API int lae_simplify_first(const int64_t* sorted_keys, const int64_t* order, uint32_t T, uint8_t* keep, void* stream);
LAE_API int lae_simplify_compact(const int32_t* tris, uint32_t T, const int32_t* vertex_map, const uint8_t* keep,
                                 const int64_t* keep_incl, uint32_t T_out, int32_t* out, void* stream);

/* ---- undistortion at the door: resample lens-distorted captures into one pinhole camera, and back (csrc/undistort.hip;
 * DESIGN.md section 4g; undistort.py restates the three kernels in numpy).  The reference's scripts/colmap2nerf.py writes
 * k1, k2, p1, p2 / is_fisheye into transforms.json; its loader ignores them ----
 * Pixel (i, j) has normalised coordinates x = (i + 0.5 - cx) / fx, y = (j + 0.5 - cy) / fy (lae_get_rays' convention).
 * A camera is LAE_CAM_FLOATS fp32 values in HOST memory: model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2, 0.
 *   LAE_CAM_OPENCV (COLMAP SIMPLE_RADIAL / RADIAL / OPENCV):  r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *     xd = x rad + 2 p1 x y + p2 (r2 + 2 x x), yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y     (k4 unused)
 *     by hand: x = 0.5, y = -0.25, k1 = 0.1, k2 = -0.05, k3 = 0, p1 = 0.01, p2 = -0.02 -> xd = 0.49443359375, yd = -0.247216796875
 *   LAE_CAM_FISHEYE (OpenCV fisheye, Instant-NGP's is_fisheye): r = sqrt(r2), theta = atan(r), t2 = theta theta,
 *     theta_d = theta (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))), (xd, yd) = (theta_d / r) (x, y), the factor 1 at r = 0   (p1, p2 unused)
 * lae_undistort_map: n_cam source cameras, one target pinhole (fx, fy, cx, cy, H, W) -> map fp32 [n_cam, H, W, 2] on the device:
 *   per target pixel the source position (xd fx_s + cx_s - 0.5, yd fy_s + cy_s - 0.5) in pixel-index units (the forward model).
 * lae_distort_map: the inverse direction, per pixel of each source camera [n_cam, Hs, Ws, 2] its position in the target camera
 *   (x fx + cx - 0.5, y fy + cy - 0.5): a Newton iteration from the distorted point, 2-D for LAE_CAM_OPENCV (analytic Jacobian),
 *   1-D in theta for LAE_CAM_FISHEYE, `iters` steps (0: LAE_UNDISTORT_NEWTON_ITERS; at most 64).  converged: optional uint8
 *   [n_cam, Hs, Ws], 1 where the forward model's residual at the result is at most LAE_UNDISTORT_TOL_PX source pixels on both
 *   axes (fisheye: on theta_d times max(fx, fy), and 0 <= theta < pi/2); elsewhere 0 and the map holds NaN.
 *   LAE_UNDISTORT_NEWTON_ITERS = 8: in float64, 3 steps leave less than 1e-12 px on a 3840 x 2160 camera with fx = 3000,
 *   k1 = 0.16, k2 = -0.23; a strong barrel (k1 = -0.3, k2 = 0.09) on a wide lens (fx = W / 2, where the start is far from the
 *   root) has 3e-9 px left after 5 and 1e-12 after 6 (tests/test_undistort_cpu.py).  Newton doubles the digits per step, so 8
 *   leaves two steps in hand, and the map is computed once per scene: the count costs nothing that matters.
 *   NULL cams / map: LAE_ENULL; H or W outside [1, 32768], a focal length <= 0, a model other than the two, a value that is
 *   not finite, map not 8-byte aligned, iters > 64: LAE_EINVAL; both before any launch.  n_cam == 0: LAE_OK.
 * lae_remap: dst[n, Ht, Wt, C] = src[n, Hs, Ws, C] sampled at map[cam, Ht, Wt, 2]; C in {1, 3, 4}; dtype LAE_IMG_U8 / _F16 / _F32
 *   (output as input); cam = cam_index[image] (device int32 [n]) or 0 when cam_index is NULL (one map shared by all images); an
 *   index outside [0, n_cam) makes the image's output invalid.  valid: optional uint8 [n, Ht, Wt].
 *   LAE_REMAP_BILINEAR: valid iff 0 <= sx <= Ws - 1 and 0 <= sy <= Hs - 1.  x0 = floor(sx), ax = sx - x0 (exact), x1 = min(x0 + 1,
 *     Ws - 1), likewise y; w00 = (1 - ax)(1 - ay), w01 = ax (1 - ay), w10 = (1 - ax) ay, w11 = ax ay;
 *     v = ((w00 p00 + w01 p01) + w10 p10) + w11 p11 in fp32 (p01 is the pixel at (x1, y0)).  C == 4: A = the same sum of the
 *     alphas, P = the same sum of colour x alpha, colour = P / A (0 where A == 0), alpha = A.  uint8 results are floor(v + 0.5),
 *     fp16 results round to nearest.
 *   LAE_REMAP_NEAREST (masks, depth and weight planes): the pixel at (floor(sx + 0.5), floor(sy + 0.5)), the sums in fp32; valid
 *     iff that pixel exists.
 *   An invalid output is all zeros with valid = 0.  NaN, infinities and magnitudes beyond the int range are invalid (the
 *   comparison comes before any conversion).  One owner per output element, no atomics, no allocation: two calls give the same
 *   bytes and the call can be captured.  NULL src / map / dst: LAE_ENULL; another dtype, C or mode, a side outside [1, 32768],
 *   n_cam == 0, src / dst not aligned to a pixel's widest access (uint8 RGBA 4, fp16 RGBA 8, fp32 RGBA 16 bytes, else the
 *   element), map not 8-byte aligned: LAE_EINVAL; both before any launch.  n == 0: LAE_OK. */
#define LAE_CAM_FLOATS 12
#define LAE_CAM_OPENCV 0
#define LAE_CAM_FISHEYE 1
#define LAE_UNDISTORT_NEWTON_ITERS 8
#define LAE_UNDISTORT_TOL_PX 0.015625f
#define LAE_REMAP_BILINEAR 0
#define LAE_REMAP_NEAREST 1
LAE_API int lae_undistort_map(const float* cams, uint32_t n_cam, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                              float* map, void* stream);
LAE_API int lae_distort_map(const float* cams, uint32_t n_cam, uint32_t Hs, uint32_t Ws, float fx, float fy, float cx, float cy,
                            uint32_t iters, float* map, uint8_t* converged, void* stream);
LAE_API int lae_remap(const void* src, int dtype, uint32_t n, uint32_t Hs, uint32_t Ws, uint32_t C, const float* map,
                      const int32_t* cam_index, uint32_t n_cam, uint32_t Ht, uint32_t Wt, int mode, void* dst, uint8_t* valid,
                      void* stream);

/* ---- occupancy-grid maintenance (nerf/renderer.py:482-649, Python in the reference) ----
 * positions: point j -> xyz = (2 c / (H-1) - 1) * (bound_c - bound_c/H) + (noise * 2 - 1) * bound_c/H and its Morton index
 *   (renderer.py:580-592).  coords NULL: c = (j / H^2, (j / H) % H, j % H) (full sweep, n <= H^3); else coords [n,3] int32.
 *   noise [n,3] in [0,1) or NULL (no jitter). */
LAE_API int lae_density_grid_positions(const int32_t* coords, uint32_t n, uint32_t H, float bound_c, const float* noise,
                               float* xyzs, int32_t* indices, void* stream);
/* partial sweep of update_extra_state on the device (renderer.py:600-612: n random cells + n draws from the occupied cells of
 * density_grid[cas] > 0, found there with nonzero() and a host-sized randint).  Writes 2n points: xyzs [2n,3], indices [2n] (Morton;
 * -1 for the occupied half when no cell is occupied: lae_density_grid_update skips them, the reference keeps the n random points
 * only).  noise [2n,3] in [0,1) or NULL.  Two ways to supply the draws:
 *   rnd == NULL: coords_rand [n,3] int32 in [0,H) and u [n] uniform in [0,1) -- draw j takes occupied cell number
 *     min(floor(u[j] * K), K - 1) in index order, K = their count (tests pin this against the reference's statements);
 *   rnd != NULL: [2, n+1] uniforms in [0,1); both halves are then drawn as SORTED i.i.d. samples (order statistics from partial sums
 *     of exponentials, no sort), cells through Morton codes (H must be a power of two) -- same distribution, points in Morton
 *     order (the encoder and the scatter run 1.7x / 2.5x faster on ordered points).  coords_rand / u are ignored.
 * scratch: lae_density_grid_partial_scratch_bytes(cells, n) bytes of device memory; cells = H^3.  No host read: K stays on the device. */
LAE_API uint64_t lae_density_grid_partial_scratch_bytes(uint32_t cells, uint32_t n);
LAE_API int lae_density_grid_partial_positions(const float* grid_c, uint32_t cells, const int32_t* coords_rand, const float* u, const float* rnd,
                                       uint32_t n, uint32_t H, float bound_c, const float* noise, float* xyzs, int32_t* indices,
                                       void* scratch, void* stream);
/* update: tmp[indices] = sigmas * density_scale (maximum where indices repeat), then on sampled cells with grid >= 0:
 *   grid = max(grid * decay, tmp)  (renderer.py:596, 627, 633-634).  grid [cells] fp32 is one cascade; tmp [cells] uint32
 *   scratch must be zero on entry and is zero again on return. */
LAE_API int lae_density_grid_update(const float* sigmas, const int32_t* indices, uint32_t n, float density_scale, float decay,
                            uint32_t cells, float* grid, uint32_t* tmp, void* stream);
/* mark_untrained_grid (renderer.py:482-554): grid[cas, morton(c)] = -1 for cells seen by no camera or closer than
 *   min_near to one.  poses [B,4,4] fp32 camera-to-world, intrinsics (fx, fy, cx, cy), grid [C, H^3] fp32 in place. */
LAE_API int lae_mark_untrained_grid(const float* poses, uint32_t B, float fx, float fy, float cx, float cy, uint32_t C, uint32_t H,
                            float bound, float min_near, int filter_close_point, float* grid, void* stream);

/* ---- marching cubes (extract_geometry's mcubes.marching_cubes, nerf/utils.py:207-219; PyMCubes on the host there).
 * u [nx, ny, nz] fp32, C order, indexed (i, j, k) as mcubes does; 2 <= nx, ny, nz <= 512 (else LAE_EINVAL, so every count fits in
 * int32).  NULL pointers (LAE_ENULL) and bad sizes are rejected before any launch.
 *   Inside rule: a lattice point is inside iff u > threshold (strictly; NaN is outside).
 *   Vertices: one per crossed lattice edge (its two ends on different sides), owned by its lower end point, ordered by (that point's
 *     linear index (i * ny + j) * nz + k, then axis x < y < z).  Position in index space: the lower point + t along the edge's axis,
 *     t = (threshold - a) / (b - a) in fp32 without contraction (a at the lower end); a non-finite t becomes 0.5, then t is clamped
 *     to [0, 1].
 *   Triangles: int32 [T, 3] vertex ids (welded: one vertex per lattice edge), ordered by (cube linear index = its lower corner's,
 *     then the case table's order).
 *   Face rule (tools/gen_mc_table.py -> csrc/mc_table.inc): on an ambiguous cube face (its inside corners on one diagonal) the
 *     inside corners are separated; the choice depends on that face's 4 corners only, so neighbouring cubes agree and the mesh is
 *     watertight.  Each polygon's right-hand normal points from inside to outside (towards lower values); polygons are fanned
 *     from their lowest cube-local edge id whose fan draws no diagonal between two edges of one face (a neighbouring cube could
 *     draw the same one), so every mesh edge of a surface closed inside the lattice lies in exactly two triangles.
 * count: counts[0] = V, counts[1] = T (device int32[2]); scratch: lae_marching_cubes_scratch_bytes(nx, ny, nz) bytes (0 for bad
 *   sizes), kept between count and emit.  emit (same u, threshold and scratch, after count on the same stream; only when V > 0):
 *   verts [V, 3] fp32, tris [T, 3] int32.  Deterministic: no atomics, the same bits on every run. */
LAE_API uint64_t lae_marching_cubes_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
LAE_API int lae_marching_cubes_count(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* scratch,
                             int32_t* counts, void* stream);
LAE_API int lae_marching_cubes_emit(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void* scratch, float* verts,
                            int32_t* tris, void* stream);

/* ---- connected components of a lattice's inside set (csrc/components.hip): what drops floaters between the density sweep and
 * marching cubes, and from the occupancy grid (laenerf_amd/components.py; the reference exports through trimesh and stops).
 * u [nx, ny, nz] fp32, C order, any 4-byte-aligned base; 2 <= nx, ny, nz <= 512 as for lae_marching_cubes_* (else LAE_EINVAL).
 * `threshold` is a double cast once to fp32; every compare is fp32.
 *   Inside rule: lae_marching_cubes_*'s: a lattice point is inside iff u > threshold (strictly; NaN is outside, +inf inside).
 *   Connectivity: two inside points are connected iff they differ by 1 in exactly one coordinate (6-connectivity); contact along
 *     an edge or at a corner does not connect.  An inside point face-adjacent to a kept inside point is therefore kept as well:
 *     removing other components changes neither end of a crossed lattice edge of a kept component, and the kept surface's
 *     marching-cubes vertices are the unfiltered mesh's, bit for bit.
 *   The result is canonical -- it does not depend on the algorithm or the schedule:
 *     labels [nx, ny, nz] int32: the smallest linear index (i * ny + j) * nz + k of the point's component (its root); -1 outside.
 *     sizes [N] int32 (N = nx * ny * nz): at a root, the number of points of its component; 0 everywhere else.
 *     stats int32[4]: {n_components, largest_root, largest_size, n_inside}; ties for the largest go to the lowest root; with no
 *       inside point {0, -1, 0, 0}.
 * lae_components_label: three launches (per-tile union-find in LDS; a lock-free merge across tile faces with agent-scope
 *   atomicMin, in which no wave waits for another; flatten).  `labels` is the only storage: no scratch.
 * lae_components_sizes: labels as written by lae_components_label (N <= 512^3, else LAE_EINVAL; a value outside [0, N) counts as
 *   outside).  Four launches; sizes and stats are zeroed by the first, the counts are integer atomics (exact, the same bits on
 *   every run), one add per label a workgroup's waves end with, not one per point; the largest component is one 64-bit atomic
 *   max of size << 32 | (0x7fffffff - root) per workgroup, kept in stats[0..1] between the passes: stats must be 8-byte aligned
 *   (LAE_EINVAL otherwise).
 * lae_components_filter: out[p] = u[p] bitwise (NaN payloads included) unless labels[p] >= 0 and p's component is not kept; then
 *   out[p] = (float)threshold, which is not > threshold: outside.  A component is kept iff sizes[root] >= min_size and
 *   (keep_root < 0 or root == keep_root).  out may alias u.  One launch (16-byte accesses where u, labels and out are 16-byte
 *   aligned, 4-byte ones otherwise).
 * No entry point reads back, allocates or synchronises: all three can be captured.  N == 0 (sizes, filter): LAE_OK before any
 * pointer is looked at; a NULL pointer: LAE_ENULL; both before any launch. */
LAE_API int lae_components_label(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, double threshold, int32_t* labels, void* stream);
LAE_API int lae_components_sizes(const int32_t* labels, uint64_t N, int32_t* sizes, int32_t* stats, void* stream);
LAE_API int lae_components_filter(const float* u, const int32_t* labels, const int32_t* sizes, uint64_t N, double threshold,
                          int32_t min_size, int32_t keep_root, float* out, void* stream);

/* ---- mesh export: per-vertex attributes of a marching-cubes mesh and the binary PLY bodies, on the device.
 * lae_mesh_vertex_attrs: u [nx, ny, nz] fp32 (the field marching cubes ran on), verts [V, 3] fp32 in index space (as
 *   lae_marching_cubes_emit writes them), the box (bmin, bmax) by value.  Outputs, each of which may be NULL: pos [V, 3],
 *   normals [V, 3], dirs [V, 3], fp32.  One thread per vertex; deterministic (no atomics).  Sizes outside 2..512: LAE_EINVAL;
 *   V == 0: LAE_OK before any launch; NULL u / verts: LAE_ENULL.
 *   Position: v / (n_a - 1) * (bmax_a - bmin_a) + bmin_a per axis a (n_a: that axis's lattice size), with (bmax_a - bmin_a) formed
 *     in fp32, the division, product and sum in fp64 without contraction, and one rounding to fp32.  On a cubic lattice this is
 *     the reference's float64 scaling (nerf/utils.py:214-217) rounded to the fp32 a PLY stores.
 *   Lattice gradient at a point p: d_a(p) = (u[p + e_a] - u[p - e_a]) * 0.5f; on a border the one-sided difference
 *     u[p + e_a] - u[p] or u[p] - u[p - e_a].
 *   Locating a vertex: a non-finite coordinate is treated as 0 (for the position too).  base = floor(v) clamped into [0, n - 1] per
 *     axis, frac = v - base.  A vertex lies on a lattice edge, so at most one axis has frac > 0: the first such axis a (x < y < z)
 *     gives t = frac_a and the edge's other end q = base + e_a, clamped; with no such axis t = 0.  Every index is clamped before any
 *     load: garbage in verts can give garbage attributes, never a read outside u.
 *   Normal: g_a = d_a(base) + t * (d_a(q) - d_a(base)); w_a = g_a * s_a with s_a = float(n_a - 1) / (bmax_a - bmin_a) in fp32 (the
 *     gradient moved from index space to the box); len = sqrtf(w.w); normals = -w / len, dirs = w / len -- the normal points
 *     towards lower values, which agrees with the face orientation above, and dirs is the direction along which a camera looking
 *     straight at the surface sees it.  Where len is 0 or not finite: normals = 0, dirs = (0, 0, 1).
 * lae_mesh_pack_ply: the bodies of a binary little-endian PLY.  vertex_bytes [V * stride]: per vertex `float x y z` from pos [V, 3],
 *   then `float nx ny nz` if normals != NULL, then `uchar red green blue` if rgb != NULL (fp32 [V, 3]; a byte is
 *   clip(x, 0, 1) * 255 truncated as in lae_eval_view's rgb_u8, NaN -> 0); stride = 12, 24, 15 or 27.  face_bytes [T * 13]: per
 *   triangle `uchar 3` and three little-endian int from tris [T, 3].  Either half is skipped when its output is NULL or its count
 *   is 0.  The bytes are those of the matching packed numpy structured arrays.  A workgroup stages its records in LDS and stores
 *   whole dwords (bytes only for a buffer's last 1-3), so both output bases must be 4-byte aligned (LAE_EINVAL otherwise); a
 *   present half with a NULL input is LAE_ENULL. */
LAE_API int lae_mesh_vertex_attrs(const float* u, uint32_t nx, uint32_t ny, uint32_t nz, const float* verts, uint32_t V, float bmin_x,
                          float bmin_y, float bmin_z, float bmax_x, float bmax_y, float bmax_z, float* pos, float* normals, float* dirs,
                          void* stream);
LAE_API int lae_mesh_pack_ply(const float* pos, const float* normals, const float* rgb, uint32_t V, const int32_t* tris, uint32_t T,
                      uint8_t* vertex_bytes, uint8_t* face_bytes, void* stream);

/* ---- nearest-neighbour feature matching (NNFM: ARF, Ref-NPR; editing/semantic_encoder.py:83-164 nn_feat_replace /
 * argmin_cos_distance / cos_loss, editing/ref_loss.py NNFMLoss) without the Na x Nb distance matrix (csrc/nnfm.hip).
 * Features are fp32, channel-major [n, C, N]; n independent matching problems (n = 1, C = L * C': the layers concatenated;
 * n = L: one matching per layer).  1 <= n <= 65535, 1 <= C <= 65536, N <= 2^23 (LAE_EINVAL otherwise); a required NULL pointer is
 * LAE_ENULL; Na == 0 (pack: N == 0) returns LAE_OK before any pointer is looked at.  No host read, no allocation: capturable.
 * lae_nnfm_pack: per position v / (sqrt(sum v^2 + 1e-8) + 1e-8), rounded to fp16, position-major [n, N_pad, C_pad] (channel
 *   contiguous; N_pad = N rounded up to 64, C_pad = C rounded up to 32; the padding is zero-filled by the kernel).  packed:
 *   lae_nnfm_packed_bytes(n, C, N) bytes, 16-byte aligned.
 * lae_nnfm_match: z [n, Na] int32 = argmax_j of the cosine of packed content row i and packed style column j < Nb (fp16 operands,
 *   fp32 accumulation on the matrix cores); d_best [n, Na] (may be NULL) = 1 - that cosine.  Among equal cosines the lowest index
 *   wins; the result does not depend on the schedule (fixed-order combination of per-chunk partial results, no atomics).
 *   workspace: lae_nnfm_match_bytes(n, Na, Nb) bytes, 8-byte aligned.  Non-finite features give z = 0 and d_best = NaN.
 * lae_nnfm_workspace_bytes: the match workspace (rounded up to 256) + the packed content side, what one loss evaluation needs
 *   beside its inputs; the three *_bytes helpers are host functions and need no GPU.
 * lae_nnfm_loss_forward: cos_loss(x, gather(s, z)) on the fp32 features: with a = x[:, i], t = s[:, z_i], a^ = a / (|a| + 1e-8),
 *   t^ = t / (|t| + 1e-8): loss[0] = mean over the n * Na positions of (1 - a^ . t^), summed in a fixed order (two runs give the same
 *   bits).  stats [4, n * Na] fp32 (written; the backward reads it): a . t^, |a|, |t|, the position's term.  z outside 0..Nb-1 is
 *   clamped before any load.
 * lae_nnfm_loss_backward: dx [n, C, Na] = -(g / (n Na)) (t^ / s_a - (a . t^) a / (|a| s_a^2)), s_a = |a| + 1e-8, g = g_loss_dev[0]
 *   (a device scalar).  One departure from the reference: a content position whose vector is exactly zero contributes 1 to the
 *   loss and a zero gradient (autograd gives NaN there through sqrt at 0). */
LAE_API uint64_t lae_nnfm_packed_bytes(uint32_t n, uint32_t C, uint32_t N);
LAE_API uint64_t lae_nnfm_match_bytes(uint32_t n, uint32_t Na, uint32_t Nb);
LAE_API uint64_t lae_nnfm_workspace_bytes(uint32_t n, uint32_t C, uint32_t Na, uint32_t Nb);
LAE_API int lae_nnfm_pack(const float* feats, uint32_t n, uint32_t C, uint32_t N, void* packed, void* stream);
LAE_API int lae_nnfm_match(const void* a_packed, const void* b_packed, uint32_t n, uint32_t Na, uint32_t Nb, uint32_t C, int32_t* z,
                   float* d_best, void* workspace, void* stream);
LAE_API int lae_nnfm_loss_forward(const float* x, const float* s, const int32_t* z, uint32_t n, uint32_t C, uint32_t Na, uint32_t Nb,
                          float* loss, float* stats, void* stream);
LAE_API int lae_nnfm_loss_backward(const float* x, const float* s, const int32_t* z, const float* stats, const float* g_loss_dev, uint32_t n,
                           uint32_t C, uint32_t Na, uint32_t Nb, float* dx, void* stream);

/* ---- ray registration of the single-reference-view stylization (Ref-NPR; editing/single_view_edit_dataset.py:317-349
 * get_ref_supervision and its caller :219-232) as a truncated nearest-neighbour search in a uniform cell grid (csrc/rayreg.hip).
 * All points fp32 [.,3]; M cloud points, n query rows, both <= 2^30; radius > 0 and finite (LAE_EINVAL otherwise); a required NULL
 * pointer is LAE_ENULL; n == 0 returns LAE_OK before any pointer is looked at.  No host read, no allocation: capturable.
 * lae_rayreg_build: the grid of the cloud ref_x [M,3] into `grid` (lae_rayreg_build_bytes(M) bytes, 16-byte aligned): a 256-byte
 *   record (fp32 lo[3], s, 1/s; uint32 G[3], cells, ...), the table of cell ends and the cell-sorted copy of the FINITE points as
 *   float4 (x, y, z, bits of the original index).  The cell side s >= radius * (1 + 2^-10) and the cells per axis G <= 1024 are
 *   chosen on the device from the bounding box (rayreg.hip derives the margin).  M == 0 builds the empty grid (ref_x may be NULL).
 * lae_rayreg_query: per row of x [n,3]: d = min(radius, distance to the nearest cloud point), nn = that point's original index or
 *   -1 where no point lies within radius (d < radius in fp32 <=> nn >= 0).  The squared distance is
 *   fmaf(dz, dz, fmaf(dy, dy, dx * dx)) on fp32 differences, d its sqrtf; among equal squared distances the lowest original index
 *   wins, so the result does not depend on the schedule.  d is exact over ALL M points whenever it is below radius.  Non-finite
 *   rows and M == 0 give d = radius, nn = -1.  radius and M must be the build's.  mode: LAE_RAYREG_BINNED (queries binned by cell, a
 *   workgroup per cell chunk, neighbour cells streamed through LDS) or LAE_RAYREG_GATHER (a lane per query; the A/B predecessor,
 *   same results).  workspace: lae_rayreg_query_bytes(n, M) bytes, 16-byte aligned; after a BINNED call its last 256 bytes start
 *   with a uint64: the distance evaluations of the call.
 * lae_rayreg_supervise: row i is registered iff nn[i] >= 0 and d[i] < reg_dist (0 < reg_dist <= radius, guide_min < radius).
 *   stats (4 uint32, written): R = registered rows, bits of dmin and of dmax over them (+inf / 0 when R == 0).  Dense outputs:
 *   nn_reg [n] = nn or -1; target [n,3] = ref_rgb[nn] (zeros when unregistered); weight [n] = |(d - dmin) / (dmax - dmin) - 1| * f,
 *   f = (clamp(cos(ref_dirs[nn], dirs[i]), -1, -0.5) + 1) / 0.5 with torch's cosine_similarity (eps 1e-8), 0 when unregistered; one
 *   departure from the reference: dmax == dmin gives weight = f (the reference divides 0 by 0);
 *   guide [n] = max(min_tv_factor, (clamp(d, guide_min, radius) - guide_min) / (radius - guide_min)). */
#define LAE_RAYREG_BINNED 0
#define LAE_RAYREG_GATHER 1
LAE_API uint64_t lae_rayreg_build_bytes(uint32_t M);
LAE_API int lae_rayreg_build(const float* ref_x, uint32_t M, float radius, void* grid, void* stream);
LAE_API uint64_t lae_rayreg_query_bytes(uint32_t n, uint32_t M);
LAE_API int lae_rayreg_query(const void* grid, uint32_t M, const float* x, uint32_t n, float radius, int mode, float* d, int32_t* nn,
                     void* workspace, void* stream);
LAE_API int lae_rayreg_supervise(const float* d, const int32_t* nn, uint32_t n, const float* ref_rgb, const float* ref_dirs, uint32_t M,
                         const float* dirs, float reg_dist, float radius, float guide_min, float min_tv_factor, int32_t* nn_reg,
                         float* target, float* weight, float* guide, uint32_t* stats, void* stream);

/* ---- fused Adam + GradScaler (torch.optim.Adam / torch.cuda.amp.GradScaler in the reference: main_nerf.py:223,
 * nerf/utils.py:1474-1482).  `state` is a 64-byte device block:
 *   [0] f32 scale  [1] i32 growth_tracker  [2] i32 found_inf  [3] i32 skip  [4] i32 step  [5] f32 1/(1-beta1^step)
 *   [6] f32 sqrt(1-beta2^step)  [7] f32 1/scale of this step  [8] i32 skipped steps
 *   [9] [10] f32 the bias corrections of step [11] (i32; 0 = none) computed with the betas [12] [13] -- left by the apply launch
 *   so that the one-thread begin launch on the step's critical path does no double-precision pow (round 3; begin computes
 *   them itself when [11] is not the step it is about to take)  [14..15] reserved.  The apply entry points therefore WRITE
 *   words 9-13 of `state` although they take it as const.
 * Per step: lae_adam_check on every gradient, ONE lae_adam_begin, lae_adam_apply on every parameter.
 * check: found_inf |= any non-finite element (grad fp16 or fp32, 16-byte aligned). */
LAE_API int lae_adam_check(const void* grad, int grad_is_half, uint64_t n, void* state, void* stream);
/* begin: found_inf -> skip (scale *= backoff, tracker = 0) or step += 1 with bias corrections (double precision) and
 * scale growth after `growth_interval` finite steps (grad_scaler.py _amp_update_scale_).  use_scaler = 0: plain Adam. */
LAE_API int lae_adam_begin(void* state, float beta1, float beta2, int growth_interval, float growth_factor, float backoff_factor,
                   int use_scaler, void* stream);
/* apply: g = grad / scale; Adam update of param / exp_avg / exp_avg_sq (fp32, torch.optim.Adam formulas); optional fp16
 * copy of the new parameters into shadow_half (the table the grid encoder gathers from); grad is zeroed.  lr is read
 * from device memory.  On a skipped step only the gradient is zeroed. */
LAE_API int lae_adam_apply(float* param, float* exp_avg, float* exp_avg_sq, void* grad, int grad_is_half, void* shadow_half, uint64_t n,
                   const void* state, const float* lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* Trainer criterion + loss scaling in one kernel (nerf/utils.py train_step: MSELoss(reduction='none')(pred, gt).mean(-1)
 * .mean(), then GradScaler.scale): loss_out[0] = mean((pred - target)^2) * scale, loss_out[1] = the unscaled loss,
 * grad[i] = d loss_out[0] / d pred[i].  scale: device float (FusedAdam state word 0) or NULL (= 1).  fp32, n elements. */
LAE_API int lae_mse_loss_forward(const float* pred, const float* target, uint32_t n, const float* scale, float* loss_out, float* grad,
                         void* stream);
/* lae_mse_loss_forward with the colour criterion chosen by loss_kind (LAE_LOSS_*, at lae_crit_term): the
 * criterion of a step that does not run the fused compositing step.  loss_out[1] = mean(v), loss_out[0] = that * scale,
 * grad[i] = ((dv * (1 / n)) * scale).  LAE_LOSS_MSE runs lae_mse_loss_forward's statements and gives its bits.  LAE_EINVAL: n == 0,
 * loss_kind out of range, a Huber delta (loss_param) that is not finite and > 0. */
LAE_API int lae_colour_loss_forward(const float* pred, const float* target, uint32_t n, int loss_kind, float loss_param, const float* scale,
                            float* loss_out, float* grad, void* stream);

/* multi-tensor forms of check / apply: host arrays of n_tensors (<= 8) device pointers / sizes; one launch each.
 * touched_lines (may be NULL, entries may be NULL): per tensor the bitmap lae_grid_encode_backward_ex maintains (one bit per 16
 * parameters); with weight_decay == 0 a line whose bit is clear is neither read nor written -- Adam's update of parameters whose
 * gradient, exp_avg and exp_avg_sq are all zero is exactly zero.
 * grad_dirty (may be NULL, entries may be NULL): per tensor the "dirty" word of its gradient accumulator
 * (lae_grid_encode_backward_ex); apply leaves every gradient zero and sets the words to 0. */
LAE_API int lae_adam_check_multi(uint32_t n_tensors, const void* const* grads, const int* grad_is_half, const uint64_t* sizes, void* state,
                         void* stream);
LAE_API int lae_adam_apply_multi(uint32_t n_tensors, float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs, void* const* grads,
                         const int* grad_is_half, void* const* shadows_half, const uint64_t* sizes, const float* const* lrs, const void* const* touched_lines,
                         void* const* grad_dirty, const void* state, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* torch_ema.ExponentialMovingAverage.update() of the reference's trainer (nerf/utils.py:407-408 construct, :1502-1503 update once per
 * epoch; decay 0.95, main_nerf.py:244): shadow -= one_minus_decay * (shadow - param) for up to 8 fp32 tensors in one launch.  The
 * caller computes one_minus_decay = 1 - min(decay, (1 + num_updates) / (10 + num_updates)) like torch_ema does. */
LAE_API int lae_ema_update_multi(uint32_t n_tensors, float* const* shadows, const float* const* params, const uint64_t* sizes,
                         float one_minus_decay, void* stream);
/* the same update once per epoch inside a captured training step (the reference updates after every epoch of one image per
 * batch): nothing happens unless *step (the int64 device step counter, i.e. the 1-based index of the step just taken) is a
 * positive multiple of epoch_len.  Then, with n = count[0] + 1: decay_t = min(decay, (1 + n) / (10 + n)) in fp64 (decay itself
 * when use_num_updates == 0), one_minus_decay = (float)(1 - decay_t), lae_ema_update_multi's arithmetic, and count[0] = n.
 * count: int32 [2] device words, the update count and a block ticket that must be 0 before the call (it is left at 0). */
LAE_API int lae_ema_update_gated(uint32_t n_tensors, float* const* shadows, const float* const* params, const uint64_t* sizes,
                         const int64_t* step, int64_t epoch_len, int32_t* count, double decay, int use_num_updates, void* stream);

/* ------------------------------------------------------------------ */
/* evaluation (evaluate.hip): evaluate_one_epoch / test (nerf/utils.py:1526-1624, :777-827) with PSNRMeter / LPIPSMeter    */
/* (:240-247, main_nerf.py:203, 242) and LAENeRF's eval_masked (nerf/gui.py:853-947)                                        */
/* ------------------------------------------------------------------ */
#define LAE_EVAL_VIEW_SCRATCH_DOUBLES 2048
/* one rendered view against its ground truth in one pass.  pred fp32 [n_pixels,3] and depth fp32 [n_pixels] (16-byte aligned;
 * depth may be NULL unless depth_u8 is asked for); gt [n_pixels, gt_channels] as stored (gt_dtype 0 uint8 = value / 255, 1 fp16,
 * 2 fp32; channels 3 or 4) or NULL when only the uint8 images are wanted.  For C = 4 the ground truth is blended over bg as
 * rgb * a + bg * (1 - a) with torch's separate fp32 roundings.  Every output is optional:
 *   sse_out         one double: sum over n_pixels * 3 of (pred - gt)^2 (differences and sum in fp64; fixed-order two-stage
 *                   reduction through scratch, LAE_EVAL_VIEW_SCRATCH_DOUBLES doubles: two calls give the same bits)
 *   masked_sse_out  one double (needs sse_out and mask, uint8 [n_pixels]): the same sum against the UNblended gt[:3] over the
 *                   pixels whose mask byte is 0 (eval_masked's m = 1 - clip(mask[..., -1], 0, 1))
 *   gt_out          fp32 [n_pixels,3], the blended ground truth
 *   rgb_u8 / depth_u8  clip(x, 0, 1) * 255 truncated, [n_pixels,3] / [n_pixels]
 *   lpips_in        fp32 [2,3,n_pixels] planes: index 0 the blended gt, 1 pred, each ((2x - 1) - shift_c) / scale_c with lpips'
 *                   ScalingLayer (shift -.030 -.088 -.188, scale .458 .448 .450) */
LAE_API int lae_eval_view(const float* pred, const float* depth, const void* gt, int gt_dtype, uint32_t gt_channels, uint32_t n_pixels,
                          float bg, const uint8_t* mask, double* scratch, double* sse_out, double* masked_sse_out, float* gt_out,
                          uint8_t* rgb_u8, uint8_t* depth_u8, float* lpips_in, void* stream);
/* LPIPS v0.1's distance head (normalize_tensor, NetLinLayer, spatial_average, sum over layers) for n_pairs pairs in one launch:
 * feats[l] fp32 [2 * n_pairs, channels[l], hw[l]] (pair p = rows 2p and 2p + 1), weights[l] fp32 [channels[l]] (host arrays of
 * n_layers <= 5 device pointers); out[p] = sum_l mean_px sum_c w_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 as double,
 * accumulated in fp64 with a fixed-order reduction.  scratch: n_pairs * sum_l ceil(hw[l] / 256) doubles. */
LAE_API int lae_lpips_head(uint32_t n_layers, const float* const* feats, const float* const* weights, const uint32_t* channels,
                           const uint32_t* hw, uint32_t n_pairs, double* scratch, double* out, void* stream);
/* The gradient of lae_lpips_head with respect to the features (LPIPS as a training term: the reference's patch loss, nerf/utils.py:
 * 594-603), all n_layers <= 5 layers and all pairs in ONE launch.  feats, weights, channels, hw, n_pairs as lae_lpips_head
 * (channels[l] <= 512, else LAE_EINVAL); gout double [n_pairs] on the device, the upstream gradient of out[p]; grad_feats[l] fp32
 * [2 * n_pairs, channels[l], hw[l]] (a host array of device pointers), every element written.  Per layer, pair and pixel, with
 *   n_i = sqrt(sum_c f_i,c^2), u_i = f_i / (n_i + 1e-10), d = u_0 - u_1, a_i = sum_c w_c d_c f_i,c:
 *   d out / d f_1,k = -(2 gout[p] / hw) * (w_k d_k / (n_1 + 1e-10) - f_1,k a_1 / (n_1 (n_1 + 1e-10)^2))
 *   d out / d f_0,k = the same expression with index 0 and the opposite sign when both != 0; with both == 0 the x_0 rows (2p) are
 *   written as zeros (the ground truth needs no gradient).
 * Zero-norm rule: a pixel whose n_i is exactly 0 gets a zero gradient on that side.  The true slope there is 1 / 1e-10, an artefact
 * of the epsilon; torch's autograd returns NaN (sqrt'(0) * 0), which would make a GradScaler skip the step.  The other side of such a
 * pixel is computed as stated, with u_i = 0.
 * Arithmetic: norms, dot products and the expression in fp64 from the fp32 features, gout multiplied in before the single rounding
 * to fp32.  One owner per output element, fixed-order wave reductions, no atomics: two calls give the same bits. */
LAE_API int lae_lpips_head_grad(uint32_t n_layers, const float* const* feats, const float* const* weights, const uint32_t* channels,
                                const uint32_t* hw, uint32_t n_pairs, const double* gout, float* const* grad_feats, int both,
                                void* stream);
/* A patch batch's rows as the input of LPIPS' trunk.  pred, gt fp32 [n_patch * P^2, 3], row r = pixel (r % P^2) / P, r % P (row-major)
 * of patch r / P^2, as lae_sample_train_batch_patch orders them; x fp32 [2 * n_patch, 3, P, P]: image 2p the ground truth of patch p,
 * 2p + 1 its prediction, the pair layout of lae_lpips_head.  x = ((normalize ? 2 v - 1 : v) - shift_c) / scale_c with lae_eval_view's
 * constants and statement order, every operation one fp32 rounding.  normalize = 0 is the reference's call ([0, 1] images into lpips
 * with its default normalize=False), normalize = 1 lpips' documented range.  P in [1, 4096], n_patch * P^2 < 2^31, else LAE_EINVAL. */
LAE_API int lae_patch_pack(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, int normalize, float* x,
                           void* stream);
/* lae_patch_pack's transpose onto the prediction: grad_pred[r, c] = grad_x[2p + 1, c, i, j] * (normalize ? 2 : 1) / scale_c, fp32
 * [n_patch * P^2, 3]; every row is written, no zero fill needed. */
LAE_API int lae_patch_unpack_grad(const float* grad_x, uint32_t n_patch, uint32_t patch_size, int normalize, float* grad_pred,
                                  void* stream);
#define LAE_CONSISTENCY_SCRATCH_DOUBLES 16384
/* multi-view consistency of two rendered views (the reference's scripts/eval/consistency_metrics.py with the optical flow
 * replaced by the reprojection through the views' own depth; the metric is written down above k_consistency_pair in
 * csrc/evaluate.hip and in DESIGN.md section 4i).  a is the source view, b the target.  frame_a / frame_b [H*W,3] as stored
 * (frame_dtype 0 uint8 = value / 255, 2 fp32; both frames of one dtype); depth_* the raw sum w t and opacity_* the weights_sum of
 * render_eval(scale_depth=False), fp32 [H*W]; pose_* device fp32 [4,4] cam2world, row-major; one set of intrinsics; a pixel has
 * geometry iff opacity >= min_opacity (> 0).  One gather pass, one lane per pixel of b; the flows are recomputed in registers.
 *   sse_out / count_out  one double each: the sum over the valid pixels of sum_c (warped_c - frame_b_c)^2 (differences and sum in
 *                   fp64) and the number of valid pixels; per-block partials in scratch (LAE_CONSISTENCY_SCRATCH_DOUBLES doubles)
 *                   added in a fixed order, no atomics: two calls give the same bits.  count == 0 is a legal result (sse = 0);
 *                   warp_mse = sse / count is the caller's division.
 *   valid           optional uint8 [H*W]: 1 where the pixel counts
 *   warped          optional fp32 [H*W,3]: frame a warped onto b, 0 where invalid
 *   lpips_in        optional fp32 [2,3,H*W] planes with lae_eval_view's scaling: index 0 valid ? warped : frame_b, index 1 frame_b
 * NULL inputs / slots: LAE_ENULL; another dtype, H or W < 2, H * W >= 2^31, fx, fy or min_opacity <= 0: LAE_EINVAL; both before
 * any launch. */
LAE_API int lae_consistency_pair(const void* frame_a, const void* frame_b, int frame_dtype, const float* depth_a, const float* opacity_a,
                                 const float* depth_b, const float* opacity_b, const float* pose_a, const float* pose_b, float fx,
                                 float fy, float cx, float cy, uint32_t H, uint32_t W, float min_opacity, double* scratch,
                                 double* sse_out, double* count_out, uint8_t* valid, float* warped, float* lpips_in, void* stream);

/* ---- SSIM (csrc/ssim.hip): the reference's SSIMMeter (nerf/utils.py:259-293, torchmetrics' structural_similarity_index_measure with
 * its defaults) as an evaluation metric, and 1 - SSIM as a training term on patches.  laenerf_amd/metrics.py restates all of it in
 * float64 (ssim_numpy, ssim_grad_numpy).  One definition, used by all three entries:
 *
 *   x is the prediction, y the target, both [H, W, 3]; values are used as given, without clamping.
 *   Window: 11 taps, g[k] = exp(-((k - 5) / 1.5)^2 / 2), normalised to sum 1; the 2-D window is g (x) g.
 *   Window positions: for every channel and every 0 <= i <= H - 11, 0 <= j <= W - 11 the five weighted sums mx, my, exx, eyy, exy of
 *   x, y, x^2, y^2, x y over the 11 x 11 pixels from (i, j) on -- only windows that lie fully inside the image count (torchmetrics
 *   reflect-pads by 5 and crops 5 again, which is the same set).  Then
 *       A1 = 2 mx my + C1        A2 = 2 (exy - mx my) + C2
 *       B1 = mx^2 + my^2 + C1    B2 = (exx - mx^2) + (eyy - my^2) + C2
 *       S  = A1 A2 / (B1 B2)     C1 = (0.01 L)^2,  C2 = (0.03 L)^2          (the variances are not clamped)
 *   Score: SSIM(x, y) = the mean of S over the 3 (H - 10)(W - 10) values.  H < 11 or W < 11: LAE_EINVAL.
 *   Data range L: a positive number, or (data_range <= 0) "from the data": max(max x - min x, max y - min y) over the whole pair, all
 *   channels.  If L from the data is 0 (two constant images) then C1 = C2 = 0 and S = 0 / 0: the score and every map value are NaN, as
 *   torch's division gives it.
 *   Gradient with respect to x for a fixed L: per window value
 *       Dm  = (2 my A2 - 2 my A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2),   Dxx = -S / B2,   Dxy = 2 A1 / (B1 B2)
 *       dSSIM / dx[u,v,c] = ((g(x)g * Dm)[u,v,c] + 2 x[u,v,c] (g(x)g * Dxx)[u,v,c] + y[u,v,c] (g(x)g * Dxy)[u,v,c]) / (3 (H - 10)(W - 10))
 *   where * spreads every window's value back over its 11 x 11 pixels (the transpose of the forward pass).
 *   Arithmetic: the inputs are fp32; every window sum, S, Dm, Dxx, Dxy and the spread are fp64 (with fp32 sums exx - mx^2 cancels);
 *   separable passes, horizontal then vertical; fixed-order reductions, no atomics: two calls give the same bits. */
#define LAE_SSIM_TILE_W 32           /* window positions per workgroup of lae_ssim: 32 columns x 16 rows */
#define LAE_SSIM_TILE_H 16
#define LAE_SSIM_MINMAX_BLOCKS 256
/* doubles of scratch lae_ssim needs for an H x W pair: 4 * LAE_SSIM_MINMAX_BLOCKS min / max partials + one partial per tile */
LAE_API uint64_t lae_ssim_scratch_doubles(uint32_t H, uint32_t W);
/* SSIM of one pair.  x, y fp32 [H*W, 3] (pred and gt_out of lae_eval_view as they are); out one double; map optional fp32
 * [H-10, W-10, 3], S rounded once; data_range <= 0 selects the data rule: a first launch leaves min / max partials in scratch and
 * the main kernel folds them on the device -- no host read, the call can be captured.  11 <= H, W <= 32768, H * W * 3 < 2^31, a
 * finite data_range, else LAE_EINVAL; NULL x, y, scratch or out: LAE_ENULL; both before any launch. */
LAE_API int lae_ssim(const float* x, const float* y, uint32_t H, uint32_t W, double data_range, double* scratch, double* out,
                     float* map, void* stream);
/* SSIM of every patch of a patch batch.  pred, gt fp32 [n_patch * P^2, 3] in lae_patch_pack's row order (row r is pixel
 * ((r % P^2) / P, r % P) of patch r / P^2); per_patch one double per patch, its SSIM(pred patch, gt patch).  One workgroup per patch.
 * 11 <= P <= 4096, n_patch <= 65535, n_patch * P^2 * 3 < 2^31 and a positive finite data_range (the data rule has no gradient, so
 * the training term does not offer it), else LAE_EINVAL. */
LAE_API int lae_ssim_patch_forward(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, double data_range,
                                   double* per_patch, void* stream);
/* grad_pred[r, c] = gout[0] * d (mean over the patches of SSIM) / d pred[r, c], fp32 [n_patch * P^2, 3], every element written by its
 * one owner; gout a device fp32 scalar read by the kernel.  Tiled (16 x 16 pixels per workgroup), so P has no upper limit but
 * lae_ssim_patch_forward's.  The same argument rules. */
LAE_API int lae_ssim_patch_backward(const float* pred, const float* gt, uint32_t n_patch, uint32_t patch_size, double data_range,
                                    const float* gout, float* grad_pred, void* stream);

/* ---- training-camera pose refinement (csrc/gridencoder.hip, csrc/pose.hip; laenerf_amd/poses.py restates all three in float64)
 *
 * lae_grid_input_grad: d loss / d x of the samples, without the reference's dy_dx buffer (K13 + K15, gridencoder.cu:201-243, 343-369:
 * L * D * C values per sample written by the forward and summed in fp16).  inputs fp32 [M,3]; embeddings the fp16 table; grad_feats
 * fp16 [L, M, 2], level-major (what lae_nerf_field_backward leaves in grad_enc); in_shift / in_scale the map of
 * lae_grid_encode_forward_ex; grad_x fp32 [M,3], overwritten.  Every (sample, level) recomputes its cell and fractional position with
 * the forward's statements, gathers the forward's eight corners and sums per axis, in fp32,
 *     scale * w(other two axes) * (table[right] - table[left]) * grad_feats[l, b, ch]   over the 4 corner pairs and 2 channels;
 * the sum over the levels is multiplied by in_scale.  A row with a coordinate outside [0,1] after the map gives zeros.  One owner per
 * output row, no atomics: two calls give the same bits.  Supported: D = 3, C = 2, dtype LAE_F16, linear interpolation, both grid
 * types, both align_corners values, 1 <= L <= 32; anything else is LAE_EINVAL before the first launch. */
LAE_API int lae_grid_input_grad(const float* inputs, const void* embeddings, const int32_t* offsets, const void* grad_feats, float* grad_x,
                                uint32_t M, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                int align_corners, uint32_t interp, int dtype, float in_shift, float in_scale, void* stream);
/* per ray, the gradient of the loss with respect to a rigid motion of the ray's camera in the world-frame tangent space: moving the
 * camera (R, T) to (Exp(w) R, T + t) moves every sample x of its rays to T + t + Exp(w)(x - T), so d loss / d t = sum_k g_k and
 * d loss / d w = sum_k (x_k - T) x g_k.  rays int32 [N,3] (ray id, offset, count: lae_march_rays_train's), xyzs and grad_x fp32
 * [M,3], rays_o fp32 [N,3] (indexed by ray id); out double [N,6] indexed by ray id = (sum g, sum (x - o) x g), products and sums in
 * fp64: lane j of the ray's wave adds its samples j, j + 64, ... in order, then the 64 lanes are added as a fixed tree (same bits on
 * every run).  A ray with count 0, or whose samples do not fit into M (offset + count > M: the compositing kernels drop it), writes
 * zeros.  The gradient through the view direction, through nears / fars and through the occupancy decisions is not part of it. */
LAE_API int lae_pose_ray_grad(const int32_t* rays, const float* xyzs, const float* grad_x, const float* rays_o, uint32_t N, uint32_t M,
                              double* out, void* stream);
/* one launch, one workgroup per image: (a) the per-ray vectors of the rays whose image is this one (image = inds[n] / hw; inds int64
 * [N] as lae_sample_train_batch writes it, either sampler mode) are added in fp64 in a fixed order; (b) a sparse Adam step in the
 * tangent space: g = sum * (double)opt_state[7] (1 / loss scale, a float), count += 1, m = beta1 m + (1 - beta1) g,
 * v = beta2 v + (1 - beta2) g^2, delta = -(lr / (1 - beta1^count)) * m / (sqrt(v) / sqrt(1 - beta2^count) + eps), torch.optim.Adam's
 * formulas in fp64 with the image's own count; lr is *lr (a float in device memory).  An image without a ray in the batch is not
 * touched at all; with opt_state[3] (skip) non-zero nothing is touched; an image whose g is not finite is skipped on its own;
 * (c) R <- Exp(delta[3:6]) R, tau <- tau + delta[0:3] on the fp64 master [n_img, 12] (rows of [R | tau]); Rodrigues' formula in fp64,
 * the series sin x / x = 1 - x^2 / 6, (1 - cos x) / x^2 = 1 / 2 - x^2 / 24 for x^2 < 1e-12; a zero rotation or translation component
 * leaves the operand's bits alone; (d) train_poses fp32 [n_img, 4, 4]: the 3 x 4 top of the image's matrix is rewritten from the
 * master.  m, v double [n_img, 6]; counts int32 [n_img]; opt_state the 16 words of the main optimizer (read only). */
LAE_API int lae_pose_step(const double* ray_grads, const int64_t* inds, uint32_t N, uint64_t hw, uint32_t n_img, double* master,
                          double* m, double* v, int32_t* counts, float* train_poses, const int32_t* opt_state, const float* lr,
                          double beta1, double beta2, double eps, void* stream);

/* ---- per-image exposure and white balance (csrc/exposure.hip; laenerf_amd/exposure.py restates both kernels in float64)
 *
 * Image i carries a log2 gain e[i][c] per colour channel; the *_gain samplers multiply the target colour by
 * gains[i][c] = 2^(e[i][c] - mean_i e[.][c]).  Every colour criterion is a function of pred - gt (MAPE's denominator is detached), so
 * d loss / d gt = -d loss / d pred and, with d gt / d e = ln 2 * fg,
 *     G[i][c] = -(ln 2 / (3 N)) * sum over the rays n with inds[n] / hw == i of  w_n^2 * dv(pred_nc - gt_nc) * fg_nc.
 * lae_exposure_step, one launch, one workgroup per image: (a) the sum in fp64 and in a fixed order (thread t of 1024 adds its rays
 * t, t + 1024, ... in order, then the partial sums are added as a fixed tree).  pred (the step's image), gt and fg (the sampler's) fp32
 * [N,3]; dv the element derivative of loss_kind (LAE_LOSS_*, loss_param Huber's delta) on the fp32 residual e = pred - gt, with one
 * difference: a NaN residual gives a NaN dv under every criterion (sign(NaN) = 0 must not hide it); w_n = weights[inds[n]] (a plane of
 * weights_dtype LAE_IMG_F16 / LAE_IMG_F32, [n_img * hw]) or 1 with weights NULL; N is the divisor of the fused step's mean.  The gradient
 * is analytic: no loss scale enters.  gray != 0: the three components are replaced by (G0 + G1) + G2 (one exposure per image, three
 * equal columns).  (b) a sparse Adam step per image: count += 1, m = beta1 m + (1 - beta1) G, v = beta2 v + (1 - beta2) G^2,
 * delta = -(lr / (1 - beta1^count)) * m / (sqrt(v) / sqrt(1 - beta2^count) + eps), torch.optim.Adam's formulas in fp64 with the image's
 * own count, lr = *lr (a float in device memory).  An image without a ray in the batch is not touched at all; with opt_state[3] (the
 * main optimizer's skip word) non-zero nothing is touched; an image whose G is not finite is skipped on its own.  (c) e <- e + delta on
 * the fp64 master [n_img,3] (a zero delta leaves the bits alone).  m, v double [n_img,3]; counts int32 [n_img].
 * lae_exposure_publish, one workgroup: mean_c = (sum over the images of master[i][c], fp64, fixed order) / n_img, or 0 with center == 0;
 * gains[i][c] = (float)exp2(master[i][c] - mean_c).  The master is not re-centred (the moments stay consistent with it) and the gradient
 * ignores the -1/n coupling through the mean: the centring is a projection after the step.  A master of zeros publishes exactly 1.0f. */
LAE_API int lae_exposure_step(const float* pred, const float* gt, const float* fg, const int64_t* inds, uint32_t N, uint64_t hw,
                              uint32_t n_img, const void* weights, int weights_dtype, int loss_kind, float loss_param, int gray,
                              double* master, double* m, double* v, int32_t* counts, const int32_t* opt_state, const float* lr,
                              double beta1, double beta2, double eps, void* stream);
LAE_API int lae_exposure_publish(const double* master, uint32_t n_img, int center, float* gains, void* stream);

/* MI355X-native: 0 (default) = fused backward (activations recomputed in registers, forward_buffer /
 * backward_buffer untouched: both are scratch the reference's Python never reads), every wave accumulating all dW tiles
 * over its own rows, operands transposed on the matrix cores (round 3); 1 = always the three-kernel path that fills both
 * buffers exactly like the reference; 3 = fused backward with the dW tiles divided among the waves of a workgroup (the
 * round-2 kernel, kept as the one A/B predecessor).  Any other value: LAE_EINVAL (round 4 removed the first fused design,
 * mode 2, and the superseded fused-head forward kernels, modes 16-18). */
LAE_API int lae_ffmlp_set_mode(int mode);

/* ffmlp.cu:721-740: the reference keeps process-global side streams for its
 * split-K CUTLASS GEMMs.  The MFMA backward reduces dW inside one stream, so
 * these are accepted and ignored (kept so FFMLP.__init__ runs unmodified). */
LAE_API int lae_allocate_splitk(uint64_t size);
LAE_API int lae_free_splitk(void);

/* MI355X-native: library workspaces (see the header comment).  lae_free_workspaces() frees the live and the retired
 * buffers of every device after synchronising it; the caller guarantees that no captured graph that used the library
 * is replayed afterwards.  lae_workspace_bytes(0 / 1) = bytes currently held live / retired. */
LAE_API int lae_free_workspaces(void);
LAE_API uint64_t lae_workspace_bytes(int retired);

#ifdef __cplusplus
}
#endif
#endif /* LAENERF_H */
