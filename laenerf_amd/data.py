"""Posed training images resident on the device, and the per-step ray batch drawn from them.

The reference's loader (NeRFDataset, nerf/provider.py) keeps the images on the GPU (`preload`) and builds every training
batch in `collate` -> `get_rays` -> `Trainer.train_step` (nerf/utils.py:62-153, 560-580): a pixel draw, a gather of the
targets, an sRGB -> linear conversion when asked, and a blend of the alpha channel over a per-pixel random background --
about 15 torch launches and host-side randomness per step.  `ResidentImages.sample` is ONE kernel
(`lae_sample_train_batch`, csrc/batch.hip) whose step number lives in device memory and is advanced by the call, so a
captured graph draws a fresh batch on every replay.  Its generator is stated in include/laenerf.h (Philox4x32-10 keyed by
the seed, counter (step, ray, word, 0)); `philox4x32_10` / `draw_indices` below restate it in numpy.

Deviation: the reference shuffles the image order once per epoch; here the image of a batch (mode 'image', the
reference's batch_size = 1) or of every ray (mode 'all', as instant-ngp) is drawn i.i.d.

With an error map (`error_map=True` / `enable_error_map`: the reference's --error_map and LAENeRF's --use_error_maps) the
pixels of a batch are drawn by 128 x 128 cell weights per image (`lae_sample_train_batch_weighted`: torch.multinomial's
without-replacement algorithm, then a uniform pixel inside each cell), and `update_error_map` writes the per-ray error back
(`lae_error_map_update`).  `draw_cells`, `cell_pixels` and `ema_update` restate both rules in numpy.

`sample(n_rays, patch_size=P)` draws n_rays / P^2 square patches of P x P pixels instead of independent pixels (the reference's
--patch_size, nerf/utils.py:88-105; `lae_sample_train_batch_patch`, restated by `draw_patches`): the batch the Trainer's LPIPS term needs.

After `enable_exposure_refinement()` the batch's targets are multiplied by a per-image, per-channel gain before the blend
(`lae_sample_train_batch_gain` / `_weighted_gain`) and `exposure_step` learns those gains from the step's image (csrc/exposure.hip;
laenerf_amd/exposure.py restates it).
"""
import json
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

__all__ = ["ResidentImages", "nerf_matrix_to_ngp", "philox4x32_10", "draw_indices", "draw_patches", "draw_background", "neg_log_u", "cell_keys",
           "draw_cells", "cell_pixels", "cell_span", "ema_update", "ERROR_MAP_CELLS"]

_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}
_MODES = {"image": 0, "all": 1}
_BGS = {"white": 0, "random": 1}
ERROR_MAP_SIDE = 128
ERROR_MAP_CELLS = ERROR_MAP_SIDE * ERROR_MAP_SIDE     # the reference's 128 x 128 error map per image


def nerf_matrix_to_ngp(pose, scale=0.33, offset=(0, 0, 0)):
    """provider.py:19-27: a NeRF (blender) cam2world matrix in instant-ngp's axis order, scaled and offset"""
    pose = np.asarray(pose, dtype=np.float32)
    return np.array([
        [pose[1, 0], -pose[1, 1], -pose[1, 2], pose[1, 3] * scale + offset[0]],
        [pose[2, 0], -pose[2, 1], -pose[2, 2], pose[2, 3] * scale + offset[1]],
        [pose[0, 0], -pose[0, 1], -pose[0, 2], pose[0, 3] * scale + offset[2]],
        [0, 0, 0, 1],
    ], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- the RNG
def philox4x32_10(ctr, key):
    """Philox4x32-10 on numpy arrays: ctr [..., 4] uint32, key [..., 2] uint32 (broadcast) -> [..., 4] uint32"""
    c = [np.asarray(ctr, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key, dtype=np.uint32)[..., 0].astype(np.uint64)
    k1 = np.asarray(key, dtype=np.uint32)[..., 1].astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & m32
        hi1, lo1 = p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([x.astype(np.uint32) for x in c], axis=-1)


def _u32(seed, step, ray, word, w3=0):
    ray = np.asarray(ray, dtype=np.uint64)
    step = np.asarray(step, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    ctr = np.stack(np.broadcast_arrays(step, ray, np.uint64(word), np.uint64(w3)), axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(ctr.astype(np.uint32), key.astype(np.uint32))[..., 0]


def _scale(u, n):
    return ((u.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def draw_indices(seed, step, n_rays, n_img, H, W, mode="image"):
    """numpy restatement of the kernel's draw -> (image [N] int64, pixel [N] int64)"""
    rays = np.arange(n_rays, dtype=np.uint64)
    pix = _scale(_u32(seed, step, rays, 0), H * W)
    img_ray = np.full(n_rays, 0xFFFFFFFF, dtype=np.uint64) if mode == "image" else rays
    img = _scale(_u32(seed, step, img_ray, 1), n_img)
    return img, pix


def draw_patches(seed, step, n_patch, P, n_img, H, W, mode="image"):
    """numpy restatement of the patch sampler's draw (lae_sample_train_batch_patch) -> (image [n_patch], row [n_patch],
    col [n_patch], inds [n_patch * P^2]), all int64: the top-left corner of patch q from words 5 and 6 of "ray" q with the
    reference's exclusive bounds H - P and W - P (nerf/utils.py:93-94), its image from word 1 of 0xFFFFFFFF ('image') or of q
    ('all'), and inds = image * H * W + y * W + x of its pixels in row-major order"""
    P = int(P)
    if not 2 <= P < min(H, W):
        raise ValueError("draw_patches: 2 <= P < min(H, W) expected")
    q = np.arange(n_patch, dtype=np.uint64)
    row = _scale(_u32(seed, step, q, 5), H - P)
    col = _scale(_u32(seed, step, q, 6), W - P)
    img_ray = np.full(n_patch, 0xFFFFFFFF, dtype=np.uint64) if mode == "image" else q
    img = _scale(_u32(seed, step, img_ray, 1), n_img)
    i, j = np.divmod(np.arange(P * P, dtype=np.int64), P)
    inds = img[:, None] * (H * W) + (row[:, None] + i[None]) * W + (col[:, None] + j[None])
    return img, row, col, inds.reshape(-1)


def draw_background(seed, step, n_rays):
    """numpy restatement of the kernel's RANDOM background -> [N,3] float32"""
    rays = np.arange(n_rays, dtype=np.uint64)
    return np.stack([(_u32(seed, step, rays, 2 + c) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
                     for c in range(3)], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- error map
_LOG_P = [7.0376836292e-2, -1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1,
          2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1]


def neg_log_u(j):
    """-ln(j * 2^-25) for odd j in [1, 2^25) (uint32 array) -> float32: the kernel's logarithm (include/laenerf.h), every
    step one fp32 rounding in the kernel's order"""
    j = np.asarray(j, dtype=np.int64)
    p = np.zeros(j.shape, np.int64)
    for b in range(26):                                                   # bit length
        p = np.where(j >> b != 0, b + 1, p)
    p = np.where(2 * j * j < (np.int64(1) << (2 * p)), p - 1, p)
    f32 = np.float32
    f = (j - (np.int64(1) << p)).astype(f32) * np.ldexp(f32(1), -p).astype(f32)
    e = (p - 25).astype(f32)
    z = f * f
    P = np.full(j.shape, f32(_LOG_P[0]), f32)
    for c in _LOG_P[1:]:
        P = P * f + f32(c)
    y = f * (z * P)
    y = y + e * f32(-2.12194440e-4)
    y = y + f32(-0.5) * z
    r = f + y
    r = r + e * f32(0.693359375)
    return -r


def cell_keys(seed, step, weights):
    """the kernel's keys w / E of one map row [16384] -> uint32 bit patterns (a weight that is negative, NaN or infinite: 0).
    `step` may be an array [S, 1] (-> keys [S, n cells]); a shorter row restates the rule on its first cells."""
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    c = np.arange(w.size, dtype=np.uint64)
    v = _u32(seed, step, c, 0, 1)
    E = neg_log_u(((v >> np.uint32(8)).astype(np.int64) << 1) | 1)
    ok = (w > 0) & np.isfinite(w)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        key = np.where(ok, np.where(ok, w, np.float32(0)) / E, np.float32(0)).astype(np.float32)
    return key.view(np.uint32)


def draw_cells(seed, step, weights, n):
    """numpy restatement of the weighted draw's cells: the n largest keys (as uint32; ties to the lower cell), in increasing
    cell order -> int64 [n] (or [S, n] for steps [S, 1])"""
    key = cell_keys(seed, step, weights).astype(np.int64)
    idx = np.broadcast_to(np.arange(key.shape[-1]), key.shape)
    order = np.lexsort((idx, -key), axis=-1)                              # key descending, then cell ascending
    return np.sort(order[..., :n], axis=-1).astype(np.int64)


def _cell_rows_cols(cells, rx, ry, H, W):
    f32 = np.float32
    sx, sy = f32(H / ERROR_MAP_SIDE), f32(W / ERROR_MAP_SIDE)
    cells = np.asarray(cells, dtype=np.int64)
    cx, cy = (cells // ERROR_MAP_SIDE).astype(f32), (cells % ERROR_MAP_SIDE).astype(f32)
    row = np.minimum((cx * sx + f32(rx) * sx).astype(np.int64), H - 1)    # astype(int64) truncates
    col = np.minimum((cy * sy + f32(ry) * sy).astype(np.int64), W - 1)
    return row, col


def cell_pixels(seed, step, cells, H, W):
    """numpy restatement of the pixel drawn in cell cells[n] by ray n -> flat pixel index row * W + col, int64 [N]"""
    rays = np.arange(len(cells), dtype=np.uint64)
    two24 = np.float32(2.0 ** -24)
    rx = (_u32(seed, step, rays, 0) >> np.uint32(8)).astype(np.float32) * two24
    ry = (_u32(seed, step, rays, 5) >> np.uint32(8)).astype(np.float32) * two24
    row, col = _cell_rows_cols(cells, rx, ry, H, W)
    return row * W + col


def cell_span(cells, H, W):
    """the pixels the rule can give in each cell: (row_lo, row_hi, col_lo, col_hi), inclusive (the rule is monotone in rx, ry)"""
    lo = _cell_rows_cols(cells, np.float32(0), np.float32(0), H, W)
    hi = _cell_rows_cols(cells, np.float32(1 - 2.0 ** -24), np.float32(1 - 2.0 ** -24), H, W)
    return lo[0], hi[0], lo[1], hi[1]


def ema_update(error_map, inds, cells, pred, gt, H, W, loss="mse", huber_delta=0.1):
    """numpy restatement of lae_error_map_update[_crit] on a copy of error_map [n_img, 16384] -> the updated map; loss: the colour
    criterion whose element loss takes the squared error's place (raymarching.colour_loss_numpy in float32)"""
    out = np.array(error_map, dtype=np.float32, copy=True)
    f32 = np.float32
    d = np.asarray(pred, f32) - np.asarray(gt, f32)
    if loss == "mse":
        err = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / f32(3)
    else:
        from .raymarching.raymarching import colour_loss_numpy
        v = colour_loss_numpy(d, np.asarray(gt, f32), loss, huber_delta, dtype=f32)[0]
        err = ((v[:, 0] + v[:, 1]) + v[:, 2]) / f32(3)
    img = np.asarray(inds, np.int64) // (H * W)
    c = np.asarray(cells, np.int64)
    out[img, c] = f32(0.1) * out[img, c] + f32(0.9) * err
    return out


# ---------------------------------------------------------------------------------------------------------------- images
class ResidentImages:
    """images [n, H, W, C] (C = 3 or 4; uint8, fp16 or fp32) + cam2world poses [n, 4, 4] + one (fx, fy, cx, cy), on the GPU.

    bg: 'random' (a per-pixel uniform background, the reference's rule for C = 4) or 'white' (its bg_color = 1, used for
    C = 3); default by C.  color_space 'linear' converts the colour to linear before the blend (nerf/utils.py:564).
    depths (optional, or set_depths): a per-pixel depth plane [n, H, W], fp16 or fp32, resident on the device: the distance
    along the pixel's ray from its origin, zero = no supervision (the reference's `d_` planes, nerf/gui.py:406, 508-511).
    sample() does not read it: the Trainer's compositing kernel gathers it by the batch's `inds`.
    pixel_weights (optional, or set_pixel_weights): a per-pixel weight plane [n, H, W], fp16 or fp32, on the images' device: the weight
    of the pixel's colour residual under Trainer(pixel_weights=True) -- a mask (0 = the pixel's colour cannot matter), a confidence
    map, the Ref-NPR distillation's target weights.  second_target (optional, or set_second_target): a second colour target
    [n, H, W, 3 or 4], fp16 or fp32, for Trainer(second_weight=...); with 4 channels it is blended over the batch's background like
    the images.  sample() reads neither: the compositing kernel gathers both by the batch's `inds`.
    undistorter: None, or the undistort.Undistorter that from_transforms(undistort=True) resampled the captures with."""
    undistorter = None

    def __init__(self, images, poses, intrinsics, bound=1.0, min_near=0.2, mode="image", bg=None, color_space="srgb", seed=0,
                 device=None, error_map=False, depths=None, pixel_weights=None, second_target=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        # (device="cpu" holds the arrays on the host -- loaders and tests without a GPU; sample() needs the GPU)
        images = images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))
        if images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError("ResidentImages: images must be [n, H, W, 3 or 4]")
        if images.dtype not in _DTYPES:
            raise ValueError("ResidentImages: image dtype must be uint8, float16 or float32")
        poses = poses if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses, dtype=np.float32))
        if poses.shape != (images.shape[0], 4, 4):
            raise ValueError("ResidentImages: poses must be [n, 4, 4]")
        if mode not in _MODES:
            raise ValueError(f"ResidentImages: mode must be one of {sorted(_MODES)}")
        self.C = int(images.shape[-1])
        bg = bg if bg is not None else ("random" if self.C == 4 else "white")
        if bg not in _BGS:
            raise ValueError(f"ResidentImages: bg must be one of {sorted(_BGS)}")
        self.images = images.to(device).contiguous()
        self.poses = poses.to(device, torch.float32).contiguous()
        self.n_img, self.H, self.W = (int(x) for x in images.shape[:3])
        self.intrinsics = tuple(float(v) for v in intrinsics)
        self.bound, self.min_near = float(bound), float(min_near)
        self.aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32, device=device)
        self.mode, self.bg, self.color_space, self.seed = mode, bg, color_space, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int64, device=device)          # the kernel's step counter
        self._out = {}
        self.error_map = None
        if error_map:
            self.enable_error_map()
        self.depths = None
        if depths is not None:
            self.set_depths(depths)
        self.train_poses = self.pose_master = self.pose_m = self.pose_v = self.pose_counts = None      # enable_pose_refinement
        self.gains = self.exposure_master = self.exposure_m = self.exposure_v = self.exposure_counts = None   # enable_exposure_refinement
        self.exposure_mode = None
        self.pixel_weights = self.second_target = None
        if pixel_weights is not None:
            self.set_pixel_weights(pixel_weights)
        if second_target is not None:
            self.set_second_target(second_target)

    def _float_plane(self, name, plane, shapes):
        """a plane as set_depths stores it: fp16 / fp32 kept, other float dtypes as fp32, integers refused, on the images' device"""
        plane = plane if torch.is_tensor(plane) else torch.from_numpy(np.ascontiguousarray(plane))
        if tuple(plane.shape) not in shapes:
            raise ValueError(f"ResidentImages: {name} must be " + " or ".join(str(list(s)) for s in shapes))
        if not plane.dtype.is_floating_point:
            raise ValueError(f"ResidentImages: {name} must be a floating-point plane")
        if plane.dtype not in (torch.float16, torch.float32):
            plane = plane.to(torch.float32)
        return plane.to(self.images.device).contiguous()

    def set_pixel_weights(self, plane):
        """set .pixel_weights: the weight plane [n_img, H, W] (fp16 / fp32 tensor or array; other float arrays are stored as fp32, uint8
        is refused), copied to the images' device; None removes it"""
        self.pixel_weights = None if plane is None else self._float_plane("pixel_weights", plane, [(self.n_img, self.H, self.W)])
        return self.pixel_weights

    def set_second_target(self, images):
        """set .second_target: the second colour target [n_img, H, W, 3 or 4] (fp16 / fp32 tensor or array; other float arrays are
        stored as fp32, uint8 is refused), copied to the images' device; None removes it"""
        self.second_target = None if images is None else self._float_plane(
            "second_target", images, [(self.n_img, self.H, self.W, 3), (self.n_img, self.H, self.W, 4)])
        return self.second_target

    def set_depths(self, plane):
        """set .depths: the depth plane [n_img, H, W] (fp16 / fp32 tensor or array; other float arrays are stored as fp32), copied
        to the images' device; None removes it"""
        if plane is None:
            self.depths = None
            return None
        plane = plane if torch.is_tensor(plane) else torch.from_numpy(np.ascontiguousarray(plane))
        if tuple(plane.shape) != (self.n_img, self.H, self.W):
            raise ValueError(f"ResidentImages: depths must be [{self.n_img}, {self.H}, {self.W}]")
        if not plane.dtype.is_floating_point:
            raise ValueError("ResidentImages: depths must be a floating-point plane")
        if plane.dtype not in (torch.float16, torch.float32):
            plane = plane.to(torch.float32)
        self.depths = plane.to(self.images.device).contiguous()
        return self.depths

    def enable_error_map(self, init=1.0):
        """create .error_map: [n_img, 16384] fp32 cell weights, every one `init` (the reference's torch.ones).  From then on
        sample() draws its pixels by these weights (mode 'image' only) and returns the cells it drew; the caller may write
        rows (LAENeRF's --use_error_maps seeds them from edit-grid weights)."""
        if self.mode != "image":
            raise ValueError("ResidentImages: an error map needs mode 'image' (one image per batch, as the reference)")
        self.error_map = torch.full((self.n_img, ERROR_MAP_CELLS), float(init), dtype=torch.float32, device=self.images.device)
        self._out = {}
        return self.error_map

    def enable_pose_refinement(self):
        """create the state of the camera refinement (Trainer(pose_refine=True)): .pose_master fp64 [n_img, 12] (the rows of [R | T]),
        .pose_m / .pose_v fp64 [n_img, 6] and .pose_counts int32 [n_img] (a sparse Adam in the world-frame tangent space, translation
        first) and .train_poses fp32 [n_img, 4, 4], equal to .poses bit for bit until the first update.  From then on sample() builds
        its rays from .train_poses; .poses stays the caller's input.  A second call changes nothing."""
        if self.train_poses is None:
            dev = self.poses.device
            self.train_poses = self.poses.clone()
            self.pose_master = self.poses[:, :3, :4].to(torch.float64).reshape(self.n_img, 12).contiguous()
            self.pose_m = torch.zeros(self.n_img, 6, dtype=torch.float64, device=dev)
            self.pose_v = torch.zeros(self.n_img, 6, dtype=torch.float64, device=dev)
            self.pose_counts = torch.zeros(self.n_img, dtype=torch.int32, device=dev)
        return self.train_poses

    def _sample_poses(self):
        return self.poses if self.train_poses is None else self.train_poses

    @staticmethod
    def pose_ray_grad(rays, xyzs, grad_x, rays_o, out=None):
        """lae_pose_ray_grad: per ray (sum g, sum (x - o) x g) as fp64 [N, 6] at the ray id's row (poses.pose_ray_grad_numpy)"""
        ts = (rays, xyzs, grad_x, rays_o)
        _lib.need_cuda(*ts); _lib.need_contig(*ts)
        if rays.dtype != torch.int32 or any(t.dtype != torch.float32 for t in ts[1:]):
            raise RuntimeError("pose_ray_grad: rays must be int32, xyzs / grad_x / rays_o float32")
        N, M = int(rays.shape[0]), int(xyzs.shape[0])
        if tuple(grad_x.shape) != (M, 3) or tuple(xyzs.shape) != (M, 3) or tuple(rays_o.shape) != (N, 3) or tuple(rays.shape) != (N, 3):
            raise RuntimeError("pose_ray_grad: rays [N,3], xyzs and grad_x [M,3], rays_o [N,3] expected")
        if out is None:
            out = torch.empty(N, 6, dtype=torch.float64, device=rays.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != (N, 6) or not out.is_contiguous() or out.device != rays.device:
            raise RuntimeError("pose_ray_grad: out must be a contiguous float64 [N, 6] tensor on the rays' device")
        check(_lib.load().lae_pose_ray_grad(ptr(rays), ptr(xyzs), ptr(grad_x), ptr(rays_o), N, M, ptr(out), stream()), "pose_ray_grad")
        return out

    @torch.no_grad()
    def pose_step(self, ray_grads, inds, opt_state, lr, betas=(0.9, 0.99), eps=1e-15):
        """lae_pose_step: reduce ray_grads fp64 [N, 6] by the image of inds [N], one sparse Adam step per image that received a ray,
        composed onto .pose_master; .train_poses is rewritten.  opt_state: the main optimizer's 16 device state words (skip decision
        and 1 / loss scale); lr: a float32 tensor on the device (poses.pose_step_numpy)"""
        if self.train_poses is None:
            raise ValueError("ResidentImages.pose_step: enable_pose_refinement() first")
        ts = (ray_grads, inds, opt_state, lr)
        _lib.need_cuda(*ts); _lib.need_contig(*ts)
        N = int(inds.shape[0])
        if ray_grads.dtype != torch.float64 or tuple(ray_grads.shape) != (N, 6) or inds.dtype != torch.int64:
            raise RuntimeError("pose_step: ray_grads must be float64 [N, 6], inds int64 [N]")
        if opt_state.dtype != torch.int32 or opt_state.numel() != 16 or lr.dtype != torch.float32 or lr.numel() < 1:
            raise RuntimeError("pose_step: opt_state must be the optimizer's 16 int32 words, lr a float32 tensor")
        check(_lib.load().lae_pose_step(ptr(ray_grads), ptr(inds), N, self.H * self.W, self.n_img, ptr(self.pose_master), ptr(self.pose_m),
                                        ptr(self.pose_v), ptr(self.pose_counts), ptr(self.train_poses), ptr(opt_state), ptr(lr),
                                        float(betas[0]), float(betas[1]), float(eps), stream()), "pose_step")

    def enable_exposure_refinement(self, mode="rgb"):
        """create the state of the exposure / white-balance refinement (Trainer(exposure_refine=True)): a log2 gain per image and colour
        channel as .exposure_master fp64 [n_img, 3], its sparse Adam's .exposure_m / .exposure_v fp64 [n_img, 3] and .exposure_counts
        int32 [n_img], and .gains fp32 [n_img, 3], all ones.  From then on sample() multiplies the target colour by the image's gains
        before the blend (`lae_sample_train_batch_gain` / `_weighted_gain`) and also returns fg [N,3], the part of gt that scales with
        them.  mode 'rgb': three gains per image; 'gray': one exposure per image (three equal columns).  A second call changes only the
        mode.  Gains are a physical exposure when training in linear colour, a per-image colour compensation on sRGB data."""
        from .exposure import MODES
        if mode not in MODES:
            raise ValueError(f"ResidentImages: exposure mode must be one of {sorted(MODES)}")
        if self.gains is None:
            dev = self.images.device
            self.exposure_master = torch.zeros(self.n_img, 3, dtype=torch.float64, device=dev)
            self.exposure_m = torch.zeros(self.n_img, 3, dtype=torch.float64, device=dev)
            self.exposure_v = torch.zeros(self.n_img, 3, dtype=torch.float64, device=dev)
            self.exposure_counts = torch.zeros(self.n_img, dtype=torch.int32, device=dev)
            self.gains = torch.ones(self.n_img, 3, dtype=torch.float32, device=dev)
            self._out = {}                                                    # the batch buffers gain an fg
        self.exposure_mode = mode
        return self.gains

    @torch.no_grad()
    def exposure_step(self, pred, batch, opt_state, lr, loss="mse", huber_delta=0.1, pixel_weights=None, betas=(0.9, 0.99), eps=1e-15,
                      center=True):
        """lae_exposure_step + lae_exposure_publish: the gradient of the step's colour criterion with respect to every image's log2
        gains from pred [N,3] (the step's image) and the batch's gt / fg / inds, one sparse Adam step per image that received a ray on
        .exposure_master, then .gains = 2^(master - mean over the images) (center=False: 2^master).  opt_state: the main optimizer's
        16 device state words (its skip decision); lr: a float32 tensor on the device; loss / huber_delta: the criterion the step
        trained on; pixel_weights: the weight plane the step used ([n_img, H, W], fp16 or fp32) or None
        (exposure.exposure_step_numpy / exposure_publish_numpy)"""
        if self.gains is None:
            raise ValueError("ResidentImages.exposure_step: enable_exposure_refinement() first")
        from .backend import loss_kind
        from .exposure import MODES
        kind, param = loss_kind("ResidentImages.exposure_step", loss, huber_delta)
        gt, fg, inds = batch["gt"], batch["fg"], batch["inds"]
        n = int(inds.shape[0])
        pred = pred.detach().reshape(-1, 3)
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        if pred.shape[0] != n or tuple(gt.shape) != (n, 3) or tuple(fg.shape) != (n, 3):
            raise ValueError("ResidentImages.exposure_step: pred, gt and fg must be [N, 3] for the batch's N rays")
        ts = (pred, gt, fg, inds, opt_state, lr)
        _lib.need_cuda(*ts); _lib.need_contig(*ts)
        if gt.dtype != torch.float32 or fg.dtype != torch.float32 or inds.dtype != torch.int64:
            raise RuntimeError("exposure_step: gt and fg must be float32, inds int64")
        if opt_state.dtype != torch.int32 or opt_state.numel() != 16 or lr.dtype != torch.float32 or lr.numel() < 1:
            raise RuntimeError("exposure_step: opt_state must be the optimizer's 16 int32 words, lr a float32 tensor")
        w = pixel_weights
        if w is not None:
            _lib.need_cuda(w); _lib.need_contig(w)
            if w.dtype not in (torch.float16, torch.float32) or w.numel() != self.n_img * self.H * self.W:
                raise RuntimeError("exposure_step: pixel_weights must be an fp16 / fp32 plane [n_img, H, W]")
        lib = _lib.load()
        check(lib.lae_exposure_step(ptr(pred), ptr(gt), ptr(fg), ptr(inds), n, self.H * self.W, self.n_img, ptr(w),
                                    0 if w is None else _DTYPES[w.dtype], kind, param, MODES[self.exposure_mode], ptr(self.exposure_master),
                                    ptr(self.exposure_m), ptr(self.exposure_v), ptr(self.exposure_counts), ptr(opt_state), ptr(lr),
                                    float(betas[0]), float(betas[1]), float(eps), stream()), "exposure_step")
        check(lib.lae_exposure_publish(ptr(self.exposure_master), self.n_img, int(bool(center)), ptr(self.gains), stream()),
              "exposure_publish")

    @classmethod
    def from_arrays(cls, images, poses, intrinsics, **kw):
        return cls(images, poses, intrinsics, **kw)

    @classmethod
    def from_transforms(cls, path, scale=0.33, offset=(0, 0, 0), downscale=1, dtype="uint8", split=None, undistort=False, balance=0.0,
                        **kw):
        """a blender-style scene: `path` is a transforms.json (or a directory holding transforms[_split].json).  Poses go
        through nerf_matrix_to_ngp; focal lengths from fl_x / fl_y or camera_angle_x / _y, cx / cy default to W/2, H/2
        (provider.py:277-290); images are decoded with PIL and resized with a box filter when `downscale` > 1 (the
        reference's cv2 INTER_AREA).  dtype 'uint8' keeps the 8-bit values (4x less memory), 'float16' / 'float32' store
        value / 255.
        Lens distortion (the k1, k2, k3, k4, p1, p2, is_fisheye / camera_model keys scripts/colmap2nerf.py writes, globally or per
        frame): undistort=False ignores it, as the reference's loader does, and warns once when a coefficient is not zero.
        undistort=True resamples the captures on the device into one pinhole camera (laenerf_amd/undistort.py): global keys and
        per-frame overrides of fl_x, fl_y, cx, cy and the coefficients are read, `downscale` is applied first (it scales fx, fy,
        cx, cy; the coefficients are scale-free), frames of different sizes are refused, .intrinsics is the target camera
        (undistort.target_intrinsics(cams, H, W, balance)) and .undistorter the Undistorter (its .redistort takes rendered frames
        back to the photographs' geometry).  balance = 0 crops to the pixels every capture covers; balance > 0 keeps more of the
        captures and leaves invalid pixels (all zeros): .pixel_weights is then set to the valid plane (times the remapped
        `pixel_weights=` where given) -- train with Trainer(pixel_weights=True), or an invalid RGBA pixel is trained as empty
        space.  Planes passed in (`depths=`, `pixel_weights=`: nearest; `second_target=`: bilinear) are given in the captures'
        geometry and are remapped the same way."""
        from PIL import Image
        if os.path.isdir(path):
            path = os.path.join(path, f"transforms_{split}.json" if split else "transforms.json")
        root = os.path.dirname(os.path.abspath(path))
        with open(path) as f:
            transform = json.load(f)
        H = W = None
        if "h" in transform and "w" in transform:
            H, W = int(transform["h"]) // downscale, int(transform["w"]) // downscale
        poses, images, used, sizes = [], [], [], set()
        for fr in transform["frames"]:
            f_path = os.path.join(root, fr["file_path"])
            if "." not in os.path.basename(f_path):
                f_path += ".png"
            if not os.path.exists(f_path):
                continue
            poses.append(nerf_matrix_to_ngp(np.array(fr["transform_matrix"], dtype=np.float32), scale=scale, offset=offset))
            im = Image.open(f_path)
            im = im.convert("RGBA" if im.mode in ("RGBA", "LA", "PA") or "transparency" in im.info else "RGB")
            used.append(fr)
            sizes.add((im.height, im.width))
            if H is None:
                H, W = im.height // downscale, im.width // downscale
            if (im.height, im.width) != (H, W):
                im = im.resize((W, H), Image.BOX)
            images.append(np.asarray(im, dtype=np.uint8))
        if not images:
            raise RuntimeError(f"ResidentImages.from_transforms: no image of {path} found")
        images = np.stack(images)
        if dtype in ("float16", "float32", torch.float16, torch.float32):
            np_dt = np.float16 if dtype in ("float16", torch.float16) else np.float32
            images = (images.astype(np.float32) / 255).astype(np_dt)
        elif dtype not in ("uint8", torch.uint8):
            raise ValueError("from_transforms: dtype must be 'uint8', 'float16' or 'float32'")
        if "fl_x" in transform or "fl_y" in transform:
            fl_x = (transform["fl_x"] if "fl_x" in transform else transform["fl_y"]) / downscale
            fl_y = (transform["fl_y"] if "fl_y" in transform else transform["fl_x"]) / downscale
        elif "camera_angle_x" in transform or "camera_angle_y" in transform:
            fl_x = W / (2 * math.tan(transform["camera_angle_x"] / 2)) if "camera_angle_x" in transform else None
            fl_y = H / (2 * math.tan(transform["camera_angle_y"] / 2)) if "camera_angle_y" in transform else None
            fl_x = fl_y if fl_x is None else fl_x
            fl_y = fl_x if fl_y is None else fl_y
        else:
            raise RuntimeError("ResidentImages.from_transforms: no focal length in the transforms file")
        cx = transform["cx"] / downscale if "cx" in transform else W / 2
        cy = transform["cy"] / downscale if "cy" in transform else H / 2
        if not undistort:
            if any(d.get(k, 0) != 0 for d in [transform] + used for k in ("k1", "k2", "k3", "k4", "p1", "p2")):
                import warnings
                warnings.warn("ResidentImages.from_transforms: the transforms file has non-zero lens distortion coefficients, which "
                              "are being ignored; pass undistort=True to resample the captures into a pinhole camera", stacklevel=2)
            return cls(images, np.stack(poses), (fl_x, fl_y, cx, cy), **kw)
        return cls._undistorted(images, np.stack(poses), transform, used, sizes, H, W, downscale, balance, kw)

    @classmethod
    def _undistorted(cls, images, poses, transform, frames, sizes, H, W, downscale, balance, kw):
        """from_transforms(undistort=True): the captures and the planes of `kw` resampled on the device into one pinhole camera"""
        from .undistort import CameraModel, Undistorter, target_intrinsics
        if len(sizes) != 1:
            raise ValueError(f"ResidentImages.from_transforms(undistort=True): frames of different sizes {sorted(sizes)} (a camera's "
                             "intrinsics belong to one size)")
        h0, w0 = next(iter(sizes))
        cams, index, seen = [], [], {}
        for fr in frames:
            cam = CameraModel.from_transforms(transform, fr, H=h0, W=w0, downscale=downscale)
            key = cam.record().tobytes()
            if key not in seen:
                seen[key] = len(cams)
                cams.append(cam)
            index.append(seen[key])
        target = target_intrinsics(cams, H, W, balance)
        device = kw.get("device")
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        und = Undistorter(cams, index, target, H, W, device=device)
        planes = {}
        for name, mode in (("depths", "nearest"), ("pixel_weights", "nearest"), ("second_target", "bilinear")):
            plane = kw.pop(name, None)
            if plane is not None:
                plane = plane if torch.is_tensor(plane) else torch.from_numpy(np.ascontiguousarray(plane))
                if not plane.dtype.is_floating_point:
                    raise ValueError(f"ResidentImages: {name} must be a floating-point plane")
                if plane.dtype not in (torch.float16, torch.float32):
                    plane = plane.to(torch.float32)
                planes[name] = und.images(plane) if name == "second_target" else und.plane(plane, mode)
        valid = und.valid
        if not bool(valid.all()):                                                 # one host read, at load time
            w = planes.get("pixel_weights")
            planes["pixel_weights"] = valid.to(torch.float32) if w is None else w * valid.to(w.dtype)
        data = cls(und.images(torch.from_numpy(images)), poses, target, **planes, **kw)
        data.undistorter = und
        return data

    def _buffers(self, n):
        out = self._out.get(n)
        if out is None:
            dev = self.images.device
            out = self._out[n] = {
                "rays_o": torch.empty(n, 3, dtype=torch.float32, device=dev), "rays_d": torch.empty(n, 3, dtype=torch.float32, device=dev),
                "nears": torch.empty(n, dtype=torch.float32, device=dev), "fars": torch.empty(n, dtype=torch.float32, device=dev),
                "gt": torch.empty(n, 3, dtype=torch.float32, device=dev), "inds": torch.empty(n, dtype=torch.int64, device=dev),
                "bg": torch.empty(n, 3, dtype=torch.float32, device=dev) if self.bg == "random" else None,
            }
            if self.error_map is not None:
                out["cells"] = torch.empty(n, dtype=torch.int32, device=dev)
            if self.gains is not None:
                out["fg"] = torch.empty(n, 3, dtype=torch.float32, device=dev)
        return out

    @torch.no_grad()
    def check_patch_size(self, n_rays, patch_size):
        """the reasons sample(n_rays, patch_size=...) refuses (ValueError); nothing is changed"""
        P = int(patch_size)
        if self.error_map is not None:
            raise ValueError("ResidentImages: patches cannot be drawn by an error map (the reference ignores the map under --patch_size; "
                             "this sampler refuses)")
        if self.gains is not None:
            raise ValueError("ResidentImages: patches cannot be combined with exposure gains (there is no gained patch sampler)")
        if not 2 <= P < min(self.H, self.W):
            raise ValueError(f"ResidentImages: patch_size must be in [2, min(H, W)) = [2, {min(self.H, self.W)}), got {P}")
        if int(n_rays) < P * P or int(n_rays) % (P * P):
            raise ValueError(f"ResidentImages: with patch_size {P}, n_rays must be a positive multiple of {P * P}, got {int(n_rays)}")
        return P

    def _sample_patch(self, n_rays, P, step, out):
        """sample() with patch_size > 1: lae_sample_train_batch_patch; the result also holds "patch_size" """
        P = self.check_patch_size(n_rays, P)
        _lib.need_cuda(self.images)
        if step is not None:
            self.step.fill_(int(step))
        o = out if out is not None else self._buffers(int(n_rays))
        fx, fy, cx, cy = self.intrinsics
        check(_lib.load().lae_sample_train_batch_patch(
            ptr(self.images), _DTYPES[self.images.dtype], self.n_img, self.H, self.W, self.C, ptr(self._sample_poses()), fx, fy, cx, cy,
            int(n_rays), P, ptr(self.aabb), self.min_near, self.seed, ptr(self.step), _MODES[self.mode], _BGS[self.bg],
            int(self.color_space == "linear"), ptr(o["rays_o"]), ptr(o["rays_d"]), ptr(o["nears"]), ptr(o["fars"]), ptr(o["gt"]),
            ptr(o["bg"]), ptr(o["inds"]), stream()), "sample_train_batch_patch")
        res = {k: v for k, v in o.items() if k != "patch_size"}
        if res["bg"] is None:
            res["bg"] = 1
        res["patch_size"] = P
        return res

    @torch.no_grad()
    def sample(self, n_rays, step=None, out=None, patch_size=1):
        """one batch of n_rays -> dict rays_o, rays_d [N,3], nears, fars [N], gt [N,3] (blended), bg [N,3] ('random') or the
        number 1 ('white'), inds [N] (image * H * W + pixel).  step=None: the device counter's value, which the call then
        advances (capturable); step=k: the counter is set to k first.  The result tensors are reused by the next call with
        the same n_rays unless `out` (a dict of tensors from an earlier call) is passed.
        patch_size=P > 1 (the reference's --patch_size): the batch is n_rays / P^2 square patches of P x P pixels, ray r being pixel
        (r % P^2) / P, r % P of patch r / P^2 (`lae_sample_train_batch_patch`; `draw_patches` restates the draw); the result gains
        "patch_size".  In mode 'all' every patch draws its own image.  Refused (ValueError) with an error map or exposure gains on
        the data."""
        if int(patch_size) != 1:
            return self._sample_patch(n_rays, patch_size, step, out)
        if self.error_map is not None:
            return self._sample_weighted(n_rays, step, out)
        _lib.need_cuda(self.images)
        if step is not None:
            self.step.fill_(int(step))
        o = out if out is not None else self._buffers(int(n_rays))
        fx, fy, cx, cy = self.intrinsics
        head = (ptr(self.images), _DTYPES[self.images.dtype], self.n_img, self.H, self.W, self.C, ptr(self._sample_poses()), fx, fy, cx, cy,
                int(n_rays), ptr(self.aabb), self.min_near, self.seed, ptr(self.step), _MODES[self.mode], _BGS[self.bg],
                int(self.color_space == "linear"))
        if self.gains is not None:
            check(_lib.load().lae_sample_train_batch_gain(
                *head, ptr(self.gains), ptr(o["rays_o"]), ptr(o["rays_d"]), ptr(o["nears"]), ptr(o["fars"]), ptr(o["gt"]), ptr(o["fg"]),
                ptr(o["bg"]), ptr(o["inds"]), stream()), "sample_train_batch_gain")
        else:
            check(_lib.load().lae_sample_train_batch(
                *head, ptr(o["rays_o"]), ptr(o["rays_d"]), ptr(o["nears"]), ptr(o["fars"]), ptr(o["gt"]), ptr(o["bg"]), ptr(o["inds"]),
                stream()), "sample_train_batch")
        res = dict(o)
        if res["bg"] is None:
            res["bg"] = 1
        return res

    def _check_error_map(self, n_rays):
        if self.mode != "image":
            raise ValueError("ResidentImages: an error map needs mode 'image' (one image per batch, as the reference)")
        if not 0 < int(n_rays) <= ERROR_MAP_CELLS:
            raise ValueError(f"ResidentImages: with an error map n_rays must be in 1..{ERROR_MAP_CELLS} (cells drawn without replacement)")
        m = self.error_map
        if not torch.is_tensor(m) or m.shape != (self.n_img, ERROR_MAP_CELLS) or m.dtype != torch.float32 or not m.is_contiguous():
            raise ValueError(f"ResidentImages: error_map must be a contiguous float32 [{self.n_img}, {ERROR_MAP_CELLS}] tensor")
        if m.device != self.images.device:
            raise ValueError("ResidentImages: error_map must live on the images' device")

    def _sample_weighted(self, n_rays, step, out):
        """sample() with an error map: lae_sample_train_batch_weighted; the result also holds cells [N] int32"""
        self._check_error_map(n_rays)
        _lib.need_cuda(self.images)
        if step is not None:
            self.step.fill_(int(step))
        o = out if out is not None else self._buffers(int(n_rays))
        fx, fy, cx, cy = self.intrinsics
        head = (ptr(self.images), _DTYPES[self.images.dtype], self.n_img, self.H, self.W, self.C, ptr(self._sample_poses()), fx, fy, cx, cy,
                int(n_rays), ptr(self.aabb), self.min_near, self.seed, ptr(self.step), _BGS[self.bg], int(self.color_space == "linear"),
                ptr(self.error_map), ptr(o["cells"]))
        if self.gains is not None:
            check(_lib.load().lae_sample_train_batch_weighted_gain(
                *head, ptr(self.gains), ptr(o["rays_o"]), ptr(o["rays_d"]), ptr(o["nears"]), ptr(o["fars"]), ptr(o["gt"]), ptr(o["fg"]),
                ptr(o["bg"]), ptr(o["inds"]), stream()), "sample_train_batch_weighted_gain")
        else:
            check(_lib.load().lae_sample_train_batch_weighted(
                *head, ptr(o["rays_o"]), ptr(o["rays_d"]), ptr(o["nears"]), ptr(o["fars"]), ptr(o["gt"]), ptr(o["bg"]), ptr(o["inds"]),
                stream()), "sample_train_batch_weighted")
        res = dict(o)
        if res["bg"] is None:
            res["bg"] = 1
        return res

    @torch.no_grad()
    def update_error_map(self, pred, batch, loss="mse", huber_delta=0.1):
        """the reference's EMA after a step (nerf/utils.py:609-631): map[image][cell] = 0.1 * map + 0.9 * mean over RGB of
        (pred - gt)^2 for every ray of `batch` (a result of sample() with the map); pred [N,3] is the step's image.
        loss / huber_delta: the colour criterion the step trained on ('mse', 'l1', 'huber', 'mape'); its element loss takes the squared
        error's place, the reference's `error = loss.detach()` (`lae_error_map_update_crit`)"""
        if self.error_map is None:
            raise ValueError("ResidentImages.update_error_map: no error map (error_map=True or enable_error_map())")
        cells, inds, gt = batch["cells"], batch["inds"], batch["gt"]
        n = int(cells.shape[0])
        pred = pred.detach().reshape(-1, 3)
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.shape[0] != n:
            pred = pred.float().contiguous()
        if pred.shape[0] != n:
            raise ValueError("ResidentImages.update_error_map: pred must be [N, 3] for the batch's N rays")
        _lib.need_cuda(self.error_map, pred, gt)
        from .backend import loss_kind
        kind, param = loss_kind("ResidentImages.update_error_map", loss, huber_delta)
        check(_lib.load().lae_error_map_update_crit(ptr(self.error_map), self.n_img, self.H, self.W, ptr(inds), ptr(cells), ptr(pred),
                                                    ptr(gt), n, kind, param, stream()), "error_map_update_crit")

    def state_dict(self):
        """what a resumed run needs of the sampler, never the images: seed (int), step (the device counter, int64 [1], on the host)
        and error_map (a host copy, or None); with pose or exposure refinement enabled also `pose` / `exposure`, their state"""
        sd = {"seed": int(self.seed), "step": self.step.detach().cpu().clone(),
              "error_map": None if self.error_map is None else self.error_map.detach().cpu().clone()}
        if self.train_poses is not None:             # the refinement's state (only with it: files of other runs stay as they were)
            sd["pose"] = {"master": self.pose_master.detach().cpu().clone(), "m": self.pose_m.detach().cpu().clone(),
                          "v": self.pose_v.detach().cpu().clone(), "counts": self.pose_counts.detach().cpu().clone()}
        if self.gains is not None:                   # likewise the exposure refinement's (the gains as published: center is the trainer's)
            sd["exposure"] = {"master": self.exposure_master.detach().cpu().clone(), "m": self.exposure_m.detach().cpu().clone(),
                              "v": self.exposure_v.detach().cpu().clone(), "counts": self.exposure_counts.detach().cpu().clone(),
                              "gains": self.gains.detach().cpu().clone()}
        return sd

    def check_state_dict(self, sd):
        """the reasons load_state_dict would refuse `sd` (a list of strings, empty when it fits); nothing is changed"""
        bad = []
        step = sd.get("step")
        if not torch.is_tensor(step) or step.numel() != 1:
            bad.append("data.step: one int64 value expected")
        m = sd.get("error_map")
        if m is not None and (not torch.is_tensor(m) or tuple(m.shape) != (self.n_img, ERROR_MAP_CELLS)):
            bad.append(f"data.error_map: saved {list(m.shape) if torch.is_tensor(m) else type(m).__name__}, "
                       f"current {[self.n_img, ERROR_MAP_CELLS]}")
        ps = sd.get("pose")
        if ps is not None:
            want = {"master": (self.n_img, 12), "m": (self.n_img, 6), "v": (self.n_img, 6), "counts": (self.n_img,)}
            for k, shape in want.items():
                t = ps.get(k) if isinstance(ps, dict) else None
                if not torch.is_tensor(t) or tuple(t.shape) != shape:
                    bad.append(f"data.pose.{k}: saved {list(t.shape) if torch.is_tensor(t) else type(t).__name__}, current {list(shape)}")
        ex = sd.get("exposure")
        if ex is not None:
            want = {"master": (self.n_img, 3), "m": (self.n_img, 3), "v": (self.n_img, 3), "counts": (self.n_img,), "gains": (self.n_img, 3)}
            for k, shape in want.items():
                t = ex.get(k) if isinstance(ex, dict) else None
                if not torch.is_tensor(t) or tuple(t.shape) != shape:
                    bad.append(f"data.exposure.{k}: saved {list(t.shape) if torch.is_tensor(t) else type(t).__name__}, current {list(shape)}")
        return bad

    @torch.no_grad()
    def load_state_dict(self, sd):
        """state_dict()'s counterpart, written in place (a captured graph keeps reading the same counter and the same map).  A file
        without a map leaves the current one alone; a map in the file creates one where there is none."""
        bad = self.check_state_dict(sd)
        if bad:
            raise ValueError("ResidentImages.load_state_dict: " + "; ".join(bad))
        self.seed = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.step.copy_(sd["step"].to(self.step.device, torch.int64).view(1))
        m = sd.get("error_map")
        if m is not None:
            if self.error_map is None:
                self.enable_error_map()
            self.error_map.copy_(m.to(self.error_map.device, torch.float32))
        ps = sd.get("pose")
        if ps is not None:
            self.enable_pose_refinement()
            dev = self.train_poses.device
            self.pose_master.copy_(ps["master"].to(dev, torch.float64))
            self.pose_m.copy_(ps["m"].to(dev, torch.float64))
            self.pose_v.copy_(ps["v"].to(dev, torch.float64))
            self.pose_counts.copy_(ps["counts"].to(dev, torch.int32))
            # the kernel's own conversion (round to nearest); the bottom row stays the input's
            self.train_poses[:, :3, :4].copy_(self.pose_master.view(self.n_img, 3, 4).to(torch.float32))
        ex = sd.get("exposure")
        if ex is not None:
            if self.gains is None:
                self.enable_exposure_refinement()
            dev = self.gains.device
            self.exposure_master.copy_(ex["master"].to(dev, torch.float64))
            self.exposure_m.copy_(ex["m"].to(dev, torch.float64))
            self.exposure_v.copy_(ex["v"].to(dev, torch.float64))
            self.exposure_counts.copy_(ex["counts"].to(dev, torch.int32))
            self.gains.copy_(ex["gains"].to(dev, torch.float32))

    def view_rays(self, i):
        """every pixel of image i (scanline order) -> rays_o, rays_d [H*W, 3] and its colour [H*W, C] as fp32 on the device"""
        from .rays import get_rays
        r = get_rays(self.poses[i:i + 1], self.intrinsics, self.H, self.W)
        img = self.images[i].reshape(-1, self.C)
        img = img.float() / 255 if img.dtype == torch.uint8 else img.float()
        return r["rays_o"][0], r["rays_d"][0], img
