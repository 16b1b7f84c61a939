"""Ray registration of the single-reference-view stylization (Ref-NPR) on the HIP kernels of csrc/rayreg.hip.

The reference's second editing entry point (`--ref_npr_config`, editing/single_view_edit_dataset.py, nerf/gui.py:231-235): a user
paints over ONE training view (the template); the edit reaches every other view by registering rays.  Per masked pixel of a view
the termination point is matched to the nearest termination point of the template's cloud (the template render plus two renders
with jittered ray directions, :102-186); closer than `reg_dist` the pixel takes that point's painted colour with a weight that
falls with the distance and with opposing view directions (get_ref_supervision, :317-349), and the distance gives the per-pixel
style guide (:228-232).  The reference searches by brute force in 1000-row chunks -- n * M distances per view; here the cloud is
put into a uniform cell grid once (`RefCloud`) and a view is one truncated nearest-neighbour query.

Semantics (cloud ref_x, ref_rgb, ref_dirs [M,3]; queries x, dirs [n,3]; 0 < reg_dist <= radius, guide_min < radius):
    d_i      = min(radius, min_j |x_i - ref_x_j|), exact over all M points whenever the minimum is below radius
    nn_i     = the index of that point (the lowest among equal distances), -1 when no point lies within radius
    registered: nn_i >= 0 and d_i < reg_dist;  R rows
    target_i = ref_rgb[nn_i]
    weight_i = |(d_i - dmin) / (dmax - dmin) - 1| * f_i, dmin / dmax over the registered rows,
               f_i = (clamp(cos(ref_dirs[nn_i], dirs_i), -1, -0.5) + 1) / 0.5 (torch's cosine_similarity, eps 1e-8)
    guide_i  = max(min_tv_factor, (clamp(d_i, guide_min, radius) - guide_min) / (radius - guide_min))
Non-finite query rows and an empty cloud give d = radius, nn = -1.  The one departure from the reference: with dmax == dmin it
computes 0 / 0 = NaN weights; here the normalised term is 0 and weight_i = f_i.

`ray_registration_numpy` restates this in float64 on the CPU (brute force in chunks); every test compares against it.

The second-stage training terms that consume these arrays -- the weighted registered MSE, the template feature term, the
colour-patch term -- are editing/ref_stage.py (RefEditSet, RefStyleTrainer) with editing/semantic_encoder.py's supervision.  Not
here yet: the guided Gram loss and `dataloader_nerf` with the NeRF distillation that follows it.
"""
import numpy as np
import torch

from ..rays import get_rays
from .edit_dataset import _crop_terms, _render_views

__all__ = ["RefCloud", "register_rays", "ray_registration_numpy", "extract_ref_cloud", "extract_ref_template", "register_views"]


def _backend():
    from ..backend import rayreg_backend
    return rayreg_backend


def _points(t, name):
    t = t.detach().to(torch.float32).reshape(-1, 3).contiguous()
    if not t.is_cuda:
        raise RuntimeError(f"ray registration: {name} must live on the GPU (there is no CPU fallback)")
    return t


class RefCloud:
    """The reference view's cloud in its cell grid, built once: points, rgb, dirs [M,3] (cuda; kept as fp32 copies).
    .query(x) -> (dist [n] fp32, nn [n] int32); .M, .radius; .lo [3], .s, .cells [3]: the grid's origin, cell side and cells per
    axis as the kernels chose them (read back from the device on first use)."""

    def __init__(self, points, rgb, dirs, radius=0.1):
        self.points, self.rgb, self.dirs = _points(points, "points"), _points(rgb, "rgb"), _points(dirs, "dirs")
        self.M = int(self.points.shape[0])
        if self.rgb.shape[0] != self.M or self.dirs.shape[0] != self.M:
            raise ValueError("RefCloud: points, rgb and dirs need the same number of rows")
        self.radius = float(radius)
        if not (self.radius > 0 and np.isfinite(self.radius)):
            raise ValueError("RefCloud: radius must be positive and finite")
        be = _backend()
        self.grid = torch.empty(be.build_bytes(self.M), dtype=torch.uint8, device=self.points.device)
        be.build(self.points, self.M, self.radius, self.grid)
        self._record = None
        self._ws = None

    def _rec(self):
        if self._record is None:
            head = self.grid[:48].cpu().numpy()
            f, u = head.view(np.float32), head.view(np.uint32)
            self._record = {"lo": f[:3].astype(np.float64), "s": float(f[3]), "inv_s": float(f[4]), "cells": u[5:8].astype(np.int64),
                            "ncells": int(u[8])}
        return self._record

    lo = property(lambda self: self._rec()["lo"])
    s = property(lambda self: self._rec()["s"])
    cells = property(lambda self: self._rec()["cells"])

    def query(self, x, mode="binned"):
        """x [n,3] cuda -> (min(radius, distance to the nearest cloud point) [n] fp32, its index or -1 [n] int32).
        mode 'binned' (queries binned by cell, neighbour cells through LDS) or 'gather' (a lane per query): same results"""
        be = _backend()
        if mode not in ("binned", "gather"):
            raise ValueError("RefCloud.query: mode must be 'binned' or 'gather'")
        x = _points(x, "x")
        n = int(x.shape[0])
        d = torch.empty(n, dtype=torch.float32, device=x.device)
        nn = torch.empty(n, dtype=torch.int32, device=x.device)
        if n:
            self._ws = torch.empty(be.query_bytes(n, self.M), dtype=torch.uint8, device=x.device)
            be.query(self.grid, self.M, x, n, self.radius, be.BINNED if mode == "binned" else be.GATHER, d, nn, self._ws)
        return d, nn

    def last_evals(self):
        """distance evaluations of the last 'binned' query (a device counter at the end of its workspace; syncs)"""
        return int(self._ws[-256:-248].view(torch.int64).item())


@torch.no_grad()
def register_rays(cloud, x_term, dirs, reg_dist=2e-2, guide_min=None, min_tv_factor=0.1):
    """get_ref_supervision + the style guide for one view's masked rows (module docstring) ->
    {min_dist [n], nn [n] int32, indices_ray_reg [R] int64 ascending, targets [R,3], target_weights [R], style_guide [n], count}"""
    be = _backend()
    guide_min = float(reg_dist if guide_min is None else guide_min)
    if not (0 < reg_dist <= cloud.radius) or not guide_min < cloud.radius:
        raise ValueError("register_rays: need 0 < reg_dist <= radius and guide_min < radius")
    x_term, dirs = _points(x_term, "x_term"), _points(dirs, "dirs")
    n = int(x_term.shape[0])
    if dirs.shape[0] != n:
        raise ValueError("register_rays: x_term and dirs need the same number of rows")
    dev = x_term.device
    d, nn = cloud.query(x_term)
    nn_reg = torch.empty(n, dtype=torch.int32, device=dev)
    target = torch.empty(n, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(n, dtype=torch.float32, device=dev)
    guide = torch.empty(n, dtype=torch.float32, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    if n:
        be.supervise(d, nn, n, cloud.rgb, cloud.dirs, cloud.M, dirs, reg_dist, cloud.radius, guide_min, min_tv_factor, nn_reg, target, weight,
                     guide, stats)
    idx = (nn_reg >= 0).nonzero(as_tuple=True)[0]                    # the compaction: plumbing, like select_edit_pixels
    return {"min_dist": d, "nn": nn, "indices_ray_reg": idx, "targets": target[idx], "target_weights": weight[idx], "style_guide": guide,
            "count": int(idx.numel())}


def ray_registration_numpy(ref_x, ref_rgb, ref_dirs, x, dirs, reg_dist=2e-2, radius=0.1, guide_min=None, min_tv_factor=0.1, chunk=512):
    """the module docstring's semantics in float64 on the CPU, brute force in chunks of rows.  The scalars are first rounded to fp32,
    the values the kernels receive.  -> the entries of register_rays as numpy arrays, plus 'min_dist_unclamped' (inf where nothing
    is comparable) and 'mask' [n] bool"""
    f32 = lambda v: float(np.float32(v))
    reg_dist, radius, min_tv = f32(reg_dist), f32(radius), f32(min_tv_factor)
    guide_min = reg_dist if guide_min is None else f32(guide_min)
    ref_x, ref_rgb, ref_dirs = (np.asarray(a, np.float64).reshape(-1, 3) for a in (ref_x, ref_rgb, ref_dirs))
    x, dirs = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    n, M = x.shape[0], ref_x.shape[0]
    raw = np.full(n, np.inf)
    nn = np.full(n, -1, np.int64)
    usable = np.isfinite(ref_x).all(1)
    cand = np.nonzero(usable)[0]
    ok = np.isfinite(x).all(1)
    if cand.size:
        pts = ref_x[cand]
        for i0 in range(0, n, chunk):
            rows = np.nonzero(ok[i0:i0 + chunk])[0] + i0
            if rows.size == 0:
                continue
            diff = x[rows, None, :] - pts[None]
            d2 = (diff * diff).sum(-1)
            j = d2.argmin(1)                                          # the first (lowest index) among equal distances
            raw[rows] = np.sqrt(d2[np.arange(rows.size), j])
            nn[rows] = cand[j]
    nn[~(raw < radius)] = -1
    d = np.minimum(raw, radius)
    mask = (nn >= 0) & (d < reg_dist)
    idx = np.nonzero(mask)[0]
    targets = ref_rgb[nn[idx]] if idx.size else np.zeros((0, 3))
    w = np.zeros(idx.size)
    if idx.size:
        dr = d[idx]
        dmin, dmax = dr.min(), dr.max()
        u = (dr - dmin) / (dmax - dmin) if dmax > dmin else np.zeros_like(dr)
        a, b = ref_dirs[nn[idx]], dirs[idx]
        cs = (a * b).sum(1) / (np.maximum(np.linalg.norm(a, axis=1), 1e-8) * np.maximum(np.linalg.norm(b, axis=1), 1e-8))
        w = np.abs(u - 1.0) * ((np.clip(cs, -1.0, -0.5) + 1.0) / 0.5)
    guide = np.maximum(min_tv, (np.clip(d, guide_min, radius) - guide_min) / (radius - guide_min))
    return {"min_dist": d, "min_dist_unclamped": raw, "nn": nn, "mask": mask, "indices_ray_reg": idx, "targets": targets, "target_weights": w,
            "style_guide": guide, "count": int(idx.size)}


def _premultiplied(image, device):
    """[H,W,3|4] -> [H*W,3] fp32; an RGBA image is premultiplied (single_view_edit_dataset.py:47-48, :214-217)"""
    t = torch.as_tensor(image).to(device=device, dtype=torch.float32)
    if t.shape[-1] == 4:
        t = t[..., :3] * t[..., -1][..., None]
    return t.reshape(-1, 3)


@torch.no_grad()
def extract_ref_cloud(renderer, pose, intrinsics, H, W, ref_image, alpha, n_jitter=2, radius=0.1):
    """single_view_edit_dataset.py:102-186: the template pose rendered once as register_views renders it and `n_jitter` more times
    with jittered ray directions (get_rays(perturb_ray_dirs=True)), every time against the density bitfield as the grid (the
    reference's distill_step(..., grow_grid=True)); the rows with alpha > 0 (alpha [H,W]: the template image's alpha) and their
    painted colours from ref_image [H,W,3|4] (values in 0..1; RGBA is premultiplied) -> RefCloud of (1 + n_jitter) * K points"""
    dev = renderer.density_bitfield.device
    pose = torch.as_tensor(pose).to(dev).reshape(1, 4, 4)
    mask = (torch.as_tensor(alpha).to(dev).reshape(-1) > 0).nonzero(as_tuple=True)[0]
    if mask.numel() != 0 and int(mask.max()) >= H * W:
        raise ValueError("extract_ref_cloud: alpha must be [H, W]")
    rgb = _premultiplied(ref_image, dev)
    if rgb.shape[0] != H * W:
        raise ValueError("extract_ref_cloud: ref_image must be [H, W, 3|4]")
    rgb = rgb[mask]
    (out, _, rays_d), = _render_views(renderer, pose, intrinsics, H, W, renderer.density_bitfield, None)
    xs, cs, ds = [out["x_term"][mask]], [rgb], [rays_d[mask]]
    for _ in range(int(n_jitter)):
        rays = get_rays(pose, intrinsics, H, W, -1, perturb_ray_dirs=True, aabb=renderer.aabb_infer, min_near=renderer.min_near)
        o, d = rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3)
        with torch.autocast("cuda", dtype=torch.float16):
            r = renderer.render_distill(o, d, renderer.density_bitfield, perturb=True, nears=rays["nears"].reshape(-1))
        xs.append(r["x_term"][mask]); cs.append(rgb); ds.append(d[mask])
    return RefCloud(torch.cat(xs), torch.cat(cs), torch.cat(ds), radius=radius)


@torch.no_grad()
def extract_ref_template(renderer, pose, intrinsics, H, W, ref_image, image):
    """single_view_edit_dataset.py:120-153: the template view rendered as extract_ref_cloud renders it; its mask is alpha > 0 of
    `image` [H,W,3|4] (the template's training image; every pixel of an RGB one), its crop box the bounding box of the masked
    pixels of non-zero opacity (exclusive upper bounds at the maxima, the reference's slicing).
    -> {painted [H,W,3]: ref_image's colours on the mask (RGBA premultiplied), zero elsewhere; original [H,W,3]: image's first
        three channels; box: (x_min, x_max, y_min, y_max)} -- build_ref_supervision's `template`"""
    dev = renderer.density_bitfield.device
    pose = torch.as_tensor(pose).to(dev).reshape(1, 4, 4)
    img = torch.as_tensor(image).to(dev).float()
    if img.shape[-1] == 4:
        mask = (img[..., -1].reshape(-1) > 0).nonzero(as_tuple=True)[0]
    else:
        mask = torch.arange(H * W, device=dev)
    rgb = _premultiplied(ref_image, dev)
    if rgb.shape[0] != H * W or img.shape[0] * img.shape[1] != H * W:
        raise ValueError("extract_ref_template: ref_image and image must be [H, W, 3|4]")
    (out, _, _), = _render_views(renderer, pose, intrinsics, H, W, renderer.density_bitfield, None)
    m = torch.zeros(H * W, dtype=torch.float32, device=dev)
    m[mask] = out["weights"][mask].float()
    x, y = m.view(H, W).nonzero(as_tuple=True)
    if x.numel() == 0:
        raise ValueError("extract_ref_template: the template view has no masked pixel of non-zero opacity")
    painted = torch.zeros(H * W, 3, dtype=torch.float32, device=dev)
    painted[mask] = rgb[mask]
    return {"painted": painted.view(H, W, 3), "original": img[..., :3].reshape(H, W, 3).contiguous(),
            "box": (int(x.min()), int(x.max()), int(y.min()), int(y.max()))}


@torch.no_grad()
def register_views(renderer, poses, intrinsics, H, W, images, cloud, reg_dist=2e-2, min_tv_factor=0.1, num_steps=512, batch_views=4):
    """single_view_edit_dataset.py:188-315: every training view rendered against the density bitfield (`batch_views` views per ray
    launch and render, like extract_views), its masked rows (alpha > 0; every pixel of an RGB image) registered to `cloud`.
    -> (views, skipped pose indices).  A view dict carries what EditSet.from_views(views, image_hw=(H, W)) needs with `targets` =
    the premultiplied ground truth (the reference's targets_gt: the dataloader_gt stage), and the registration: ref_targets [R,3],
    target_weights [R], indices_ray_reg [R] (rows of the view), min_dist [K], style_guide (the guide scattered into the crop, zeros
    off the mask), image (the caller's images[i], not copied: build_ref_supervision reads its first three channels).  A view without a masked pixel of non-zero opacity is skipped."""
    dev = renderer.density_bitfield.device
    poses = torch.as_tensor(poses).to(dev).reshape(-1, 4, 4)
    step = max(1, int(batch_views))
    views, skipped = [], []
    for i0 in range(0, poses.shape[0], step):
        rendered = _render_views(renderer, poses[i0:i0 + step], intrinsics, H, W, renderer.density_bitfield, None)
        for j, (out, _, rays_d) in enumerate(rendered):
            img = torch.as_tensor(images[i0 + j]).to(dev)
            if img.shape[-1] == 4:
                mask = (img[..., -1].reshape(-1) > 0).nonzero(as_tuple=True)[0]
            else:
                mask = torch.arange(H * W, device=dev)
            w_sel = out["weights"][mask]
            if mask.numel() == 0 or not bool((w_sel != 0).any()):
                skipped.append(i0 + j)
                continue
            x_term, dirs, d_mask = out["x_term"][mask], rays_d[mask], out["depth"][mask]
            target = _premultiplied(img, dev)[mask]
            reg = register_rays(cloud, x_term, dirs, reg_dist=reg_dist, min_tv_factor=min_tv_factor)
            v = {"w8s": w_sel, "targets": target, "x_term": x_term, "dirs": dirs, "depths": d_mask, "indices": mask,
                 "depth_factor": (d_mask.max() - d_mask.min()) / num_steps, "weights_densitygrid": out["weights"], "pred_imgs": out["image"],
                 "ref_targets": reg["targets"], "target_weights": reg["target_weights"], "indices_ray_reg": reg["indices_ray_reg"],
                 "min_dist": reg["min_dist"], "pose_idx": i0 + j, "image": images[i0 + j]}
            v.update(_crop_terms(H, W, mask, w_sel, target, d_mask))
            x0, x1, y0, y1 = (int(t) for t in v["cut_min_max_xy"])
            g = torch.zeros(H * W, dtype=torch.float32, device=dev)
            g[mask] = reg["style_guide"]
            v["style_guide"] = g.view(H, W)[x0:x1, y0:y1]
            views.append(v)
    return views, skipped
