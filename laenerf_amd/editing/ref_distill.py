"""The third stage of the single-reference-view stylization (Ref-NPR): the stylization distilled into the NeRF -- the reference's
`dataloader_nerf` / `collate_nerf_train` (editing/single_view_edit_dataset.py:414-429, 447-519), `train_step_npr`
(nerf/utils.py:487-533) and `train_gui_npr` (nerf/utils.py:830-889, the GUI's "Distill" button, nerf/gui.py:195-199, 1570-1581).

The reference rebuilds its data view by view on the host side: per view five dense planes scattered with torch indexing, one call of
the palette network, five device-to-host copies and five PNG files.  Here the registered rows and the extracted rows of ALL views
are packed once on the device (`pack_ref_rows`, in DistillSet's layout), the palette network runs over the extracted rows in a few large chunks,
and the four planes are written by two launches (`lae_ref_distill_init`, a dense pass; `lae_ref_distill_scatter`, one thread per
packed row).  The result is a new `ResidentImages` that carries them:

  images        [n, H, W, 4]  rgb 0 and the training image's alpha a everywhere; rgb = ref_targets[r] at each registered pixel
  pixel_weights [n, H, W]     1 - a everywhere; max(target_weights[r], 0) + (1 - a) at each registered pixel
  second_target [n, H, W, 4]  0 everywhere; at each of a view's K extracted pixels alpha = a and rgb = style_enc(x_term, d=dirs)
  depths        [n, H, W]     0 everywhere; the view's `depths` at the K pixels (fp32, the convention of distill_images(depth_sup=True))

a is 1 for 3-channel data (the reference reads the blue channel there, a bug that is not reproduced).  Views that register_views
skipped, and images no view points at, keep the background rule.  The training is the existing graph-replayed Trainer with
`pixel_weights=True, second_weight=style_weight_d, depth_weight=depth_weight_d`: train_step_npr's loss
    mean((w (pred - gt))^2) + style_weight_d * mean(((1 - w / 2) (gt_style - pred))^2) + depth_weight_d * depth term
inside the fused compositing kernel (`lae_composite_rays_train_step` with its weight term), 16 steps per captured graph.

Departures from the reference:
  * the view of a batch is drawn i.i.d. by the resident sampler, not by a shuffled loader over the views;
  * rays come from the poses (the sampler's pinhole rays), not from the per-pixel rays stored at the extraction;
  * the depth term is always on, not behind the host read `outputs['depth'].sum() > 0`;
  * the depth term's weight is `z > 0`, not a separate plane of ones at the extracted pixels: equal unless an extracted depth is
    exactly 0.
"""
import numpy as np
import torch

from .. import _lib
from ..data import _DTYPES, ResidentImages
from .distill import _CHUNK, _DTYPE_CODES, distill_steps

__all__ = ["pack_ref_rows", "build_ref_distill_data", "distill_ref_npr", "ref_distill_numpy"]


def pack_ref_rows(views, n_img, HW, device=None):
    """the rows of every view, packed once on `device` (default: the host) like DistillSet's:
      registered rows  reg_img, reg_pix int32 [R] (pose_idx, indices[indices_ray_reg]: `indices` read as EditSet.from_views reads it),
                       reg_rgb float32 [R, 3] (ref_targets), reg_w float32 [R] (target_weights);
      extracted rows   ext_img, ext_pix int32 [sum K], and -- from the views that carry them -- x_term, dirs float32 [sum K, 3] and
                       ext_depth float32 [sum K] (`depths`).
    The views' tensors are moved to `device` as they are and packed there (DistillSet.from_views packs on the host, and also packs the
    edit weights and the distill render, which this stage does not read: at 100 views of 800 x 800 that is most of the time).
    Checks what the scatter needs -- one view per image, rows inside the planes, distinct pixels within a view (two rows on one pixel
    would leave an unspecified one of their values: asserted) -- with one host read for all views."""
    device = torch.device("cpu" if device is None else device)
    dev = lambda a, dt: (a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device, dt).reshape(-1)
    n_img, HW = int(n_img), int(HW)
    out = {k: [] for k in ("reg_img", "reg_pix", "reg_rgb", "reg_w", "ext_img", "ext_pix", "x_term", "dirs", "ext_depth")}
    bad, seen = [], set()
    for k, v in enumerate(views):
        i = int(v["pose_idx"])
        if not 0 <= i < n_img or i in seen:
            raise ValueError(f"pack_ref_rows: view {k}: pose_idx {i} is outside the {n_img} images or given twice")
        seen.add(i)
        idx, reg = dev(v["indices"], torch.int64), dev(v["indices_ray_reg"], torch.int64)
        K, R = idx.numel(), reg.numel()
        t, tw = dev(v["ref_targets"], torch.float32).reshape(-1, 3), dev(v["target_weights"], torch.float32)
        if t.shape[0] != R or tw.numel() != R:
            raise ValueError(f"pack_ref_rows: view {k}: ref_targets / target_weights need one entry per row of indices_ray_reg")
        # the range checks are gathered and read once; the gather below stays inside the rows whatever reg holds
        bad.append(torch.stack([((reg < 0) | (reg >= K)).any() if R else torch.zeros((), dtype=torch.bool, device=device),
                                ((idx < 0) | (idx >= HW)).any() if K else torch.zeros((), dtype=torch.bool, device=device)]))
        p = idx[reg.clamp(0, max(K - 1, 0))] if K else reg
        out["reg_img"].append(torch.full((R,), i, dtype=torch.int32, device=device)); out["reg_pix"].append(p.int())
        out["reg_rgb"].append(t); out["reg_w"].append(tw)
        out["ext_img"].append(torch.full((K,), i, dtype=torch.int32, device=device)); out["ext_pix"].append(idx.int())
        for name, key, width in (("x_term", "x_term", 3), ("dirs", "dirs", 3), ("ext_depth", "depths", 1)):
            if v.get(key) is not None:
                a = dev(v[key], torch.float32)
                if a.numel() != K * width:
                    raise ValueError(f"pack_ref_rows: view {k}: {key} needs one entry per row of indices")
                out[name].append(a.reshape(-1, 3) if width == 3 else a)
    empty = {"reg_rgb": (0, 3), "x_term": (0, 3), "dirs": (0, 3)}
    res = {}
    for name, parts in out.items():
        if name in ("x_term", "dirs", "ext_depth") and len(parts) != len(seen):
            continue                                                   # some view lacks it: not packed
        dt = torch.int32 if name.endswith(("_img", "_pix")) else torch.float32
        res[name] = torch.cat(parts).contiguous() if parts else torch.zeros(empty.get(name, (0,)), dtype=dt, device=device)
    if bad:
        flags = torch.stack(bad).any(0).tolist()                       # the one host read of the range checks
        if flags[0]:
            raise ValueError("pack_ref_rows: indices_ray_reg points outside a view's rows")
        if flags[1]:
            raise ValueError("pack_ref_rows: indices lie outside the image")
        key = res["ext_img"].long() * HW + res["ext_pix"].long()
        assert torch.unique(key).numel() == key.numel(), "pack_ref_rows: two rows of a view name the same pixel"
        key = res["reg_img"].long() * HW + res["reg_pix"].long()
        assert torch.unique(key).numel() == key.numel(), "pack_ref_rows: two registered rows of a view name the same pixel"
    return res


@torch.no_grad()
def _network_colours(style_enc, x_term, dirs):
    """style_enc(x_term, d=dirs) of every row -> [R, 3] float32 in [0, 1]: eval mode, fp16 autocast, in chunks, as
    distill._network_outputs runs the network"""
    R = x_term.shape[0]
    out = torch.empty(R, 3, dtype=torch.float32, device=x_term.device)
    use_dirs = style_enc.dir_encoding is not None
    was_training = style_enc.training
    style_enc.eval()
    try:
        for r0 in range(0, R, _CHUNK):
            r1 = min(R, r0 + _CHUNK)
            with torch.autocast("cuda", dtype=torch.float16):
                out[r0:r1].copy_(style_enc(x_term[r0:r1], d=dirs[r0:r1] if use_dirs else None))
    finally:
        style_enc.train(was_training)
    return out


@torch.no_grad()
def build_ref_distill_data(data, views, style_enc, dtype=torch.float16):
    """dataloader_nerf (single_view_edit_dataset.py:447-519) on the device over all views at once -> a NEW ResidentImages (same poses,
    intrinsics, bound, mode, bg, colour space and seed as `data`, which is left untouched) with the planes of the module docstring;
    images, pixel_weights and second_target in `dtype` (float16 / float32: values computed in fp32, rounded once), depths in fp32.
    views: register_views' result (pose_idx, indices, indices_ray_reg, ref_targets, target_weights, x_term, dirs, depths, ...)."""
    if dtype not in _DTYPE_CODES:
        raise ValueError("build_ref_distill_data: dtype must be torch.float16 or torch.float32")
    views = list(views)
    dev = data.images.device
    if dev != style_enc.color_palette.device:
        raise ValueError("build_ref_distill_data: the data and the network must live on the same device")
    for key in ("depths", "x_term", "dirs"):
        if any(v.get(key) is None for v in views):
            raise ValueError(f"build_ref_distill_data: every view needs `{key}` (register_views returns them)")
    n, H, W, C = data.n_img, data.H, data.W, data.C
    HW = H * W
    rows = pack_ref_rows(views, n, HW, device=dev)
    R_reg, R_ext = int(rows["reg_img"].numel()), int(rows["ext_img"].numel())
    images = torch.empty(n, H, W, 4, dtype=dtype, device=dev)
    weights = torch.empty(n, H, W, dtype=dtype, device=dev)
    second = torch.empty(n, H, W, 4, dtype=dtype, device=dev)
    depths = torch.empty(n, H, W, dtype=torch.float32, device=dev)
    _lib.need_cuda(data.images, images)
    lib, p = _lib.load(), _lib.ptr
    code, src_code = _DTYPE_CODES[dtype], _DTYPES[data.images.dtype]
    _lib.check(lib.lae_ref_distill_init(p(data.images), src_code, n, HW, C, code, p(images), p(weights), p(second), p(depths), _lib.stream()),
               "ref_distill_init")
    if R_reg or R_ext:
        colours = _network_colours(style_enc, rows["x_term"], rows["dirs"]).contiguous() if R_ext else None
        _lib.check(lib.lae_ref_distill_scatter(R_reg, p(rows["reg_img"]), p(rows["reg_pix"]), p(rows["reg_rgb"]), p(rows["reg_w"]), R_ext,
                                               p(rows["ext_img"]), p(rows["ext_pix"]), p(colours), p(rows["ext_depth"]), p(data.images),
                                               src_code, n, HW, C, code, p(images), p(weights), p(second), p(depths), _lib.stream()),
                   "ref_distill_scatter")
    return ResidentImages(images, data.poses, data.intrinsics, bound=data.bound, min_near=data.min_near, mode=data.mode, bg=data.bg,
                          color_space=data.color_space, seed=data.seed, device=dev, depths=depths, pixel_weights=weights, second_target=second)


def distill_ref_npr(renderer, optimizer, data, style_enc, views, steps=3000, lr=1e-2, style_weight_d=0.5, depth_weight_d=1e-3,
                    depth_grad=True, trainer_kw=None):
    """train_gui_npr: build_ref_distill_data, then a new Trainer(renderer, optimizer, distilled, iters=steps, lr=lr, pixel_weights=True,
    second_weight=style_weight_d, depth_weight=depth_weight_d) run for distill_steps(steps) steps -> (distilled ResidentImages,
    Trainer).  Defaults: the reference's style_weight_d / depth_weight_d (main_nerf.py:142-143).  depth_grad=True lets the depth term
    hold the geometry in place; False is the reference's effective behaviour (its compositing backward drops the depth gradient).
    trainer_kw: further Trainer arguments (num_rays, seed, distort_weight, ...)."""
    from ..trainer import Trainer
    distilled = build_ref_distill_data(data, views, style_enc)
    tr = Trainer(renderer, optimizer, distilled, iters=steps, lr=lr, pixel_weights=True, second_weight=style_weight_d,
                 depth_weight=depth_weight_d, depth_grad=depth_grad, **(trainer_kw or {}))
    tr.train(distill_steps(steps))
    return distilled, tr


# ------------------------------------------------------------------------------------------------------------ numpy restatement
def ref_distill_numpy(src_images, reg_img, reg_pix, reg_rgb, reg_w, ext_img, ext_pix, ext_rgb, ext_depth, dtype=np.float16):
    """lae_ref_distill_init and lae_ref_distill_scatter restated in numpy (include/laenerf.h), every operation one fp32 rounding,
    the stores rounded to `dtype` (float16 / float32).  src_images [n, H, W, 3 or 4] (uint8, float16 or float32): read for their
    alpha; rows outside the planes are skipped.  -> images [n, H, W, 4], weights [n, H, W], second [n, H, W, 4] (dtype), depths
    [n, H, W] float32"""
    f32 = np.float32
    src = np.asarray(src_images)
    n, H, W, C = src.shape
    HW = H * W
    if C == 4:
        a = src[..., 3].astype(f32) / f32(255) if src.dtype == np.uint8 else src[..., 3].astype(f32)
    else:
        a = np.ones((n, H, W), f32)
    a = a.reshape(n, HW)
    images, second = np.zeros((n, HW, 4), f32), np.zeros((n, HW, 4), f32)
    images[..., 3] = a
    weights = f32(1) - a
    depths = np.zeros((n, HW), f32)

    def inside(img, pix):
        img, pix = np.asarray(img, np.int64).reshape(-1), np.asarray(pix, np.int64).reshape(-1)
        ok = (img >= 0) & (img < n) & (pix >= 0) & (pix < HW)
        return img[ok], pix[ok], ok

    i, q, ok = inside(reg_img, reg_pix)
    images[i, q, :3] = np.asarray(reg_rgb, f32).reshape(-1, 3)[ok]
    weights[i, q] = np.maximum(np.asarray(reg_w, f32).reshape(-1)[ok], f32(0)) + (f32(1) - a[i, q])
    i, q, ok = inside(ext_img, ext_pix)
    second[i, q, :3] = np.asarray(ext_rgb, f32).reshape(-1, 3)[ok]
    second[i, q, 3] = a[i, q]
    depths[i, q] = np.asarray(ext_depth, f32).reshape(-1)[ok]
    return (images.astype(dtype).reshape(n, H, W, 4), weights.astype(dtype).reshape(n, H, W), second.astype(dtype).reshape(n, H, W, 4),
            depths.reshape(n, H, W))
