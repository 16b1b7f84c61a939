"""Distilling a LAENeRF palette edit into the NeRF: the stage that produces LAENeRF's result (nerf/gui.py:357-541 `distill_dataset`,
then `train_gui(distill=True)` for --train_steps_distill steps, gui.py:1420-1430, 1935-1990, nerf/utils.py:892-950).

The reference rewrites the training images view by view on the host side: forward_train over the view's edit pixels, ~20 torch ops
(scatter, blend, mask, clamp), a copy of the image to the host and back, a torchvision Resize for the error map.  Here the extracted
rows of all views are packed once (`DistillSet`), the palette network runs over them in a few large chunks, and the rewrite is ONE
launch (`lae_distill_compose`) into a device copy of the images; the error-map seed is one more (`lae_error_map_seed`).  The result
is a new `ResidentImages`, and the distillation training is the existing graph-replayed `Trainer` on it, unchanged:
  * its learning rate restarts as lr * 0.1 ** min(it / steps, 1): the reference's new LambdaLR over the same optimizer
    (gui.py:1428); FusedAdam keeps Adam's moments and its GradScaler, as torch's optimizer and scaler carry over;
  * the occupancy grid refreshes every 16 steps from the start (the reference's GUI leaves global_step on a multiple of 16);
  * mark_untrained_grid on the first call is a no-op on a grid already marked from the same poses: it sets to -1 only cells no
    camera covers, and update_extra_state never revives a negative cell (nerf/renderer.py:552, 633-634);
  * the error map is 'ema': gui.py:540-541 hands the seeded map to the trainer, whose train_step updates it (nerf/utils.py:609-631).

The rules and the deviations (fp32 instead of fp16 arithmetic, zero weights instead of 0 / 0, no NaN leak at pixels at or below the
threshold) are stated in include/laenerf.h; `compose_distill_numpy` and `error_map_seed_numpy` restate both kernels.
"""
import numpy as np
import torch

from .. import _lib
from ..data import ERROR_MAP_CELLS, ERROR_MAP_SIDE, ResidentImages

__all__ = ["DistillSet", "distill_images", "distill_steps", "distill_nerf", "compose_distill_numpy", "error_map_seed_numpy"]

_DTYPE_CODES = {torch.float16: 1, torch.float32: 2}          # include/laenerf.h lae_distill_compose (ResidentImages' codes)
_NO_BG = 1
_CHUNK = 1 << 18                                             # rows per palette-network call (a multiple of 16)


def distill_steps(n):
    """the steps the reference runs for --train_steps_distill n: its GUI trains in 16-step calls until step > n (gui.py:1941)"""
    return (int(n) // 16 + 1) * 16


class DistillSet:
    """The extracted edit rows of every non-occluded view, packed once: img_idx, pix [R] int32 (target image, pixel), w [R] (the edit
    weight, weights_editgrid[indices]), pred [R,3] (the distill render's colour there), x_term, dirs [R,3] (the palette network's
    inputs), dist [R] (the smooth-transition weight, 0 off indices_interp; None without a grow grid), and per view offsets [V] int64,
    counts [V] int32, view_img [V] int32 (pose_idx).  occluded: the image indices without rows; n_img: images of the training set.
    depth [R] (optional): the distill render's depth at the rows (the views' `depths`), for distill_images(depth_sup=True)."""

    def __init__(self, img_idx, pix, w, pred, x_term, dirs, dist, counts, view_img, occluded, n_img, device=None, depth=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = lambda a, dt: a.detach().to(device, dt).contiguous()
        self.img_idx, self.pix = t(img_idx, torch.int32), t(pix, torch.int32)
        self.w, self.pred = t(w, torch.float32), t(pred, torch.float32).reshape(-1, 3)
        self.x_term, self.dirs = t(x_term, torch.float32).reshape(-1, 3), t(dirs, torch.float32).reshape(-1, 3)
        self.dist = None if dist is None else t(dist, torch.float32)
        self.depth = None if depth is None else t(depth, torch.float32).reshape(-1)
        if self.depth is not None and self.depth.numel() != self.w.numel():
            raise ValueError("DistillSet: depth needs a value per row")
        self.counts_host = np.asarray(counts, np.int64).reshape(-1)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.counts_host)[:-1]]).astype(np.int64)
        self.view_img_host = np.asarray(view_img, np.int64).reshape(-1)
        self.counts = torch.from_numpy(self.counts_host.astype(np.int32)).to(device)
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.view_img = torch.from_numpy(self.view_img_host.astype(np.int32)).to(device)
        self.occluded = sorted(int(i) for i in occluded)
        self.n_img, self.V, self.R = int(n_img), int(self.counts_host.size), int(self.counts_host.sum())

    @property
    def device(self):
        return self.w.device

    def save(self, path):
        """one .npz of the packed arrays, like EditSet.save; dist / depth only when the set has them"""
        cpu = lambda a: a.detach().cpu().numpy()
        extra = {k: cpu(getattr(self, k)) for k in ("dist", "depth") if getattr(self, k) is not None}
        np.savez(path, img_idx=cpu(self.img_idx), pix=cpu(self.pix), w=cpu(self.w), pred=cpu(self.pred), x_term=cpu(self.x_term),
                 dirs=cpu(self.dirs), counts=self.counts_host.astype(np.int64), view_img=self.view_img_host.astype(np.int64),
                 occluded=np.asarray(self.occluded, np.int64), n_img=np.int64(self.n_img), **extra)

    @classmethod
    def load(cls, path, device=None):
        """a set written by save()"""
        with np.load(path) as z:
            t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])) if k in z.files else None
            return cls(t("img_idx"), t("pix"), t("w"), t("pred"), t("x_term"), t("dirs"), t("dist"), z["counts"], z["view_img"],
                       z["occluded"].tolist(), int(z["n_img"]), device=device, depth=t("depth"))

    @classmethod
    def from_views(cls, views, occluded, n_img, device=None):
        """the per-view dicts of extract_views (CPU or device tensors; `pose_idx` is the target image) and its occluded list.
        Rows: the view's `indices` (pixels), `w8s` (= weights_editgrid[indices]), pred_imgs[indices], x_term, dirs; with a grow grid,
        dist_weights scattered to the rows at indices_interp; `depths` (K values, the render's depth at the rows) when every view
        has them."""
        views = list(views)
        occ = {int(i) for i in occluded}
        n_img = int(n_img)
        seen = set()
        for v in views:
            i = int(v["pose_idx"])
            if not 0 <= i < n_img or i in occ or i in seen:
                raise ValueError(f"DistillSet.from_views: pose_idx {i} is outside the {n_img} images, occluded or given twice")
            seen.add(i)
        if any(not 0 <= i < n_img for i in occ):
            raise ValueError("DistillSet.from_views: an occluded index lies outside the images")
        smooth = [("indices_interp" in v) for v in views]
        if any(smooth) and not all(smooth):
            raise ValueError("DistillSet.from_views: indices_interp / dist_weights in some views only")
        cpu = lambda a: a.detach().cpu()
        img, pix, w, pred, xt, dr, dist, counts, dep = [], [], [], [], [], [], [], [], []
        has_depth = bool(views) and all(v.get("depths") is not None for v in views)
        for v in views:
            idx = cpu(v["indices"]).long().reshape(-1)
            K = int(idx.numel())
            if K == 0 or int(v["x_term"].shape[0]) != K or int(v["w8s"].numel()) != K:
                raise ValueError("DistillSet.from_views: a view's indices, w8s and x_term must have the same K >= 1 rows")
            counts.append(K)
            img.append(torch.full((K,), int(v["pose_idx"]), dtype=torch.int32))
            pix.append(idx.int())
            w.append(cpu(v["w8s"]).float().reshape(-1))
            pred.append(cpu(v["pred_imgs"]).float().reshape(-1, 3)[idx])
            xt.append(cpu(v["x_term"]).float().reshape(-1, 3))
            dr.append(cpu(v["dirs"]).float().reshape(-1, 3))
            if has_depth:
                if int(v["depths"].numel()) != K:
                    raise ValueError("DistillSet.from_views: a view's depths must have one value per row of indices")
                dep.append(cpu(v["depths"]).float().reshape(-1))
            if all(smooth) and views:
                d = torch.zeros(K, dtype=torch.float32)
                d[cpu(v["indices_interp"]).long().reshape(-1)] = cpu(v["dist_weights"]).float().reshape(-1)
                dist.append(d)
        if not views:
            z3 = torch.zeros(0, 3)
            return cls(torch.zeros(0), torch.zeros(0), torch.zeros(0), z3, z3, z3, None, [], [], sorted(occ), n_img, device=device)
        return cls(torch.cat(img), torch.cat(pix), torch.cat(w), torch.cat(pred), torch.cat(xt), torch.cat(dr),
                   torch.cat(dist) if all(smooth) else None, counts, [int(v["pose_idx"]) for v in views], sorted(occ), n_img, device=device,
                   depth=torch.cat(dep) if has_depth else None)


@torch.no_grad()
def _network_outputs(style_enc, x_term, dirs):
    """the palette network's raw outputs (LAENeRF._logits) of every row: eval mode, fp16 autocast, in chunks -> w_logits, o_raw
    [round_up(R, 16), 16] fp16"""
    R = x_term.shape[0]
    Rp = max(16, (R + 15) // 16 * 16)
    dev = x_term.device
    w_logits = torch.zeros(Rp, 16, dtype=torch.float16, device=dev)
    o_raw = torch.zeros(Rp, 16, dtype=torch.float16, device=dev)
    use_dirs = style_enc.dir_encoding is not None
    was_training = style_enc.training
    style_enc.eval()
    try:
        for r0 in range(0, R, _CHUNK):
            r1 = min(R, r0 + _CHUNK)
            with torch.autocast("cuda", dtype=torch.float16):
                wl, ol, _ = style_enc._logits(x_term[r0:r1], dirs[r0:r1] if use_dirs else None)
            w_logits[r0:r1].copy_(wl[:r1 - r0, :16])
            o_raw[r0:r1].copy_(ol[:r1 - r0, :16])
    finally:
        style_enc.train(was_training)
    return w_logits, o_raw


def _edit(style_enc, palette, p_weights, p_bias):
    """the edit as fp32 device arrays of the active bases: (palette_mod, palette_og, p_weights, p_bias); defaults as RecolorView.compose
    (the network's active palette, ones, zeros); palette_og = original_color_palette[active] when set, else the current palette
    (gui.py:373-377)"""
    mask = int(style_enc._active_mask)
    n_active = bin(mask).count("1")
    dev = style_enc.color_palette.device
    idx = torch.tensor([j for j in range(16) if (mask >> j) & 1], dtype=torch.long, device=dev)
    current = torch.index_select(style_enc.color_palette.detach().float(), 0, idx).contiguous()
    og = style_enc.original_color_palette
    palette_og = current if og is None else torch.index_select(og.detach().to(dev, torch.float32), 0, idx).contiguous()
    f = lambda a, default: default if a is None else torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous()
    palette = f(palette, current)
    p_weights = f(p_weights, torch.ones(n_active, device=dev)).reshape(-1)
    p_bias = f(p_bias, torch.zeros(n_active, device=dev)).reshape(-1)
    if tuple(palette.shape) != (n_active, 3) or p_weights.numel() != n_active or p_bias.numel() != n_active:
        raise ValueError(f"distill_images: palette [{n_active}, 3], p_weights / p_bias [{n_active}] (the active bases)")
    return palette, palette_og, p_weights, p_bias


def _copy_images(images, dtype):
    if images.dtype == torch.uint8:
        return (images.float() / 255).to(dtype).contiguous()
    return images.to(dtype, copy=True).contiguous()


@torch.no_grad()
def distill_images(data, style_enc, dset, palette=None, p_weights=None, p_bias=None, blend_thresh=0.5, no_bg=False,
                   smooth_transition=False, error_maps=False, dtype=torch.float16, depth_sup=False):
    """distill_dataset (gui.py:357-541) on the device -> a NEW ResidentImages (same poses, intrinsics, bound, mode, bg, colour space)
    whose images are the recoloured targets; `data` is left untouched.
    The images are copied in `dtype` (uint8 as value / 255 in fp32, then dtype), the palette network runs once over the packed rows,
    one lae_distill_compose launch rewrites every view.  palette [n_active, 3], p_weights / p_bias [n_active]: the edit (default:
    the network's active palette, ones, zeros).  smooth_transition: interpolate towards the original palette by the rows' distance
    weights (needs a DistillSet extracted with a grow grid), applied only when the edit is not the identity (gui.py:447).
    error_maps: a map of ones, the non-occluded views' rows seeded from the edit weights (lae_error_map_seed, gui.py:419-425).
    depth_sup: the result carries a depth plane [n_img, H, W] fp32 (`.depths`): the rows' depths scattered to their pixels,
    `d_[indices] = depth`, zero elsewhere and on occluded views (gui.py:406, 508-511) -- once per distillation, torch indexing."""
    if dtype not in _DTYPE_CODES:
        raise ValueError("distill_images: dtype must be torch.float16 or torch.float32 (quantised targets would deviate from the "
                         "reference, which trains on float images)")
    if dset.n_img != data.n_img:
        raise ValueError(f"distill_images: the set was packed for {dset.n_img} images, the data has {data.n_img}")
    if dset.device != data.images.device or dset.device != style_enc.color_palette.device:
        raise ValueError("distill_images: the data, the set and the network must live on the same device")
    if depth_sup and dset.depth is None:
        raise ValueError("distill_images: depth_sup needs views that carry `depths` (extract_views returns them)")
    if smooth_transition and dset.dist is None:
        raise ValueError("distill_images: smooth_transition needs views extracted with a grow grid (indices_interp / dist_weights)")
    images = _copy_images(data.images, dtype)
    palette, palette_og, p_weights, p_bias = _edit(style_enc, palette, p_weights, p_bias)
    identity = torch.allclose(palette, palette_og) and bool((p_weights == 1).all()) and bool((p_bias == 0).all())
    dist = dset.dist if smooth_transition and not identity else None
    if dset.R:
        w_logits, o_raw = _network_outputs(style_enc, dset.x_term, dset.dirs)
        _lib.need_cuda(images, dset.w, w_logits, palette, palette_og, p_weights, p_bias)
        compose_launch(dset, w_logits, o_raw, style_enc, palette, palette_og, p_weights, p_bias, images, blend_thresh, no_bg, dist)
    out = ResidentImages(images, data.poses, data.intrinsics, bound=data.bound, min_near=data.min_near, mode=data.mode, bg=data.bg,
                         color_space=data.color_space, seed=data.seed, device=images.device)
    if error_maps:
        out.enable_error_map()
        seed_launch(dset, out.error_map, data.H, data.W)
    if depth_sup:
        plane = torch.zeros(data.n_img, data.H * data.W, dtype=torch.float32, device=images.device)
        plane[dset.img_idx.long(), dset.pix.long()] = dset.depth
        out.set_depths(plane.view(data.n_img, data.H, data.W))
    return out


def compose_launch(dset, w_logits, o_raw, style_enc, palette, palette_og, p_weights, p_bias, images, blend_thresh=0.5, no_bg=False,
                   dist=None):
    """one lae_distill_compose launch over every row of `dset` into images [n_img, H, W, C] (fp16 / fp32, in place); dist: the rows'
    smooth-transition weights or None.  Every argument a device tensor: the launch can be captured and replayed with new edit values."""
    n_img, H, W, C = (int(s) for s in images.shape)
    if images.dtype not in _DTYPE_CODES or not images.is_contiguous():
        raise ValueError("compose_launch: contiguous float16 / float32 images")
    if w_logits.dtype != torch.float16 or o_raw.dtype != torch.float16 or w_logits.shape[0] < dset.R or o_raw.shape[0] < dset.R:
        raise ValueError("compose_launch: w_logits / o_raw float16 with a row per set row")
    ts = (dset.img_idx, dset.pix, dset.w, dset.pred, dist, w_logits, o_raw, palette, palette_og, p_weights, p_bias, images)
    _lib.need_cuda(*ts)
    _lib.need_contig(*ts)
    _lib.check(_lib.load().lae_distill_compose(
        dset.R, _lib.ptr(dset.img_idx), _lib.ptr(dset.pix), _lib.ptr(dset.w), _lib.ptr(dset.pred), _lib.ptr(dist), _lib.ptr(w_logits),
        w_logits.shape[1], _lib.ptr(o_raw), o_raw.shape[1], style_enc.num_color_bases, int(style_enc._active_mask), _lib.ptr(palette),
        _lib.ptr(palette_og), _lib.ptr(p_weights), _lib.ptr(p_bias), float(blend_thresh), _NO_BG if no_bg else 0, _lib.ptr(images),
        _DTYPE_CODES[images.dtype], n_img, H * W, C, _lib.stream()), "distill_compose")


def seed_launch(dset, error_map, H, W):
    """one lae_error_map_seed call: rows of the non-occluded views of error_map [n_img, 16384] from the edit weights"""
    if error_map.shape != (dset.n_img, ERROR_MAP_CELLS) or error_map.dtype != torch.float32 or not error_map.is_contiguous():
        raise ValueError(f"seed_launch: error_map must be a contiguous float32 [{dset.n_img}, {ERROR_MAP_CELLS}] tensor")
    dense = torch.empty(dset.n_img, H * W, dtype=torch.float32, device=error_map.device)
    _lib.need_cuda(error_map, dset.w, dense)
    _lib.check(_lib.load().lae_error_map_seed(dset.R, _lib.ptr(dset.img_idx), _lib.ptr(dset.pix), _lib.ptr(dset.w), _lib.ptr(dset.view_img),
                                              dset.V, dset.n_img, int(H), int(W), _lib.ptr(dense), _lib.ptr(error_map), _lib.stream()),
               "error_map_seed")


def distill_nerf(renderer, optimizer, data, style_enc, views, occluded, steps=3000, lr=1e-2, error_maps=False, trainer_kw=None,
                 depth_sup=False, depth_weight=1e-3, depth_grad=True, distort_weight=None, **compose_kw):
    """the whole stage: distill_images, then a new Trainer(renderer, optimizer, distilled, iters=steps, lr=lr, error_map='ema' with
    error maps) run for distill_steps(steps) steps -> (distilled ResidentImages, Trainer).  views / occluded: extract_views' result;
    compose_kw: distill_images' edit arguments; trainer_kw: further Trainer arguments (num_rays, seed, ...).
    depth_sup: train with the reference's depth term (its `depth_sup = style_weight > 0`, gui.py:202) on the views' extracted
    depths, weight depth_weight (1e-3 and the mask depth > 0: nerf/utils.py:587-589, 635).  depth_grad=True lets the term hold the
    geometry in place; depth_grad=False is the reference's effective behaviour, where the term only changes the logged loss.
    distort_weight: None, or the weight of the Trainer's distortion regularizer (Trainer(distort_weight=...)): it keeps the
    fine-tuning from growing floaters around the edited region."""
    from ..trainer import Trainer
    dset = DistillSet.from_views(views, occluded, data.n_img, device=data.images.device)
    distilled = distill_images(data, style_enc, dset, error_maps=error_maps, depth_sup=depth_sup, **compose_kw)
    depth_kw = {"depth_weight": depth_weight, "depth_grad": depth_grad} if depth_sup else {}
    if distort_weight is not None:
        depth_kw["distort_weight"] = distort_weight
    tr = Trainer(renderer, optimizer, distilled, iters=steps, lr=lr, error_map="ema" if error_maps else None, **depth_kw,
                 **(trainer_kw or {}))
    tr.train(distill_steps(steps))
    return distilled, tr


# ------------------------------------------------------------------------------------------------------------ numpy restatements
def _softmax_edit_numpy(w_logits, active_mask, p_weights, p_bias):
    """(w_og, w') of rows [R, >= 16] fp16 logits: lae_recolor_compose's softmax, the edit and its normalisation, fp32 per operation"""
    f32 = np.float32
    cols = [j for j in range(16) if (int(active_mask) >> j) & 1]
    lg = np.asarray(w_logits)[:, cols].astype(f32)
    e = np.exp((lg - lg.max(1, keepdims=True)).astype(np.float64)).astype(f32)
    tot = f32(0) + e[:, 0]
    for j in range(1, len(cols)):
        tot = tot + e[:, j]
    w_og = (e / tot[:, None]).astype(f32)
    w = np.maximum(np.asarray(p_bias, f32).reshape(1, -1) + np.asarray(p_weights, f32).reshape(1, -1) * w_og, f32(0))
    ws = f32(0) + w[:, 0]
    for j in range(1, len(cols)):
        ws = ws + w[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(ws[:, None] > 0, w / ws[:, None], f32(0)).astype(f32)
    return w_og, w


def compose_distill_numpy(images, img_idx, pix, w, pred, w_logits, o_raw, active_mask, palette_mod, p_weights, p_bias,
                          blend_thresh=0.5, no_bg=False, dist=None, palette_og=None):
    """lae_distill_compose restated in numpy (include/laenerf.h), every operation one fp32 rounding in the kernel's order, exp / tanh in
    float64 rounded once.  images [n_img, H, W, C] (float16 / float32; a copy is returned, rounded to its dtype); img_idx, pix, w [R];
    pred [R,3]; w_logits / o_raw [>= R, >= 16 / >= 3] fp16; palette_mod / palette_og [n_active, 3]; p_weights / p_bias [n_active];
    dist [R] or None."""
    f32 = np.float32
    out = np.array(images, copy=True)
    n_img, H, W, C = out.shape
    flat = out.reshape(n_img, H * W, C)
    w = np.asarray(w, f32).reshape(-1)
    sel = np.nonzero(w > f32(blend_thresh))[0]
    if sel.size == 0:
        return out
    img, px = np.asarray(img_idx, np.int64)[sel], np.asarray(pix, np.int64)[sel]
    wr = w[sel][:, None]
    o = np.tanh(np.asarray(o_raw)[sel, :3].astype(f32).astype(np.float64)).astype(f32)
    w_og, we = _softmax_edit_numpy(np.asarray(w_logits)[sel], active_mask, p_weights, p_bias)
    pm = np.asarray(palette_mod, f32).reshape(-1, 3)
    acc = np.zeros((sel.size, 3), f32)
    if dist is None:
        for j in range(pm.shape[0]):
            acc = acc + we[:, j:j + 1] * pm[j]
    else:
        po = np.asarray(palette_og, f32).reshape(-1, 3)
        d = np.asarray(dist, f32).reshape(-1)[sel][:, None]
        e = f32(1) - d
        for j in range(pm.shape[0]):
            wi = d * w_og[:, j:j + 1] + e * we[:, j:j + 1]
            acc = acc + wi * (d * po[j] + e * pm[j])
    col = np.clip(acc + o, f32(0), f32(1))
    if no_bg:
        s = wr * col
    else:
        s = (f32(1) - wr) * np.asarray(pred, f32).reshape(-1, 3)[sel] + wr * col
    flat[img, px, :3] = np.clip(s, f32(0), f32(1)).astype(out.dtype)
    return out


def _linear_numpy(n_in, n_out):
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    src = np.maximum(scale * (np.arange(n_out).astype(f32) + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    lam = np.clip(src - i0.astype(f32), f32(0), f32(1))
    return i0, i1, lam


def error_map_seed_numpy(weight_img):
    """lae_error_map_seed restated in numpy: the dense edit-weight image [H, W] (or [V, H, W]) -> clamp(bilinear 128 x 128 resize
    (align_corners=False, no antialiasing) + 0.15, 0, 1) as [16384] (or [V, 16384]) float32, fp32 per operation in the kernel's order"""
    f32 = np.float32
    x = np.asarray(weight_img, f32)
    one = x.ndim == 2
    x = x[None] if one else x
    _, H, W = x.shape
    y0, y1, ly = _linear_numpy(H, ERROR_MAP_SIDE)
    x0, x1, lx = _linear_numpy(W, ERROR_MAP_SIDE)
    wx0, wy0 = (f32(1) - lx)[None, None, :], (f32(1) - ly)[None, :, None]
    lx, ly = lx[None, None, :], ly[None, :, None]
    top = x[:, y0][:, :, x0] * wx0 + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * wx0 + x[:, y1][:, :, x1] * lx
    v = np.clip((top * wy0 + bot * ly) + f32(0.15), f32(0), f32(1)).astype(f32).reshape(-1, ERROR_MAP_CELLS)
    return v[0] if one else v
