"""Training of the LAENeRF palette network on extracted views: the reference's `train_LAENeRF_step` loop (nerf/utils.py:953-1055,
driven 16 steps per call by nerf/gui.py:1997-2026) on a device-resident edit set, one captured HIP graph per buffer capacity.

Per step: the step's view (`lae_sample_edit_view`: the schedule entry at the device step counter, the depth jitter of
`EditDataset.collate`, rows padded to the capacity with copies of the last jittered row, the live row count K in device memory)
-> `LAENeRF.forward_train_loss(..., m_dev=K)` (MSE + weights_loss + offset_loss + palet_loss as one node; rows >= K excluded)
-> FusedAdam's backward and step (its GradScaler) -> the unscaled loss and the MSE recorded on the device at the step's row.

What makes one graph serve many steps although every view has its own K:
  * the host knows each step's view (the schedule is drawn up front), so a step runs at capacity `capacity_for(K)`: 'bucket'
    rounds K up to 8 steps per octave (at most 12.5 % pad rows, few graphs), 'exact' to the next multiple of 16 (a graph per
    distinct K: the no-padding floor);
  * the sampler writes K into device memory and the loss kernels read it there, so a graph captured at a capacity serves every
    view that fits it.  Pad rows are copies of a real row: they touch only hash-table lines the view touches, so FusedAdam's
    touched-line update and with it every parameter are those of the exact-size step.
The first step at an unseen capacity runs eagerly (library workspaces may not grow inside a capture), the next one is captured;
all graphs share one memory pool.  The palette distillation (style_encoder.py:160-173) runs once, eagerly, before step
`distill_step(iters, distill_palette_steps)`; it changes the active-base mask, a host argument of the palette kernels, so every
graph is dropped and recaptured.

Stylization (nerf/utils.py:997-1033): on steps where (style_weight > 0 or tv_weight > 0) and the 16-step group's first step is past
warmup_iterations, the step also runs the image block -- editing/style_image.py's kernels gather the crop and write the VGG input and
the TV / smooth-transition / depth-discontinuity sums, the VGG layers (torch / MIOpen) and the Gram MSE give the style term, and the
image terms' dL/dpred joins the point loss's in its one palette-backward launch.  Such steps have graphs of their own (key (cap,
True)); if the capture is refused they run eagerly (capture_error).

Deviations from the reference: the jitter comes from Philox (include/laenerf.h lae_sample_edit_view), not torch's
device generator; with fewer than 16 views a 16-step group continues with further fresh permutations where the reference's
exhausted DataLoader raises StopIteration.  Refused with NotImplementedError: intensity_weight, and the image terms when the caller
supplies no image arrays / no style network.
"""
import math
import time

import numpy as np
import torch

from .. import _lib
from ..backend import style_backend as _backend
from ..trainer import bucket_capacity

__all__ = ["EditSet", "StyleTrainer", "jitter_numpy", "draw_schedule", "view_schedule", "capacity_for", "distill_step", "image_terms_on",
           "pack_image_arrays"]

GROUP = 16                          # steps per train_LAENeRF_step call (nerf/gui.py:1997-2026)
_JITTER_WORD3 = 2                   # Philox counter word 3 of the jitter draw (include/laenerf.h)


# ------------------------------------------------------------------------------------------------------------ host-side rules
def jitter_numpy(x_term, dirs, depth_factor, seed, step, rows=None):
    """numpy restatement of lae_sample_edit_view's jitter: x = x_term + ((u - 0.5) * depth_factor) * dirs in float32, u = (w >> 8)
    * 2^-24, w = Philox4x32-10 word 0 at counter (step, row, 0, 2).  x_term, dirs [K,3] are the view's rows; rows: their row numbers
    (default 0..K-1) -> [K,3] float32"""
    from ..data import _u32
    x_term = np.asarray(x_term, np.float32)
    dirs = np.asarray(dirs, np.float32)
    rows = np.arange(x_term.shape[0], dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    w = _u32(int(seed) & 0xFFFFFFFFFFFFFFFF, step, rows, 0, _JITTER_WORD3)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    t = (u - np.float32(0.5)) * np.float32(depth_factor)
    return x_term + t[:, None] * dirs


def draw_schedule(gen, V, n_steps, preserve_color=False):
    """the view of each of ceil(n_steps / 16) * 16 steps: every 16-step group is the first 16 entries of a fresh torch.randperm(V,
    generator=gen) (the reference re-creates its shuffled DataLoader iterator at every 16-step call); with V < 16 the group continues
    with further fresh permutations (the reference raises StopIteration there) -> int32 [n].
    preserve_color=True: the first entry of each group's permutation is the view the style image is colour-matched to
    (nerf/utils.py:974-976 takes it from the same fresh iterator) and the group's 16 steps take the next ones -> (int32 [n], int32
    [groups] colour views)"""
    if V < 1:
        raise ValueError("draw_schedule: no views")
    out, colour = [], []
    for _ in range(-(-int(n_steps) // GROUP)):
        group = []
        need = GROUP + (1 if preserve_color else 0)
        while len(group) < need:
            group.extend(torch.randperm(V, generator=gen)[:need - len(group)].tolist())
        if preserve_color:
            colour.append(group[0])
            group = group[1:]
        out.extend(group)
    if preserve_color:
        return np.asarray(out, dtype=np.int32), np.asarray(colour, dtype=np.int32)
    return np.asarray(out, dtype=np.int32)


def image_terms_on(step, warmup_iterations=1000):
    """whether global step `step` (0-based) carries the image terms: the reference tests `global_step > warmup_iterations` once
    per 16-step call with global_step = the style step counter at the call's start (nerf/gui.py:327-336), so the gate opens per
    group: with the default 1000, steps 0..1007 are off and 1008 on"""
    return GROUP * (int(step) // GROUP) > int(warmup_iterations)


def view_schedule(V, n_steps, seed=0):
    """draw_schedule from torch.Generator().manual_seed(seed): StyleTrainer's schedule for `seed`"""
    return draw_schedule(torch.Generator().manual_seed(int(seed)), V, n_steps)


def capacity_for(K, capacity="bucket"):
    """buffer rows of a step on a view of K points: 'exact' = K rounded up to 16 (the MLP tile); 'bucket' = K rounded up to 8 steps per
    octave (trainer.bucket_capacity with 16-row alignment: at most 12.5 % pad rows above 128 points)"""
    K = int(K)
    if K < 1:
        raise ValueError("capacity_for: a view has at least one point")
    if capacity == "exact":
        return -(-K // 16) * 16
    if capacity == "bucket":
        return bucket_capacity(K, 16)
    raise ValueError("capacity must be 'bucket' or 'exact'")


def distill_step(iters, distill_palette_steps):
    """the global step before which the palette distillation runs: the first multiple of 16 (a call boundary of the reference's
    16-step loop) greater than iters - distill_palette_steps, if it is < iters (nerf/gui.py:1997-2004); None: never (also for
    distill_palette_steps < 0, the reference's 'done' marker)"""
    if distill_palette_steps is None or distill_palette_steps < 0:
        return None
    s = max(0, ((int(iters) - int(distill_palette_steps)) // GROUP + 1) * GROUP)
    return s if s < int(iters) else None


def pack_image_arrays(views, image_hw):
    """the image arrays of the stylization terms for EditSet (host numpy): per view v with crop box (x_min, x_max, y_min, y_max)
    (cut_min_max_xy; exclusive upper bounds, h = x_max - x_min, w = y_max - y_min) its h*w crop pixels at img_off[v]:
      pix2row  int32  the view's row whose flat pixel indices[r] = x * W + y is that crop pixel, -1 where none;
      row2pix  int32  per row (in the packed row order) its crop pixel, -1 for rows outside the crop (last edit row / column);
      cut_gt [.,3], tv_h (cut_tv_h [h-1,w] padded to h rows with 0), tv_v (cut_tv_v [h,w-1] padded to w columns), smooth
      (cut_smooth_trans, only when every view has it) fp32;
      vmax [V,2] fp32: max cut_tv_h, max cut_tv_v (0 for an empty one) -- the depth-discontinuity term's divisors."""
    H, W = (int(v) for v in image_hw)
    has_sm = ["cut_smooth_trans" in v and v["cut_smooth_trans"] is not None for v in views]
    if any(has_sm) and not all(has_sm):
        raise ValueError("pack_image_arrays: cut_smooth_trans in some views only")
    arr = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    box, off, p2r, r2p, gt, th, tv, sm, vmax = [], [], [], [], [], [], [], [], []
    o = 0
    for k, v in enumerate(views):
        b = arr(v["cut_min_max_xy"]).astype(np.int64).reshape(4)
        x0, x1, y0, y1 = (int(t) for t in b)
        h, w = x1 - x0, y1 - y0
        if h < 1 or w < 1 or x0 < 0 or y0 < 0 or x1 > H or y1 > W:
            raise ValueError(f"pack_image_arrays: view {k}: crop {b.tolist()} is empty or leaves the {H}x{W} image")
        idx = arr(v["indices"]).astype(np.int64).reshape(-1)
        K = int(v["x_term"].shape[0])
        if idx.size != K:
            raise ValueError(f"pack_image_arrays: view {k}: {idx.size} indices for {K} rows")
        xi, yi = idx // W, idx % W
        inside = (xi >= x0) & (xi < x1) & (yi >= y0) & (yi < y1)
        cp = np.where(inside, (xi - x0) * w + (yi - y0), -1).astype(np.int32)
        pm = np.full(h * w, -1, np.int32)
        pm[cp[inside]] = np.nonzero(inside)[0].astype(np.int32)
        g = arr(v["cut_gt"]).astype(np.float32).reshape(h, w, 3)
        a_h = arr(v["cut_tv_h"]).astype(np.float32).reshape(h - 1, w)
        a_v = arr(v["cut_tv_v"]).astype(np.float32).reshape(h, w - 1)
        ph, pv = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        ph[:h - 1], pv[:, :w - 1] = a_h, a_v
        box.append([x0, x1, y0, y1]); off.append(o); p2r.append(pm); r2p.append(cp); gt.append(g.reshape(-1, 3))
        th.append(ph.reshape(-1)); tv.append(pv.reshape(-1))
        vmax.append([a_h.max() if a_h.size else 0.0, a_v.max() if a_v.size else 0.0])
        if has_sm[0]:
            sm.append(arr(v["cut_smooth_trans"]).astype(np.float32).reshape(-1))
        o += h * w
    out = {"box": np.asarray(box, np.int32), "img_off": np.asarray(off, np.int64), "pix2row": np.concatenate(p2r), "row2pix": np.concatenate(r2p),
           "cut_gt": np.concatenate(gt), "tv_h": np.concatenate(th), "tv_v": np.concatenate(tv), "vmax": np.asarray(vmax, np.float32),
           "image_hw": np.array([H, W], np.int64)}
    if has_sm[0]:
        out["smooth"] = np.concatenate(sm)
    return out


# ------------------------------------------------------------------------------------------------------------------ the set
class EditSet:
    """The training views of the palette network, packed once: x_term, dirs, targets [sum K, 3] fp32, offsets [V] int64, counts [V]
    int32, depth_factor [V] fp32, a device step counter and a device view schedule (default: step mod V; StyleTrainer installs its
    own).  device='cpu' keeps the arrays on the host (loaders, tests); sample() needs the GPU."""

    def __init__(self, x_term, dirs, targets, counts, depth_factor, seed=0, device=None, image=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device, dt).contiguous()
        counts_h = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, dtype=np.int64).reshape(-1)
        if counts_h.size == 0 or (counts_h < 1).any() or counts_h.max() >= 2 ** 31:
            raise ValueError("EditSet: every view needs 1 .. 2^31 - 1 points")
        n = int(counts_h.sum())
        self.x_term, self.dirs, self.targets = t(x_term, torch.float32), t(dirs, torch.float32), t(targets, torch.float32)
        for name, a in (("x_term", self.x_term), ("dirs", self.dirs), ("targets", self.targets)):
            if tuple(a.shape) != (n, 3):
                raise ValueError(f"EditSet: {name} must be [sum(counts) = {n}, 3]")
        self.depth_factor = t(np.asarray(depth_factor.cpu() if torch.is_tensor(depth_factor) else depth_factor, np.float32).reshape(-1),
                              torch.float32)
        if self.depth_factor.numel() != counts_h.size:
            raise ValueError("EditSet: one depth_factor per view")
        self.counts_host = counts_h
        self.offsets_host = np.concatenate([[0], np.cumsum(counts_h)[:-1]]).astype(np.int64)
        self.counts = torch.from_numpy(counts_h.astype(np.int32)).to(device)
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.V = int(counts_h.size)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.set_schedule(np.arange(self.V, dtype=np.int32))
        self._out = {}
        self.image = None               # the image arrays of the stylization terms (from_views(..., image_hw=...)): see _check_image
        self.image_host = None
        if image is not None:
            self._set_image(image, device)

    _IMAGE_KEYS = ("box", "img_off", "pix2row", "row2pix", "cut_gt", "tv_h", "tv_v", "vmax", "image_hw")

    def _set_image(self, image, device):
        """validate the packed image arrays on the host and move them to the device (dtypes: box int32 [V,4], img_off int64 [V],
        pix2row int32 [N], row2pix int32 [sum K], cut_gt fp32 [N,3], tv_h / tv_v / smooth fp32 [N], vmax fp32 [V,2], image_hw int64 [2])"""
        host = {k: np.asarray(v.cpu() if torch.is_tensor(v) else v) for k, v in image.items() if v is not None}
        for k in self._IMAGE_KEYS:
            if k not in host:
                raise ValueError(f"EditSet: image array {k!r} missing")
        V = self.V
        box, off = host["box"].astype(np.int32).reshape(V, 4), host["img_off"].astype(np.int64).reshape(V)
        H, W = (int(v) for v in host["image_hw"].reshape(2))
        h, w = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
        if (box[:, 0] < 0).any() or (box[:, 1] > H).any() or (box[:, 2] < 0).any() or (box[:, 3] > W).any() or (h < 1).any() or (w < 1).any():
            raise ValueError("EditSet: every crop box must be non-empty and inside the image (the reference's resize fails on an empty crop)")
        npix = (h.astype(np.int64) * w).astype(np.int64)
        if not np.array_equal(off, np.concatenate([[0], np.cumsum(npix)[:-1]])):
            raise ValueError("EditSet: img_off must be the running sum of the crop sizes")
        N = int(npix.sum())
        p2r, r2p = host["pix2row"].astype(np.int32).reshape(-1), host["row2pix"].astype(np.int32).reshape(-1)
        if p2r.size != N or r2p.size != int(self.counts_host.sum()):
            raise ValueError("EditSet: pix2row needs one entry per crop pixel, row2pix one per row")
        for v in range(V):
            pv = p2r[off[v]:off[v] + npix[v]]
            rv = r2p[self.offsets_host[v]:self.offsets_host[v] + self.counts_host[v]]
            if (pv < -1).any() or (pv >= self.counts_host[v]).any() or (rv < -1).any() or (rv >= npix[v]).any():
                raise ValueError(f"EditSet: view {v}: pixel / row maps out of range")
        for k, shape in (("cut_gt", (N, 3)), ("tv_h", (N,)), ("tv_v", (N,)), ("vmax", (V, 2))) + ((("smooth", (N,)),) if "smooth" in host else ()):
            host[k] = host[k].astype(np.float32).reshape(shape)
        host.update(box=box, img_off=off, pix2row=p2r, row2pix=r2p, image_hw=np.array([H, W], np.int64))
        self.image_host = host
        self.image = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items() if k != "image_hw"}
        self.image_hw = (H, W)
        self.max_crop_pixels = int(npix.max())

    @property
    def device(self):
        return self.x_term.device

    @classmethod
    def from_arrays(cls, x_term, dirs, targets, counts, depth_factor, **kw):
        return cls(x_term, dirs, targets, counts, depth_factor, **kw)

    @classmethod
    def from_views(cls, views, image_hw=None, **kw):
        """the per-view dicts of extract_views / extract_view (x_term, dirs, targets, depth_factor; CPU or device tensors).
        image_hw=(H, W): also pack the image arrays of the stylization terms (pack_image_arrays; needs indices, cut_min_max_xy, cut_gt,
        cut_tv_h, cut_tv_v and, in every view or in none, cut_smooth_trans)"""
        views = list(views)
        if not views:
            raise ValueError("EditSet.from_views: no views")
        cat = lambda key: torch.cat([v[key].detach().float().reshape(-1, 3).cpu() for v in views])
        counts = [int(v["x_term"].shape[0]) for v in views]
        df = [float(v["depth_factor"]) for v in views]
        image = pack_image_arrays(views, image_hw) if image_hw is not None else None
        return cls(cat("x_term"), cat("dirs"), cat("targets"), counts, np.asarray(df, np.float32), image=image, **kw)

    def save(self, path):
        """one .npz of the packed arrays (the counterpart of the reference's --save/--load_edit_dataset); the image arrays as img_*"""
        extra = {"img_" + k: v for k, v in self.image_host.items()} if self.image_host is not None else {}
        np.savez(path, x_term=self.x_term.cpu().numpy(), dirs=self.dirs.cpu().numpy(), targets=self.targets.cpu().numpy(),
                 counts=self.counts_host.astype(np.int32), depth_factor=self.depth_factor.cpu().numpy(), seed=np.uint64(self.seed), **extra)

    @classmethod
    def load(cls, path, device=None):
        """files without image arrays load as before"""
        with np.load(path) as z:
            image = {k[4:]: z[k] for k in z.files if k.startswith("img_")} or None
            return cls(z["x_term"], z["dirs"], z["targets"], z["counts"], z["depth_factor"], seed=int(z["seed"]), device=device, image=image)

    def set_schedule(self, views):
        """the device table the sampler reads at step s: views[s mod len(views)]"""
        v = np.asarray(views, dtype=np.int64).reshape(-1)
        if v.size == 0 or (v < 0).any() or (v >= self.V).any():
            raise ValueError(f"EditSet.set_schedule: view indices must lie in 0..{self.V - 1}")
        self.schedule_host = v.astype(np.int32)
        self.schedule = torch.from_numpy(self.schedule_host).to(self.device)

    def view_points(self, v):
        """the un-jittered x_term [K,3] of view v (a view of the packed array)"""
        o, k = int(self.offsets_host[v]), int(self.counts_host[v])
        return self.x_term[o:o + k]

    def view_arrays(self, v):
        """(x_term, dirs, targets) of view v, un-jittered"""
        o, k = int(self.offsets_host[v]), int(self.counts_host[v])
        return self.x_term[o:o + k], self.dirs[o:o + k], self.targets[o:o + k]

    def _buffers(self, cap):
        out = self._out.get(cap)
        if out is None:
            dev = self.device
            out = self._out[cap] = (torch.empty(cap, 3, dtype=torch.float32, device=dev), torch.empty(cap, 3, dtype=torch.float32, device=dev),
                                    torch.empty(cap, 3, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
        return out

    @torch.no_grad()
    def sample(self, cap, step=None):
        """the view of the schedule at the device step counter -> (x, d, target [cap,3] fp32, m_dev [1] int32 = K) through
        lae_sample_edit_view; the counter is then advanced (capturable).  step=k sets the counter to k first.  cap must be a multiple
        of 4 (16 for the palette network) and >= the view's K, which is otherwise cut to cap rows.  The tensors are reused by the
        next call with the same cap."""
        cap = int(cap)
        if cap < 1 or cap % 4:
            raise ValueError("EditSet.sample: cap must be a positive multiple of 4")
        _lib.need_cuda(self.x_term)
        if step is not None:
            self.step.fill_(int(step))
        x, d, t, m = self._buffers(cap)
        _backend.sample_edit_view(self.x_term, self.dirs, self.targets, self.offsets, self.counts, self.depth_factor, self.schedule, cap,
                                  self.seed, self.step, x, d, t, m)
        return x, d, t, m


# -------------------------------------------------------------------------------------------------------------- the trainer
_IMAGE_TERMS = ("style_weight", "tv_weight", "depth_disc_weight", "smooth_trans_weight")


def fused_step_loss(enc, x, d, target, m_dev, params, opt):
    """the loss of one step as StyleTrainer computes it: forward_train + MSE + weights_loss + offset_loss + palet_loss
    (nerf/utils.py:987-995) as one node over the first *m_dev rows of the [cap,3] buffers, scaled by opt's GradScaler"""
    with torch.autocast("cuda", dtype=torch.float16):
        loss, *_ = enc.forward_train_loss(x, d, target, params, opt, with_palet_loss=True, m_dev=m_dev)
    return loss


class StyleTrainer:
    """StyleTrainer(style_enc, edit_set, params, iters): trains the LAENeRF `style_enc` on the EditSet `edit_set` for the reference's
    `train_steps_style` = iters steps (more are allowed: train() is resumable and the schedule is extended).  `params` carries the
    loss weights (weight_loss_uniform, weight_loss_non_uniform, offset_loss, palette_loss_valid, palette_loss_distinct) and the
    stylization terms (style_weight, tv_weight, tv_depth_guide, depth_disc_weight, smooth_trans_weight, warmup_iterations (1000),
    crop_size (256), preserve_color).
    Optimizer: FusedAdam over style_enc.get_params(lr) (palette 2 lr), betas (0.9, 0.999), eps 1e-8, with its GradScaler (.opt).
    graph=False runs the same steps eagerly; capacity 'bucket' / 'exact' (module docstring).
    Stylization: the image terms need an edit set with image arrays (EditSet.from_views(..., image_hw=...)); the style
    term and preserve_color a StyleNetwork (`style_net`, default style_enc.style_transfer_net).  They run on steps where
    (style_weight > 0 or tv_weight > 0) and image_terms_on(step, warmup_iterations).
    Counters: captures (graphs captured), cache_misses (steps that found no graph for their capacity), steps_skipped (GradScaler);
    capture_error: why image steps run eagerly (None: they are graph-replayed)."""

    _N_TERMS = 4                        # columns of terms(); a subclass with further terms widens the record

    def __init__(self, style_enc, edit_set, params, iters, distill_palette_steps=1500, seed=0, graph=True, capacity="bucket", lr=1e-3,
                 style_net=None):
        from ..optim import FusedAdam
        if capacity not in ("bucket", "exact"):
            raise ValueError("StyleTrainer: capacity must be 'bucket' or 'exact'")
        w = {name: float(getattr(params, name, 0) or 0) for name in _IMAGE_TERMS}
        if float(getattr(params, "intensity_weight", 0) or 0) > 0:
            raise NotImplementedError("StyleTrainer: intensity_weight > 0 (the reference's unused experiment) is not supported (DESIGN.md 4c)")
        if any(v > 0 for v in w.values()) and getattr(edit_set, "image", None) is None:
            raise NotImplementedError("StyleTrainer: the image terms (style / tv / depth_disc / smooth_trans weights) need an edit set with "
                                      "image arrays: EditSet.from_views(views, image_hw=(H, W)) (DESIGN.md 4c)")
        preserve = bool(getattr(params, "preserve_color", False))
        net = style_net if style_net is not None else getattr(style_enc, "style_transfer_net", None)
        if (w["style_weight"] > 0 or preserve) and net is None:
            raise NotImplementedError("StyleTrainer: style_weight > 0 / preserve_color need a style network (LAENeRF built with a style "
                                      "image and VGG weights, or style_net=StyleNetwork(...)) (DESIGN.md 4c)")
        if w["smooth_trans_weight"] > 0 and "smooth" not in edit_set.image:
            raise NotImplementedError("StyleTrainer: smooth_trans_weight > 0 needs cut_smooth_trans in the edit set (a grow grid at extraction)")
        if edit_set.device != style_enc.color_palette.device:
            raise ValueError("StyleTrainer: the edit set and the network must live on the same device")
        self.enc, self.es, self.params = style_enc, edit_set, params
        self.iters, self.graph, self.capacity = int(iters), bool(graph), capacity
        self.weights = w
        self.style_net = net
        self.preserve_color = preserve
        self.warmup = int(getattr(params, "warmup_iterations", 1000) if getattr(params, "warmup_iterations", None) is not None else 1000)
        self.image_block = w["style_weight"] > 0 or w["tv_weight"] > 0          # the reference's gate (nerf/utils.py:997)
        self.flags = 0
        if self.image_block:
            from . import style_image as si
            depth = bool(getattr(params, "tv_depth_guide", False))
            self.flags = (si.IMG_RESIZE if w["style_weight"] > 0 else 0) | (si.IMG_TV if w["tv_weight"] > 0 else 0) \
                | (si.IMG_TV_DEPTH if depth else 0) | (si.IMG_TV_SMOOTH if depth and w["smooth_trans_weight"] > 0 else 0) \
                | (si.IMG_SMOOTH if w["smooth_trans_weight"] > 0 else 0) | (si.IMG_DISC if w["depth_disc_weight"] > 0 else 0)
            self.n_blocks = si.image_blocks(edit_set.max_crop_pixels)
        self.S = int(getattr(params, "crop_size", None) or (net.size if net is not None else 256))
        if net is not None and w["style_weight"] > 0 and net.size != self.S:
            raise ValueError(f"StyleTrainer: crop_size {self.S} differs from the style network's size {net.size}")
        self.lr = float(lr)
        self.opt = FusedAdam(style_enc, param_groups=style_enc.get_params(lr), betas=(0.9, 0.999), eps=1e-8)
        self.gen = torch.Generator().manual_seed(int(seed))
        edit_set.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._sched, self._colour = self._draw(max(self.iters, 1))
        edit_set.set_schedule(self._sched)
        self.rec = torch.zeros(self._sched.size, 2, dtype=torch.float32, device=edit_set.device)     # per step: loss, mse
        self.trec = torch.zeros(self._sched.size, self._N_TERMS, dtype=torch.float32, device=edit_set.device)    # style, tv, smooth, disc
        self.s_d = distill_step(self.iters, distill_palette_steps)
        self.distilled = False
        self.distill_ms = None
        self.global_step = 0
        self.started = False
        self.graphs = {}
        self._pool = None
        self._warm = set()
        self.captures = self.cache_misses = 0
        self.capture_error = None
        self._hist = []
        self._thist = []

    def _draw(self, n):
        if self.preserve_color:
            return draw_schedule(self.gen, self.es.V, n, preserve_color=True)
        return draw_schedule(self.gen, self.es.V, n), None

    def cap_of_step(self, s):
        """the buffer capacity of global step s"""
        return capacity_for(self.es.counts_host[self._sched[s]], self.capacity)

    def image_step(self, s):
        """whether global step s carries the image terms"""
        return self.image_block and image_terms_on(s, self.warmup)

    # ------------------------------------------------------------------ one step
    def _step(self, cap, image=False):
        x, d, t, m = self.es.sample(cap)
        if not image:
            loss = fused_step_loss(self.enc, x, d, t, m, self.params, self.opt)
            self.opt.backward(loss)
            self.opt.step()
            with torch.no_grad():
                self.rec.index_copy_(0, self.es.step - 1, loss.terms[1:3].view(1, 2))
            return
        from .style_image import style_image
        with torch.autocast("cuda", dtype=torch.float16):
            loss, pred, _, _, pred32 = self.enc.forward_train_loss(x, d, t, self.params, self.opt, with_palet_loss=True, m_dev=m,
                                                                  with_pred32=True)
        vgg_in, terms = style_image(pred32, pred, self.es, cap, m, self.S, self.flags, self.n_blocks)
        w = self.weights
        zero = terms.new_zeros(())
        style = self.style_net.loss_from_input(vgg_in) if w["style_weight"] > 0 else zero
        # nerf/utils.py:1008-1033: each term in fp32, cast .half(), times its weight, added to the (fp32) point loss in this order
        img = zero
        for val, name in ((style, "style_weight"), (terms[0], "tv_weight"), (terms[1], "smooth_trans_weight"), (terms[2], "depth_disc_weight")):
            if w[name] > 0:
                img = img + (val.half() * w[name]).float()
        scale = self.opt._scale_view[0] if self.opt.use_scaler else 1.0
        total = loss + img * scale                        # loss is the scaled point loss; the scale is a power of two
        self.opt.backward(total)
        self.opt.step()
        with torch.no_grad():
            row = self.es.step - 1
            self.rec.index_copy_(0, row, torch.stack((loss.terms[1] + img, loss.terms[2])).view(1, 2))
            self.trec.index_copy_(0, row, torch.stack((style.detach(), terms[0], terms[1], terms[2])).view(1, 4))

    def _graph_step(self, cap, image=False):
        key = (cap, image)
        if image and self.capture_error is not None:
            self._step(cap, image)                        # capture refused once: image steps run eagerly
            return
        g = self.graphs.get(key)
        if g is None:
            self.cache_misses += 1
            if key not in self._warm:
                # the encoder / MLP / loss workspaces (and MIOpen's) may have to grow, which is refused inside a capture: this step
                # runs eagerly (the same kernels, hence the same bits) and the next one with this key is captured
                self._step(cap, image)
                self._warm.add(key)
                return
            g = torch.cuda.CUDAGraph()
            step0 = None
            try:
                if image:
                    step0 = self.es.step.clone()
                with torch.cuda.graph(g, pool=self._pool):
                    self._step(cap, image)
            except RuntimeError as e:
                if not image:
                    raise
                # MIOpen (the VGG layers) refused the capture: nothing of the step ran; it and every later image step run eagerly
                self.capture_error = f"{type(e).__name__}: {e}".splitlines()[0]
                torch.cuda.synchronize()
                self.es.step.copy_(step0)
                self._step(cap, image)
                return
            if self._pool is None:
                self._pool = g.pool()
            self.graphs[key] = g
            self.captures += 1
        g.replay()

    def _extend(self):
        """training past the schedule: more 16-step groups from the same generator (the table and the records are reallocated, so
        the graphs, which hold their addresses, are dropped)"""
        more, colour = self._draw(max(self._sched.size, GROUP))
        self._sched = np.concatenate([self._sched, more])
        if colour is not None:
            self._colour = np.concatenate([self._colour, colour])
        self.es.set_schedule(self._sched)
        rec = torch.zeros(self._sched.size, 2, dtype=torch.float32, device=self.es.device)
        rec[:self.rec.shape[0]].copy_(self.rec)
        self.rec = rec
        trec = torch.zeros(self._sched.size, self._N_TERMS, dtype=torch.float32, device=self.es.device)
        trec[:self.trec.shape[0]].copy_(self.trec)
        self.trec = trec
        self.graphs.clear()

    @torch.no_grad()
    def _distill(self):
        """distill_color_palettes on 10 views drawn from the trainer's generator, un-jittered (style_encoder.py:160-173), once"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = torch.randint(0, self.es.V, (10,), generator=self.gen)
        xs = [self.es.view_points(v) for v in range(self.es.V)]
        with torch.autocast("cuda", dtype=torch.float16):
            self.enc.distill_color_palettes(xs, n=10, thresh=0.025, idx=idx)
        self.graphs.clear()                    # n_active / the active mask are host arguments of the captured palette kernels
        self.distilled = True
        torch.cuda.synchronize()
        self.distill_ms = (time.perf_counter() - t0) * 1e3

    def train(self, n_steps):
        """n_steps steps of the reference's loop; the palette distillation runs before global step s_d (once)"""
        if not self.started:
            self.es.set_schedule(self._sched)
            self.es.step.fill_(self.global_step)
            self.started = True
        self.enc.train()
        start = self.global_step
        for _ in range(int(n_steps)):
            s = self.global_step
            if self.s_d is not None and s >= self.s_d and not self.distilled:
                self._distill()
            if s >= self._sched.size:
                self._extend()
            if self.preserve_color and s % GROUP == 0:
                self._match_color(s // GROUP)
            cap = self.cap_of_step(s)
            image = self.image_step(s)
            if self.graph:
                self._graph_step(cap, image)
            else:
                self._step(cap, image)
            self.global_step += 1
        if self.global_step > start:
            self._hist.append(self.rec[start:self.global_step].cpu().numpy())        # the one host read of the call
            self._thist.append(self.trec[start:self.global_step].cpu().numpy())
        return self

    @torch.no_grad()
    def _match_color(self, group):
        """preserve_color (nerf/utils.py:974-976): the style image colour-matched to the group's colour view's targets [3,K,1]; its Gram
        becomes the style network's target (a buffer the captured steps read)"""
        v = int(self._colour[group])
        self.style_net.match_color(self.es.view_arrays(v)[2].T)

    # ------------------------------------------------------------------ checkpoints
    _POINT_WEIGHTS = ("weight_loss_uniform", "weight_loss_non_uniform", "offset_loss", "palette_loss_valid", "palette_loss_distinct")

    def config(self):
        """what a checkpoint is checked against (checkpoint.check_config): everything the drawn schedule and the step's arithmetic depend on"""
        p = self.params
        return {"iters": self.iters, "capacity": self.capacity, "lr": self.lr, "warmup_iterations": self.warmup, "distill_step": self.s_d,
                "weights": dict(self.weights), "point_weights": {k: float(getattr(p, k, 0) or 0) for k in self._POINT_WEIGHTS},
                "tv_depth_guide": bool(getattr(p, "tv_depth_guide", False)), "preserve_color": self.preserve_color, "flags": int(self.flags),
                "crop_size": self.S, "edit_set": {"V": self.es.V, "counts": [int(c) for c in self.es.counts_host]}}

    def state_dict(self):
        """everything a bit-exact resume needs, on the host: the network's state_dict (palette, original palette and
        active-base mask included), the optimizer in torch.optim.Adam's layout with its GradScaler and its sixteen raw state words, the
        host generator's state (further schedule groups and the distillation's views are drawn from it), the drawn view schedule and
        colour schedule, global_step, the edit set's seed and device step, the `distilled` flag, the style network's fixed crop offset
        and its target buffers (match_color rewrites them per group), and config()."""
        from .. import _lib, checkpoint as C
        from ..trainer import _to_host
        o = self.opt.state_dict()
        sc = o.pop("scaler")
        net = self.style_net
        return {"format": C.FORMAT, "lae_version": _lib.load().lae_version().decode(), "config": self.config(),
                "model": _to_host(dict(self.enc.state_dict())), "optimizer": _to_host(o),
                "scaler": C.scaler_to_reference(sc["scale"], sc["growth_tracker"], self.opt.growth_factor, self.opt.backoff_factor,
                                                self.opt.growth_interval),
                "optimizer_words": self.opt.raw_state(), "generator": self.gen.get_state().clone(),
                "sched": torch.from_numpy(np.ascontiguousarray(self._sched, dtype=np.int32).copy()),
                "colour": None if self._colour is None else torch.from_numpy(np.ascontiguousarray(self._colour, dtype=np.int32).copy()),
                "global_step": int(self.global_step), "edit_set": {"seed": int(self.es.seed), "step": self.es.step.detach().cpu().clone()},
                "distilled": bool(self.distilled), "crop_offset": None if net is None else [int(v) for v in net.crop_offset],
                "style_net": None if net is None else _to_host({k: v for k, v in net.state_dict().items()
                                                                if not k.startswith("vgg.") and k != "image"})}

    def _check_load(self, ck, model_only):
        from .. import checkpoint as C
        if not isinstance(ck, dict) or not isinstance(ck.get("model"), dict) or "sched" not in ck:
            raise ValueError("StyleTrainer.load_checkpoint: not a StyleTrainer checkpoint")
        if int(ck.get("format", 0)) > C.FORMAT:
            raise ValueError(f"StyleTrainer.load_checkpoint: checkpoint format {ck.get('format')} is newer than this package's {C.FORMAT}")
        optional = {"model.original_color_palette"}
        cur, saved = C.shapes_of(dict(self.enc.state_dict()), "model."), C.shapes_of(ck["model"], "model.")
        diffs = [(k, saved.get(k, "<missing>"), cur.get(k, "<missing>")) for k in sorted(set(cur) | set(saved))
                 if cur.get(k) != saved.get(k) and not (k in optional and (k not in cur or k not in saved))]
        if model_only:
            return diffs
        diffs += C.check_config(ck["config"], self.config())
        st = ck["optimizer"].get("state", {})
        if sorted(st) != list(range(len(self.opt.items))):
            diffs.append(("optimizer.state", sorted(st), list(range(len(self.opt.items)))))
        else:
            for i, (p, *_) in enumerate(self.opt.items):
                for key in ("exp_avg", "exp_avg_sq"):
                    t = st[i].get(key)
                    if not torch.is_tensor(t) or list(t.shape) != list(p.shape):
                        diffs.append((f"optimizer.state.{i}.{key}", list(t.shape) if torch.is_tensor(t) else "<missing>", list(p.shape)))
        w = ck.get("optimizer_words")
        if not torch.is_tensor(w) or w.dtype != torch.int32 or w.numel() != 16:
            diffs.append(("optimizer_words", "malformed", [16]))
        g = ck.get("generator")
        if not torch.is_tensor(g) or g.dtype != torch.uint8 or g.numel() != self.gen.get_state().numel():
            diffs.append(("generator", "malformed", [int(self.gen.get_state().numel())]))
        sched = ck["sched"]
        if not torch.is_tensor(sched) or sched.numel() == 0 or int(sched.min()) < 0 or int(sched.max()) >= self.es.V:
            diffs.append(("sched", "view indices outside the edit set", self.es.V))
        if (ck.get("colour") is None) != (self._colour is None):
            diffs.append(("colour", ck.get("colour") is not None, self._colour is not None))
        if (ck.get("style_net") is None) != (self.style_net is None):
            diffs.append(("style_net", ck.get("style_net") is not None, self.style_net is not None))
        elif self.style_net is not None:
            have = C.shapes_of(dict(self.style_net.state_dict()), "style_net.")
            diffs += [(k, v, have.get(k, "<missing>")) for k, v in C.shapes_of(ck["style_net"], "style_net.").items() if have.get(k) != v]
        return diffs

    @torch.no_grad()
    def load_state_dict(self, ck, model_only=False, strict_config=True):
        """state_dict()'s counterpart: the dict is checked first (configuration and every shape; a refused load changes nothing; with
        strict_config a difference raises ValueError naming the fields, without it a warning is issued and the load goes on where the
        shapes fit), then everything is restored in place, the records are reallocated for the loaded schedule, the captured graphs are
        dropped and `started` is set.  model_only=True restores the network alone (enough for forward, RecolorView and distill).
        losses() / terms() of a resumed trainer hold the steps since the resume."""
        import warnings
        from .. import checkpoint as C
        diffs = self._check_load(ck, model_only)
        shape_diffs = [d for d in diffs if d[0].split(".")[0] in ("model", "optimizer", "optimizer_words", "generator", "sched", "colour", "style_net")]
        if diffs and (strict_config or shape_diffs):
            raise ValueError("StyleTrainer.load_checkpoint: the checkpoint does not fit this trainer -- " + C.format_differences(diffs))
        if diffs:
            warnings.warn("StyleTrainer.load_checkpoint: the configuration differs -- " + C.format_differences(diffs))
        self.enc.load_state_dict(ck["model"])
        self.opt.sync_shadows()
        self.graphs.clear()
        self._pool = None
        if model_only:
            return self
        o = dict(ck["optimizer"])
        sc = C.scaler_from_reference(ck.get("scaler") or {})
        if sc is not None:
            o["scaler"] = {"scale": sc["scale"], "growth_tracker": sc["growth_tracker"]}
        self.opt.load_state_dict(o)
        self.opt.load_raw_state(ck["optimizer_words"])
        self.gen.set_state(ck["generator"])
        self._sched = ck["sched"].numpy().astype(np.int32)
        self._colour = None if ck.get("colour") is None else ck["colour"].numpy().astype(np.int32)
        self.global_step = int(ck["global_step"])
        self.es.seed = int(ck["edit_set"]["seed"]) & 0xFFFFFFFFFFFFFFFF
        self.es.set_schedule(self._sched)
        self.es.step.copy_(ck["edit_set"]["step"].to(self.es.step.device).view(1))
        self.distilled = bool(ck["distilled"])
        if self.style_net is not None:
            self.style_net.crop_offset = tuple(int(v) for v in ck["crop_offset"])
            own = dict(self.style_net.state_dict())
            for k, v in ck["style_net"].items():
                own[k].copy_(v.to(own[k].device))
        self.rec = torch.zeros(self._sched.size, 2, dtype=torch.float32, device=self.es.device)
        self.trec = torch.zeros(self._sched.size, self._N_TERMS, dtype=torch.float32, device=self.es.device)
        self._hist, self._thist = [], []
        self.started = True
        return self

    def save_checkpoint(self, path):
        """state_dict() written with checkpoint.atomic_save (blocking, between train() calls) -> path"""
        from .. import checkpoint as C
        return C.atomic_save(self.state_dict(), path)

    def load_checkpoint(self, path, model_only=False, strict_config=True):
        """read `path` (torch.load(weights_only=True)) and load_state_dict it"""
        from .. import checkpoint as C
        return self.load_state_dict(C.read_checkpoint(path), model_only=model_only, strict_config=strict_config)

    # ------------------------------------------------------------------ results
    def _records(self):
        return np.concatenate(self._hist) if self._hist else np.zeros((0, 2), np.float32)

    def terms(self):
        """per-step unweighted image terms [n,4] float32: style (Gram MSE), tv, smooth transition, depth discontinuity (0 on steps
        without the image terms or with the term's weight at 0)"""
        return np.concatenate(self._thist) if self._thist else np.zeros((0, self._N_TERMS), np.float32)

    def losses(self):
        """per-step unscaled losses (MSE + weight + offset + palette terms, nerf/utils.py:990-995, + the weighted image terms on
        steps that carry them) as float32"""
        return self._records()[:, 0]

    def mse(self):
        """per-step MSE term"""
        return self._records()[:, 1]

    def group_psnr(self):
        """what the reference prints per 16-step call: 10 log10(1 / average loss) (nerf/utils.py:1041-1049), one value per complete
        group"""
        lo = self.losses().astype(np.float64)
        n = lo.size // GROUP
        return np.array([10.0 * math.log10(1.0 / lo[g * GROUP:(g + 1) * GROUP].mean()) for g in range(n)])

    @property
    def steps_skipped(self):
        """optimizer steps the GradScaler skipped (non-finite gradients)"""
        return self.opt.steps_skipped
