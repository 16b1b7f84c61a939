"""The second stage of the single-reference-view stylization (Ref-NPR): the palette network trained on registered views -- the
reference's `train_styleenc_step_npr` (nerf/utils.py:1058-1176) driven by `SingleViewEditDataset.collate_gt` / `collate`
(editing/single_view_edit_dataset.py:351-412), on the HIP kernels of csrc/ref_stage.hip and StyleTrainer's bucketed graphs.

Per step: the view (lae_sample_edit_view) -> LAENeRF.forward_train_loss(..., mse_weight=0): the regularisers as one node, pred as a
differentiable fp32 tensor -> `ref_terms`: pred' = fp16(pred * w8s) and the phase's colour term
    gt phase  (while not image_terms_on(step, warmup_iterations); collate_gt): MSE(pred', ground truth) over the view's K rows;
    ref phase (afterwards; collate): the weighted MSE over the registered rows, divided by 3 R, and the colour-patch MSE of the
              canvas resized to the VGG relu5 grid (H // 16 x W // 16), as at most four (row, weight) taps per output;
ref phase only: editing/style_image.py's kernels on pred' (the crop resized to feature_size for VGG, the TV / depth-discontinuity
sums with the style guide in the TV weights), VGG-16 layers 11/13/15 in torch, and the template feature term
`lae_nnfm_loss_forward(x, style_feat, z)` with the step's relation z selected on the device.  All gradients meet in `ref_terms`'
backward and enter the palette backward as its g_pred.

The loss is summed in the reference's order and precision: registered term (times mse_loss in the ref phase; the gt phase has no
factor, utils.py:1104), the three regularisers (each rounded to fp16, inside the node), cos term times cos_loss_factor (fp32), patch
term times color_patch_loss (fp32), TV and depth discontinuity (`.half()` times weight).

Departures from the reference: a view without a registered row gives a zero registered term (the reference: the mean
of an empty tensor, NaN); the crop is resized and then normalized (the reference's encode_feats normalizes first; the resize's
weights sum to one, so the two differ by roundings); the template term keeps the relation z and one shared style_feat instead of
the gathered features.  Refused with NotImplementedError: style_weight > 0 (the guided Gram loss), smooth_trans_weight > 0 (the
reference passes cut_smooth=None there), intensity_weight, and cos_loss_factor / color_patch_loss > 0 without the supervision.
The NeRF distillation that follows (`train_step_npr`) is editing/ref_distill.py.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Function

from .style_trainer import EditSet, StyleTrainer, image_terms_on, pack_image_arrays

__all__ = ["pack_ref_arrays", "ref_stage_numpy", "reference_ref_terms", "reference_ref_step", "ref_phase", "ref_terms", "nnfm_loss_at",
           "RefEditSet", "RefStyleTrainer", "GT", "REF"]

GT, REF = 0, 1                       # include/laenerf.h LAE_REF_MODE_*
PATCH_STRIDE = 16                    # VGG-16's relu5 grid: four 2 x 2 pools


def ref_phase(step, warmup_iterations=1000):
    """the phase of global step `step`: REF once image_terms_on(step, warmup_iterations) (the reference swaps its dataloader when
    `distill_step > warmup_iterations` at a 16-step call's start, nerf/gui.py:342), GT before"""
    return REF if image_terms_on(step, warmup_iterations) else GT


# ------------------------------------------------------------------------------------------------------------------- packing
def _axis_taps(n_in, n_out):
    """PyTorch's bilinear source index (align_corners=False) in float32: src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out;
    i0 = int(src), i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1 -> (i0, i1 int64, l0, l1 float32) per output"""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (dst + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1.0) - l1).astype(np.float32), l1


def pack_ref_arrays(views, image_hw, supervision=None):
    """the arrays of the registered terms for RefEditSet (host numpy), view v's rows at the running sum of the row counts:
      w8s16       fp16 [sum K]       the view's opacity weights (`w8s`), rounded as the reference's `.half()`;
      ref_target  fp32 [sum K, 3], ref_weight fp32 [sum K]: `ref_targets` / max(`target_weights`, 0) scattered to the rows
                  `indices_ray_reg`, zero elsewhere (weight 0 = the row adds nothing); ref_count int32 [V] = R;
      tap_row int32 / tap_w fp32 [V, ph * pw, 4], ph = H // 16, pw = W // 16: F.interpolate(canvas[None], (ph, pw), mode="bilinear",
                  align_corners=False, antialias=False) of the H x W x 3 canvas that is zero except at the view's `indices`, as
                  taps on the view's rows: weight = ly * lx (one fp32 product), duplicate source pixels of an output merged (their
                  weights added), row -1 where the source pixel is off the mask or the slot is unused;
      row_tap     int32 [sum K]      the tap (output * 4 + slot) that reads the row, -1: none.  With a scale >= 2 no row is under
                  two outputs (checked: ValueError otherwise), so the backward is one gather per row;
      color_patch fp32 [V, 3, ph * pw]   supervision["color_patch"], or zeros without supervision."""
    H, W = (int(v) for v in image_hw)
    ph, pw = H // PATCH_STRIDE, W // PATCH_STRIDE
    if ph < 1 or pw < 1:
        raise ValueError(f"pack_ref_arrays: a {H}x{W} image has no relu5 grid (H // 16 and W // 16 must be >= 1)")
    arr = lambda t: np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    n_out = ph * pw
    y0, y1, ly0, ly1 = _axis_taps(H, ph)
    x0, x1, lx0, lx1 = _axis_taps(W, pw)
    iy = np.stack([y0, y0, y1, y1], -1)[:, None, :].repeat(pw, 1)                      # [ph, pw, 4]
    ix = np.stack([x0, x1, x0, x1], -1)[None, :, :].repeat(ph, 0)
    wy = np.stack([ly0, ly0, ly1, ly1], -1)[:, None, :]
    wx = np.stack([lx0, lx1, lx0, lx1], -1)[None, :, :]
    pix = (iy * W + ix).reshape(n_out, 4)
    wgt = (wy * wx).astype(np.float32).reshape(n_out, 4)
    for t in range(1, 4):                                                              # merge duplicate source pixels of an output
        for u in range(t):
            dup = (pix[:, t] == pix[:, u]) & (pix[:, t] >= 0)
            wgt[dup, u] = wgt[dup, u] + wgt[dup, t]
            wgt[dup, t] = 0.0
            pix[dup, t] = -1
    w8, rt, rw, rc, trow, tw, rtap, cp = [], [], [], [], [], [], [], []
    for k, v in enumerate(views):
        K = int(v["x_term"].shape[0])
        idx = arr(v["indices"]).astype(np.int64).reshape(-1)
        w = arr(v["w8s"]).astype(np.float32).reshape(-1)
        if idx.size != K or w.size != K or (idx < 0).any() or (idx >= H * W).any():
            raise ValueError(f"pack_ref_arrays: view {k}: indices / w8s need one entry per row, inside the {H}x{W} image")
        reg = arr(v["indices_ray_reg"]).astype(np.int64).reshape(-1)
        t_reg = arr(v["ref_targets"]).astype(np.float32).reshape(-1, 3)
        w_reg = arr(v["target_weights"]).astype(np.float32).reshape(-1)
        if t_reg.shape[0] != reg.size or w_reg.size != reg.size or (reg < 0).any() or (reg >= K).any() or np.unique(reg).size != reg.size:
            raise ValueError(f"pack_ref_arrays: view {k}: ref_targets / target_weights need one entry per distinct row of indices_ray_reg")
        dense_t, dense_w = np.zeros((K, 3), np.float32), np.zeros(K, np.float32)
        dense_t[reg], dense_w[reg] = t_reg, np.maximum(w_reg, 0.0)                     # clamp_min(target_weights, 0), :226
        p2r = np.full(H * W, -1, np.int32)
        p2r[idx] = np.arange(K, dtype=np.int32)
        rows = np.where(pix >= 0, p2r[np.maximum(pix, 0)], -1).astype(np.int32)
        flat = rows.reshape(-1)
        hit = np.nonzero(flat >= 0)[0]
        if np.unique(flat[hit]).size != hit.size:
            raise ValueError(f"pack_ref_arrays: view {k}: a row lies under two outputs of the colour patch (resize scale below 2)")
        tap_of = np.full(K, -1, np.int32)
        tap_of[flat[hit]] = hit.astype(np.int32)
        w8.append(w.astype(np.float16)); rt.append(dense_t); rw.append(dense_w); rc.append(reg.size)
        trow.append(rows); tw.append(wgt.copy()); rtap.append(tap_of)
        if supervision is not None:
            c = arr(supervision["color_patch"][k]).astype(np.float32)
            if c.shape != (3, ph, pw):
                raise ValueError(f"pack_ref_arrays: view {k}: color_patch is {c.shape}, the relu5 grid of a {H}x{W} image is {(3, ph, pw)}")
            cp.append(c.reshape(3, n_out))
        else:
            cp.append(np.zeros((3, n_out), np.float32))
    return {"w8s16": np.concatenate(w8), "ref_target": np.concatenate(rt), "ref_weight": np.concatenate(rw),
            "ref_count": np.asarray(rc, np.int32), "tap_row": np.stack(trow), "tap_w": np.stack(tw), "row_tap": np.concatenate(rtap),
            "color_patch": np.stack(cp), "patch_hw": np.array([ph, pw], np.int64)}


# --------------------------------------------------------------------------------------------------------------- restatements
def ref_stage_numpy(pred16, w8s16, mode, target=None, ref_target=None, ref_weight=None, R=None, tap_row=None, tap_w=None, color_patch=None,
                    g_predw=None, g_terms=(1.0, 1.0)):
    """lae_ref_terms_forward / _backward in float64 on the same fp16 / fp32 inputs, for one view's K rows.
    pred16 [K,3], w8s16 [K] fp16; mode GT: target [K,3]; mode REF: ref_target [K,3], ref_weight [K], R, tap_row / tap_w [n_out,4],
    color_patch [3,n_out]; g_predw [K,3] or None, g_terms = the two upstream gradients.
    -> {predw [K,3] fp16 (bit for bit the kernel's), terms [2], resid [n_out,3], g_pred [K,3]} (float64)"""
    p16, w16 = np.asarray(pred16, np.float16).reshape(-1, 3), np.asarray(w8s16, np.float16).reshape(-1)
    predw = (p16.astype(np.float32) * w16.astype(np.float32)[:, None]).astype(np.float16)      # exact fp32 product, one rounding
    p = predw.astype(np.float64)
    K = p.shape[0]
    g = np.zeros((K, 3)) if g_predw is None else np.asarray(g_predw, np.float64).reshape(K, 3).copy()
    g0, g1 = float(g_terms[0]), float(g_terms[1])
    terms, resid = np.zeros(2), None
    if mode == GT:
        d = p - np.asarray(target, np.float64).reshape(K, 3)
        terms[0] = (d * d).sum() / (3.0 * K)
        g += g0 * 2.0 * d / (3.0 * K)
    else:
        w = np.asarray(ref_weight, np.float64).reshape(K)
        d = np.where(w[:, None] != 0, p - np.asarray(ref_target, np.float64).reshape(K, 3), 0.0)
        R = int(R)
        if R > 0:
            terms[0] = (w[:, None] * d * d).sum() / (3.0 * R)
            g += g0 * 2.0 * w[:, None] * d / (3.0 * R)
        rows = np.asarray(tap_row, np.int64).reshape(-1, 4)
        tw = np.asarray(tap_w, np.float64).reshape(-1, 4)
        n_out = rows.shape[0]
        ok = (rows >= 0) & (rows < K)
        vals = np.where(ok[..., None], p[np.clip(rows, 0, K - 1)], 0.0)                          # [n_out, 4, 3]
        resid = (tw[..., None] * vals).sum(1) - np.asarray(color_patch, np.float64).reshape(3, n_out).T
        terms[1] = (resid * resid).sum() / (3.0 * n_out)
        gp = g1 * 2.0 * resid / (3.0 * n_out)
        np.add.at(g, rows[ok], (tw[..., None] * gp[:, None, :])[ok])
    return {"predw": predw, "terms": terms, "resid": resid, "g_pred": w16.astype(np.float64)[:, None] * g}


def reference_ref_terms(pred, w8s, mode, target=None, ref_targets=None, target_weights=None, indices_ray_reg=None, indices=None,
                        image_hw=None, color_patch=None):
    """the reference's torch lines (nerf/utils.py:1096-1104, :1110-1111, :1120-1122) on one view, CPU or device: pred [K,3] fp16 ->
    (pred' = pred * w8s.half(), the registered term, the colour-patch term (0 in the gt phase)).  Differentiable in pred.
    color_patch [3,ph,pw]; a view without registered rows gives NaN, as the reference's empty mean does."""
    pc = pred * w8s.to(pred.device)[..., None].half()
    zero = torch.zeros((), dtype=torch.float32, device=pred.device)
    if mode == GT:
        return pc, F.mse_loss(pc.float(), target.float()), zero
    idx = indices_ray_reg.long()
    reg = (torch.pow(ref_targets.float() - pc[idx], 2) * target_weights.float()[..., None]).mean()
    H, W = (int(v) for v in image_hw)
    canvas = torch.zeros((H * W, 3), dtype=torch.float32, device=pred.device).index_put((indices.long(),), pc.float()).reshape(H, W, 3)
    got = F.interpolate(canvas.permute(2, 0, 1)[None], size=tuple(color_patch.shape[-2:]), mode="bilinear", align_corners=False, antialias=False)[0]
    return pc, reg, F.mse_loss(got, color_patch.float())


def reference_ref_step(enc, params, x, d, target, view, image_hw, mode, sem=None, style_feat=None, tmpl_z=None, color_patch=None):
    """the reference-shaped step (nerf/utils.py:1092-1148 minus the refused terms) as a torch autograd chain on one view's K rows:
    enc.forward_train under autocast, reference_ref_terms, the regularisers, and in the ref phase the crop's VGG-16 features against
    gather(style_feat, tmpl_z), the colour patch, TV and depth discontinuity (style_image.reference_image_terms with smooth = 1 -
    style_guide).  x, d, target [K,3] on the device; view: register_views' dict.  -> (loss fp32, differentiable; dict of the terms)"""
    from .style_image import IMG_DISC, IMG_RESIZE, IMG_TV, IMG_TV_DEPTH, IMG_TV_SMOOTH, reference_image_terms
    dev = x.device
    t = lambda k: torch.as_tensor(view[k]).to(dev)
    g = lambda name, default=0.0: float(getattr(params, name, default) or 0)
    with torch.autocast("cuda", dtype=torch.float16):
        rp, rw, ro = enc.forward_train(x, d)
    ref = mode == REF
    pc, reg, patch = reference_ref_terms(rp, t("w8s").float(), mode, target=target, ref_targets=t("ref_targets") if ref else None,
                                         target_weights=torch.clamp_min(t("target_weights"), 0) if ref else None,
                                         indices_ray_reg=t("indices_ray_reg") if ref else None, indices=t("indices"), image_hw=image_hw,
                                         color_patch=color_patch)
    loss = reg * g("mse_loss", 6.0) if ref else reg
    loss = loss + enc.weights_loss(rw.float(), params).half()
    loss = loss + enc.offset_loss(ro.float(), params).half()
    loss = loss + enc.palet_loss(params).half()
    out = {"reg": reg.detach(), "patch": patch.detach(), "cos": torch.zeros((), device=dev), "tv": torch.zeros((), device=dev),
           "disc": torch.zeros((), device=dev)}
    if ref:
        cos_f, patch_f, tv_w, disc_w = g("cos_loss_factor", 2.5), g("color_patch_loss", 30.0), g("tv_weight"), g("depth_disc_weight")
        depth = bool(getattr(params, "tv_depth_guide", False))
        flags = (IMG_RESIZE if cos_f > 0 else 0) | (IMG_TV if tv_w > 0 else 0) | ((IMG_TV_DEPTH | IMG_TV_SMOOTH) if depth and tv_w > 0 else 0) \
            | (IMG_DISC if disc_w > 0 else 0)
        H, W = (int(v) for v in image_hw)
        S = int(getattr(params, "feature_size", 256) or 256)
        vgg_in, tv, _, disc = reference_image_terms(pc, t("indices"), [int(b) for b in view["cut_min_max_xy"]], H, W, None, t("cut_tv_h"),
                                                    t("cut_tv_v"), 1.0 - t("style_guide").float(), S, flags)
        if cos_f > 0:
            feat = sem.features_from_input(vgg_in).flatten(2)
            z = tmpl_z.long()[:, None, :].expand(-1, style_feat.shape[1], -1)
            cos = sem.cos_loss(feat, torch.gather(style_feat, 2, z))
            loss = loss + cos * cos_f
            out["cos"] = cos.detach()
        loss = loss + patch * patch_f
        if tv_w > 0:
            loss = loss + tv.half() * tv_w
            out["tv"] = tv.detach()
        if disc_w > 0:
            loss = loss + disc.half() * disc_w
            out["disc"] = disc.detach()
    return loss.float(), out


# ------------------------------------------------------------------------------------------------------------ autograd nodes
class _ref_terms(Function):
    @staticmethod
    def forward(ctx, pred32, pred16, es, cap, m_dev, target, mode):
        from ..backend import ref_stage_backend as be
        dev = pred16.device
        predw16 = torch.empty(cap, 3, dtype=torch.float16, device=dev)
        predw32 = torch.empty(cap, 3, dtype=torch.float32, device=dev)
        resid = torch.empty(es.n_out if mode == REF else 0, 3, dtype=torch.float64, device=dev)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        be.forward(es, pred16, cap, m_dev, target, mode, predw16, predw32, resid, terms)
        ctx.save_for_backward(pred16, m_dev, target, resid)
        ctx.args = (es, cap, mode)
        ctx.mark_non_differentiable(predw16)
        ctx.set_materialize_grads(False)
        return predw32, predw16, terms

    @staticmethod
    def backward(ctx, g_predw, _g16, g_terms):
        from ..backend import ref_stage_backend as be
        if g_predw is None and g_terms is None:
            return (None,) * 7
        pred16, m_dev, target, resid = ctx.saved_tensors
        es, cap, mode = ctx.args
        if g_terms is None:
            g_terms = torch.zeros(2, dtype=torch.float32, device=pred16.device)
        g_pred = torch.empty(cap, 3, dtype=torch.float32, device=pred16.device)
        be.backward(es, pred16, cap, m_dev, target, mode, resid, None if g_predw is None else g_predw.float().contiguous(),
                    g_terms.float().contiguous(), g_pred)
        return g_pred, None, None, None, None, None, None


def ref_terms(pred32, pred16, es, cap, m_dev, target, mode):
    """the registered terms of the RefEditSet `es`'s current step (the view the sampler drew last, its K in m_dev): pred32 [cap,3]
    fp32 (differentiable), pred16 the same values in fp16, target the step's [cap,3] ground-truth buffer, mode GT / REF ->
    (pred' [cap,3] fp32 (differentiable), pred' fp16, terms [2] fp32 = registered MSE, colour-patch MSE (0 in the gt phase))"""
    if getattr(es, "ref", None) is None:
        raise RuntimeError("ref_terms: the edit set carries no registration arrays (RefEditSet.from_views)")
    if mode not in (GT, REF):
        raise ValueError("ref_terms: mode must be GT or REF")
    return _ref_terms.apply(pred32, pred16, es, int(cap), m_dev, target, int(mode))


class _nnfm_loss_at(Function):
    @staticmethod
    def forward(ctx, x, s, z):
        from ..backend import nnfm_backend as be
        n, C, Na = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        stats = torch.empty(4, n * Na, dtype=torch.float32, device=x.device)
        be.loss_forward(x, s, z, n, C, Na, s.shape[2], loss, stats)
        ctx.save_for_backward(x, s, z, stats)
        return loss[0]

    @staticmethod
    def backward(ctx, g_loss):
        from ..backend import nnfm_backend as be
        x, s, z, stats = ctx.saved_tensors
        n, C, Na = x.shape
        dx = torch.empty_like(x)
        be.loss_backward(x, s, z, stats, g_loss.float().reshape(1).contiguous(), n, C, Na, s.shape[2], dx)
        return dx, None, None


def nnfm_loss_at(x, style, z):
    """cos_loss(x, gather(style, z)) (semantic_encoder.py:128-135) at a GIVEN relation: x [n,C,Na], style [n,C,Nb] fp32, z [n,Na]
    int32 with values in 0..Nb-1 (the caller validates) -> a scalar whose gradient reaches x (lae_nnfm_loss_forward / _backward)"""
    x, style, z = x.float().contiguous(), style.float().contiguous(), z.contiguous()
    if x.dim() != 3 or style.dim() != 3 or x.shape[:2] != style.shape[:2] or tuple(z.shape) != (x.shape[0], x.shape[2]) or z.dtype != torch.int32:
        raise ValueError(f"nnfm_loss_at: x {tuple(x.shape)}, style {tuple(style.shape)}, z {tuple(z.shape)} {z.dtype} do not fit")
    return _nnfm_loss_at.apply(x, style, z)


# ------------------------------------------------------------------------------------------------------------------- the set
class RefEditSet(EditSet):
    """EditSet plus the registration arrays of pack_ref_arrays (`.ref`, on the set's device; `.ref_host`), `.n_out` / `.patch_hw`,
    and with `supervision` (semantic_encoder.build_ref_supervision) `.tmpl_z` [V,3,P] int32, `.style_feat` [3,C,P] fp32 and
    `.feature_size`.  The image pack's `smooth` array is 1 - style_guide: IMG_TV_SMOOTH's weights (1 - tv) * (1 - smooth) are then the
    reference's tv_loss_depth_weighted(..., weights_trans=1 - style_guide)."""

    def __init__(self, *args, ref=None, supervision=None, **kw):
        super().__init__(*args, **kw)
        if ref is None:
            raise ValueError("RefEditSet: the registration arrays are missing (RefEditSet.from_views)")
        dev = self.device
        V, n = self.V, int(self.counts_host.sum())
        host = {k: np.asarray(v) for k, v in ref.items()}
        ph, pw = (int(v) for v in host["patch_hw"].reshape(2))
        n_out = ph * pw
        shapes = {"w8s16": (n,), "ref_target": (n, 3), "ref_weight": (n,), "ref_count": (V,), "tap_row": (V, n_out, 4), "tap_w": (V, n_out, 4),
                  "row_tap": (n,), "color_patch": (V, 3, n_out)}
        for k, shape in shapes.items():
            if k not in host or tuple(host[k].shape) != shape:
                raise ValueError(f"RefEditSet: {k} must be {shape}")
        for v in range(V):
            o, K = int(self.offsets_host[v]), int(self.counts_host[v])
            tr, rtp = host["tap_row"][v], host["row_tap"][o:o + K]
            if (tr < -1).any() or (tr >= K).any() or (rtp < -1).any() or (rtp >= n_out * 4).any() or not 0 <= int(host["ref_count"][v]) <= K:
                raise ValueError(f"RefEditSet: view {v}: tap rows, row taps or the registered count out of range")
        dt = {"w8s16": np.float16, "ref_target": np.float32, "ref_weight": np.float32, "ref_count": np.int32, "tap_row": np.int32,
              "tap_w": np.float32, "row_tap": np.int32, "color_patch": np.float32}
        self.ref_host = {k: np.ascontiguousarray(host[k].astype(dt[k])) for k in shapes}
        self.ref = {k: torch.from_numpy(v).to(dev) for k, v in self.ref_host.items()}
        self.patch_hw, self.n_out = (ph, pw), n_out
        self.tmpl_z = self.style_feat = self.feature_size = None
        if supervision is not None:
            z = torch.as_tensor(supervision["tmpl_z"]).to(torch.int32)
            sf = torch.as_tensor(supervision["style_feat"]).float()
            if z.dim() != 3 or z.shape[0] != V or sf.dim() != 3 or z.shape[1] != sf.shape[0] or z.numel() == 0 or int(z.min()) < 0 \
                    or int(z.max()) >= sf.shape[2]:
                raise ValueError("RefEditSet: tmpl_z must be [V, L, P] with values inside style_feat [L, C, P']")
            self.tmpl_z, self.style_feat = z.to(dev).contiguous(), sf.to(dev).contiguous()
            self.feature_size = int(supervision["feature_size"])

    @classmethod
    def from_views(cls, views, image_hw, supervision=None, **kw):
        """register_views' dicts (EditSet.from_views' keys plus w8s, ref_targets, target_weights, indices_ray_reg, style_guide)"""
        views = list(views)
        if not views:
            raise ValueError("RefEditSet.from_views: no views")
        if image_hw is None:
            raise ValueError("RefEditSet.from_views: image_hw=(H, W) is needed (the colour patch covers the whole image)")
        guided = [dict(v, cut_smooth_trans=1.0 - torch.as_tensor(v["style_guide"]).float()) for v in views]
        cat = lambda key: torch.cat([v[key].detach().float().reshape(-1, 3).cpu() for v in views])
        counts = [int(v["x_term"].shape[0]) for v in views]
        df = [float(v["depth_factor"]) for v in views]
        return cls(cat("x_term"), cat("dirs"), cat("targets"), counts, np.asarray(df, np.float32), image=pack_image_arrays(guided, image_hw),
                   ref=pack_ref_arrays(views, image_hw, supervision), supervision=supervision, **kw)

    def save(self, path):
        raise NotImplementedError("RefEditSet.save: pack the set again with RefEditSet.from_views (the registration is not written)")

    @classmethod
    def load(cls, path, device=None):
        raise NotImplementedError("RefEditSet.load: pack the set again with RefEditSet.from_views")


# --------------------------------------------------------------------------------------------------------------- the trainer
_REF_WEIGHTS = (("mse_loss", 6.0), ("cos_loss_factor", 2.5), ("color_patch_loss", 30.0))


class RefStyleTrainer(StyleTrainer):
    """RefStyleTrainer(style_enc, ref_edit_set, params, iters, sem=None, ...): StyleTrainer's loop with the step of the module
    docstring.  `params` also carries mse_loss (6), cos_loss_factor (2.5), color_patch_loss (30), feature_size (256); `sem`: the
    SemanticEncoder of the template term (needed with cos_loss_factor > 0).  Graphs are keyed (capacity, phase); the first step of an
    unseen key runs eagerly.  rec column 1 (mse()) holds the registered term; terms() columns: style (0), tv, smooth (0), depth
    discontinuity, cos, colour patch.  Save and resume are StyleTrainer's; config() names the class and the new weights, so a plain
    StyleTrainer refuses the file."""
    _N_TERMS = 6

    def __init__(self, style_enc, edit_set, params, iters, sem=None, **kw):
        g = lambda name: float(getattr(params, name, 0) or 0)
        if g("style_weight") > 0:
            raise NotImplementedError("RefStyleTrainer: style_weight > 0 (the guided Gram loss, style_network.py:160-179) is not supported (DESIGN.md 4c)")
        if g("smooth_trans_weight") > 0:
            raise NotImplementedError("RefStyleTrainer: smooth_trans_weight > 0: the reference passes cut_smooth=None in this stage (DESIGN.md 4c)")
        if g("intensity_weight") > 0:
            raise NotImplementedError("RefStyleTrainer: intensity_weight > 0 (the reference's unused experiment) is not supported (DESIGN.md 4c)")
        rw = {name: float(getattr(params, name, None) if getattr(params, name, None) is not None else default) for name, default in _REF_WEIGHTS}
        if not isinstance(edit_set, RefEditSet):
            raise TypeError("RefStyleTrainer: the edit set must be a RefEditSet (RefEditSet.from_views)")
        if (rw["cos_loss_factor"] > 0 or rw["color_patch_loss"] > 0) and edit_set.tmpl_z is None:
            raise NotImplementedError("RefStyleTrainer: cos_loss_factor / color_patch_loss > 0 need the supervision: RefEditSet.from_views(views, "
                                      "image_hw, supervision=build_ref_supervision(...)) (DESIGN.md 4c)")
        if rw["cos_loss_factor"] > 0 and sem is None:
            raise NotImplementedError("RefStyleTrainer: cos_loss_factor > 0 needs the semantic encoder (sem=SemanticEncoder(...))")
        super().__init__(style_enc, edit_set, params, iters, **kw)
        from . import style_image as si
        self.ref_weights, self.sem = rw, sem
        fs = getattr(params, "feature_size", None)
        self.S = int(fs if fs is not None else 256)
        if rw["cos_loss_factor"] > 0 and (edit_set.feature_size != self.S or edit_set.tmpl_z.shape[2] != (self.S // 4) ** 2):
            raise ValueError(f"RefStyleTrainer: feature_size {self.S} differs from the supervision's ({edit_set.feature_size}, "
                             f"{edit_set.tmpl_z.shape[2]} positions)")
        w = self.weights
        depth = bool(getattr(params, "tv_depth_guide", False))
        self.flags = (si.IMG_RESIZE if rw["cos_loss_factor"] > 0 else 0) | (si.IMG_TV if w["tv_weight"] > 0 else 0) \
            | ((si.IMG_TV_DEPTH | si.IMG_TV_SMOOTH) if depth and w["tv_weight"] > 0 else 0) | (si.IMG_DISC if w["depth_disc_weight"] > 0 else 0)
        self.n_blocks = si.image_blocks(edit_set.max_crop_pixels)

    def image_step(self, s):
        """whether global step s is a ref-phase step"""
        return ref_phase(s, self.warmup) == REF

    def phase_of_step(self, s):
        """GT or REF"""
        return ref_phase(s, self.warmup)

    def step_loss(self, cap, image=False, scaler=None):
        """sample the step's view and build its loss: -> (total: the loss times the loss scale, differentiable; loss: the scaled
        regularisers' node; acc: the unscaled colour / feature / image terms; the unweighted terms reg, patch, cos, tv, disc).
        scaler: the trainer's optimizer (default), or a 1-element fp32 device tensor holding the loss scale"""
        es, rw, w = self.es, self.ref_weights, self.weights
        scaler = self.opt if scaler is None else scaler
        x, d, t, m = es.sample(cap)
        with torch.autocast("cuda", dtype=torch.float16):
            loss, pred, _, _, pred32 = self.enc.forward_train_loss(x, d, t, self.params, scaler, with_palet_loss=True, m_dev=m,
                                                                  with_pred32=True, mse_weight=0.0)
        predw32, predw16, rt = ref_terms(pred32, pred, es, cap, m, t, REF if image else GT)
        zero = rt.new_zeros(())
        cos = tv = disc = zero
        if not image:
            acc = rt[0]                                    # collate_gt: plain MSE, no factor (nerf/utils.py:1104)
        else:
            from .style_image import IMG_DISC, IMG_TV, style_image
            acc = rt[0] * rw["mse_loss"]
            if self.flags:
                vgg_in, it = style_image(predw32, predw16, es, cap, m, self.S, self.flags, self.n_blocks)
                tv, disc = (it[0] if self.flags & IMG_TV else zero), (it[2] if self.flags & IMG_DISC else zero)
            if rw["cos_loss_factor"] > 0:
                n = es.schedule.numel()
                v = es.schedule.index_select(0, torch.remainder(es.step - 1, n)).long()          # the step's view, on the device
                z = es.tmpl_z.index_select(0, v)[0]
                cos = nnfm_loss_at(self.sem.features_from_input(vgg_in).flatten(2), es.style_feat, z)
                acc = acc + cos * rw["cos_loss_factor"]
            acc = acc + rt[1] * rw["color_patch_loss"]
            if w["tv_weight"] > 0:
                acc = acc + (tv.half() * w["tv_weight"]).float()
            if w["depth_disc_weight"] > 0:
                acc = acc + (disc.half() * w["depth_disc_weight"]).float()
        scale = scaler[0] if torch.is_tensor(scaler) else (scaler._scale_view[0] if scaler.use_scaler else 1.0)
        total = loss + acc * scale                         # loss: the scaled regularisers; the scale is a power of two
        return total, loss, acc, rt[0], (rt[1] if image else zero), cos, tv, disc

    def _step(self, cap, image=False):
        es = self.es
        total, loss, acc, reg, patch, cos, tv, disc = self.step_loss(cap, image)
        zero = reg.new_zeros(())
        self.opt.backward(total)
        self.opt.step()
        with torch.no_grad():
            row = es.step - 1
            self.rec.index_copy_(0, row, torch.stack((loss.terms[1] + acc, reg)).view(1, 2))
            self.trec.index_copy_(0, row, torch.stack((zero, tv, zero, disc, cos, patch)).view(1, 6))

    def config(self):
        c = super().config()
        c.update({"class": "RefStyleTrainer", "ref_weights": dict(self.ref_weights), "feature_size": self.S,
                  "supervision": self.es.tmpl_z is not None})
        return c
