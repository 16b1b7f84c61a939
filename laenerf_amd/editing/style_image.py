"""The image-space half of LAENeRF's stylization step (nerf/utils.py:997-1033) as one autograd node on the HIP kernels of
csrc/style_image.hip, plus the reference's torch formulation of the same block (tests and tools/style_mode_bench.py compare the two).

Per step with the image terms on: the fused point loss hands over pred as a differentiable fp32 [cap,3] tensor
(LAENeRF.forward_train_loss(..., with_pred32=True)); `style_image(...)` gathers the step's crop through the edit set's pixel -> row
map and writes the resized, normalized VGG input [3,S,S] and the TV / smooth-transition / depth-discontinuity sums; its backward
turns dL/d(VGG input) and the three terms' upstream gradients into dL/dpred [cap,3] fp32, which the point-loss node adds to the
criterion's in its one palette-backward launch.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from ..backend import style_backend as _backend

__all__ = ["IMG_TV", "IMG_TV_DEPTH", "IMG_TV_SMOOTH", "IMG_SMOOTH", "IMG_DISC", "IMG_RESIZE", "style_image", "image_blocks",
           "reference_image_terms"]

# include/laenerf.h LAE_STYLE_IMG_*
IMG_TV, IMG_TV_DEPTH, IMG_TV_SMOOTH, IMG_SMOOTH, IMG_DISC, IMG_RESIZE = 1, 2, 4, 8, 16, 32
_TERMS = IMG_TV | IMG_SMOOTH | IMG_DISC


def image_blocks(max_crop_pixels):
    """the fixed workgroup count of the terms' reduction for crops of up to max_crop_pixels pixels (one graph serves every view)"""
    return max(1, min(1024, -(-int(max_crop_pixels) // 256)))


class _style_image(Function):
    @staticmethod
    def forward(ctx, pred32, pred16, es, cap, m_dev, S, flags, n_blocks):
        dev = pred16.device
        vgg_in = torch.empty(3, S, S, dtype=torch.float32, device=dev) if flags & IMG_RESIZE else torch.empty(0, dtype=torch.float32, device=dev)
        terms = torch.empty(3, dtype=torch.float32, device=dev)
        _backend.style_image_forward(es, pred16, cap, m_dev, S, vgg_in if flags & IMG_RESIZE else None, flags, n_blocks, terms)
        ctx.save_for_backward(pred16, m_dev)
        ctx.args = (es, cap, S, flags)
        if not flags & IMG_RESIZE:
            ctx.mark_non_differentiable(vgg_in)
        ctx.set_materialize_grads(False)
        return vgg_in, terms

    @staticmethod
    def backward(ctx, g_vgg, g_terms):
        pred16, m_dev = ctx.saved_tensors
        es, cap, S, flags = ctx.args
        if g_vgg is None:
            flags &= ~IMG_RESIZE
        if g_terms is None:
            flags &= ~(_TERMS | IMG_TV_DEPTH | IMG_TV_SMOOTH)
        g_pred = torch.empty(cap, 3, dtype=torch.float32, device=pred16.device)
        _backend.style_image_backward(es, pred16, cap, m_dev, S, None if g_vgg is None else g_vgg.float().contiguous(),
                                      None if g_terms is None else g_terms.float().contiguous(), flags, g_pred)
        return g_pred, None, None, None, None, None, None, None


def style_image(pred32, pred16, es, cap, m_dev, S, flags, n_blocks):
    """the image terms of the edit set `es`'s current step (the view the sampler drew last, its K in m_dev): pred32 [cap,3] fp32
    (differentiable), pred16 the same values in fp16 -> (vgg_in [3,S,S] fp32 (empty without IMG_RESIZE), terms [3] fp32 = tv, smooth,
    disc)"""
    if es.image is None:
        raise RuntimeError("style_image: the edit set carries no image arrays (EditSet.from_views(..., image_hw=(H, W)))")
    return _style_image.apply(pred32, pred16, es, int(cap), m_dev, int(S), int(flags), int(n_blocks))


def reference_image_terms(pred, indices, box, H, W, cut_gt=None, tv_h=None, tv_v=None, smooth=None, S=256, flags=IMG_TV | IMG_RESIZE):
    """the reference's torch block (nerf/utils.py:999-1033 with editing/style_encoder.py:207-235 and the Resize / Normalize of
    editing/style_network.py) on one view: pred [K,3] (fp16 or fp32) at the flat pixels `indices` of an H x W canvas, crop box
    (x_min, x_max, y_min, y_max) with exclusive upper bounds -> (vgg_in [3,S,S] or None, tv, smooth, disc) as fp32 tensors (0 where
    the flag is off).  smooth: cut_smooth_trans, used in the TV weights only with IMG_TV_SMOOTH (the reference's cut_smooth is None
    unless smooth_trans_weight > 0).  Differentiable in pred."""
    x0, x1, y0, y1 = (int(b) for b in box)
    img = torch.zeros((H, W, 3), dtype=torch.float32, device=pred.device)
    img = img.flatten(0, 1).index_put((indices.long(),), pred.float()).reshape(H, W, 3)
    img = img[x0:x1, y0:y1]
    chw = img.permute(-1, 0, 1)
    zero = torch.zeros((), dtype=torch.float32, device=pred.device)
    vgg_in = None
    if flags & IMG_RESIZE:
        mean = torch.tensor((0.485, 0.456, 0.406), device=pred.device).view(-1, 1, 1)
        std = torch.tensor((0.229, 0.224, 0.225), device=pred.device).view(-1, 1, 1)
        r = F.interpolate(chw[None], size=(S, S), mode="bilinear", align_corners=False, antialias=False)[0]
        vgg_in = (r - mean) / std
    tv = zero
    if flags & IMG_TV:
        dh = torch.pow(chw[:, :-1, :] - chw[:, 1:, :], 2)
        dv = torch.pow(chw[..., :-1] - chw[..., 1:], 2)
        if flags & IMG_TV_DEPTH:
            if flags & IMG_TV_SMOOTH:
                wv = (1 - tv_v) * (1 - smooth[:, 1:])
                wh = (1 - tv_h) * (1 - smooth[1:, :])
            else:
                wv, wh = 1 - tv_v, 1 - tv_h
            tv = torch.sum(dh * wh[None]) + torch.sum(dv * wv[None])
        else:
            tv = torch.sum(dh) + torch.sum(dv)
    sm = zero
    if flags & IMG_SMOOTH:
        sm = (torch.pow(img - cut_gt, 2).sum(-1) * smooth).sum()
    disc = zero
    if flags & IMG_DISC:
        dvv = tv_v / tv_v.max() if tv_v.numel() else tv_v
        dhv = tv_h / tv_h.max() if tv_h.numel() else tv_h
        w_var = torch.pow(chw[:, :-1, :] - chw[:, 1:, :], 2) * dhv[None]
        v_var = torch.pow(chw[..., :-1] - chw[..., 1:], 2) * dvv[None]
        disc = -w_var.sum() - v_var.sum()
    return vgg_in, tv, sm, disc
