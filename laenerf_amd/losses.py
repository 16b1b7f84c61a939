"""Fused training criterion: MSE + loss scaling in one kernel.

    loss = mse_loss_scaled(pred_rgb, gt_rgb, opt)      # opt: FusedAdam (its loss scale) or None
    loss.backward(); opt.step()

`loss` is the SCALED loss (what `GradScaler.scale(loss)` would return); `loss.unscaled` holds the plain MSE for
logging.  Equivalent to the reference's `criterion(pred, gt).mean(-1).mean()` followed by `scaler.scale(...)`
(nerf/utils.py train_step / train_one_epoch).
"""
import torch
from torch.autograd import Function

from . import _lib


class _mse_scaled(Function):
    @staticmethod
    def forward(ctx, pred, target, scale):
        pred = pred.float().contiguous()
        target = target.float().contiguous()
        _lib.need_cuda(pred, target, scale)
        if pred.shape != target.shape:
            raise RuntimeError("mse_loss_scaled: shapes differ")
        out = torch.empty(2, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        _lib.check(_lib.load().lae_mse_loss_forward(pred.data_ptr(), target.data_ptr(), pred.numel(), _lib.ptr(scale),
                                                    out.data_ptr(), grad.data_ptr(), _lib.stream()), "mse_loss_forward")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, grad_out, _):
        if grad_out is None:
            return None, None, None
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None


def loss_scale_of(scaler):
    """the loss scale on the device, a 1-element fp32 tensor or None, of `scaler`: a FusedAdam (its device-side loss scale; None when it
    scales nothing), such a tensor itself, or None"""
    if scaler is None or torch.is_tensor(scaler):
        return scaler
    return scaler._scale_view[:1] if scaler.use_scaler else None


def mse_loss_scaled(pred, target, scaler=None):
    """scaler: a FusedAdam (uses its device-side loss scale), a 1-element fp32 cuda tensor, or None"""
    loss, both = _mse_scaled.apply(pred, target, loss_scale_of(scaler))
    loss.unscaled = both[1]
    return loss


class _colour_scaled(Function):
    @staticmethod
    def forward(ctx, pred, target, scale, kind, param):
        pred = pred.float().contiguous()
        target = target.float().contiguous()
        _lib.need_cuda(pred, target, scale)
        if pred.shape != target.shape:
            raise RuntimeError("colour_loss_scaled: shapes differ")
        out = torch.empty(2, dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(pred)
        _lib.check(_lib.load().lae_colour_loss_forward(pred.data_ptr(), target.data_ptr(), pred.numel(), kind, param, _lib.ptr(scale),
                                                       out.data_ptr(), grad.data_ptr(), _lib.stream()), "colour_loss_forward")
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return out[0], out

    @staticmethod
    def backward(ctx, grad_out, _):
        if grad_out is None:
            return None, None, None, None, None
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None, None


class _patch_pack(Function):
    """lae_patch_pack forward, lae_patch_unpack_grad backward: a patch batch's rows <-> the input of LPIPS' trunk"""

    @staticmethod
    def forward(ctx, pred, gt, P, normalize):
        pred = pred.float().contiguous()
        gt = gt.float().contiguous()
        _lib.need_cuda(pred, gt)
        n = pred.shape[0] // (P * P)
        x = torch.empty(2 * n, 3, P, P, dtype=torch.float32, device=pred.device)
        _lib.check(_lib.load().lae_patch_pack(pred.data_ptr(), gt.data_ptr(), n, P, int(normalize), x.data_ptr(), _lib.stream()),
                   "patch_pack")
        ctx.dims = (n, P, int(normalize))
        return x

    @staticmethod
    def backward(ctx, grad_x):
        n, P, normalize = ctx.dims
        grad_x = grad_x.float().contiguous()
        grad_pred = torch.empty(n * P * P, 3, dtype=torch.float32, device=grad_x.device)
        _lib.check(_lib.load().lae_patch_unpack_grad(grad_x.data_ptr(), n, P, normalize, grad_pred.data_ptr(), _lib.stream()),
                   "patch_unpack_grad")
        return grad_pred, None, None, None


def patch_pack(pred_rows, gt_rows, patch_size, normalize=False):
    """pred_rows / gt_rows [n_patch * P^2, 3] (the rows of a patch batch, ResidentImages.sample(patch_size=P)) -> the trunk's input
    [2 * n_patch, 3, P, P] (image 2p the ground truth, 2p + 1 the prediction) with autograd onto pred_rows"""
    P = int(patch_size)
    if pred_rows.dim() != 2 or pred_rows.shape[1] != 3 or pred_rows.shape != gt_rows.shape or P < 1 or pred_rows.shape[0] % (P * P) \
            or pred_rows.shape[0] == 0:
        raise ValueError("patch_pack: pred_rows and gt_rows must be [n_patch * patch_size^2, 3]")
    return _patch_pack.apply(pred_rows, gt_rows, P, bool(normalize))


def lpips_patch_loss(pred_rows, gt_rows, patch_size, lpips, normalize=False):
    """the reference's perceptual term on a patch batch (nerf/utils.py:594-603): the mean over the patches of
    LPIPS_alex(pred_patch, gt_patch) as an fp32 scalar with autograd onto pred_rows; `.per_patch` holds the float64 distances.
    The chain: lae_patch_pack -> `lpips`' AlexNet trunk through torch autograd (MIOpen) -> lae_lpips_head, and back through
    lae_lpips_head_grad -> the trunk -> lae_patch_unpack_grad: one launch per kernel, no host read, capturable.
    normalize=False is the reference's call ([0, 1] images into lpips with its default normalize=False); True is lpips' documented
    input range.  patch_size >= 32: below it AlexNet's second max-pool has no output."""
    from .metrics import lpips_features, lpips_head
    if int(patch_size) < 32:
        raise ValueError("lpips_patch_loss: patch_size must be at least 32 (below it AlexNet's second max-pool has no output)")
    x = patch_pack(pred_rows, gt_rows, patch_size, normalize)
    d = lpips_head(lpips, lpips_features(lpips, x), both=False)
    out = d.mean().float()
    out.per_patch = d.detach()
    return out


class _ssim_patch(Function):
    """lae_ssim_patch_forward / lae_ssim_patch_backward: the mean over the patches of SSIM(pred patch, gt patch)"""

    @staticmethod
    def forward(ctx, pred, gt, P, data_range):
        pred = pred.float().contiguous()
        gt = gt.float().contiguous()
        _lib.need_cuda(pred, gt)
        n = pred.shape[0] // (P * P)
        per_patch = torch.empty(n, dtype=torch.float64, device=pred.device)
        _lib.check(_lib.load().lae_ssim_patch_forward(pred.data_ptr(), gt.data_ptr(), n, P, data_range, per_patch.data_ptr(),
                                                      _lib.stream()), "ssim_patch_forward")
        ctx.save_for_backward(pred, gt)
        ctx.dims = (n, P, data_range)
        ctx.mark_non_differentiable(per_patch)
        return per_patch.mean().float(), per_patch

    @staticmethod
    def backward(ctx, gout, _):
        n, P, data_range = ctx.dims
        pred, gt = ctx.saved_tensors
        gout = gout.float().contiguous()
        grad_pred = torch.empty_like(pred)
        _lib.check(_lib.load().lae_ssim_patch_backward(pred.data_ptr(), gt.data_ptr(), n, P, data_range, gout.data_ptr(),
                                                       grad_pred.data_ptr(), _lib.stream()), "ssim_patch_backward")
        return grad_pred, None, None, None


def ssim_patch_loss(pred_rows, gt_rows, patch_size, data_range=1.0):
    """the D-SSIM term of a patch batch: 1 - the mean over the patches of SSIM(pred patch, gt patch) (the definition: include/laenerf.h
    above lae_ssim; 11-tap Gaussian windows inside the patch) as an fp32 scalar with autograd onto pred_rows; `.per_patch` holds the
    float64 SSIMs.  pred_rows / gt_rows [n_patch * P^2, 3] as patch_pack takes them; patch_size >= 11; data_range positive (the data's
    own range has no gradient).  One launch forward, one backward, no host read: capturable."""
    P = int(patch_size)
    if P < 11:
        raise ValueError("ssim_patch_loss: patch_size must be at least 11 (the window)")
    if pred_rows.dim() != 2 or pred_rows.shape[1] != 3 or pred_rows.shape != gt_rows.shape or pred_rows.shape[0] % (P * P) \
            or pred_rows.shape[0] == 0:
        raise ValueError("ssim_patch_loss: pred_rows and gt_rows must be [n_patch * patch_size^2, 3]")
    L = float(data_range) if data_range is not None else 0.0
    if not (L > 0.0 and L < float("inf")):
        raise ValueError("ssim_patch_loss: data_range must be a positive finite number")
    mean, per_patch = _ssim_patch.apply(pred_rows, gt_rows.detach(), P, L)
    out = 1.0 - mean
    out.per_patch = per_patch
    return out


def colour_loss_scaled(pred, target, scaler=None, loss="mse", huber_delta=0.1):
    """mse_loss_scaled with the criterion chosen by `loss`: 'mse', 'l1', 'huber' (the reference's loss.py huber_loss =
    torch's HuberLoss(huber_delta) / huber_delta) or 'mape' (loss.py mape_loss), the mean over all elements
    (`lae_colour_loss_forward`).  The same contract: the scaled loss, `loss.unscaled` the plain one; 'mse' gives mse_loss_scaled's bits."""
    from .backend import loss_kind
    kind, param = loss_kind("colour_loss_scaled", loss, huber_delta)
    out, both = _colour_scaled.apply(pred, target, loss_scale_of(scaler), kind, param)
    out.unscaled = both[1]
    return out
