"""Training on posed images, the loop of the reference's `Trainer.train_one_epoch` (nerf/utils.py:1442-1503), with every
16-step group between two occupancy-grid refreshes replayed as ONE captured HIP graph.

Per step: learning rate from a device table -> ray batch (ResidentImages.sample, one kernel) -> occupancy march ->
field + compositing + fused criterion (render_train's second half) -> backward -> FusedAdam.step.  Every 16 steps,
between groups and eagerly: update_extra_state (renderer.py:555-649), with its single host read; `mark_untrained_grid`
once before the first step (nerf/utils.py:752).

What makes a group capturable although the reference changes two host values in it:
  * the march's truncation threshold M = round_up(mean_count, 128) changes at every refresh.  The group is captured with a
    buffer capacity M_cap >= M and reads M from device memory (`m_limit`, lae_march_rays_train_limit), so a graph serves
    every M up to its capacity.  capacity='bucket' rounds M up to 1/8-octave steps (at most 12.5 % padding rows, few
    distinct graphs); 'exact' uses M_cap = M (a new graph for every new M).
  * the learning rate `lr * 0.1 ** min(it / iters, 1)` changes every step.  The schedule is uploaded once (fp64 on the
    host, cast to fp32: the bits FusedAdam.set_lr writes) and each step copies its row into FusedAdam.lrs on the device.
The first 16 steps run eagerly (mean_count = 0: the march sizes its buffers from a host read, as in the reference).
The graphs share one memory pool: they never run concurrently.

error_map='ema' is the reference's --error_map: the batch is drawn by the data's per-image error map
(ResidentImages.sample with a map) and the step's per-ray error is written back into it (ResidentImages.update_error_map)
after the compositing, as train_step does (nerf/utils.py:609-631).  'fixed' is the same draw from a map the caller seeded,
never updated; the reference has no such mode.  LAENeRF's --use_error_maps seeds the map from the edit weights
(nerf/gui.py:419-425) and hands it to the trainer, whose train_step then updates it: that is 'ema' on a seeded map
(laenerf_amd.editing.distill).  Both kernels read and write only device memory, so they run inside the captured group like
the rest of the step.

depth_weight (with a depth plane on the data, ResidentImages.depths) adds the reference's depth supervision
`depth_weight * mean(((depth - (gt_depth - nears)) * (gt_depth > 0))^2)` (nerf/utils.py:585-589, 634-635; 1e-3 during the
distillation) to the step's loss inside the fused compositing kernel, which gathers the plane by the batch's pixel indices: the same
captured 16-step groups, every pointer constant, nothing new on the host inside a group.  depth_grad=True carries the term's gradient
to the densities; the reference's compositing backward drops it (raymarching/raymarching.py:273-275), so there the term changes the
logged loss and nothing else -- depth_grad=False restates that, with parameters bit-equal to a run without depth.

distort_weight adds the distortion regularizer of mip-NeRF 360, `distort_weight * mean over the batch's rays of
(1/3) sum_k delta_k w_k^2 + sum_ij w_i w_j |t_i - t_j|` (the O(n) form of the reference's loss.py eff_distloss, which its CUDA-ray
path never calls; lengths in the march's own units), inside the same kernel and the same captured groups, alone or together with
depth_weight.  distort_grad=False computes the value only: parameters bit-equal to a run without the term.

loss chooses the colour criterion of the same kernel -- 'mse', 'l1', 'huber' (the reference's loss.py huber_loss with huber_delta,
torch-ngp's HuberLoss(beta=0.1) / Instant-NGP's NeRF preset) or 'mape' -- and opacity_weight adds the opacity-entropy regularizer
`opacity_weight * mean over the batch's rays of -(o log2 o + (1 - o) log2(1 - o))`, o = clamp(weights_sum, 1e-5, 1 - 1e-5) (torch-ngp's
lambda_entropy), alone or together with the depth and distortion terms, inside the same captured groups.  opacity_grad=False computes
the value only.  With error_map='ema' the map holds the trained criterion's per-ray mean, the reference's `error = loss.detach()`.

pixel_weights=True (with a weight plane on the data, ResidentImages.pixel_weights) weights every pixel's colour residual,
`mean((w * (pred - gt))^2)`, and second_weight (with ResidentImages.second_target) adds a second colour target,
`second_weight * mean(((1 - w / 2) * (gt2 - pred))^2)` -- the reference's train_step_npr (nerf/utils.py:523-526), and mask- or
confidence-weighted training in general -- inside the same kernel, which gathers both planes by the batch's pixel indices, and the same
captured groups, alone or with the depth, distortion and opacity terms.  MSE only, and not with error_map='ema': the reference's
rule would put the weighted loss into the map, and nothing in the reference does that.

pose_refine=True refines the training cameras by gradient descent inside the same captured groups (Instant-NGP's extrinsics
optimisation; the reference takes its poses as exact).  After the backward, `lae_grid_input_grad` turns the feature gradients the field
backward left into the gradient of the sample positions (the cells are recomputed: no dy_dx buffer), `lae_pose_ray_grad` reduces it per
ray to (sum g, sum (x - o) x g) in fp64 and, after the optimizer's step, `lae_pose_step` adds the rays of every image, takes a sparse
Adam step per image in the world-frame tangent space (skipped with the optimizer's step, divided by its loss scale) and composes it onto
an fp64 master, R <- Exp(dw) R, T <- T + dt, from which the fp32 poses the next batch is built from are rewritten
(ResidentImages.enable_pose_refinement; laenerf_amd/poses.py restates the three kernels).  pose_lr follows the network's decay table.
Not part of the gradient: the view direction, nears / fars and the occupancy decisions of the march.

exposure_refine=True learns a log2 gain per training image and colour channel -- exposure and white balance, Instant-NGP's per-image
exposure; the reference takes every image as shot alike -- inside the same captured groups.  The gain multiplies the TARGET colour in
the sampler (`lae_sample_train_batch_gain`), so the compositing kernels are untouched; every criterion is a function of pred - gt, hence
d loss / d gt = -d loss / d pred, which `lae_exposure_step` recomputes per ray from the step's image and the batch's gt, reduces per image
in fp64 and a fixed order and feeds to a sparse Adam step on an fp64 master (skipped with the optimizer's step); `lae_exposure_publish`
rewrites the fp32 gains the next batch reads as 2^(e - mean over the images): the mean fixes the gauge (a common gain is a brighter
scene), the master is not re-centred, and the -1/n coupling through the mean is left out of the gradient -- a projection after the step
(ResidentImages.enable_exposure_refinement; laenerf_amd/exposure.py restates both kernels).  exposure_lr follows the network's decay
table.  Gains are a physical exposure only on color_space='linear' data; on sRGB data they are a per-image colour compensation.
"""
import contextlib
import copy
import math
import os

import numpy as np
import torch

from .optim import EMA
from .raymarching import raymarching

__all__ = ["Trainer", "lr_schedule", "bucket_capacity", "psnr"]

GROUP = 16                      # update_extra_interval of the reference (main_nerf.py), = the step_counter ring length


def lr_schedule(lr, iters, n_rows, n_groups=1):
    """[n_rows, n_groups] float32: row it = float32(lr * 0.1 ** min(it / iters, 1)) (main_nerf.py:239-245's LambdaLR)"""
    lrs = np.broadcast_to(np.asarray(lr, dtype=np.float64).reshape(-1), (n_groups,))
    it = np.arange(n_rows, dtype=np.float64)
    return np.stack([np.array([float(l) * 0.1 ** min(float(i) / iters, 1.0) for i in it], dtype=np.float64) for l in lrs],
                    axis=1).astype(np.float32)


def round_up_always(m, align=128):
    """the reference's `m += align - m % align` (raymarching.py:125-127)"""
    return m + (align - m % align)


def bucket_capacity(M, align=128):
    """M rounded up to the next of 8 steps per octave (and to `align`): at most 12.5 % of the rows are padding"""
    if M <= 8 * align:
        return -(-M // align) * align
    step = max(align, 1 << (int(M).bit_length() - 1 - 3))
    return -(-M // step) * step


def psnr(pred, gt):
    """PSNRMeter (nerf/utils.py:222): -10 log10(mean squared error)"""
    mse = float(((pred.float() - gt.float()) ** 2).mean())
    return -10.0 * math.log10(max(mse, 1e-20))


def _to_host(obj):
    """a checkpoint's containers with every tensor cloned to the host"""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _to_host(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_host(v) for v in obj)
    return obj


class _TrainerEMA(EMA):
    """the Trainer's EMA of the renderer's parameters (the reference's ema_decay, main_nerf.py:244).  copy_to() and restore()
    re-derive the optimizer's fp16 shadow tables: a graph replay reads them without the version check of an eager forward."""

    def __init__(self, renderer, optimizer, decay):
        super().__init__(renderer.parameters(), decay)
        self._opt = optimizer
        self.device_count()

    def copy_to(self):
        super().copy_to()
        self._opt.sync_shadows()

    def restore(self):
        super().restore()
        self._opt.sync_shadows()


class Trainer:
    """Trainer(renderer, optimizer, data, iters, lr): `optimizer` is a FusedAdam over the renderer's network (its device
    learning rates are taken over: device_lr is switched on), `data` a ResidentImages, `iters` the decay horizon of the
    learning rate, `lr` its start value (one number for every parameter group, or one per group).
    graph=False runs the same steps eagerly; capacity 'bucket' / 'exact' (see the module docstring).
    error_map: None (uniform pixels), 'ema' (drawn by the data's error map, updated after every step) or 'fixed' (drawn by
    it, never updated); a map of ones is created on the data when it has none.
    ema_decay: None (no EMA, nothing added to a step) or the decay of an EMA of the renderer's parameters (`self.ema`), updated
    after every step whose 1-based global index is a multiple of epoch_len (default data.n_img: the reference's epoch of one
    image per batch, nerf/utils.py:1502-1503) by one gated launch inside the captured group; evaluate_one_epoch / test render
    with it swapped in.
    depth_weight: None (no depth term; the step is the one without this argument, bit for bit) or the weight of the depth term, which
    needs data.depths; depth_grad: whether its gradient reaches the densities (False: the reference's value-only behaviour).
    With it losses() holds the total, MSE + depth_weight * depth term, and depth_losses() the per-step depth term without its
    weight: one lae_loss_finish node per step, off the gradient path.
    distort_weight: None (no distortion term; the step is the one without this argument, bit for bit) or the weight of the
    distortion regularizer (module docstring); distort_grad: whether its gradient reaches the densities.  With it losses() holds the
    total and distort_losses() the per-step term without its weight, finished like the depth term's.
    loss: the colour criterion, 'mse' (the step without this argument, bit for bit), 'l1', 'huber' (with huber_delta) or 'mape'; the
    error map follows it.  opacity_weight: None (no term; the step without this argument, bit for bit) or the weight of the
    opacity-entropy regularizer (module docstring); opacity_grad: whether its gradient reaches the densities.  With it losses() holds
    the total and opacity_losses() the per-step term without its weight, finished like the other two.
    pixel_weights: False (the step without this argument, bit for bit) or True: the colour residual of every pixel is multiplied by
    data.pixel_weights (a weight of 0 removes the pixel's colour from the run exactly; a plane of ones is the default run bit for bit).
    second_weight: None (no second term) or the weight of the second colour target data.second_target (module docstring); with it
    losses() holds the total and second_losses() the per-step term without its weight, finished like the others.  Both need
    loss='mse' and are refused with error_map='ema' (ValueError).
    pose_refine: False (every path as it is, bit for bit) or True: the training cameras are refined with learning rate pose_lr (decayed
    like lr; pose_betas / pose_eps are its Adam's) inside the same groups (module docstring); refined_poses() and pose_deltas() report
    them, a checkpoint carries their state (the data's entry), pose_lr=0 leaves the run's losses and parameters bit for bit as without it.
    Needs the renderer's fused_post_ops and the fused field op (ValueError); combines with every other term.
    exposure_refine: False (every path as it is, bit for bit) or True: a log2 gain per training image and channel is learned with learning
    rate exposure_lr (default 1e-2, measured against 1e-3: DESIGN.md 4g; decayed like lr; exposure_betas / exposure_eps are its
    Adam's; exposure_mode 'rgb' or 'gray': three gains or one per image; exposure_center: publish 2^(e - mean) rather than 2^e) inside the same groups (module docstring); exposures() and gains()
    report them, a checkpoint carries their state (the data's entry), exposure_lr=0 leaves the run's losses and parameters bit for bit
    as without it.  Combines with every other term but second_weight, whose second target is synthetic and is not gained (ValueError).
    patch_size: 1 (every path as it is, bit for bit) or P >= 32, the reference's --patch_size: a step trains num_rays // P^2 square patches
    of P x P pixels (ResidentImages.sample(patch_size=P)) on `colour criterion + perceptual_weight * LPIPS_alex(pred patches, gt patches)`
    (nerf/utils.py:594-603), with lpips a metrics.LPIPS (required; its frozen weights are not part of a checkpoint: pass the same object
    again on a resume) and perceptual_normalize lpips' `normalize` flag (False: the reference's call).  The step renders the
    differentiable image (shade_train without gt; the fused criterion kernel is not used) and evaluates losses.colour_loss_scaled and
    losses.lpips_patch_loss on it.  The march's limit is min(N * max_steps, round_up(patch_headroom * the largest per-step sample
    count seen so far, 128)) -- a patch on empty space has no samples, one on the object many, so the mean would truncate -- and the
    steps before any count exists march with force_all_rays.  perceptual_losses() holds the per-step LPIPS mean without its weight,
    truncated_steps() the steps that asked for more samples than their limit, peak_to_mean() the largest count over the mean.  All
    four `loss` kinds and ema_decay work; error_map, depth_weight, distort_weight, opacity_weight, pixel_weights, second_weight,
    pose_refine and exposure_refine are refused (ValueError) before anything is changed on the data.
    ssim_weight: None (every path as it is, bit for bit) or a weight >= 0 of the D-SSIM term `1 - mean over the patches of SSIM(pred
    patch, gt patch)` (losses.ssim_patch_loss, data range 1; the 1 - SSIM that 3DGS-style recipes add to L1) in a patch step, scaled by
    the loss scale like the LPIPS term and inside the same captured groups; ssim_losses() holds the per-step term without its weight.
    With it lpips=None is allowed -- the LPIPS chain is left out, no weights are needed -- and then patch_size >= 11 suffices; with
    both terms the rule stays patch_size >= 32.  Part of a checkpoint's configuration only when set.
    Counters: captures (graphs captured), cache_misses (groups whose capacity had no graph yet), warm_groups (groups run
    eagerly because their capacity exceeded every size run before: library workspaces cannot grow inside a capture)."""

    def __init__(self, renderer, optimizer, data, iters, lr, num_rays=4096, seed=0, graph=True, capacity="bucket",
                 max_steps=1024, dt_gamma=0.0, error_map=None, ema_decay=None, epoch_len=None, depth_weight=None, depth_grad=True,
                 distort_weight=None, distort_grad=True, loss="mse", huber_delta=0.1, opacity_weight=None, opacity_grad=True,
                 pixel_weights=False, second_weight=None, pose_refine=False, pose_lr=1e-3, pose_betas=(0.9, 0.99), pose_eps=1e-15,
                 exposure_refine=False, exposure_lr=1e-2, exposure_mode="rgb", exposure_betas=(0.9, 0.99), exposure_eps=1e-15,
                 exposure_center=True, patch_size=1, perceptual_weight=1e-3, lpips=None, perceptual_normalize=False, patch_headroom=2.0,
                 ssim_weight=None):
        if capacity not in ("bucket", "exact"):
            raise ValueError("Trainer: capacity must be 'bucket' or 'exact'")
        if error_map not in (None, "ema", "fixed"):
            raise ValueError("Trainer: error_map must be None, 'ema' or 'fixed'")
        patch_size = int(patch_size)
        if ssim_weight is not None:                                   # refused before anything is changed on the data
            ssim_weight = raymarching.check_weight("Trainer", "ssim_weight", ssim_weight)
            if patch_size == 1:
                raise ValueError("Trainer: ssim_weight needs patch_size > 1 (the D-SSIM term is a loss on patches)")
            if patch_size < 11:
                raise ValueError("Trainer: ssim_weight needs patch_size >= 11 (SSIM's 11 x 11 window must fit in a patch)")
        if patch_size != 1:                                           # refused before anything is changed on the data
            from .metrics import LPIPS
            if patch_size < 32 and (ssim_weight is None or lpips is not None):
                raise ValueError("Trainer: patch_size must be 1 or at least 32 (below 32 AlexNet's second max-pool has no output, "
                                 "so the LPIPS term does not exist)")
            if not isinstance(lpips, LPIPS) and (ssim_weight is None or lpips is not None):
                raise ValueError("Trainer: patch_size > 1 needs lpips=, a metrics.LPIPS (load_lpips_alex(...) or LPIPS.random(seed))")
            on = {"error_map": error_map is not None or getattr(data, "error_map", None) is not None, "depth_weight": depth_weight is not None,
                  "distort_weight": distort_weight is not None, "opacity_weight": opacity_weight is not None,
                  "pixel_weights": bool(pixel_weights), "second_weight": second_weight is not None, "pose_refine": bool(pose_refine),
                  "exposure_refine": bool(exposure_refine) or getattr(data, "gains", None) is not None}
            bad = [k for k, v in on.items() if v]
            if bad:
                raise ValueError("Trainer: patch_size > 1 cannot be combined with " + ", ".join(bad) + " (they live in or around the fused "
                                 "criterion kernel, which a patch step does not use)")
            if patch_size >= min(data.H, data.W):
                raise ValueError(f"Trainer: patch_size must be smaller than the images ({data.H} x {data.W})")
            if int(num_rays) // (patch_size * patch_size) < 1:
                raise ValueError(f"Trainer: num_rays = {int(num_rays)} holds no patch of {patch_size} x {patch_size} pixels")
            raymarching.check_weight("Trainer", "perceptual_weight", perceptual_weight)
            if not (float(patch_headroom) >= 1.0) or float(patch_headroom) == float("inf"):
                raise ValueError("Trainer: patch_headroom must be finite and >= 1")
            from .backend import loss_kind
            loss_kind("Trainer", loss, huber_delta)
        if pixel_weights or second_weight is not None:                # refused before anything is changed on the data
            from .backend import loss_kind
            loss_kind("Trainer", loss, huber_delta)
            if loss != "mse":
                raise ValueError("Trainer: pixel_weights / second_weight need loss='mse' (the reference has no weighted L1 / Huber / MAPE)")
            if error_map == "ema":
                raise ValueError("Trainer: pixel_weights / second_weight cannot be combined with error_map='ema'")
        if pose_refine:                                               # refused before anything is changed on the data
            if not renderer.fused_post_ops:
                raise ValueError("Trainer: pose_refine needs the renderer's fused_post_ops")
            if not getattr(renderer.model, "fused_field", False) or renderer.model.encoder.interp_id != 0:
                raise ValueError("Trainer: pose_refine needs the fused field op (hash grid with linear interpolation, fused heads)")
            raymarching.check_weight("Trainer", "pose_lr", pose_lr)
        if exposure_refine:                                           # refused before anything is changed on the data
            from .exposure import MODES
            if second_weight is not None:
                raise ValueError("Trainer: exposure_refine cannot be combined with second_weight (the second target is not gained)")
            raymarching.check_weight("Trainer", "exposure_lr", exposure_lr)
            if exposure_mode not in MODES:
                raise ValueError(f"Trainer: exposure_mode must be one of {sorted(MODES)}")
        if error_map is not None and data.error_map is None:
            data.enable_error_map()
        self.r, self.opt, self.data = renderer, optimizer, data
        self.iters, self.num_rays, self.graph, self.capacity = int(iters), int(num_rays), bool(graph), capacity
        self.lr = [float(v) for v in np.asarray(lr, dtype=np.float64).reshape(-1)]
        self.max_steps, self.dt_gamma = int(max_steps), float(dt_gamma)
        self.error_map = error_map
        if depth_weight is not None:
            if getattr(data, "depths", None) is None:
                raise ValueError("Trainer: depth_weight needs a depth plane on the data (ResidentImages(depths=...) / set_depths)")
            depth_weight = raymarching.check_weight("Trainer", "depth_weight", depth_weight)
            if not renderer.fused_post_ops:
                raise ValueError("Trainer: depth supervision needs the renderer's fused_post_ops")
        self.depth_weight, self.depth_grad = depth_weight, bool(depth_grad)
        if distort_weight is not None:
            distort_weight = raymarching.check_weight("Trainer", "distort_weight", distort_weight)
            if not renderer.fused_post_ops:
                raise ValueError("Trainer: the distortion term needs the renderer's fused_post_ops")
        self.distort_weight, self.distort_grad = distort_weight, bool(distort_grad)
        from .backend import loss_kind
        loss_kind("Trainer", loss, huber_delta)
        if opacity_weight is not None:
            opacity_weight = raymarching.check_weight("Trainer", "opacity_weight", opacity_weight)
            if not renderer.fused_post_ops:
                raise ValueError("Trainer: the opacity term needs the renderer's fused_post_ops")
        self.loss, self.huber_delta = loss, float(huber_delta)
        self.opacity_weight, self.opacity_grad = opacity_weight, bool(opacity_grad)
        if pixel_weights or second_weight is not None:
            if pixel_weights and getattr(data, "pixel_weights", None) is None:
                raise ValueError("Trainer: pixel_weights=True needs a weight plane on the data (ResidentImages(pixel_weights=...) / "
                                 "set_pixel_weights)")
            if second_weight is not None:
                second_weight = raymarching.check_weight("Trainer", "second_weight", second_weight)
                if getattr(data, "second_target", None) is None:
                    raise ValueError("Trainer: second_weight needs a second target on the data (ResidentImages(second_target=...) / "
                                     "set_second_target)")
            if not renderer.fused_post_ops:
                raise ValueError("Trainer: pixel weights and a second target need the renderer's fused_post_ops")
        self.pixel_weights, self.second_weight = bool(pixel_weights), second_weight
        # the static part of what a step hands through shade_train to composite_rays_train_blend_mse; _step adds the step's tensors.
        # Every value of a term that is off is that function's default: the call without the term
        self._term_kw = dict(depth_weight=0.0 if depth_weight is None else depth_weight, depth_grad=self.depth_grad,
                             distort_weight=distort_weight, distort_grad=self.distort_grad, loss=loss, huber_delta=self.huber_delta,
                             opacity_weight=opacity_weight, opacity_grad=self.opacity_grad,
                             second_weight=0.0 if second_weight is None else second_weight)
        dev = renderer.density_grid.device
        data.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        data.aabb = renderer.aabb_train.to(dev, torch.float32).contiguous()      # the batch's near / far = the march's
        data.min_near = float(renderer.min_near)
        optimizer.device_lr = True
        n_groups = len(optimizer.param_groups)
        lr_table = lambda base, groups: torch.from_numpy(lr_schedule(base, self.iters, self.iters + 1, groups)).to(dev)
        self.lr_table = lr_table(lr, n_groups)
        self.m_limit = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss_slots = torch.zeros(GROUP, dtype=torch.float32, device=dev)
        # per-step records: name -> (the group's device slots, the history of their copies); the enabled terms of raymarching.TERMS, in
        # its order, hold [GROUP, 2] slots that finish_term_loss writes (column 1 is the record)
        self._records = {"loss": (self.loss_slots, [])}
        weights = {"depth": depth_weight, "distort": distort_weight, "opacity": opacity_weight, "second": second_weight}
        self._records.update({t: (torch.zeros(GROUP, 2, dtype=torch.float32, device=dev), []) for t in raymarching.TERMS
                              if weights[t] is not None})
        self.pose_refine, self.pose_lr = bool(pose_refine), float(pose_lr)
        self.pose_betas, self.pose_eps = (float(pose_betas[0]), float(pose_betas[1])), float(pose_eps)
        if self.pose_refine:
            data.enable_pose_refinement()
            self.pose_lr_table = lr_table(self.pose_lr, 1)
            self.pose_lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
            self._pose_ray_grads = torch.zeros(self.num_rays, 6, dtype=torch.float64, device=dev)
        self.exposure_refine, self.exposure_lr, self.exposure_mode = bool(exposure_refine), float(exposure_lr), exposure_mode
        self.exposure_betas, self.exposure_eps = (float(exposure_betas[0]), float(exposure_betas[1])), float(exposure_eps)
        self.exposure_center = bool(exposure_center)
        if self.exposure_refine:
            data.enable_exposure_refinement(exposure_mode)
            self.exposure_lr_table = lr_table(self.exposure_lr, 1)
            self.exposure_lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.patch_size, self.perceptual_weight = patch_size, float(perceptual_weight)
        self.perceptual_normalize, self.patch_headroom = bool(perceptual_normalize), float(patch_headroom)
        self.lpips = None
        self.skip_perceptual = False             # patch mode only: leave the LPIPS chain out of the step (what perceptual_weight=0 must equal)
        self.n_rays = self.num_rays              # the rays a step trains
        self.perceptual_slots = None
        self.ssim_weight, self.ssim_slots = ssim_weight, None
        if patch_size != 1:
            if lpips is not None:
                self.lpips = lpips.to(dev)
            else:                                # ssim_weight alone: the LPIPS chain is never run
                self.skip_perceptual = True
            if ssim_weight is not None:
                self.ssim_slots = torch.zeros(GROUP, dtype=torch.float32, device=dev)
                self._records["ssim"] = (self.ssim_slots, [])
            self.n_rays = (self.num_rays // (patch_size * patch_size)) * patch_size * patch_size
            self.perceptual_slots = torch.zeros(GROUP, dtype=torch.float32, device=dev)
            self._records["perceptual"] = (self.perceptual_slots, [])
            renderer.count_limit = self.m_limit  # the refresh keeps the largest per-step count and the truncated steps (renderer.py)
        self.global_step = 0
        self.started = False
        self.graphs = {}
        self._pool = None
        self._rows_seen = 0
        self.captures = self.cache_misses = self.warm_groups = 0
        from .checkpoint import new_stats
        self.stats = new_stats()                 # the reference Trainer's stats; 'results' and 'checkpoints' are kept (checkpoints below)
        self.epoch_len = int(epoch_len) if epoch_len is not None else data.n_img
        if self.epoch_len < 1:
            raise ValueError("Trainer: epoch_len must be at least 1")
        self.ema = None if ema_decay is None else _TrainerEMA(renderer, optimizer, float(ema_decay))

    # ------------------------------------------------------------------ one step
    def _sized(self):
        """whether a sample count of earlier steps exists to size the march from (else: a host-sized march)"""
        return self.r.mean_count > 0 if self.patch_size == 1 else self.r.peak_count > 0

    def _all_rows(self):
        return self.n_rays * self.max_steps      # force_all_rays' buffer: no ray can be truncated

    def _m(self):
        if self.patch_size != 1:
            # patch batches differ far more in samples per step than uniform ones (a patch on empty space has none): the limit is
            # patch_headroom times the LARGEST count seen so far, not the mean
            want = int(math.ceil(self.patch_headroom * self.r.peak_count))
            return min(self._all_rows(), -(-want // 128) * 128)
        return round_up_always(self.r.mean_count, 128)

    def _m_cap(self):
        M = self._m()
        return M if self.capacity == "exact" else bucket_capacity(M)

    def _lr_tables(self):
        """(schedule table, the device learning rate a step copies its row into) for the network, the poses and the exposures"""
        tables = [(self.lr_table, self.opt.lrs)]
        if self.pose_refine:
            tables.append((self.pose_lr_table, self.pose_lr_dev))
        if self.exposure_refine:
            tables.append((self.exposure_lr_table, self.exposure_lr_dev))
        return tables

    def _march(self, b, m_cap, force_all_rays=False):
        """the occupancy march of batch b -> xyzs, dirs, deltas, rays.  m_cap None: host-sized, as in the reference (force_all_rays:
        every ray keeps all its samples); else a buffer of m_cap rows whose limit is read from m_limit on the device"""
        r = self.r
        counter = r.step_counter[r.local_step % GROUP]
        counter.zero_()
        r.local_step += 1
        if m_cap is None:
            marched = raymarching.march_rays_train(
                b["rays_o"], b["rays_d"], r.bound, r.density_bitfield, r.cascade, r.grid_size, b["nears"], b["fars"], counter,
                r.mean_count, True, 128, force_all_rays, self.dt_gamma, self.max_steps)
        else:
            marched = raymarching.march_rays_train(
                b["rays_o"], b["rays_d"], r.bound, r.density_bitfield, r.cascade, r.grid_size, b["nears"], b["fars"], counter,
                perturb=True, dt_gamma=self.dt_gamma, max_steps=self.max_steps, m_limit=self.m_limit, capacity=m_cap)
        if not torch.cuda.is_current_stream_capturing():
            self._rows_seen = max(self._rows_seen, marched[0].shape[0])
        return marched

    def _step(self, k, m_cap):
        """one training step (eager or under capture); k = its slot in the group.  m_cap None: host-sized march."""
        r, opt, data = self.r, self.opt, self.data
        with torch.no_grad():
            row = torch.clamp(data.step, max=self.iters)
            for table, dest in self._lr_tables():
                dest.copy_(table.index_select(0, row).view(-1))
        if self.patch_size != 1:
            return self._patch_step(k, m_cap)
        b = data.sample(self.num_rays)
        weights = data.pixel_weights if self.pixel_weights else None
        with torch.autocast("cuda", dtype=torch.float16):
            xyzs, dirs, deltas, rays = self._march(b, m_cap)
            grad_x = torch.empty(xyzs.shape, dtype=torch.float32, device=xyzs.device) if self.pose_refine else None
            res = r.shade_train((xyzs, dirs, deltas, rays, b["nears"], b["fars"]), bg_color=b["bg"], gt=b["gt"], scaler=opt,
                                depth=data.depths if self.depth_weight is not None else None, depth_inds=b["inds"],
                                pixel_weights=weights, pixel_inds=b["inds"],
                                second_target=data.second_target if self.second_weight is not None else None, grad_x=grad_x,
                                **self._term_kw)
        if self.error_map == "ema":
            data.update_error_map(res["image"], b, loss=self.loss, huber_delta=self.huber_delta)
        loss = res["loss"]
        for term in raymarching.TERMS:                                 # the finishing launches in the table's order
            if term in self._records:
                raymarching.finish_term_loss(loss, term, out=self._records[term][0][k])
        opt.backward(loss)
        if self.pose_refine:                                           # grad_x holds d (scaled loss) / d xyzs now
            data.pose_ray_grad(rays, xyzs, grad_x, b["rays_o"], out=self._pose_ray_grads)
        opt.step()
        if self.pose_refine:                                           # after the step: its skip decision and 1 / scale are in the state words
            data.pose_step(self._pose_ray_grads, b["inds"], opt.dev_state, self.pose_lr_dev, self.pose_betas, self.pose_eps)
        if self.exposure_refine:                                       # likewise after the step; the analytic gradient needs no 1 / scale
            data.exposure_step(res["image"], b, opt.dev_state, self.exposure_lr_dev, loss=self.loss, huber_delta=self.huber_delta,
                               pixel_weights=weights, betas=self.exposure_betas, eps=self.exposure_eps, center=self.exposure_center)
        if self.ema is not None:
            self.ema.update_gated(data.step, self.epoch_len)           # sample() has advanced the counter to this step's index
        with torch.no_grad():
            self.loss_slots[k].copy_(loss.unscaled.view(()))

    def _patch_step(self, k, m_cap):
        """_step with patch_size > 1: a patch batch, the differentiable image of composite_rays_train_blend (shade_train without gt),
        then colour criterion + perceptual_weight * LPIPS on the patches (losses.lpips_patch_loss), operator by operator"""
        from .losses import colour_loss_scaled, lpips_patch_loss
        r, opt = self.r, self.opt
        b = self.data.sample(self.n_rays, patch_size=self.patch_size)
        with torch.autocast("cuda", dtype=torch.float16):
            xyzs, dirs, deltas, rays = self._march(b, m_cap, force_all_rays=True)      # no count yet: every ray keeps all its samples
            res = r.shade_train((xyzs, dirs, deltas, rays, b["nears"], b["fars"]), bg_color=b["bg"])
        image = res["image"]
        loss = colour_loss_scaled(image, b["gt"], opt, self.loss, self.huber_delta)
        total = loss.unscaled
        if not self.skip_perceptual:
            lp = lpips_patch_loss(image, b["gt"], self.patch_size, self.lpips, self.perceptual_normalize)
            term = self.perceptual_weight * lp
            total = total + term.detach()
            loss = loss + (term * opt._scale_view[0] if opt.use_scaler else term)
            with torch.no_grad():
                self.perceptual_slots[k].copy_(lp.detach())
        if self.ssim_weight is not None:
            from .losses import ssim_patch_loss
            ds = ssim_patch_loss(image, b["gt"], self.patch_size)
            term = self.ssim_weight * ds
            total = total + term.detach()
            loss = loss + (term * opt._scale_view[0] if opt.use_scaler else term)
            with torch.no_grad():
                self.ssim_slots[k].copy_(ds.detach())
        opt.backward(loss)
        opt.step()
        if self.ema is not None:
            self.ema.update_gated(self.data.step, self.epoch_len)
        with torch.no_grad():
            self.loss_slots[k].copy_(total.view(()))

    def _refresh(self):
        with torch.autocast("cuda", dtype=torch.float16):
            self.r.update_extra_state()

    # ------------------------------------------------------------------ groups
    def _run_group(self, m_cap):
        g = self.graphs.get(m_cap)
        if g is None:
            self.cache_misses += 1
            if m_cap > self._rows_seen:
                # the encoder / MLP workspaces may have to grow to m_cap rows, which is refused inside a capture: this group
                # runs eagerly (the same kernels, hence the same bits) and the next one with this capacity is captured
                self.warm_groups += 1
                for k in range(GROUP):
                    self._step(k, m_cap)
                self._rows_seen = max(self._rows_seen, m_cap)
                return
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool):
                for k in range(GROUP):
                    self._step(k, m_cap)
            if self._pool is None:
                self._pool = g.pool()
            self.graphs[m_cap] = g
            self.captures += 1
        g.replay()
        self.r.local_step = GROUP

    def train(self, n_steps):
        """n_steps steps of the reference's loop (refresh every 16 global steps, before the step)"""
        r = self.r
        if not self.started:
            r.mark_untrained_grid(self.data.poses, self.data.intrinsics)
            self.data.step.fill_(self.global_step)
            self.started = True
        r.model.train()
        done = 0
        while done < n_steps:
            if self.global_step % GROUP == 0:
                self._refresh()
            pos = self.global_step % GROUP
            sized = self._sized()
            if sized:
                self.m_limit.fill_(self._m())
            elif self.patch_size != 1:
                self.m_limit.fill_(self._all_rows())                   # what a force_all_rays step marches under
            if self.graph and sized and pos == 0 and n_steps - done >= GROUP:
                self._run_group(self._m_cap())
                n = GROUP
            else:
                self._step(pos, self._m_cap() if sized else None)
                n = 1
            for slots, hist in self._records.values():
                hist.append((slots[pos:pos + n] if slots.dim() == 1 else slots[pos:pos + n, 1]).clone())
            done += n
            self.global_step += n
        return self

    # ------------------------------------------------------------------ results
    # the accessors of every per-step record (a resume's test compares them all)
    RECORDS = ("losses", "depth_losses", "distort_losses", "opacity_losses", "second_losses", "perceptual_losses", "ssim_losses")

    def _record(self, name):
        """the history of per-step record `name` as a float32 numpy array; empty when this trainer does not keep it"""
        _, hist = self._records.get(name, (None, None))
        return torch.cat(hist).cpu().numpy() if hist else np.zeros(0, np.float32)

    def losses(self):
        """per-step losses (the unscaled loss of every step so far: the colour criterion's mean -- the MSE under loss='mse', else the
        mean of the L1 / Huber / MAPE element loss --, plus depth_weight * the depth term with depth supervision, plus distort_weight *
        the distortion term and opacity_weight * the opacity entropy with them) as a float32 numpy array.  After load_checkpoint /
        load_state_dict: the steps since the resume (the history is not part of a checkpoint); likewise depth_losses(),
        distort_losses() and opacity_losses()"""
        return self._record("loss")

    def depth_losses(self):
        """per-step depth term mean(((depth - (gt_depth - nears)) * (gt_depth > 0))^2), without its weight, as a float32 numpy
        array (empty without depth supervision).  Each step finishes it with one lae_loss_finish node off the gradient path."""
        return self._record("depth")

    def distort_losses(self):
        """per-step distortion term L_dist (the batch's mean of l_ray), without its weight, as a float32 numpy array (empty without
        distort_weight).  Each step finishes it with one lae_loss_finish node off the gradient path."""
        return self._record("distort")

    def opacity_losses(self):
        """per-step opacity entropy L_op (the batch's mean of h(weights_sum)), without its weight, as a float32 numpy array (empty
        without opacity_weight).  Each step finishes it with one lae_loss_finish node off the gradient path."""
        return self._record("opacity")

    def second_losses(self):
        """per-step second colour term mean(((1 - w / 2) * (second_target - pred))^2), without its weight, as a float32 numpy array
        (empty without second_weight).  Each step finishes it with one lae_loss_finish node off the gradient path."""
        return self._record("second")

    def perceptual_losses(self):
        """per-step LPIPS term (the mean over the step's patches), without its weight, as a float32 numpy array (empty without
        patch_size > 1; zeros for steps run with skip_perceptual)"""
        return self._record("perceptual")

    def ssim_losses(self):
        """per-step D-SSIM term (1 - the mean over the step's patches of SSIM), without its weight, as a float32 numpy array (empty
        without ssim_weight)"""
        return self._record("ssim")

    def truncated_steps(self):
        """patch mode: the number of steps so far whose requested sample count exceeded the limit they marched under, so that rays
        inside patches lost samples (0 is what patch_headroom is chosen for); from the step counters: the groups already refreshed
        were counted with the refresh's host read, the steps since then cost one read here.  Always 0 without patch_size > 1."""
        if self.patch_size == 1:
            return 0
        r = self.r
        n = min(GROUP, r.local_step)
        tail = int((r.step_counter[:n, 0] > self.m_limit).sum().item()) if n > 0 else 0
        return int(r.truncated_steps) + tail

    def peak_to_mean(self):
        """patch mode: the largest per-step sample count seen so far over the last refresh's mean count (0.0 before either exists)"""
        r = self.r
        return float(r.peak_count) / float(r.mean_count) if self.patch_size != 1 and r.mean_count > 0 else 0.0

    def refined_poses(self):
        """the training cameras as the next batch reads them, [n_img, 4, 4] fp32 on the device (a copy; data.poses without pose_refine)"""
        d = self.data
        return (d.poses if d.train_poses is None else d.train_poses).clone()

    def pose_deltas(self):
        """(rotation angle in radians [n_img], translation distance [n_img]) of the refined cameras against data.poses, as float64
        numpy arrays (from the fp64 master with pose_refine; zeros without)"""
        from .poses import pose_error
        d = self.data
        ref = d.poses.detach().cpu().numpy().astype(np.float64)
        cur = ref if d.pose_master is None else d.pose_master.detach().cpu().numpy().reshape(d.n_img, 3, 4)
        return pose_error(cur, ref)

    def exposures(self):
        """the log2 gains of the training images as published, master - mean over the images (the master itself with
        exposure_center=False), as a float64 numpy array [n_img, 3]; zeros without exposure_refine"""
        d = self.data
        if d.exposure_master is None:
            return np.zeros((d.n_img, 3))
        from .exposure import exposure_publish_numpy
        return exposure_publish_numpy(d.exposure_master.detach().cpu().numpy(), center=self.exposure_center, full=True)[1]

    def gains(self):
        """the gains the next batch's targets are multiplied by, [n_img, 3] fp32 on the device (a copy; ones without exposure_refine)"""
        d = self.data
        return torch.ones(d.n_img, 3, dtype=torch.float32, device=d.images.device) if d.gains is None else d.gains.clone()

    @property
    def steps_skipped(self):
        """optimizer steps the GradScaler skipped (non-finite gradients)"""
        return self.opt.steps_skipped

    # ------------------------------------------------------------------ checkpoints
    def config(self, model_only=False):
        """the run configuration a checkpoint is checked against (checkpoint.check_config); model_only: the renderer's part alone"""
        d, r = self.data, self.r
        rend = {"bound": r.bound, "grid_size": int(r.grid_size), "density_thresh": float(r.density_thresh), "min_near": float(r.min_near),
                "density_scale": r.density_scale}
        if model_only:
            return {"renderer": rend}
        cfg = {"iters": self.iters, "lr": list(self.lr), "num_rays": self.num_rays, "capacity": self.capacity, "max_steps": self.max_steps,
               "dt_gamma": self.dt_gamma, "error_map": self.error_map, "ema_decay": None if self.ema is None else float(self.ema.decay),
               "epoch_len": self.epoch_len, "depth_weight": self.depth_weight, "depth_grad": self.depth_grad,
               "distort_weight": self.distort_weight, "distort_grad": self.distort_grad,
               "data": {"n_img": d.n_img, "H": d.H, "W": d.W, "C": d.C, "mode": d.mode, "bg": d.bg, "color_space": d.color_space},
               "renderer": rend}
        # the criterion's keys only where they differ from the defaults: check_config counts a key missing on one side as a difference,
        # and files written before these arguments existed -- and a default trainer's file -- stay as they were
        if self.loss != "mse":
            cfg["loss"] = self.loss
            if self.loss == "huber":
                cfg["huber_delta"] = self.huber_delta
        if self.opacity_weight is not None:
            cfg["opacity_weight"], cfg["opacity_grad"] = self.opacity_weight, self.opacity_grad
        if self.pixel_weights:
            cfg["pixel_weights"] = True
        if self.second_weight is not None:
            cfg["second_weight"] = self.second_weight
        if self.pose_refine:
            cfg["pose_refine"], cfg["pose_lr"] = True, self.pose_lr
            cfg["pose_betas"], cfg["pose_eps"] = list(self.pose_betas), self.pose_eps
        if self.exposure_refine:
            cfg["exposure_refine"], cfg["exposure_lr"], cfg["exposure_mode"] = True, self.exposure_lr, self.exposure_mode
            cfg["exposure_betas"], cfg["exposure_eps"] = list(self.exposure_betas), self.exposure_eps
            cfg["exposure_center"] = self.exposure_center
        if self.patch_size != 1:
            cfg["patch_size"], cfg["perceptual_weight"] = self.patch_size, self.perceptual_weight
            cfg["perceptual_normalize"], cfg["patch_headroom"] = self.perceptual_normalize, self.patch_headroom
            if self.ssim_weight is not None:         # only when set: files written without it stay as they were
                cfg["ssim_weight"] = self.ssim_weight
        return cfg

    def state_dict(self, full=True):
        """everything save_checkpoint writes, on the host: the reference Trainer's dict (nerf/utils.py:1631-1655: epoch = global_step //
        epoch_len, global_step, stats, mean_count, mean_density, model in the reference's key layout; with `full` also optimizer in
        torch.optim.Adam's layout, lr_scheduler as a LambdaLR dict, scaler in GradScaler's layout and ema in torch_ema's) plus the
        entry `laenerf_amd` with what a bit-exact resume needs beyond it: a format number, lae_version(), config(), the
        tensor shapes, the renderer's iter_density and local_step, the data's seed, step and error map, the device's generator state
        (the march's perturbation and the refresh's jitter are torch.rand draws) and, with `full`, the optimizer's sixteen state
        words and the EMA's device count.  The touched-lines bitmaps are not written: load marks every line touched, which is exact
        (a line whose gradient and moments are zero is left unchanged by the update)."""
        from . import _lib, checkpoint as C
        r, opt = self.r, self.opt
        dev = r.density_grid.device
        model = _to_host(dict(r.state_dict(reference_layout=True)))
        sd = {"epoch": self.global_step // self.epoch_len, "global_step": self.global_step, "stats": copy.deepcopy(self.stats),
              "mean_count": int(r.mean_count), "mean_density": r.mean_density, "model": model}
        extra = {"format": C.FORMAT, "lae_version": _lib.load().lae_version().decode(), "config": self.config(),
                 "shapes": C.shapes_of(model, "model."), "iter_density": int(r.iter_density), "local_step": int(r.local_step),
                 "data": self.data.state_dict(), "rng_state": torch.cuda.get_rng_state(dev).clone(), "touched_lines": None}
        if self.patch_size != 1:                     # the march's size follows the largest count seen (only with patches: other files stay)
            extra["patch"] = {"peak_count": int(r.peak_count), "truncated_steps": int(r.truncated_steps)}
        if full:
            o = opt.state_dict()
            sc = o.pop("scaler")
            sd["optimizer"] = _to_host(o)
            base = self.lr if len(self.lr) > 1 else self.lr * len(opt.param_groups)
            sd["lr_scheduler"] = C.scheduler_to_reference(self.global_step, base, self.iters)
            sd["scaler"] = C.scaler_to_reference(sc["scale"], sc["growth_tracker"], opt.growth_factor, opt.backoff_factor,
                                                 opt.growth_interval) if opt.use_scaler else {}
            extra["optimizer_words"] = opt.raw_state()
            if self.ema is not None:
                sd["ema"] = _to_host(self.ema.state_dict())
                extra["ema_count"] = self.ema.device_count().detach().cpu().clone()
        sd[C.KEY] = extra
        return sd

    def _check_load(self, ck, model_only):
        """-> the differences [(name, saved, current)] between the checkpoint dict and this trainer; nothing is changed"""
        from . import checkpoint as C
        if not isinstance(ck, dict) or not isinstance(ck.get("model"), dict):
            raise ValueError("Trainer.load_checkpoint: not a Trainer checkpoint (a dict with a 'model' entry expected)")
        extra = ck.get(C.KEY)
        diffs = []
        if extra is not None:
            if int(extra.get("format", 0)) > C.FORMAT:
                raise ValueError(f"Trainer.load_checkpoint: checkpoint format {extra.get('format')} is newer than this package's {C.FORMAT}")
            saved_cfg = extra["config"] if not model_only else {"renderer": extra["config"]["renderer"]}
            diffs += C.check_config(saved_cfg, self.config(model_only))
        cur = C.shapes_of(dict(self.r.state_dict(reference_layout=True)), "model.")
        saved = C.shapes_of(ck["model"], "model.")
        for k in sorted(set(cur) | set(saved)):
            if k in cur and k in saved:
                if cur[k] != saved[k]:
                    diffs.append((k, saved[k], cur[k]))
            elif extra is not None and k != "model.density_grid":          # own files are complete, but for the grid of a `best` file;
                diffs.append((k, saved.get(k, "<missing>"), cur.get(k, "<missing>")))   # reference files load with strict=False
        if self.ema is not None and "ema" in ck:
            sh = ck["ema"].get("shadow_params") or []
            want = [list(p.shape) for p in self.ema.shadow_params]
            if [list(t.shape) for t in sh] != want:
                diffs.append(("ema.shadow_params", [list(t.shape) for t in sh], want))
            cnt = None if extra is None else extra.get("ema_count")
            if cnt is not None and (not torch.is_tensor(cnt) or cnt.numel() != 2):
                diffs.append(("ema.count", "malformed", [2]))
        if model_only:
            return diffs
        if "optimizer" in ck:
            st = ck["optimizer"].get("state", {})
            groups = ck["optimizer"].get("param_groups", [])
            want_groups = [len(g["params"]) for g in self.opt.param_groups]
            if [len(g.get("params", [])) for g in groups] != want_groups:
                diffs.append(("optimizer.param_groups", [len(g.get("params", [])) for g in groups], want_groups))
            elif sorted(st) != list(range(len(self.opt.items))):
                diffs.append(("optimizer.state", sorted(st), list(range(len(self.opt.items)))))
            else:
                for i, (p, *_) in enumerate(self.opt.items):
                    for key in ("exp_avg", "exp_avg_sq"):
                        t = st[i].get(key)
                        if not torch.is_tensor(t) or list(t.shape) != list(p.shape):
                            diffs.append((f"optimizer.state.{i}.{key}", list(t.shape) if torch.is_tensor(t) else "<missing>", list(p.shape)))
        if extra is not None:
            w = extra.get("optimizer_words")
            if w is not None and (not torch.is_tensor(w) or w.dtype != torch.int32 or w.numel() != 16):
                diffs.append(("optimizer_words", "malformed", [16]))
            diffs += [("data", msg, "") for msg in self.data.check_state_dict(extra["data"])]
            rng = extra.get("rng_state")
            n_rng = int(torch.cuda.get_rng_state(self.r.density_grid.device).numel())
            if not torch.is_tensor(rng) or rng.dtype != torch.uint8 or rng.numel() != n_rng:
                diffs.append(("rng_state", "malformed", [n_rng]))
        return diffs

    @torch.no_grad()
    def load_state_dict(self, ck, model_only=False, strict_config=True):
        """state_dict()'s counterpart.  The whole dict is checked against this trainer first -- the run configuration and every tensor
        shape (checkpoint.check_config) -- and a refused load leaves the trainer exactly as it was: with strict_config a difference
        raises ValueError naming the fields; without it a warning is issued and what fits is loaded (fine-tuning with another
        num_rays).  Then everything listed at state_dict() is restored in place, what is derived is re-derived (the fp16 shadow
        tables, the bitfield from the grid when the file has none, m_limit), the captured graphs are dropped (the next group is
        captured afresh) and `started` is set, so mark_untrained_grid does not run over a trained grid.  The trainer may have trained
        before.  losses() / depth_losses() / distort_losses() of a resumed trainer hold the steps since the resume.
        A file without the `laenerf_amd` entry, as the reference's save_checkpoint writes it, restores what it has as the reference
        does: the model through strict=False, mean_count and mean_density, a torch.optim.Adam state, a GradScaler state, a torch_ema
        state, global_step (also the data's step) and stats; iter_density becomes global_step // 16 and local_step 0.  Such a resume
        is not bit-exact: the file carries neither the generator state nor the sampler's seed.
        model_only=True restores the model, the two means and the EMA shadows: enough for evaluate*, test, save_mesh and the editing
        stages."""
        import warnings
        from . import checkpoint as C
        diffs = self._check_load(ck, model_only)
        if diffs:
            if strict_config:
                raise ValueError("Trainer.load_checkpoint: the checkpoint does not fit this trainer -- " + C.format_differences(diffs))
            warnings.warn("Trainer.load_checkpoint: loading what fits -- " + C.format_differences(diffs))
        bad = {n for n, _, _ in diffs}
        skip = lambda prefix: any(n == prefix or n.startswith(prefix + ".") for n in bad)
        r, opt = self.r, self.opt
        extra = ck.get(C.KEY)
        cur = C.shapes_of(dict(r.state_dict(reference_layout=True)), "model.")
        model = {k: v for k, v in ck["model"].items() if "model." + k not in bad and "model." + k in cur}
        r.load_state_dict(model, strict=False)                               # in place; the fp16 shadow tables follow
        opt.sync_shadows()
        r.mean_count = int(ck.get("mean_count", r.mean_count))
        r.mean_density = ck.get("mean_density", r.mean_density)
        if "density_bitfield" not in model and "density_grid" in model:
            r.density_bitfield = raymarching.packbits(r.density_grid, min(r.mean_density, r.density_thresh), r.density_bitfield)
        if self.ema is not None and "ema" in ck and not skip("ema"):
            self.ema.load_state_dict(ck["ema"])
            if extra is not None and extra.get("ema_count") is not None:
                self.ema.device_count().copy_(extra["ema_count"].to(self.ema.device_count().device))
        if model_only:
            return self
        if "optimizer" in ck and not skip("optimizer"):
            o = dict(ck["optimizer"])
            sc = C.scaler_from_reference(ck.get("scaler") or {})
            if sc is not None and opt.use_scaler:
                o["scaler"] = {"scale": sc["scale"], "growth_tracker": sc["growth_tracker"]}
            opt.load_state_dict(o)                                           # moments in place, step count, every line touched
            if extra is not None and extra.get("optimizer_words") is not None and not skip("optimizer_words"):
                opt.load_raw_state(extra["optimizer_words"])
        self.global_step = int(ck.get("global_step", 0))
        if isinstance(ck.get("stats"), dict):
            self.stats = {**C.new_stats(), **copy.deepcopy(ck["stats"])}
        if extra is not None:
            r.iter_density, r.local_step = int(extra["iter_density"]), int(extra["local_step"])
            if not skip("data"):
                self.data.load_state_dict(extra["data"])
            if not skip("rng_state"):
                torch.cuda.set_rng_state(extra["rng_state"], r.density_grid.device)
        else:
            r.iter_density, r.local_step = self.global_step // GROUP, 0
            self.data.step.fill_(self.global_step)
        if self.patch_size != 1 and extra is not None and isinstance(extra.get("patch"), dict):
            r.peak_count, r.truncated_steps = int(extra["patch"]["peak_count"]), int(extra["patch"]["truncated_steps"])
        if self._sized():
            self.m_limit.fill_(self._m())
        elif self.patch_size != 1:
            self.m_limit.fill_(self._all_rows())
        self.graphs = {}
        self._pool = None
        for _, hist in self._records.values():
            hist.clear()
        self.started = True
        return self

    def save_checkpoint(self, path_or_dir, name="ngp", full=True, best=False, remove_old=True, max_keep_ckpt=2):
        """write state_dict(full) with checkpoint.atomic_save, blocking, between train() calls -> the path written (None when a `best`
        save had nothing to write).  path_or_dir: a `.pth` path, or a directory, where the file is `{name}_ep{epoch:04d}.pth` and
        (remove_old) stats['checkpoints'] keeps the newest max_keep_ckpt files, the older ones being removed (nerf/utils.py:1659-1665).
        full: the reference's flag -- optimizer, scheduler, scaler and EMA are written only with it; a file without them restores the
        model and the counters, not an exact resume.
        best=True (nerf/utils.py:1669-1689): written (to `{name}.pth` in a directory) only when stats['results'][-1] improves on
        stats['best_result'] (lower is better: evaluate_one_epoch appends a mean squared error), with the EMA weights swapped in for the
        write and restored after, and without density_grid."""
        from . import checkpoint as C
        path, in_dir = C.resolve_path(path_or_dir, name, self.global_step // self.epoch_len, best=best)
        if best:
            res = self.stats["results"]
            if not res or (self.stats["best_result"] is not None and not res[-1] < self.stats["best_result"]):
                return None
            self.stats["best_result"] = res[-1]
            if self.ema is not None:
                self.ema.store()
                self.ema.copy_to()
            try:
                sd = self.state_dict(full)
            finally:
                if self.ema is not None:
                    self.ema.restore()
            del sd["model"]["density_grid"]
            del sd[C.KEY]["shapes"]["model.density_grid"]
            return C.atomic_save(sd, path)
        if in_dir and remove_old:
            C.rotate(self.stats, path, max_keep_ckpt)
        return C.atomic_save(self.state_dict(full), path)

    def load_checkpoint(self, path_or_dir=None, name="ngp", model_only=False, strict_config=True, trusted=False):
        """read a checkpoint file and load_state_dict it (see there for what is checked and restored).  path_or_dir: a file; a
        directory, or None for the current one, means its latest `{name}_ep*.pth` (the reference's sorted-glob rule, --ckpt latest).
        The file is read with torch.load(weights_only=True); trusted=True switches to a full unpickle, for reference files that
        carry other objects."""
        from . import checkpoint as C
        path = "." if path_or_dir is None else os.fspath(path_or_dir)
        if os.path.isdir(path):
            found = C.latest_checkpoint(path, name)
            if found is None:
                raise FileNotFoundError(f"Trainer.load_checkpoint: no {name}_ep*.pth in {path!r}")
            path = found
        return self.load_state_dict(C.read_checkpoint(path, trusted=trusted), model_only=model_only, strict_config=strict_config)

    def save_mesh(self, path, resolution=256, threshold=10, normals=False, colors=False, keep_largest=False, min_component=None,
                  min_component_fraction=None, **kwargs):
        """nerf/utils.py:722-741: the renderer's mesh as a binary PLY; normals / colors add per-vertex attributes; keep_largest /
        min_component / min_component_fraction drop floaters (connected components of the density lattice) before marching cubes;
        simplify=<cell in lattice spacings> (a keyword of NeRFRenderer.save_mesh) simplifies the mesh on the device"""
        if keep_largest or min_component is not None or min_component_fraction is not None:
            kwargs.update(keep_largest=keep_largest, min_component=min_component, min_component_fraction=min_component_fraction)
        if not normals and not colors:
            return self.r.save_mesh(path, resolution=resolution, threshold=threshold,
                                    **{k: v for k, v in kwargs.items() if k in ("keep_largest", "min_component", "min_component_fraction", "simplify")})
        return self.r.save_mesh(path, resolution=resolution, threshold=threshold, normals=normals, colors=colors, **kwargs)

    def save_mesh_tsdf(self, path, data=None, frames=None, **kwargs):
        """the surface the renders show as a binary PLY with normals and colours (NeRFRenderer.save_mesh_tsdf; DESIGN.md section
        4h): the views of `data` (a ResidentImages; default the training data) are rendered with the EMA weights, fused into a
        truncated signed distance field and meshed at zero.  frames: [n, H, W, 3] uint8 or fp32 on the device in the data's
        camera order (recolor_views(...), tr.test(...)[0], ...) -- their colours are baked into the vertices, so a palette edit
        or a stylization leaves as a mesh without being distilled first; None bakes the model's own renders.  kwargs:
        resolution, trunc_voxels, min_views, normals, colors, keep_largest, ... of NeRFRenderer.extract_mesh_tsdf."""
        data = self.data if data is None else data
        with self._eval_weights():
            return self.r.save_mesh_tsdf(path, data.poses, data.intrinsics, data.H, data.W, frames=frames, **kwargs)

    def save_mesh_textured(self, path, data=None, frames=None, **kwargs):
        """the mesh as `name.obj` + `name.mtl` + `name.png` with a per-triangle texture atlas (NeRFRenderer.save_mesh_textured;
        DESIGN.md section 4h), with the EMA weights.  The cameras of `data` (a ResidentImages; default the training data) serve
        source="views" and geometry="tsdf"; frames: [n, H, W, 3] uint8 or fp32 on the device in the data's camera order
        (recolor_views(...), tr.test(...)[0], ...) are baked into the texture with source="views" -- a palette edit or a
        stylization leaves with its detail; None bakes the model's own renders.  kwargs: resolution, cell, texture_size, source,
        geometry, min_cos, fallback, keep_largest, ... of NeRFRenderer.extract_mesh_textured."""
        data = self.data if data is None else data
        with self._eval_weights():
            return self.r.save_mesh_textured(path, poses=data.poses, intrinsics=data.intrinsics, H=data.H, W=data.W, frames=frames, **kwargs)

    @torch.no_grad()
    def evaluate(self, views, data=None, bg_color=1.0):
        """mean PSNR over `views` (image indices of `data`, default the training set) rendered with render_eval over a plain
        background `bg_color` (the ground truth is blended over the same background)"""
        data = self.data if data is None else data
        r = self.r
        was_training = r.model.training
        r.model.eval()
        vals = []
        try:
            for i in views:
                o, d, img = data.view_rays(int(i))
                if img.shape[-1] == 4:
                    a = img[:, 3:]
                    gt = img[:, :3] * a + bg_color * (1 - a)
                else:
                    gt = img
                with torch.autocast("cuda", dtype=torch.float16):
                    pred = r.render_eval(o, d, bg_color=bg_color, image_hw=(data.H, data.W))["image"]
                vals.append(psnr(pred.reshape(-1, 3), gt))
        finally:
            r.model.train(was_training)
        return float(np.mean(vals))

    @contextlib.contextmanager
    def _eval_weights(self):
        """the model in eval mode with the EMA weights swapped in (nerf/utils.py:1539-1541), both undone afterwards"""
        r = self.r
        was_training = r.model.training
        if self.ema is not None:
            self.ema.store()
            self.ema.copy_to()
        r.model.eval()
        try:
            yield
        finally:
            r.model.train(was_training)
            if self.ema is not None:
                self.ema.restore()

    def _render_view(self, data, i, scale_depth):
        """eval_step / test_step's render of view i (bg_color 1, perturb False) -> image [HW,3], depth [HW] fp32"""
        from .rays import get_rays
        if data.color_space == "linear":
            raise NotImplementedError("Trainer: color_space='linear' data is not supported here (every shipped config uses srgb)")
        ray = get_rays(data.poses[i:i + 1], data.intrinsics, data.H, data.W)
        with torch.autocast("cuda", dtype=torch.float16):
            res = self.r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=scale_depth,
                                     image_hw=(data.H, data.W))
        return res["image"].float().contiguous(), res["depth"].float().contiguous()

    @staticmethod
    def _write_pngs(out_dir, name, i, rgb_u8, depth_u8):
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        Image.fromarray(rgb_u8.cpu().numpy()).save(os.path.join(out_dir, f"{name}_{i:04d}_rgb.png"))
        Image.fromarray(depth_u8.cpu().numpy()).save(os.path.join(out_dir, f"{name}_{i:04d}_depth.png"))

    @torch.no_grad()
    def evaluate_one_epoch(self, data, lpips=None, masks=None, out_dir=None, name="ngp", ssim=False, ssim_data_range=None):
        """the reference's evaluate_one_epoch (nerf/utils.py:1526-1624, eval_step :674-698) over every view of `data` (a
        ResidentImages): rendered with the EMA weights over white, scale_depth=False; per view one lae_eval_view pass (PSNRMeter's
        squared error into a device slot; with `lpips` (metrics.LPIPS) its input, then the trunk and the head; with `masks` (a list
        of uint8 [H, W] or None per view, metrics.load_masks) eval_masked's MSE); one host read for the whole split.  out_dir:
        `{name}_{i:04d}_rgb.png` / `_depth.png` (uint8, clipped).  -> dict psnr [n], lpips [n] or None, masked_mse [n] (NaN where
        a view has no mask) or None, mean_psnr, mean_lpips, mean_masked_mse (over the views with a mask), ssim [n] or None, mean_ssim.
        ssim=True: the reference's SSIMMeter (nerf/utils.py:259-293) -- eval_view also writes the blended ground truth and one
        metrics.ssim call per view scores it against the render into a device slot, read with the same host read; ssim_data_range None is
        the reference's call (the range of each view's own pair), else a positive number.  ssim=False launches and allocates nothing new.
        Also appends the mean squared error over the evaluated views to stats['results'], which save_checkpoint(best=True) compares:
        lower is better.  (The reference appends its PSNR there and still keeps the minimum, nerf/utils.py:1606-1611, :1671 -- a quirk
        not kept.)"""
        from . import metrics as M
        n, H, W = data.n_img, data.H, data.W
        if masks is not None and len(masks) != n:
            raise ValueError("evaluate_one_epoch: one mask (or None) per view expected")
        dev = data.images.device
        sums = torch.zeros(n, 2, dtype=torch.float64, device=dev)
        scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
        lp = torch.zeros(n, dtype=torch.float64, device=dev) if lpips is not None else None
        lp_in = torch.empty(2, 3, H, W, dtype=torch.float32, device=dev) if lpips is not None else None
        rgb_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if out_dir else None
        depth_u8 = torch.empty(H, W, dtype=torch.uint8, device=dev) if out_dir else None
        ss = gt_out = ss_scratch = None
        if ssim:
            if H < 11 or W < 11:
                raise ValueError(f"evaluate_one_epoch: ssim needs views of at least 11 x 11 pixels, got {H} x {W}")
            if ssim_data_range is not None and not (0.0 < float(ssim_data_range) < float("inf")):
                raise ValueError("evaluate_one_epoch: ssim_data_range must be a positive finite number, or None for each view's own range")
            ss = torch.zeros(n, dtype=torch.float64, device=dev)
            gt_out = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
            ss_scratch = torch.empty(M.ssim_scratch_doubles(H, W), dtype=torch.float64, device=dev)
        has_mask = np.zeros(n, bool)
        with self._eval_weights():
            for i in range(n):
                m = None if masks is None else masks[i]
                if m is not None:
                    m = m.to(dev, torch.uint8).contiguous()
                    if m.numel() != H * W:
                        raise ValueError(f"evaluate_one_epoch: mask {i} must have H x W = {H} x {W} values")
                    has_mask[i] = True
                pred, depth = self._render_view(data, i, scale_depth=False)
                M.eval_view(pred, data.images[i], depth=depth, bg=1.0, sse=sums[i, 0:1], mask=m,
                            masked_sse=sums[i, 1:2] if m is not None else None, rgb_u8=rgb_u8, depth_u8=depth_u8, lpips_in=lp_in,
                            scratch=scratch, gt_out=gt_out)
                if lpips is not None:
                    lpips(lp_in, out=lp[i:i + 1])
                if ssim:
                    M.ssim(pred, gt_out, H, W, data_range=ssim_data_range, out=ss[i:i + 1], scratch=ss_scratch)
                if out_dir:
                    self._write_pngs(out_dir, name, i, rgb_u8, depth_u8)
        if ssim:                                                       # one host read for the whole split: the SSIMs ride with the sums
            s = torch.cat([sums, ss[:, None]], 1).cpu().numpy()
        else:
            s = sums.cpu().numpy()
        res = {"psnr": M.psnr_from_sse(s[:, 0], 3 * H * W), "lpips": None if lp is None else lp.cpu().numpy(), "masked_mse": None}
        if masks is not None:
            res["masked_mse"] = np.where(has_mask, s[:, 1] / (3 * H * W), np.nan)
        res["mean_psnr"] = float(np.mean(res["psnr"]))
        res["mean_lpips"] = None if lp is None else float(np.mean(res["lpips"]))
        res["mean_masked_mse"] = float(np.mean(res["masked_mse"][has_mask])) if has_mask.any() else None
        res["ssim"] = s[:, 2].copy() if ssim else None
        res["mean_ssim"] = float(np.mean(res["ssim"])) if ssim else None
        self.stats["results"].append(float(s[:, 0].sum() / (n * 3 * H * W)))
        return res

    def _render_view_geometry(self, data, i):
        """_render_view's render of view i with scale_depth=False, and its opacity -> image [HW,3], depth [HW] (the raw sum w t),
        weights_sum [HW], fp32"""
        from .rays import get_rays
        ray = get_rays(data.poses[i:i + 1], data.intrinsics, data.H, data.W)
        with torch.autocast("cuda", dtype=torch.float16):
            res = self.r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=False,
                                     image_hw=(data.H, data.W))
        return res["image"].float().contiguous(), res["depth"].float().contiguous(), res["weights_sum"].float().contiguous()

    @torch.no_grad()
    def evaluate_consistency(self, data, step=1, frames=None, lpips=None, min_opacity=0.5, out_dir=None, name="ngp"):
        """short-range (step=1) and long-range (step=7) view consistency as LAENeRF, ARF and Ref-NPR report it (the reference's
        scripts/eval/consistency_metrics.py), for results that have no ground truth: frame i is warped onto frame i + step and
        compared with it where neither an occlusion nor a motion boundary is in the way (metrics.consistency_pair; the flow is
        the reprojection through this trainer's model, not RAFT's).  The views of `data` (a ResidentImages) are taken as a camera
        path in the data's order (the script sorts file names; from_transforms keeps the file's order).  Every view is rendered
        ONCE with the EMA weights over white (perturb=False, scale_depth=False) and kept in a ring of step + 1 views on the device;
        the pairs (i, i + step), i < n - step, are one kernel call each into a device [n - step, 2] float64 tensor, plus one
        `lpips(lp_in, out=...)` with `lpips` (metrics.LPIPS); one host read for the whole split.
        frames: [n, H, W, 3] uint8 or fp32 on the device, in the data's camera order (recolor_views(...), render_recolored,
        tr.test(...)[0], ...): they replace the colours, the geometry still comes from the model; None scores the model's own
        renders.  out_dir: `{name}_{i:04d}_warp.png`, frame i warped onto i + step, invalid pixels black.
        -> dict warp_mse [n - step] (sse / count, the script's "RSME", which takes no root; NaN where no pixel is valid),
        valid_share [n - step], lpips [n - step] or None, mean_warp_mse and mean_lpips (over the pairs as in the script, the NaN
        pairs left out of mean_warp_mse), empty_pairs (their number)."""
        from . import metrics as M
        n, H, W = data.n_img, data.H, data.W
        step = int(step)
        if step < 1 or step >= n:
            raise ValueError(f"evaluate_consistency: step must be in [1, {n - 1}] for {n} views")
        if data.color_space == "linear":
            raise ValueError("evaluate_consistency: color_space='linear' data is not supported here (every shipped config uses srgb)")
        dev = data.images.device
        if frames is not None:
            if not torch.is_tensor(frames) or tuple(frames.shape) != (n, H, W, 3) or frames.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"evaluate_consistency: frames must be a uint8 or fp32 tensor of shape {(n, H, W, 3)}")
            frames = frames.to(dev).contiguous()
        pairs = n - step
        sums = torch.zeros(pairs, 2, dtype=torch.float64, device=dev)
        scratch = torch.empty(M.CONSISTENCY_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
        lp = torch.zeros(pairs, dtype=torch.float64, device=dev) if lpips is not None else None
        lp_in = torch.empty(2, 3, H, W, dtype=torch.float32, device=dev) if lpips is not None else None
        warped = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if out_dir else None
        ring = [None] * (step + 1)
        with self._eval_weights():
            for j in range(n):
                image, depth, opacity = self._render_view_geometry(data, j)
                ring[j % (step + 1)] = (frames[j] if frames is not None else image, depth, opacity)
                i = j - step
                if i < 0:
                    continue
                (fa, da, aa), (fb, db, ab) = ring[i % (step + 1)], ring[j % (step + 1)]
                M.consistency_pair(fa, fb, da, aa, db, ab, data.poses[i], data.poses[j], data.intrinsics, H, W,
                                   min_opacity=min_opacity, sse=sums[i, 0:1], count=sums[i, 1:2], warped=warped, lpips_in=lp_in,
                                   scratch=scratch)
                if lpips is not None:
                    lpips(lp_in, out=lp[i:i + 1])
                if out_dir:
                    from PIL import Image
                    os.makedirs(out_dir, exist_ok=True)
                    u8 = (warped.clamp(0, 1) * 255).to(torch.uint8)
                    Image.fromarray(u8.cpu().numpy()).save(os.path.join(out_dir, f"{name}_{i:04d}_warp.png"))
        s = sums.cpu().numpy()
        sse, count = s[:, 0], s[:, 1]
        empty = count == 0
        res = {"warp_mse": np.where(empty, np.nan, sse / np.where(empty, 1.0, count)), "valid_share": count / (H * W),
               "lpips": None if lp is None else lp.cpu().numpy(), "empty_pairs": int(empty.sum())}
        res["mean_warp_mse"] = float(np.mean(res["warp_mse"][~empty])) if not empty.all() else float("nan")
        res["mean_lpips"] = None if lp is None else float(np.mean(res["lpips"]))
        return res

    @torch.no_grad()
    def test(self, data, out_dir=None, name="ngp"):
        """the reference's test (nerf/utils.py:777-827, test_step :701-719): every view of `data` rendered with the EMA weights
        over white, scale_depth=True -> rgb [n, H, W, 3] and depth [n, H, W] uint8 on the device (clip to [0,1], * 255, truncate);
        out_dir: the same as `{name}_{i:04d}_rgb.png` / `_depth.png`"""
        from . import metrics as M
        n, H, W = data.n_img, data.H, data.W
        dev = data.images.device
        rgb = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        depth = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
        scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
        with self._eval_weights():
            for i in range(n):
                pred, d = self._render_view(data, i, scale_depth=True)
                M.eval_view(pred, None, depth=d, rgb_u8=rgb[i], depth_u8=depth[i], scratch=scratch)
        if out_dir:
            for i in range(n):
                self._write_pngs(out_dir, name, i, rgb[i], depth[i])
        return rgb, depth
