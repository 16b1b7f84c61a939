"""Host-side mirror of the reference's `raymarching/raymarching.py` on the HIP backend.

Same public names, argument order, defaults, output shapes and in-place behaviour as the
reference (cited per function), so `nerf/renderer.py` / `editing/*` written against the
reference call these unchanged.  Every output/workspace is allocated here and handed to the
backend, exactly like the reference's autograd.Functions do.  GPU tensors only: there is no
CPU fallback (the reference's wrappers likewise `.cuda()` everything, raymarching.py:34-35).
"""
import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from ..backend import raymarching_backend as _backend
from ..losses import loss_scale_of

__all__ = ["near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "packbits", "march_rays_train",
           "composite_rays_train", "march_rays", "march_rays_distill", "composite_rays", "composite_rays_distill",
           "compact_rays_alive", "render_frame", "composite_rays_train_blend", "composite_rays_train_blend_mse",
           "composite_rays_train_blend_depth", "finish_term_loss", "finish_depth_loss", "composite_depth_numpy", "composite_rays_train_blend_distort",
           "finish_distort_loss", "finish_second_loss", "composite_distort_numpy", "density_grid_positions",
           "density_grid_partial_positions", "density_grid_update", "mark_untrained_grid"]


def _gpu(t):
    return t if t.is_cuda else t.cuda()


def _rays(t):
    return _gpu(t).contiguous().view(-1, 3)


class _near_far_from_aabb(Function):
    """raymarching.py:19-49"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rays_o, rays_d, aabb, min_near=0.2):
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        N = rays_o.shape[0]
        nears = torch.empty(N, dtype=rays_o.dtype, device=rays_o.device)
        fars = torch.empty(N, dtype=rays_o.dtype, device=rays_o.device)
        _backend.near_far_from_aabb(rays_o, rays_d, _gpu(aabb).contiguous(), N, min_near, nears, fars)
        return nears, fars


near_far_from_aabb = _near_far_from_aabb.apply


class _sph_from_ray(Function):
    """raymarching.py:52-80"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rays_o, rays_d, radius):
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        N = rays_o.shape[0]
        coords = torch.empty(N, 2, dtype=rays_o.dtype, device=rays_o.device)
        _backend.sph_from_ray(rays_o, rays_d, radius, N, coords)
        return coords


sph_from_ray = _sph_from_ray.apply


class _morton3D(Function):
    """raymarching.py:83-104: coords [N,3] int in [0,128) -> indices [N] int32"""

    @staticmethod
    def forward(ctx, coords):
        coords = _gpu(coords)
        N = coords.shape[0]
        indices = torch.empty(N, dtype=torch.int32, device=coords.device)
        _backend.morton3D(coords.int().contiguous(), N, indices)
        return indices


morton3D = _morton3D.apply


class _morton3D_invert(Function):
    """raymarching.py:106-126"""

    @staticmethod
    def forward(ctx, indices):
        indices = _gpu(indices)
        N = indices.shape[0]
        coords = torch.empty(N, 3, dtype=torch.int32, device=indices.device)
        _backend.morton3D_invert(indices.int().contiguous(), N, coords)
        return coords


morton3D_invert = _morton3D_invert.apply


class _packbits(Function):
    """raymarching.py:129-155: grid [C, H^3] float -> bitfield [C*H^3/8] uint8"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, grid, thresh, bitfield=None):
        grid = _gpu(grid).contiguous()
        N = grid.shape[0] * grid.shape[1] // 8
        if bitfield is None:
            bitfield = torch.empty(N, dtype=torch.uint8, device=grid.device)
        _backend.packbits(grid, N, thresh, bitfield)
        return bitfield


packbits = _packbits.apply


def _round_up_always(m, align):
    """the reference's `m += align - m % align` (adds a full `align` when already aligned)"""
    return m + (align - m % align) if align > 0 else m


class _march_rays_train(Function):
    """raymarching.py:161-235.  Differences, all invisible to callers: rows of `rays` come out in ray-id
    order with offsets = exclusive scan of counts (the reference's order depends on atomic arrival)."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, step_counter=None, mean_count=-1,
                perturb=False, align=-1, force_all_rays=False, dt_gamma=0, max_steps=1024):
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        density_bitfield = _gpu(density_bitfield).contiguous()
        dev, dt = rays_o.device, rays_o.dtype
        N = rays_o.shape[0]
        M = N * max_steps
        if not force_all_rays and mean_count > 0:
            M = _round_up_always(mean_count, align)
        # rows no ray owns are zero-filled by the kernel (the reference's torch.zeros, raymarching.py:207-209)
        xyzs = torch.empty(M, 3, dtype=dt, device=dev)
        dirs = torch.empty(M, 3, dtype=dt, device=dev)
        deltas = torch.empty(M, 2, dtype=dt, device=dev)
        rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
        rows_end = torch.empty(1, dtype=torch.int32, device=dev)
        if step_counter is None:
            step_counter = torch.zeros(2, dtype=torch.int32, device=dev)
        noises = torch.rand(N, dtype=dt, device=dev) if perturb else torch.zeros(N, dtype=dt, device=dev)
        _backend.march_rays_train(rays_o, rays_d, density_bitfield, bound, dt_gamma, max_steps, N, C, H, M,
                                  nears.contiguous(), fars.contiguous(), xyzs, dirs, deltas, rays, step_counter, noises, rows_end)
        rays.rows_end = rows_end                         # consumed by composite_rays_train_blend (not part of the reference API)
        if force_all_rays or mean_count <= 0:
            m = _round_up_always(int(step_counter[0].item()), align)      # D2H sync, first 16 steps only
            xyzs, dirs, deltas = xyzs[:m], dirs[:m], deltas[:m]
        return xyzs, dirs, deltas, rays


def march_rays_train(*args, m_limit=None, capacity=None, **kwargs):
    """raymarching.py:161-235 (arguments as there).  MI355X-native keywords m_limit=<device int32 tensor of 1 element>,
    capacity=<int>: the sample buffers get `capacity` rows and rays are truncated where a call with the host threshold
    M = min(m_limit, capacity) truncates them (lae_march_rays_train_limit) -- so one captured graph serves every threshold up to
    its capacity.  mean_count, align and force_all_rays are then ignored and no host read happens.  Without them: unchanged."""
    if m_limit is None and capacity is None:
        return _march_rays_train.apply(*args, **kwargs)
    if m_limit is None or capacity is None:
        raise ValueError("march_rays_train: m_limit and capacity go together")
    import inspect
    bound_args = inspect.signature(_march_rays_train.forward).bind(None, *args, **kwargs)
    bound_args.apply_defaults()
    a = bound_args.arguments
    return _march_limit(a["rays_o"], a["rays_d"], a["bound"], a["density_bitfield"], a["C"], a["H"], a["nears"], a["fars"],
                        a["step_counter"], a["perturb"], a["dt_gamma"], a["max_steps"], m_limit, int(capacity))


@torch.no_grad()
def _march_limit(rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, step_counter, perturb, dt_gamma, max_steps, m_limit,
                 M_cap):
    rays_o, rays_d = _rays(rays_o).float(), _rays(rays_d).float()
    density_bitfield = _gpu(density_bitfield).contiguous()
    if not (torch.is_tensor(m_limit) and m_limit.is_cuda and m_limit.dtype == torch.int32 and m_limit.numel() == 1):
        raise RuntimeError("march_rays_train: m_limit must be a 1-element int32 tensor on the GPU")
    if M_cap <= 0:
        raise ValueError("march_rays_train: capacity must be positive")
    dev, dt = rays_o.device, rays_o.dtype
    N = rays_o.shape[0]
    xyzs = torch.empty(M_cap, 3, dtype=dt, device=dev)
    dirs = torch.empty(M_cap, 3, dtype=dt, device=dev)
    deltas = torch.empty(M_cap, 2, dtype=dt, device=dev)
    rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    rows_end = torch.empty(1, dtype=torch.int32, device=dev)
    if step_counter is None:
        step_counter = torch.zeros(2, dtype=torch.int32, device=dev)
    noises = torch.rand(N, dtype=dt, device=dev) if perturb else torch.zeros(N, dtype=dt, device=dev)
    _backend.march_rays_train_limit(rays_o, rays_d, density_bitfield, bound, dt_gamma, max_steps, N, C, H, M_cap, m_limit,
                                    nears.float().contiguous(), fars.float().contiguous(), xyzs, dirs, deltas, rays, step_counter,
                                    noises, rows_end)
    rays.rows_end = rows_end
    return xyzs, dirs, deltas, rays


class _composite_rays_train(Function):
    """raymarching.py:238-291"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh=1e-4):
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        weights_sum = torch.empty(N, dtype=sigmas.dtype, device=sigmas.device)
        depth = torch.empty(N, dtype=sigmas.dtype, device=sigmas.device)
        image = torch.empty(N, 3, dtype=sigmas.dtype, device=sigmas.device)
        _backend.composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image)
        ctx.dims = [M, N, T_thresh]
        return weights_sum, depth, image

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_weights_sum, grad_depth, grad_image):
        # grad_depth is not propagated (raymarching.py:275)
        sigmas, rgbs, deltas, rays, weights_sum, depth, image = ctx.saved_tensors
        M, N, T_thresh = ctx.dims
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        _backend.composite_rays_train_backward(grad_weights_sum.contiguous(), grad_image.contiguous(), sigmas, rgbs,
                                               deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs)
        return grad_sigmas, grad_rgbs, None, None, None


composite_rays_train = _composite_rays_train.apply


def _train_outputs(N, dt, dev):
    """weights_sum [N], raw depth [N], un-blended image [N,3], depth_out [N], image_out [N,3] of the BLEND forward"""
    return (torch.empty(N, dtype=dt, device=dev), torch.empty(N, dtype=dt, device=dev), torch.empty(N, 3, dtype=dt, device=dev),
            torch.empty(N, dtype=dt, device=dev), torch.empty(N, 3, dtype=dt, device=dev))


class _composite_rays_train_blend(Function):
    """MI355X-native: composite_rays_train + the post-ops of run_cuda (nerf/renderer.py:321, 325) in the same kernels:
    image + (1 - weights_sum) * bg_color and clamp(depth - nears, min=0) / (fars - nears).  The backward writes every
    gradient row itself (no zero fills).  `rays` must come from this package's march_rays_train (ray-id order).
    Also returns the RAW depth D = sum_k w_k t_k, differentiable: where it receives a gradient the backward is
    lae_composite_rays_train_backward_blend_ex with grad_depth, which carries what the reference's backward drops (raymarching.py:273-275)."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh):
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        weights_sum, depth, image, depth_out, image_out = _train_outputs(N, sigmas.dtype, sigmas.device)
        _backend.composite_rays_train_forward_blend(sigmas, rgbs, deltas, rays, M, N, T_thresh, nears.contiguous(),
                                                    fars.contiguous(), bg_rays, bg, weights_sum, depth, image, depth_out, image_out)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg_rays, rows_end)
        ctx.dims = [M, N, T_thresh, bg]
        ctx.mark_non_differentiable(depth_out)
        ctx.set_materialize_grads(False)                 # an unused output's gradient arrives as None, not as a zero fill
        return weights_sum, depth, depth_out, image_out

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_weights_sum, grad_depth, grad_depth_out, grad_image):
        sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg_rays, rows_end = ctx.saved_tensors
        M, N, T_thresh, bg = ctx.dims
        if grad_image is None and grad_weights_sum is None and grad_depth is None:
            return (None,) * 10
        if grad_image is None:
            grad_image = torch.zeros_like(image)
        gws = None if grad_weights_sum is None else grad_weights_sum.float().contiguous()     # None: the kernel takes zero
        grad_sigmas, grad_rgbs = torch.empty_like(sigmas), torch.empty_like(rgbs)
        if grad_depth is None:
            _backend.composite_rays_train_backward_blend(gws, grad_image.float().contiguous(), sigmas, rgbs, deltas, rays, weights_sum,
                                                         image, M, N, T_thresh, bg_rays, bg, rows_end, grad_sigmas, grad_rgbs)
        else:
            _backend.composite_rays_train_backward_blend_depth(gws, grad_image.float().contiguous(), grad_depth.float().contiguous(),
                                                               sigmas, rgbs, deltas, rays, weights_sum, depth, image, M, N, T_thresh,
                                                               bg_rays, bg, rows_end, grad_sigmas, grad_rgbs)
        return (grad_sigmas, grad_rgbs) + (None,) * 8


def _bg_args(bg_color, device):
    bg_rays, bg = None, (0.0, 0.0, 0.0)
    if torch.is_tensor(bg_color) and bg_color.numel() > 3:
        bg_rays = bg_color.to(device, torch.float32).reshape(-1, 3).contiguous()
    elif torch.is_tensor(bg_color):
        v = [float(x) for x in bg_color.reshape(-1).tolist()]
        bg = tuple(v * 3 if len(v) == 1 else v)
    elif isinstance(bg_color, (int, float)):
        bg = (float(bg_color),) * 3
    else:
        bg = tuple(float(x) for x in bg_color)
    return bg_rays, bg


def _blend_args(who, rays, bg_color, device):
    """-> rows_end, bg_rays, bg of a composite_rays_train_blend* call (`who`: the function the user called)"""
    rows_end = getattr(rays, "rows_end", None)
    if rows_end is None:
        raise RuntimeError(f"{who}: `rays` must be the tensor returned by laenerf_amd march_rays_train")
    return (rows_end,) + _bg_args(bg_color, device)


def composite_rays_train_blend(sigmas, rgbs, deltas, rays, nears, fars, bg_color=1, T_thresh=1e-4):
    """-> weights_sum [N], depth normalised to [0,1] [N], image blended over bg_color [N,3]
    bg_color: number, 3 numbers / tensor of 3, or a per-ray [N,3] tensor (renderer.py:313-321)"""
    rows_end, bg_rays, bg = _blend_args("composite_rays_train_blend", rays, bg_color, sigmas.device)
    weights_sum, _, depth_out, image = _composite_rays_train_blend.apply(sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end,
                                                                         T_thresh)
    return weights_sum, depth_out, image


def composite_rays_train_blend_depth(sigmas, rgbs, deltas, rays, nears, fars, bg_color=1, T_thresh=1e-4):
    """-> weights_sum [N], depth_raw [N], depth_out [N] (normalised to [0,1], no gradient), image blended over bg_color [N,3].
    depth_raw = sum_k w_k t_k (t from the ray's first sample, the `depth` of composite_rays_train) carries a gradient to the
    densities: the building block of depth losses (DS-NeRF-style sparse depth, the distillation's depth term).  The
    reference-named composite_rays_train keeps ignoring the gradient of depth."""
    rows_end, bg_rays, bg = _blend_args("composite_rays_train_blend_depth", rays, bg_color, sigmas.device)
    return _composite_rays_train_blend.apply(sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh)


class _composite_rays_train_blend_dist(Function):
    """_composite_rays_train_blend with one more differentiable output: dist [N], the distortion l_ray of every ray's weights
    (`lae_composite_rays_train_forward_blend` with dist; formulas in include/laenerf.h).  Where dist receives a gradient the backward
    is lae_composite_rays_train_backward_blend_ex with grad_dist, otherwise the one _composite_rays_train_blend would have run."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh):
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        weights_sum, depth, image, depth_out, image_out = _train_outputs(N, sigmas.dtype, sigmas.device)
        dist = torch.empty(N, dtype=sigmas.dtype, device=sigmas.device)
        _backend.composite_rays_train_forward_blend_dist(sigmas, rgbs, deltas, rays, M, N, T_thresh, nears.contiguous(),
                                                         fars.contiguous(), bg_rays, bg, weights_sum, depth, image, depth_out, image_out,
                                                         dist)
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image, dist, bg_rays, rows_end)
        ctx.dims = [M, N, T_thresh, bg]
        ctx.mark_non_differentiable(depth_out)
        ctx.set_materialize_grads(False)
        return weights_sum, depth, depth_out, image_out, dist

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_weights_sum, grad_depth, grad_depth_out, grad_image, grad_dist):
        sigmas, rgbs, deltas, rays, weights_sum, depth, image, dist, bg_rays, rows_end = ctx.saved_tensors
        M, N, T_thresh, bg = ctx.dims
        if grad_image is None and grad_weights_sum is None and grad_depth is None and grad_dist is None:
            return (None,) * 10
        grad_image = torch.zeros_like(image) if grad_image is None else grad_image.float().contiguous()
        gws = None if grad_weights_sum is None else grad_weights_sum.float().contiguous()
        gD = None if grad_depth is None else grad_depth.float().contiguous()
        grad_sigmas, grad_rgbs = torch.empty_like(sigmas), torch.empty_like(rgbs)
        if grad_dist is not None:
            _backend.composite_rays_train_backward_blend_dist(gws, grad_image, gD, grad_dist.float().contiguous(), sigmas, rgbs, deltas,
                                                              rays, weights_sum, depth, dist, image, M, N, T_thresh, bg_rays, bg,
                                                              rows_end, grad_sigmas, grad_rgbs)
        elif gD is not None:
            _backend.composite_rays_train_backward_blend_depth(gws, grad_image, gD, sigmas, rgbs, deltas, rays, weights_sum, depth, image,
                                                               M, N, T_thresh, bg_rays, bg, rows_end, grad_sigmas, grad_rgbs)
        else:
            _backend.composite_rays_train_backward_blend(gws, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh,
                                                         bg_rays, bg, rows_end, grad_sigmas, grad_rgbs)
        return (grad_sigmas, grad_rgbs) + (None,) * 8


def composite_rays_train_blend_distort(sigmas, rgbs, deltas, rays, nears, fars, bg_color=1, T_thresh=1e-4):
    """-> weights_sum [N], depth_raw [N], depth_out [N] (no gradient), image blended over bg_color [N,3], dist [N].
    composite_rays_train_blend_depth plus the raw per-ray distortion of the weights (mip-NeRF 360, the O(n) form of the reference's
    loss.py eff_distloss with m = t, interval = deltas[:,0]; lengths in the march's units, not divided by far - near):
    dist = (1/3) sum_k delta_k w_k^2 + sum_ij w_i w_j |t_i - t_j|, differentiable towards the densities: the building block of
    custom regularizers (dist.mean() is the L_dist of composite_rays_train_blend_mse(distort_weight=...))."""
    rows_end, bg_rays, bg = _blend_args("composite_rays_train_blend_distort", rays, bg_color, sigmas.device)
    return _composite_rays_train_blend_dist.apply(sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh)


# root gradients known to be all ones (laenerf_amd.optim.FusedAdam.backward registers the tensor it passes to
# loss.backward): for them the fused node below hands its stored sample gradients on unchanged.  address -> weak reference:
# an address whose tensor has died may belong to anything by now
_unit_root_grads = {}


def register_unit_root_grad(t):
    import weakref
    _unit_root_grads[t.data_ptr()] = weakref.ref(t)


def _is_unit_root_grad(t):
    r = _unit_root_grads.get(t.data_ptr())
    return r is not None and r() is not None and r().shape == t.shape


class _DepthPlane:
    """holds the depth plane on its way through Function.apply: custom_fwd(cast_inputs=float32) would copy a fp16 plane of the whole
    image set to fp32 in every step under autocast; the kernel reads fp16 itself"""
    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


# the auxiliary terms of the fused training step, in the order their buffers are made and their losses finished:
# term -> (its partial sums' attribute on `loss`, elements per ray, its per-ray buffers' attributes, what a loss without it lacks).
# The backend takes a term's buffers as the per-ray ones [N] in this order, then the partial sums [cdiv(N, 4)].
TERMS = {
    "depth": ("depth_partials", 1, ("grad_depth",), "a depth criterion"),
    "distort": ("dist_partials", 1, ("dist", "grad_dist"), "a distortion term"),
    "opacity": ("opac_partials", 1, ("opac", "grad_ws"), "an opacity term"),
    "second": ("second_partials", 3, (), "a second target"),
}


def _rays_name(parts_name):
    return parts_name.replace("_partials", "_rays")      # the attribute that holds the ray count the partial sums were taken over


def _terms_on(depth_sup, dist_sup, crit, weight_sup):
    """the terms of TERMS, in its order, that the arguments of _composite_rays_train_blend_mse switch on"""
    on = {"depth": depth_sup is not None, "distort": dist_sup is not None, "opacity": crit is not None and crit[2] is not None,
          "second": weight_sup is not None and weight_sup[1] is not None}
    return [t for t in TERMS if on[t]]


def _term_buffers(term, N, dev):
    per_ray = tuple(torch.empty(N, dtype=torch.float32, device=dev) for _ in TERMS[term][2])
    return per_ray + (torch.empty((N + 3) // 4, dtype=torch.float32, device=dev),)


class _composite_rays_train_blend_mse(Function):
    """composite_rays_train_blend + the trainer's criterion and loss scaling (`MSELoss(pred_rgb, gt).mean()` then
    `scaler.scale(loss)`, nerf/utils.py train_step) as ONE autograd node and ONE kernel: d loss / d pixel of a ray depends on
    that ray's pixel only, so the compositing forward, the criterion and the compositing backward of a ray run back to back
    in the wavefront that owns it (`lae_composite_rays_train_step`; three launches and two kernel boundaries in the middle of
    the step before).  The sample gradients are therefore computed in forward() for an upstream gradient of 1 and stored;
    backward() returns them -- multiplied by the upstream gradient unless that is known to be ones.
    depth_sup = (_DepthPlane, depth_inds, depth_weight, value_only) adds the depth criterion in the same kernel
    (`lae_depth_term`): loss = MSE + depth_weight * mean(((D - (z - nears)) * (z > 0))^2), z gathered from the
    depth plane by the kernel; its outputs are grad_depth (d loss / d D) and depth_partials (the depth partial sums).
    dist_sup = (distort_weight, value_only) adds distort_weight * mean(l_ray), the distortion term
    (`lae_dist_term`, with or without depth_sup); its outputs are l_ray per ray, d loss / d l_ray and its
    partial sums.
    crit = (loss_kind, loss_param, None or (opacity_weight, value_only)) chooses the colour criterion and adds the opacity-entropy term
    (`lae_crit_term`, with or without the other two); the term's outputs are the entropy per ray,
    d loss / d weights_sum and the entropy's partial sums.  crit=None is the call as it was.
    weight_sup = (_DepthPlane or None, _DepthPlane or None, pix_inds, second_weight) adds the per-pixel weights and the second colour
    target (`lae_weight_term`, MSE only); a second target's output is the term's partial sums.
    weight_sup=None is the call as it was.
    -> (loss, weights_sum, depth, image, [scaled loss, loss]) and then, for each term that is on in TERMS' order, the outputs named
    there (a term that is off has none)."""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh, target, scale, defer_loss=False,
                depth_sup=None, dist_sup=None, crit=None, weight_sup=None):
        sigmas, rgbs, deltas = sigmas.contiguous(), rgbs.contiguous(), deltas.contiguous()
        M, N = sigmas.shape[0], rays.shape[0]
        dev = sigmas.device
        weights_sum, depth, image, depth_out, image_out = _train_outputs(N, sigmas.dtype, dev)
        target = target.float().contiguous()
        if target.shape != image_out.shape:
            raise RuntimeError("composite_rays_train_blend_mse: target must be [N,3]")
        out = torch.empty(2, dtype=torch.float32, device=dev)
        grad_image = torch.empty_like(image_out)
        grad_sigmas, grad_rgbs = torch.empty_like(sigmas), torch.empty_like(rgbs)
        partials = torch.empty((N + 3) // 4, dtype=torch.float32, device=dev)
        bufs = {t: _term_buffers(t, N, dev) for t in _terms_on(depth_sup, dist_sup, crit, weight_sup)}
        if depth_sup is not None:
            depth_sup = (depth_sup[0].t,) + depth_sup[1:] + bufs["depth"]
        if dist_sup is not None:
            dist_sup = dist_sup + bufs["distort"]
        if "opacity" in bufs:
            crit = crit[:2] + (crit[2] + bufs["opacity"],)
        if weight_sup is not None:
            w_plane, t2_plane = weight_sup[:2]
            weight_sup = (None if w_plane is None else w_plane.t, None if t2_plane is None else t2_plane.t) + weight_sup[2:] + \
                bufs.get("second", (None,))
        _backend.composite_rays_train_step(sigmas, rgbs, deltas, rays, M, N, T_thresh, nears.contiguous(), fars.contiguous(), bg_rays,
                                           bg, rows_end, target, scale, weights_sum, depth, image, depth_out, image_out, grad_image,
                                           grad_sigmas, grad_rgbs, out, partials, defer_loss=defer_loss, depth_sup=depth_sup,
                                           dist_sup=dist_sup, crit=crit, weight_sup=weight_sup)
        ctx.save_for_backward(grad_sigmas, grad_rgbs)
        aux = (weights_sum, depth_out, image_out, out) + sum(bufs.values(), ())
        ctx.mark_non_differentiable(*aux)
        ctx.set_materialize_grads(False)                 # no zero-filled gradients for the auxiliary outputs (a fill launch each)
        return (out[0],) + aux

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_loss, *_):
        if grad_loss is None:
            return (None,) * 17
        grad_sigmas, grad_rgbs = ctx.saved_tensors
        if not _is_unit_root_grad(grad_loss):              # a general upstream gradient: d(loss) scales every sample gradient
            gl = grad_loss.float()
            scaled = grad_sigmas * gl
            from ..backend import retarget_pending_loss
            retarget_pending_loss(grad_sigmas, scaled)     # a deferred loss value follows the tensor the head backward will receive
            grad_sigmas, grad_rgbs = scaled, grad_rgbs * gl
        return (grad_sigmas, grad_rgbs) + (None,) * 15


def finish_term_loss(loss, term, out=None):
    """one auxiliary term of TERMS alone, without its weight, of a `loss` made by composite_rays_train_blend_mse with that term: one
    lae_loss_finish launch over the step's partial sums of the term, off the gradient path.  out: a float32 tensor of 2 elements to
    write to (both receive the value); -> out[1] as a 0-dim tensor"""
    parts_name, elems, _, without = TERMS[term]
    parts = getattr(loss, parts_name, None)
    if parts is None:
        raise RuntimeError(f"finish_{term}_loss: the loss was made without {without}")
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=parts.device)
    _backend.loss_finish(parts, parts.numel(), elems * getattr(loss, _rays_name(parts_name)), None, out)
    return out[1]


def finish_depth_loss(loss, out=None):
    """finish_term_loss for the depth term of composite_rays_train_blend_mse(depth=...): mean(((D - (z - nears)) * (z > 0))^2)"""
    return finish_term_loss(loss, "depth", out)


def finish_distort_loss(loss, out=None):
    """finish_term_loss for the distortion term of composite_rays_train_blend_mse(distort_weight=...): L_dist = mean over all rays
    of l_ray"""
    return finish_term_loss(loss, "distort", out)


def finish_opacity_loss(loss, out=None):
    """finish_term_loss for the opacity-entropy term of composite_rays_train_blend_mse(opacity_weight=...): L_op = mean over all
    rays of h(weights_sum)"""
    return finish_term_loss(loss, "opacity", out)


def finish_second_loss(loss, out=None):
    """finish_term_loss for the second colour term of composite_rays_train_blend_mse(second_target=...): the mean over the 3 N
    elements of ((1 - w / 2) (second_target - pred))^2"""
    return finish_term_loss(loss, "second", out)


def check_weight(who, name, value):
    """-> float(value); ValueError unless it is finite and >= 0"""
    w = float(value)
    if not (w >= 0.0) or w == float("inf"):
        raise ValueError(f"{who}: {name} must be finite and >= 0")
    return w


def composite_rays_train_blend_mse(sigmas, rgbs, deltas, rays, nears, fars, target, bg_color=1, T_thresh=1e-4, scaler=None,
                                   defer_loss=None, depth=None, depth_inds=None, depth_weight=0.0, depth_grad=True,
                                   distort_weight=None, distort_grad=True, loss="mse", huber_delta=0.1, opacity_weight=None,
                                   opacity_grad=True, pixel_weights=None, pixel_inds=None, second_target=None, second_weight=0.0):
    """-> (loss, weights_sum, depth, image): loss = MSE(image, target) times the loss scale of `scaler` (a FusedAdam, a
    1-element fp32 cuda tensor, or None); `loss.unscaled` holds the plain MSE.  Only `loss` carries a gradient.
    defer_loss (default: True when `scaler` is a FusedAdam): the VALUE of loss / loss.unscaled is NaN until the backward pass
    has run (the fused head's backward sums it in its reduction launch; FusedAdam.backward() / step() finish it otherwise) --
    the gradients do not depend on it, and the trainer reads it after the step (nerf/utils.py `loss.item()` for logging).
    depth (default None: today's call, bit for bit): depth supervision in the same kernel.  A float16 / float32 tensor of
    ray-origin distances, zero = no supervision: one value per ray, or with depth_inds [N] int64 (ResidentImages.sample's `inds`)
    any plane they index.  loss becomes MSE + depth_weight * mean(((D - (depth - nears)) * (depth > 0))^2), the reference's depth
    term (nerf/utils.py:585-589, 634-635, weight 1e-3 there); D is the raw composited depth.  A ray that misses the bounding box
    (nears == fars, the sentinel of near_far_from_aabb) is unsupervised whatever the plane holds: it has no near.  depth_grad=True carries the
    term's gradient to the densities -- the reference's backward drops it (raymarching.py:273-275), depth_grad=False restates
    that: the value only, the sample gradients of the call without depth bit for bit.  `loss.grad_depth` [N] holds d loss / d D,
    finish_depth_loss(loss) the unweighted depth term.
    distort_weight (default None: today's call, bit for bit): the distortion regularizer of mip-NeRF 360 in the same kernel, with or
    without depth.  loss becomes ... + distort_weight * L_dist, L_dist = mean over all rays of
    l_ray = (1/3) sum_k delta_k w_k^2 + sum_ij w_i w_j |t_i - t_j| (the O(n) form of the reference's loss.py eff_distloss, called
    with m = t and interval = deltas[:,0]: lengths in the march's own units, not divided by far - near, so the weight that suits a
    scene scales with 1 / its extent).  distort_grad=False: the value only, the sample gradients of the call without the term bit
    for bit.  `loss.dist` [N] holds l_ray, `loss.grad_dist` [N] d loss / d l_ray, finish_distort_loss(loss) L_dist.
    loss (default 'mse': today's call, bit for bit): the colour criterion, the mean over the 3 N elements of 'mse' (e^2), 'l1' (|e|),
    'huber' (the reference's loss.py huber_loss, = torch's HuberLoss(huber_delta) / huber_delta) or 'mape' (|e| / (|target| + 1e-2),
    loss.py mape_loss); `loss.unscaled` then holds that criterion in the MSE's place.
    opacity_weight (default None: today's call, bit for bit): the opacity-entropy regularizer (torch-ngp's lambda_entropy) in the same
    kernel.  loss becomes ... + opacity_weight * L_op, L_op = mean over all rays of h = -(o log2 o + (1 - o) log2(1 - o)) with
    o = clamp(weights_sum, 1e-5, 1 - 1e-5); its gradient reaches a ray whose weights_sum lies inside the clamp (bounds included).
    opacity_grad=False: the value only, the sample gradients of the call without the term bit for bit.  `loss.opac` [N] holds h,
    `loss.grad_ws` [N] d loss / d weights_sum, finish_opacity_loss(loss) L_op.
    pixel_weights / second_target (default None: today's call, bit for bit; loss='mse' only): a per-pixel weight w on the colour
    residual and a second colour target t with its own weight, in the same kernel (`lae_weight_term` of the step), alone,
    together, and with every other term: the colour criterion becomes mean((w (image - target))^2) + second_weight *
    mean(((1 - w / 2) (t - image))^2), the reference's train_step_npr (nerf/utils.py:523-526).  Both are float16 / float32 tensors --
    pixel_weights one value per ray, second_target [N, 3 or 4] -- or, with pixel_inds [N] int64 (ResidentImages.sample's `inds`), any
    planes they index.  A 4-channel second target is blended over the ray's background, as the sampler blends `target`.  A weight of
    0 removes the pixel's colour from the step exactly.  finish_second_loss(loss) is the second term without its weight."""
    from ..backend import loss_kind
    kind, param = loss_kind("composite_rays_train_blend_mse", loss, huber_delta)
    weight_sup = None
    if pixel_weights is not None or second_target is not None:
        if kind != 0:
            raise ValueError("composite_rays_train_blend_mse: pixel_weights / second_target need loss='mse'")
        for name, t in (("pixel_weights", pixel_weights), ("second_target", second_target)):
            if t is not None and (not torch.is_tensor(t) or t.dtype not in (torch.float16, torch.float32)):
                raise RuntimeError(f"composite_rays_train_blend_mse: {name} must be a float16 or float32 tensor")
        if second_target is not None and second_target.shape[-1] not in (3, 4):
            raise RuntimeError("composite_rays_train_blend_mse: second_target must be [.., 3 or 4]")
        weight_sup = (None if pixel_weights is None else _DepthPlane(pixel_weights.contiguous()),
                      None if second_target is None else _DepthPlane(second_target.contiguous()),
                      None if pixel_inds is None else pixel_inds.contiguous(),
                      check_weight("composite_rays_train_blend_mse", "second_weight", second_weight))
    crit = None
    if kind != 0 or opacity_weight is not None:
        crit = (kind, param, None if opacity_weight is None else
                (check_weight("composite_rays_train_blend_mse", "opacity_weight", opacity_weight), not opacity_grad))
    dist_sup = None
    if distort_weight is not None:
        dist_sup = (check_weight("composite_rays_train_blend_mse", "distort_weight", distort_weight), not distort_grad)
    rows_end, bg_rays, bg = _blend_args("composite_rays_train_blend_mse", rays, bg_color, sigmas.device)
    scale = loss_scale_of(scaler)
    if defer_loss is None:
        defer_loss = scaler is not None and not torch.is_tensor(scaler) and hasattr(scaler, "finish_loss")
    depth_sup = None
    if depth is not None:
        if not torch.is_tensor(depth) or depth.dtype not in (torch.float16, torch.float32):
            raise RuntimeError("composite_rays_train_blend_mse: depth must be a float16 or float32 tensor")
        depth_sup = (_DepthPlane(depth.contiguous()), None if depth_inds is None else depth_inds.contiguous(),
                     check_weight("composite_rays_train_blend_mse", "depth_weight", depth_weight), not depth_grad)
    out = _composite_rays_train_blend_mse.apply(sigmas, rgbs, deltas, rays, nears, fars, bg_rays, bg, rows_end, T_thresh, target, scale,
                                                bool(defer_loss), depth_sup, dist_sup, crit, weight_sup)
    loss, weights_sum, depth_o, image, both = out[:5]
    loss.unscaled = both[1]
    rest = iter(out[5:])                                   # the enabled terms' buffers, as _term_buffers made them
    for term in _terms_on(depth_sup, dist_sup, crit, weight_sup):
        parts_name, _, per_ray, _ = TERMS[term]
        for name in per_ray + (parts_name,):
            setattr(loss, name, next(rest))
        setattr(loss, _rays_name(parts_name), rays.shape[0])
    return loss, weights_sum, depth_o, image


def _infer_buffers(n_alive, n_step, align, dt, dev):
    M = n_alive * n_step
    if align > 0:
        M += align - (M % align)
    return (M, torch.zeros(M, 3, dtype=dt, device=dev), torch.zeros(M, 3, dtype=dt, device=dev),
            torch.zeros(M, 2, dtype=dt, device=dev))


class _march_rays(Function):
    """raymarching.py:297-348"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, C, H, near, far,
                align=-1, perturb=False, dt_gamma=0, max_steps=1024):
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        dev, dt = rays_o.device, rays_o.dtype
        M, xyzs, dirs, deltas = _infer_buffers(n_alive, n_step, align, dt, dev)
        noises = torch.rand(n_alive, dtype=dt, device=dev) if perturb else torch.zeros(n_alive, dtype=dt, device=dev)
        _backend.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H,
                            density_bitfield, near, far, xyzs, dirs, deltas, noises)
        return xyzs, dirs, deltas


march_rays = _march_rays.apply


class _march_rays_distill(Function):
    """raymarching.py:355-411"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, edit_bitfield, C, H,
                near, far, align=-1, perturb=False, dt_gamma=0, max_steps=1024):
        rays_o, rays_d = _rays(rays_o), _rays(rays_d)
        dev, dt = rays_o.device, rays_o.dtype
        M, xyzs, dirs, deltas = _infer_buffers(n_alive, n_step, align, dt, dev)
        edit_occ = torch.zeros(M, dtype=torch.bool, device=dev)
        noises = torch.rand(n_alive, dtype=dt, device=dev) if perturb else torch.zeros(n_alive, dtype=dt, device=dev)
        _backend.march_rays_distill(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C,
                                    H, density_bitfield, edit_bitfield, near, far, xyzs, dirs, deltas, edit_occ, noises)
        return xyzs, dirs, deltas, edit_occ


march_rays_distill = _march_rays_distill.apply


class _composite_rays(Function):
    """raymarching.py:413-435 (in place on rays_alive, rays_t, weights_sum, depth, image)"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh=1e-2):
        _backend.composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas.contiguous(), rgbs.contiguous(),
                                deltas, weights_sum, depth, image)
        return tuple()


composite_rays = _composite_rays.apply


class _composite_rays_distill(Function):
    """raymarching.py:437-461"""

    @staticmethod
    @custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, weights_edit_sum, depth,
                depth_edit, image, int_edit, T_thresh=1e-2):
        _backend.composite_rays_distill(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas.contiguous(),
                                        rgbs.contiguous(), deltas, weights_sum, weights_edit_sum, depth, depth_edit,
                                        int_edit, image)
        return tuple()


composite_rays_distill = _composite_rays_distill.apply


def compact_rays_alive(rays_alive, n_alive=None):
    """MI355X-native replacement for `rays_alive = rays_alive[rays_alive >= 0]` (renderer.py:375): stable
    device-side compaction.  Returns (out_alive [n_alive] int32, n_out device int32[1]); the caller may keep
    n_out on the device (no sync) or read it."""
    n_alive = rays_alive.shape[0] if n_alive is None else n_alive
    out = torch.empty(max(n_alive, 1), dtype=torch.int32, device=rays_alive.device)
    n_out = torch.empty(1, dtype=torch.int32, device=rays_alive.device)
    _backend.compact_rays_alive(rays_alive, n_alive, out, n_out)
    return out, n_out


@torch.no_grad()
def render_frame(rays_o, rays_d, aabb, min_near, density_bitfield, bound, C, H, table_half, offsets, per_level_scale,
                 base_resolution, sigma_weights_half, color_weights_half, edit_bitfield=None, gridtype_id=0, align_corners=False,
                 interp_id=0, density_scale=1.0, dt_gamma=0, max_steps=1024, T_thresh=1e-4, max_n_step=8, row_budget=0,
                 noises=None, bg_color=None, scale_depth=True, want_stats=False, offsets_host=None):
    """MI355X-native: the inference loop of NeRFRenderer.run_cuda (nerf/renderer.py:335-387; run_cuda_distill :394-480
    when `edit_bitfield` is given) as ONE backend call -- loop state on the device, no host sync per iteration.
    Same per-ray arithmetic and iteration schedule as march_rays / network / composite_rays called in the Python loop.

    row_budget: rows (samples) one iteration may put through the network; 0 = N, the reference's rule
    `n_step = max(min(N // n_alive, 8), 1)`.  A larger budget means fewer, larger iterations (same per-ray samples).
    bg_color: None (no blend, as run_cuda_distill), a scalar / 3 numbers, or a [N,3] tensor.
    Returns dict(image [N,3], depth [N], weights_sum [N]) (+ weights_edit, depth_edit; + stats when want_stats)."""
    import numpy as np
    rays_o, rays_d = _rays(rays_o), _rays(rays_d)
    N, dev = rays_o.shape[0], rays_o.device
    weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    image = torch.empty(N, 3, dtype=torch.float32, device=dev)
    weights_edit = depth_edit = None
    if edit_bitfield is not None:
        weights_edit = torch.empty(N, dtype=torch.float32, device=dev)
        depth_edit = torch.empty(N, dtype=torch.float32, device=dev)
    bg_rays, bg_rgb = None, (0.0, 0.0, 0.0)
    if torch.is_tensor(bg_color) and bg_color.numel() == 3 * N and N > 1:
        bg_rays = _gpu(bg_color).float().reshape(N, 3).contiguous()
    elif bg_color is not None:
        v = [float(x) for x in (bg_color.flatten().tolist() if torch.is_tensor(bg_color) else np.atleast_1d(bg_color))]
        bg_rgb = tuple(v * 3) if len(v) == 1 else tuple(v)
    stats = _backend.render_frame(rays_o, rays_d, N, _gpu(aabb).float().contiguous(), min_near, density_bitfield, edit_bitfield,
                                  bound, dt_gamma, max_steps, C, H, table_half, offsets, offsets.shape[0] - 1,
                                  np.log2(per_level_scale), base_resolution, gridtype_id, align_corners, interp_id,
                                  sigma_weights_half, color_weights_half, density_scale, T_thresh, max_n_step, row_budget,
                                  None if noises is None else _gpu(noises).float().contiguous(), bg_rays, bg_rgb,
                                  bg_color is not None, scale_depth, weights_sum, depth, image, weights_edit, depth_edit,
                                  want_stats, offsets_host=offsets_host)
    out = {"image": image, "depth": depth, "weights_sum": weights_sum}
    if edit_bitfield is not None:
        out["weights_edit"], out["depth_edit"] = weights_edit, depth_edit
    if want_stats:
        out["stats"] = stats
    return out


# ---------------------------------------------------------------- occupancy-grid maintenance (MI355X-native kernels)
@torch.no_grad()
def density_grid_positions(n, H, bound_c, noise=None, coords=None):
    """positions + Morton indices of `update_extra_state`'s density queries (nerf/renderer.py:580-592, 602-621).
    coords None: the n = H^3 cells in meshgrid order (full sweep); else coords [n,3] int32.  noise [n,3] in [0,1)."""
    dev = (coords if coords is not None else noise).device if (coords is not None or noise is not None) else torch.device("cuda")
    xyzs = torch.empty(n, 3, dtype=torch.float32, device=dev)
    indices = torch.empty(n, dtype=torch.int32, device=dev)
    _backend.density_grid_positions(None if coords is None else _gpu(coords).int().contiguous(), n, H, bound_c,
                                    None if noise is None else _gpu(noise).float().contiguous(), xyzs, indices)
    return xyzs, indices


def density_grid_partial_positions(grid_c, coords_rand, u, H, bound_c, noise=None, rnd=None, n=None):
    """MI355X-native: the 2n query points of update_extra_state's PARTIAL sweep (nerf/renderer.py:600-621) without the host read
    of `nonzero`: coords_rand [n,3] random cells, u [n] uniform in [0,1) choosing among the occupied cells of grid_c [H^3] (> 0,
    in index order), noise [2n,3] jitter -- or rnd [2, n+1] uniforms from which both halves are drawn sorted on the device (H a
    power of two).  Returns xyzs [2n,3], indices [2n] int32 (Morton; -1 where no cell is occupied)."""
    n = coords_rand.shape[0] if rnd is None else (rnd.numel() // 2 - 1 if n is None else n)
    xyzs = torch.empty(2 * n, 3, dtype=torch.float32, device=grid_c.device)
    indices = torch.empty(2 * n, dtype=torch.int32, device=grid_c.device)
    _backend.density_grid_partial_positions(grid_c.contiguous(), None if rnd is not None else _gpu(coords_rand).int().contiguous(),
                                            None if rnd is not None else _gpu(u).float().contiguous(),
                                            None if rnd is None else _gpu(rnd).float().contiguous(), n, H, bound_c,
                                            None if noise is None else _gpu(noise).float().contiguous(), xyzs, indices)
    return xyzs, indices


@torch.no_grad()
def density_grid_update(grid_c, sigmas, indices, tmp, density_scale=1.0, decay=0.95):
    """in place on one cascade `grid_c` [H^3]: tmp[indices] = sigmas * density_scale; grid = max(grid * decay, tmp)
    on sampled, trainable cells (renderer.py:596, 627, 633-634).  tmp [H^3] int32 scratch, zero before and after."""
    _backend.density_grid_update(sigmas.float().contiguous(), indices.contiguous(), indices.numel(), density_scale, decay,
                                 grid_c.numel(), grid_c, tmp)
    return grid_c


@torch.no_grad()
def mark_untrained_grid(density_grid, poses, intrinsics, bound, min_near=0.2, filter_close_point=False, H=128):
    """in place: density_grid [C, H^3] = -1 where no training camera sees the cell (renderer.py:482-554)"""
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    poses = _gpu(torch.as_tensor(poses)).float().contiguous()
    _backend.mark_untrained_grid(poses, poses.shape[0], fx, fy, cx, cy, density_grid.shape[0], H, bound, min_near,
                                 filter_close_point, density_grid)
    return density_grid


# ---------------------------------------------------------------- numpy restatement of the depth-supervised compositing
def composite_depth_numpy(sigmas, rgbs, deltas, rays, T_thresh=1e-4, dtype=None, bg=None, grad_weights_sum=None, grad_image=None,
                          grad_depth=None, target=None, z=None, nears=None, depth_weight=0.0, scale=1.0, depth_grad=True, n_rays=None,
                          fars=None, samples=False):
    """The training compositing with the depth gradient, restated sample by sample in `dtype` (default float64): the forward
    (k_composite_train_fwd: early stop after the first sample with T_post < T_thresh, that sample included; rays with
    num_steps == 0 or offset + num_steps > M dropped), optionally the depth term of lae_composite_rays_train_step
    (target [N,3], z [N] already gathered, nears [N], optionally fars [N]: rays with nears >= fars, the sentinel interval of a ray
    that misses the bounding box, are unsupervised; grad_image / grad_depth are then the criterion's) and the backward
    (lae_composite_rays_train_backward_blend_ex with grad_depth; bg: None = no blend term, [3] or [N,3]).  Everything is indexed as the
    kernels do: per-ray values by rays[n, 0]; n_rays: the length of the per-ray arrays when `rays` holds only some rows of a table.
    -> dict weights_sum, depth (raw D), image [N,3], stop [N] (index of the last sample used, -1 for a ray without samples),
    margin (the smallest |T_post / T_thresh - 1| over the samples used: how far the early stop is from flipping), and with
    gradients grad_sigmas [M], grad_rgbs [M,3] (zero on rows no ray uses); with a criterion also image_out, res, grad_image,
    grad_depth, mse, depth_mse, loss (= mse + depth_weight * depth_mse).  samples=True: also `samples`, {row of rays: (w, t, T_post)}
    of the samples each ray uses."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    sig, col, dl = np.asarray(sigmas).astype(dt), np.asarray(rgbs).astype(dt).reshape(-1, 3), np.asarray(deltas).astype(dt).reshape(-1, 2)
    rays = np.asarray(rays).astype(np.int64).reshape(-1, 3)
    M, N = sig.shape[0], rays.shape[0] if n_rays is None else int(n_rays)
    one, thr = dt(1), dt(T_thresh)
    ws, D, img = np.zeros(N, dt), np.zeros(N, dt), np.zeros((N, 3), dt)
    stop = np.full(N, -1, np.int64)
    margin = np.inf
    per_ray = {}
    for n in range(rays.shape[0]):
        index, offset, steps = (int(v) for v in rays[n])
        if steps == 0 or offset + steps > M:
            continue
        T, t = one, dt(0)
        w_l, t_l, tp_l = [], [], []
        for k in range(steps):
            i = offset + k
            alpha = one - dt(np.exp(-sig[i] * dl[i, 0]))
            w = alpha * T
            t = t + dl[i, 1]
            T = T * (one - alpha)
            w_l.append(w); t_l.append(t); tp_l.append(T)
            ws[index] = ws[index] + w
            D[index] = D[index] + w * t
            img[index] = img[index] + w * col[i]
            margin = min(margin, abs(float(T) / float(thr) - 1.0))
            stop[index] = k
            if T < thr:
                break
        per_ray[n] = (np.array(w_l, dt), np.array(t_l, dt), np.array(tp_l, dt))
    res = {"weights_sum": ws, "depth": D, "image": img, "stop": stop, "margin": margin}
    if samples:
        res["samples"] = per_ray
    bgv = None if bg is None else np.broadcast_to(np.asarray(bg).astype(dt).reshape(-1, 3), (N, 3))
    if target is not None:
        lam, sc = dt(depth_weight), dt(scale)
        out = img + (one - ws)[:, None] * (bgv if bgv is not None else dt(0))
        err = out - np.asarray(target).astype(dt).reshape(N, 3)
        zz = np.asarray(z).astype(dt).reshape(N)
        nr = np.asarray(nears).astype(dt).reshape(N)
        sup = zz > 0 if fars is None else (zz > 0) & (nr < np.asarray(fars).astype(dt).reshape(N))
        with np.errstate(over="ignore"):
            r = np.where(sup, D - (zz - nr), dt(0))
        grad_image = (err * (dt(2) / dt(3 * N))) * sc
        grad_depth = (r * (dt(2) * lam / dt(N))) * sc if depth_grad else np.zeros(N, dt)
        mse, dmse = (err * err).sum() / dt(3 * N), (r * r).sum() / dt(N)
        res.update(image_out=out, res=r, grad_image=grad_image, grad_depth=grad_depth, mse=mse, depth_mse=dmse, loss=mse + lam * dmse)
    if grad_image is None and grad_depth is None and grad_weights_sum is None:
        return res
    zero = np.zeros(N, dt)
    g_img = np.zeros((N, 3), dt) if grad_image is None else np.asarray(grad_image).astype(dt).reshape(N, 3)
    g_ws = zero if grad_weights_sum is None else np.asarray(grad_weights_sum).astype(dt).reshape(N)
    g_D = zero if grad_depth is None else np.asarray(grad_depth).astype(dt).reshape(N)
    gs, gc = np.zeros(M, dt), np.zeros((M, 3), dt)
    for n, (w_l, t_l, tp_l) in per_ray.items():
        index, offset, _ = (int(v) for v in rays[n])
        g = g_img[index]
        gws = g_ws[index] - (g * bgv[index]).sum() if bgv is not None else g_ws[index]
        tail = gws * (one - ws[index])
        c_run, d_run = np.zeros(3, dt), dt(0)
        for k in range(len(w_l)):
            i = offset + k
            c_run = c_run + w_l[k] * col[i]
            d_run = d_run + w_l[k] * t_l[k]
            gc[i] = g * w_l[k]
            br = (g * (tp_l[k] * col[i] - (img[index] - c_run))).sum() + tail
            gs[i] = dl[i, 0] * (br + g_D[index] * (tp_l[k] * t_l[k] - (D[index] - d_run)))
    res.update(grad_sigmas=gs, grad_rgbs=gc)
    return res


def composite_distort_numpy(sigmas, rgbs, deltas, rays, T_thresh=1e-4, dtype=None, bg=None, grad_weights_sum=None, grad_image=None,
                            grad_depth=None, grad_dist=None, target=None, z=None, nears=None, depth_weight=0.0, distort_weight=0.0,
                            scale=1.0, depth_grad=True, distort_grad=True, n_rays=None, fars=None):
    """composite_depth_numpy with the distortion term of the lae_composite_rays_train_* entries, restated sample by sample in `dtype`
    (default float64).  Per ray, over the samples the forward uses, lengths in the march's units (m = t, interval = deltas[:,0]):
      dist = l_ray = (1/3) sum_k delta_k w_k^2 + 2 sum_k w_k (t_k W_<k - WT_<k)
      q_k  = dl / dw_k = (2/3) delta_k w_k + 2 (t_k (W_<k - (W - W_k)) + ((D - WT_k) - WT_<k))
      grad_sigmas_k += delta_k * g * (T_post_k * q_k - (Q - Q_k)),  Q_k = sum_{j<=k} q_j w_j,  Q = 2 l_ray (l is of degree 2 in w)
    With a criterion (target; z / nears optional: no depth term without z) loss = mse + depth_weight * depth_mse + distort_weight *
    dist_mean and g = grad_dist = (distort_weight / N) * scale for every ray (zeros with distort_grad=False); otherwise g is the
    grad_dist [N] handed in.  -> the dict of composite_depth_numpy plus dist [N], q [M] (zero on rows no ray uses), dist_mean
    (= sum(dist) / N, all rays), grad_dist [N]; grad_sigmas / grad_rgbs whenever any gradient is present."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    dl = np.asarray(deltas).astype(dt).reshape(-1, 2)
    rays_a = np.asarray(rays).astype(np.int64).reshape(-1, 3)
    M, N = dl.shape[0], rays_a.shape[0] if n_rays is None else int(n_rays)
    if target is not None and z is None:
        z, nears, depth_weight = np.zeros(N, dt), np.zeros(N, dt), 0.0
    res = composite_depth_numpy(sigmas, rgbs, deltas, rays, T_thresh, dtype=dtype, bg=bg, grad_weights_sum=grad_weights_sum,
                                grad_image=grad_image, grad_depth=grad_depth, target=target, z=z, nears=nears, depth_weight=depth_weight,
                                scale=scale, depth_grad=depth_grad, n_rays=n_rays, fars=fars, samples=True)
    per_ray = res.pop("samples")
    dist, q = np.zeros(N, dt), np.zeros(M, dt)
    third, two = dt(1) / dt(3), dt(2)
    pre = {}
    for n, (w, t, tp) in per_ray.items():
        index, offset, _ = (int(v) for v in rays_a[n])
        d0 = dl[offset:offset + len(w), 0]
        W_k, WT_k = np.cumsum(w), np.cumsum(w * t)
        W_lt, WT_lt = np.concatenate([[dt(0)], W_k[:-1]]), np.concatenate([[dt(0)], WT_k[:-1]])      # exclusive prefixes
        dist[index] = (third * d0 * w * w).sum() + (two * w * (t * W_lt - WT_lt)).sum()
        q[offset:offset + len(w)] = two * third * d0 * w + two * (t * (W_lt - (W_k[-1] - W_k)) + ((WT_k[-1] - WT_k) - WT_lt))
        pre[n] = (w, tp, d0)
    res.update(dist=dist, q=q, dist_mean=dist.sum() / dt(N))
    if target is not None:
        lam = dt(distort_weight)
        grad_dist = np.full(N, (lam / dt(N)) * dt(scale), dt) if distort_grad else np.zeros(N, dt)
        res["loss"] = res["loss"] + lam * res["dist_mean"]
    res["grad_dist"] = None if grad_dist is None else np.asarray(grad_dist).astype(dt).reshape(N)
    if res["grad_dist"] is None and "grad_sigmas" not in res:
        return res
    if res["grad_dist"] is None:
        res["grad_dist"] = np.zeros(N, dt)
    if "grad_sigmas" not in res:
        res.update(grad_sigmas=np.zeros(M, dt), grad_rgbs=np.zeros((M, 3), dt))
    gs = res["grad_sigmas"]
    for n, (w, tp, d0) in pre.items():
        index, offset, _ = (int(v) for v in rays_a[n])
        qr = q[offset:offset + len(w)]
        Q_k = np.cumsum(qr * w)
        gs[offset:offset + len(w)] += d0 * res["grad_dist"][index] * (tp * qr - (two * dist[index] - Q_k))
    return res


# ---------------------------------------------------------------- numpy restatement of the fused step's criteria
OPAC_LO, OPAC_HI = 1e-5, 1.0 - 1e-5          # the clamp of the opacity entropy; the kernel holds both as float32


def colour_loss_numpy(e, target, loss="mse", huber_delta=0.1, dtype=None):
    """the element loss v and dv = d v / d pred of the colour criteria (include/laenerf.h LAE_LOSS_*) for e = pred - target, in `dtype`
    (default float64); huber_delta is taken at its float32 value, as the kernels receive it.  -> (v, dv), shaped like e"""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    e, t = np.asarray(e).astype(dt), np.asarray(target).astype(dt)
    r, sg = np.abs(e), np.sign(e)
    if loss == "mse":
        return e * e, dt(2) * e
    if loss == "l1":
        return r, sg
    if loss == "huber":
        d = dt(np.float32(huber_delta))
        return np.where(r > d, r - dt(0.5) * d, (dt(0.5) / d * r) * r), np.where(r > d, sg, e / d)
    if loss == "mape":
        k = dt(1) / (np.abs(t) + dt(np.float32(1e-2)))
        return r * k, sg * k
    raise ValueError("colour_loss_numpy: loss must be 'mse', 'l1', 'huber' or 'mape'")


def opacity_entropy_numpy(weights_sum, dtype=None):
    """h = -(o log2 o + (1 - o) log2(1 - o)), o = clamp(weights_sum, 1e-5, 1 - 1e-5) (the bounds at their float32 values), and
    dh = d h / d weights_sum = log2(1 - o) - log2 o inside the clamp (bounds included), 0 outside, in `dtype` -> (h, dh)"""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    w = np.asarray(weights_sum).astype(dt)
    lo, hi = dt(np.float32(OPAC_LO)), dt(np.float32(1) - np.float32(OPAC_LO))
    o = np.minimum(np.maximum(w, lo), hi)
    la, lb = np.log2(o), np.log2(dt(1) - o)
    return -(o * la + (dt(1) - o) * lb), np.where((w >= lo) & (w <= hi), lb - la, dt(0))


def composite_train_step_numpy(sigmas, rgbs, deltas, rays, target, T_thresh=1e-4, dtype=None, bg=None, z=None, nears=None, fars=None,
                               depth_weight=0.0, distort_weight=0.0, scale=1.0, depth_grad=True, distort_grad=True, n_rays=None,
                               loss="mse", huber_delta=0.1, opacity_weight=None, opacity_grad=True, pixel_weights=None, second_target=None,
                               second_weight=0.0):
    """lae_composite_rays_train_step with its criterion and weight terms restated in `dtype` (default float64): the forward, the colour criterion `loss`,
    the depth term (with z), the distortion term and the opacity entropy, then the backward with the criterion's gradients
      grad_image = ((dv * (1 / (3 N))) * scale)  (mse: (e * (2 / (3 N))) * scale),   grad_ws = ((opacity_weight / N) * dh) * scale.
    pixel_weights [N] (the gathered weights w) and second_target [N, 3 or 4] (the gathered second target s; 4 channels are blended
    over bg: t = s_rgb * s_a + bg * (1 - s_a)), loss='mse' only: with u = 1 - w / 2, a = w e, b = u (t - pred),
      colour = mean(a^2),  second = mean(b^2) (both over the 3 N elements),  grad_image = (((w a) - second_weight * (u b)) * (2 / (3 N))) * scale.
    (The kernel evaluates that bracket in double when a second target is present -- its two parts cancel -- and in fp32 otherwise.)
    -> the dict of composite_distort_numpy (grad_sigmas, grad_rgbs, weights_sum, depth, image, dist, ...) plus image_out, grad_image,
    grad_depth, grad_dist, grad_ws, opac [N], colour (= mean(v)), second, depth_mse, dist_mean, opac_mean (all N rays) and
    loss = colour + second_weight * second + depth_weight * depth_mse + distort_weight * dist_mean + opacity_weight * opac_mean."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    f = composite_distort_numpy(sigmas, rgbs, deltas, rays, T_thresh, dtype=dtype, bg=bg, n_rays=n_rays)
    N = f["weights_sum"].shape[0]
    one, sc = dt(1), dt(scale)
    bgv = dt(0) if bg is None else np.broadcast_to(np.asarray(bg).astype(dt).reshape(-1, 3), (N, 3))
    out = f["image"] + (one - f["weights_sum"])[:, None] * bgv
    tgt = np.asarray(target).astype(dt).reshape(N, 3)
    e = out - tgt
    v, dv = colour_loss_numpy(e, tgt, loss, huber_delta, dtype)
    grad_image = (e * (dt(2) / dt(3 * N))) * sc if loss == "mse" else (dv * (one / dt(3 * N))) * sc
    second, lam_2 = dt(0), dt(second_weight)
    if pixel_weights is not None or second_target is not None:
        if loss != "mse":
            raise ValueError("composite_train_step_numpy: pixel_weights / second_target need loss='mse'")
        pw = np.ones(N, dt) if pixel_weights is None else np.asarray(pixel_weights).astype(dt).reshape(N)
        a = pw[:, None] * e
        v = a * a
        g = pw[:, None] * a
        if second_target is not None:
            s2 = np.asarray(second_target).astype(dt).reshape(N, -1)
            t2 = s2[:, :3] * s2[:, 3:] + bgv * (one - s2[:, 3:]) if s2.shape[1] == 4 else s2
            u = (one - dt(0.5) * pw)[:, None]
            b = u * (t2 - out)
            second = (b * b).sum() / dt(3 * N)
            g = g - lam_2 * (u * b)
        grad_image = (g * (dt(2) / dt(3 * N))) * sc
    res_d, grad_depth = np.zeros(N, dt), None
    if z is not None:
        zz, nr = np.asarray(z).astype(dt).reshape(N), np.asarray(nears).astype(dt).reshape(N)
        sup = zz > 0 if fars is None else (zz > 0) & (nr < np.asarray(fars).astype(dt).reshape(N))
        with np.errstate(over="ignore"):
            res_d = np.where(sup, f["depth"] - (zz - nr), dt(0))
        grad_depth = (res_d * (dt(2) * dt(depth_weight) / dt(N))) * sc if depth_grad else np.zeros(N, dt)
    lam_x = dt(distort_weight)
    grad_dist = np.full(N, (lam_x / dt(N)) * sc, dt) if distort_grad else np.zeros(N, dt)
    h, dh = opacity_entropy_numpy(f["weights_sum"], dtype)
    lam_o = dt(0 if opacity_weight is None else opacity_weight)
    grad_ws = ((lam_o / dt(N)) * dh) * sc if opacity_grad else np.zeros(N, dt)
    res = composite_distort_numpy(sigmas, rgbs, deltas, rays, T_thresh, dtype=dtype, bg=bg, grad_weights_sum=grad_ws, grad_image=grad_image,
                                  grad_depth=grad_depth, grad_dist=grad_dist, n_rays=n_rays)
    colour, dmse, omean = v.sum() / dt(3 * N), (res_d * res_d).sum() / dt(N), h.sum() / dt(N)
    res.update(image_out=out, grad_image=grad_image, grad_depth=grad_depth, grad_ws=grad_ws, opac=h, colour=colour, second=second,
               depth_mse=dmse, opac_mean=omean,
               loss=colour + lam_2 * second + dt(depth_weight) * dmse + lam_x * res["dist_mean"] + lam_o * omean)
    return res
