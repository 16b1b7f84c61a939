"""TSDF mesh export: rendered depth (and colour) views fused into a truncated signed distance field on a lattice, and the
colours of the marching-cubes vertices of that field (csrc/tsdf.hip, where the rule is written down in full).

    render_packed_views(renderer, poses, intrinsics, H, W)   the views' surface distance planes [V, H, W] (mask_lift_pack's plane)
    tsdf_fuse(packed, poses, intrinsics, H, W, axes, trunc)  the field u = -tsdf [Nx, Ny, Nz], per-voxel counts and fused colours
    tsdf_vertex_colors(rgb, counts, verts)                   per-vertex colours for marching_cubes(u, 0.0)'s vertices
    tsdf_numpy / tsdf_vertex_colors_numpy                    both kernels restated in a chosen dtype

`NeRFRenderer.extract_mesh_tsdf / save_mesh_tsdf` and `Trainer.save_mesh_tsdf` chain them with mesh.drop_components,
mesh.marching_cubes, mesh.vertex_attributes and mesh.pack_ply.

The fill rule and its price: a voxel that fewer than `min_views` views see near the surface or in free space is solid (u = +1)
if any view sees it behind a surface, so the unobserved interior of the object grows no second wall behind the truncation band.
A region that some view sees only as occluded and that no view sees empty therefore stays solid -- a box corner behind the
object, say -- and comes out as a blob of its own; `keep_largest=True` (mesh.drop_components) removes it."""
import numpy as np
import torch

from . import _lib

POSE_CHUNK = 64                     # LAE_TSDF_POSE_CHUNK (include/laenerf.h): views per LDS stage of lae_tsdf_fuse
BEHIND, OUTSIDE, UNSEEN, OCCLUDED, FREE, NEAR = 0, 1, 2, 3, 4, 5       # tsdf_numpy's outcome of a (voxel, view) pair
MAX_SIDE = 512                      # marching cubes' shape limit (mesh.MAX_SIDE)


def _frame_bytes(frames, V, H, W, dev, who):
    """frames [V, H, W, 3] uint8 (as is) or fp32 (lae_eval_view's byte rule: clip(x, 0, 1) * 255 truncated, NaN -> 0) -> uint8 on dev"""
    if not torch.is_tensor(frames) or frames.numel() != V * H * W * 3 or frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{who}: frames must be a uint8 or fp32 tensor of {V} x {H} x {W} x 3 values")
    frames = frames.to(dev).contiguous()
    if frames.dtype == torch.uint8:
        return frames.reshape(V, H, W, 3)
    from . import metrics as M
    out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
    scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    src = frames.reshape(V, H * W, 3)
    for v in range(V):
        M.eval_view(src[v], None, rgb_u8=out[v], scratch=scratch)
    return out


def tsdf_fuse(packed, poses, intrinsics, H, W, axes, trunc, frames=None, min_views=1, counts=False):
    """V packed views fused on a lattice (lae_tsdf_fuse).  packed fp32 [V, H, W] on the device (mask_lift_pack /
    render_packed_views: |value| is the surface distance along the pixel's ray, +inf a transparent pixel, NaN no observation),
    poses fp32 [V, 4, 4] cam2world, intrinsics (fx, fy, cx, cy), axes three fp32 1-D tensors (mesh.lattice(...); moved to the
    device), trunc > 0 the truncation distance in world units, frames optional [V, H, W, 3] uint8 or fp32 (converted to bytes by
    lae_eval_view's rule first), min_views >= 1 the observations (near or free) a voxel needs for a fused value.
    -> dict: u fp32 [Nx, Ny, Nz] = -tsdf in [-1, 1], larger inside (marching_cubes(u, 0.0)); rgb fp32 [Nx, Ny, Nz, 3] in [0, 1]
    with frames, else None; counts uint16 [Nx, Ny, Nz, 4] = (near, free, occluded, 0) when asked for (always with frames:
    tsdf_vertex_colors needs them), else None.  The fill rule and its price: the module's docstring."""
    H, W = int(H), int(W)
    if len(intrinsics) != 4:
        raise ValueError("tsdf_fuse: intrinsics = (fx, fy, cx, cy)")
    if not torch.is_tensor(packed) or packed.dtype != torch.float32 or not packed.is_contiguous() or H < 1 or W < 1 or \
            packed.numel() == 0 or packed.numel() % (H * W):
        raise ValueError("tsdf_fuse: packed must be a contiguous fp32 tensor of V x H x W values")
    V = packed.numel() // (H * W)
    if V > 65535:
        raise ValueError("tsdf_fuse: at most 65535 views")
    if not torch.is_tensor(poses) or poses.dtype != torch.float32 or poses.numel() != 16 * V or not poses.is_contiguous():
        raise ValueError(f"tsdf_fuse: poses must be a contiguous fp32 tensor of {V} x 4 x 4 values")
    if len(axes) != 3 or any(not torch.is_tensor(a) or a.dtype != torch.float32 or a.dim() != 1 or not 2 <= a.numel() <= MAX_SIDE for a in axes):
        raise ValueError(f"tsdf_fuse: axes must be three 1-D fp32 tensors of 2 to {MAX_SIDE} values")
    if not float(trunc) > 0.0 or not np.isfinite(float(trunc)):
        raise ValueError("tsdf_fuse: trunc must be positive and finite")
    if int(min_views) < 1:
        raise ValueError("tsdf_fuse: min_views must be at least 1")
    dev = packed.device
    xs, ys, zs = (a.to(dev).contiguous() for a in axes)
    nx, ny, nz = xs.numel(), ys.numel(), zs.numel()
    fb = None if frames is None else _frame_bytes(frames, V, H, W, dev, "tsdf_fuse")
    u = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    cnt = torch.empty(nx, ny, nz, 4, dtype=torch.uint16, device=dev) if counts or fb is not None else None
    rgb = torch.empty(nx, ny, nz, 3, dtype=torch.float32, device=dev) if fb is not None else None
    _lib.need_cuda(packed, poses, xs, ys, zs, fb)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    _lib.check(_lib.load().lae_tsdf_fuse(packed.data_ptr(), poses.data_ptr(), V, fx, fy, cx, cy, H, W, xs.data_ptr(), ys.data_ptr(),
                                        zs.data_ptr(), nx, ny, nz, _lib.ptr(fb), float(trunc), int(min_views), u.data_ptr(),
                                        _lib.ptr(cnt), _lib.ptr(rgb), _lib.stream()), "tsdf_fuse")
    return {"u": u, "rgb": rgb, "counts": cnt}


def tsdf_vertex_colors(rgb, counts, verts):
    """colours of marching-cubes vertices from a fused field (lae_tsdf_vertex_colors).  rgb fp32 [Nx, Ny, Nz, 3] and counts uint16
    [Nx, Ny, Nz, 4] as tsdf_fuse returns them, verts fp32 [V, 3] in index space (marching_cubes(u, 0.0)[0]).  A vertex lies on a
    lattice edge: both endpoints coloured (n_near > 0) -> the colours interpolated along the edge, one -> its colour, neither ->
    grey 0.5.  -> (colors fp32 [V, 3] on the device, ready for pack_ply(colors=); the number of grey vertices, one host read)"""
    if not torch.is_tensor(rgb) or rgb.dtype != torch.float32 or rgb.dim() != 4 or rgb.shape[3] != 3 or not rgb.is_contiguous() or \
            any(not 2 <= n <= MAX_SIDE for n in rgb.shape[:3]):
        raise ValueError(f"tsdf_vertex_colors: rgb must be a contiguous fp32 tensor [Nx, Ny, Nz, 3] with 2 <= N <= {MAX_SIDE}")
    if not torch.is_tensor(counts) or counts.dtype != torch.uint16 or tuple(counts.shape) != tuple(rgb.shape[:3]) + (4,) or \
            not counts.is_contiguous():
        raise ValueError(f"tsdf_vertex_colors: counts must be a contiguous uint16 tensor {tuple(rgb.shape[:3]) + (4,)}")
    if not torch.is_tensor(verts) or verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3 or not verts.is_contiguous():
        raise ValueError("tsdf_vertex_colors: verts must be a contiguous fp32 tensor [V, 3]")
    _lib.need_cuda(rgb, counts, verts)
    V = verts.shape[0]
    colors = torch.empty(V, 3, dtype=torch.float32, device=verts.device)
    if V == 0:
        return colors, 0
    n_grey = torch.empty(1, dtype=torch.int32, device=verts.device)
    nx, ny, nz = rgb.shape[:3]
    _lib.check(_lib.load().lae_tsdf_vertex_colors(rgb.data_ptr(), counts.data_ptr(), nx, ny, nz, verts.data_ptr(), V, colors.data_ptr(),
                                                 n_grey.data_ptr(), _lib.stream()), "tsdf_vertex_colors")
    return colors, int(n_grey.item())


@torch.no_grad()
def render_packed_views(renderer, poses, intrinsics, H, W, depths=None, opacities=None, min_opacity=0.5, return_frames=False):
    """the surface distance plane of every view, [V, H, W] fp32 on the device: the render loop of EditGrid.new_from_masks with an
    all-clear mask (render_eval, perturb=False, scale_depth=False, over white, fp16 autocast, the model in eval mode; each view
    packed by mask_lift_pack and dropped before the next is rendered).  depths / opacities (lists or tensors; fp32 H*W values per
    view: sensor depth with opacity 1, or renders the caller has, as `sum w t` and `weights_sum`) replace the render.
    return_frames=True -> (packed, frames uint8 [V, H, W, 3]): the renders' colours by lae_eval_view's byte rule (rendered even
    where depths are given)."""
    from .editing.mask_lift import mask_lift_pack
    from .rays import get_rays
    H, W = int(H), int(W)
    poses = poses.reshape(-1, 4, 4)
    V = poses.shape[0]
    if (depths is None) != (opacities is None):
        raise ValueError("render_packed_views: depths and opacities come together")
    if depths is not None and (len(depths) != V or len(opacities) != V):
        raise ValueError(f"render_packed_views: {len(depths)} depths and {len(opacities)} opacities for {V} poses")
    dev = renderer.density_bitfield.device
    packed = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    frames = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev) if return_frames else None
    clear = torch.zeros(H * W, dtype=torch.uint8, device=dev)
    scratch = None
    if return_frames:
        from . import metrics as M
        scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    was_training = renderer.model.training
    renderer.model.eval()
    try:
        for i in range(V):
            res = None
            if depths is None or return_frames:
                ray = get_rays(poses[i:i + 1], intrinsics, H, W)
                with torch.autocast("cuda", dtype=torch.float16):
                    res = renderer.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=False,
                                               image_hw=(H, W))
            if depths is not None:
                depth, opacity = (t[i].to(dev).float().contiguous() for t in (depths, opacities))
                if depth.numel() != H * W or opacity.numel() != H * W:
                    raise ValueError(f"render_packed_views: view {i}'s depth and opacity must have {H} x {W} values")
            else:
                depth, opacity = res["depth"].float().contiguous(), res["weights_sum"].float().contiguous()
            mask_lift_pack(depth, opacity, clear, min_opacity, out=packed[i])
            if return_frames:
                M.eval_view(res["image"].float().contiguous(), None, rgb_u8=frames[i], scratch=scratch)
    finally:
        renderer.model.train(was_training)
    return (packed, frames) if return_frames else packed


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements

def tsdf_numpy(packed, poses, intrinsics, H, W, axes, trunc, frames=None, min_views=1, dtype=np.float64):
    """numpy restatement of lae_tsdf_fuse with every quantity in `dtype` (float64 by default; np.float32 writes the kernel's
    statements in their order, so with fp32 inputs these are the kernel's bits).  packed [V, H, W], poses [V, 4, 4], axes three
    1-D arrays, frames uint8 [V, H, W, 3] or None; inputs are converted to `dtype` as they come, trunc through fp32 (the value
    the kernel receives).  -> dict:
      u        [Nx, Ny, Nz] in `dtype`: -tsdf
      counts   uint16 [Nx, Ny, Nz, 4]: (near, free, occluded, 0)
      rgb      [Nx, Ny, Nz, 3] in `dtype`, or None without frames
      outcome  uint8 [n, V], n = Nx Ny Nz in the outputs' order: BEHIND (q.z <= 0), OUTSIDE (the frame), UNSEEN (a NaN surface),
               OCCLUDED, FREE, NEAR -- the first that applies
      margin   float64 [n, V]: the distance of the nearest decision the pair took from its threshold, each in its own units, as
               mask_lift_numpy gives it: |q.z| (world units); for a pair outside the frame the distance it would have to move to
               come inside (pixels); for a pair inside the distance of u and of v from the nearest pixel border (pixels) and
               min(|s - trunc|, |s + trunc|) (world units), which is inf where the surface is +inf or NaN: an undefined input
               decides there, not a threshold"""
    dt = np.dtype(dtype).type
    H, W = int(H), int(W)
    pk = np.asarray(packed).reshape(-1, H, W).astype(dt)
    V = pk.shape[0]
    P = np.asarray(poses).reshape(V, 4, 4).astype(dt)
    fx, fy, cx, cy = (dt(v) for v in intrinsics)
    tr = dt(np.float32(trunc))
    xs, ys, zs = (np.asarray(a).reshape(-1).astype(dt) for a in axes)
    nx, ny, nz = xs.size, ys.size, zs.size
    n = nx * ny * nz
    gx, gy, gz = np.meshgrid(xs, ys, zs, indexing="ij")
    w = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], -1)
    t_all = np.abs(pk)
    fr = None if frames is None else np.asarray(frames, dtype=np.uint8).reshape(V, H, W, 3)
    outcome = np.zeros((n, V), np.uint8)
    margin = np.full((n, V), np.inf)
    n_near, n_free, n_occ = (np.zeros(n, np.uint32) for _ in range(3))
    sums = np.zeros((n, 3), np.uint32)
    S = np.zeros(n, dt)
    with np.errstate(all="ignore"):
        for v in range(V):
            R, o = P[v, :3, :3], P[v, :3, 3]
            d = w - o
            q = [(d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k] for k in range(3)]
            front = q[2] > 0
            qz = np.where(front, q[2], dt(1.0))
            pu, pv = (fx * q[0]) / qz + cx, (fy * q[1]) / qz + cy
            inside = front & (pu >= 0) & (pu < dt(W)) & (pv >= 0) & (pv < dt(H))
            px = np.where(inside, np.minimum(np.floor(np.where(inside, pu, 0)), W - 1), 0).astype(np.int64)
            py = np.where(inside, np.minimum(np.floor(np.where(inside, pv, 0)), H - 1), 0).astype(np.int64)
            ts = t_all[v, py, px]
            seen = inside & ~np.isnan(ts)
            t_vox = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            s = ts - t_vox
            occ = seen & (s < -tr)
            free = seen & ~occ & (s > tr)
            near = seen & ~occ & ~free
            outcome[:, v] = np.select([~front, ~inside, ~seen, occ, free], [BEHIND, OUTSIDE, UNSEEN, OCCLUDED, FREE], NEAR)
            n_occ += occ
            n_free += free
            n_near += near
            S = np.where(near, S + s / tr, S)
            if fr is not None:
                sums += np.where(near[:, None], fr[v, py, px].astype(np.uint32), np.uint32(0))
            # margins, in float64 of the `dtype` values
            u64, v64, z64 = pu.astype(np.float64), pv.astype(np.float64), np.abs(q[2].astype(np.float64))
            viol = np.maximum(np.maximum(-u64, u64 - W), np.maximum(-v64, v64 - H))          # > 0 (or = 0 at u = W) outside
            to_border = np.minimum(np.abs(u64 - np.round(u64)), np.abs(v64 - np.round(v64)))
            s64 = s.astype(np.float64)
            gap = np.minimum(np.abs(s64 - float(tr)), np.abs(s64 + float(tr)))
            gap = np.where(np.isfinite(ts), gap, np.inf)
            mg = np.where(inside, np.minimum(z64, np.minimum(to_border, gap)), np.minimum(z64, np.abs(viol)))
            mg = np.where(front, mg, z64)
            margin[:, v] = np.where(np.isnan(mg), np.inf, mg)
        n_obs = n_near + n_free
        fused = n_obs >= np.uint32(min_views)
        tsdf = np.where(fused, (S + n_free.astype(dt)) / np.where(fused, n_obs, 1).astype(dt), np.where(n_occ > 0, dt(-1.0), dt(1.0)))
        rgb = None
        if fr is not None:
            has = n_near > 0
            rgb = np.where(has[:, None], sums.astype(dt) / np.where(has, n_near, 1).astype(dt)[:, None] / dt(255.0), dt(0.0))
            rgb = rgb.astype(dt).reshape(nx, ny, nz, 3)
    counts = np.zeros((n, 4), np.uint16)
    counts[:, 0], counts[:, 1], counts[:, 2] = n_near, n_free, n_occ
    return {"u": (-tsdf).astype(dt).reshape(nx, ny, nz), "counts": counts.reshape(nx, ny, nz, 4), "rgb": rgb, "outcome": outcome,
            "margin": margin}


def tsdf_vertex_colors_numpy(rgb, counts, verts, dtype=np.float64):
    """numpy restatement of lae_tsdf_vertex_colors in `dtype` (np.float32 with fp32 inputs: the kernel's bits).  The vertex's
    lattice edge (base, axis, t) is found in fp32 as mesh.edge_gradients_numpy finds it.  -> (colors [V, 3], n_grey)"""
    f = np.dtype(dtype).type
    rgb = np.asarray(rgb)
    n = np.array(rgb.shape[:3])
    c = rgb.astype(f)
    near = np.asarray(counts)[..., 0] > 0
    v = np.array(verts, dtype=np.float32).reshape(-1, 3)
    v[~np.isfinite(v)] = 0
    base_f = np.clip(np.floor(v), np.float32(0), (n - 1).astype(np.float32)[None, :])
    base = base_f.astype(np.int64)
    frac = v - base_f                                                        # fp32
    has = frac > 0
    on_edge = has.any(axis=1)
    axis = np.argmax(has, axis=1)                                            # the first axis with frac > 0
    rows = np.arange(len(v))
    t = np.where(on_edge, frac[rows, axis], np.float32(0)).astype(f)
    q = base.copy()
    q[rows[on_edge], axis[on_edge]] = np.minimum(base[on_edge, axis[on_edge]] + 1, n[axis[on_edge]] - 1)
    ca, cb = c[base[:, 0], base[:, 1], base[:, 2]], c[q[:, 0], q[:, 1], q[:, 2]]
    ha, hb = near[base[:, 0], base[:, 1], base[:, 2]], near[q[:, 0], q[:, 1], q[:, 2]]
    both = ca + t[:, None] * (cb - ca)
    out = np.select([(ha & hb)[:, None], ha[:, None], hb[:, None]], [both, ca, cb], f(0.5)).astype(f)
    return out, int((~ha & ~hb).sum())
