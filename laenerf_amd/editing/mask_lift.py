"""The edit grid from 2D masks: lift the masks of a few posed views into the selection bitfield (csrc/masklift.hip, where the
rule is written down in full), and the way back (`selection_masks`), so that a user can check what they got.

The reference starts a selection from mouse clicks in its GUI; here the first link of the editing chain is
`EditGrid.new_from_masks(renderer, poses, intrinsics, H, W, masks)` with the masks `metrics.load_masks` reads, or any other
uint8 planes.  `mask_lift_numpy` restates both kernels in a chosen dtype."""
import numpy as np
import torch

from .. import _lib

POSE_CHUNK = 64                     # LAE_MASK_LIFT_POSE_CHUNK (include/laenerf.h): views per LDS stage of lae_mask_lift
BEHIND, OUTSIDE, OCCLUDED, IN, OUT = 0, 1, 2, 3, 4       # mask_lift_numpy's outcome of a (cell, view) pair


def mask_lift_pack(depth, opacity, mask, min_opacity=0.5, out=None):
    """one view's planes as ONE fp32 plane (lae_mask_lift_pack): |t_surf| with the sign bit set iff the mask is set, t_surf =
    depth / opacity where opacity >= min_opacity, else +inf.  depth / opacity: the raw `sum w t` and `weights_sum` of
    render_eval(scale_depth=False), fp32 with H*W values; mask uint8 with H*W values, nonzero = selected.  -> out (fp32, the
    shape of depth)"""
    n = depth.numel()
    for name, t, dt in (("depth", depth, torch.float32), ("opacity", opacity, torch.float32), ("mask", mask, torch.uint8)):
        if not torch.is_tensor(t) or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"mask_lift_pack: {name} must be a contiguous {dt} tensor of {n} values")
    if out is None:
        out = torch.empty_like(depth)
    if out.dtype != torch.float32 or out.numel() != n or not out.is_contiguous():
        raise ValueError(f"mask_lift_pack: out must be a contiguous fp32 tensor of {n} values")
    if not float(min_opacity) > 0.0:
        raise ValueError("mask_lift_pack: min_opacity must be positive")
    _lib.need_cuda(depth, opacity, mask, out)
    _lib.check(_lib.load().lae_mask_lift_pack(depth.data_ptr(), opacity.data_ptr(), mask.data_ptr(), n, float(min_opacity),
                                             out.data_ptr(), _lib.stream()), "mask_lift_pack")
    return out


def lift_masks(packed, poses, intrinsics, H, W, density_bitfield, cascade, bound, grid_size=128, depth_margin=2.0, min_views=1,
               min_share=0.5, votes=False, out=None):
    """the selection bitfield of V packed views (lae_mask_lift).  packed fp32 [V, H, W] (mask_lift_pack), poses fp32 [V, 4, 4]
    cam2world on the device, intrinsics (fx, fy, cx, cy), density_bitfield the renderer's ([cascade * grid_size^3 / 8] uint8).
    A cell is selected iff it is occupied, at least `min_views` views see it inside their mask, and those are at least `min_share`
    of the views that see it at all; a view sees a cell iff the cell's centre projects into the frame and lies no further than
    `depth_margin` cell sides behind the pixel's surface.

    depth_margin = 2.0 is a choice, not a derived value: the expected termination depth `sum w t / sum w` lies a little behind the
    first surface, and a cell whose centre is just behind the surface is still part of it.  It also sets how many cells deep the
    selected shell is; cells hidden in every view are never selected (there is no visual-hull fill: masks mark visible surface,
    not silhouettes through occluders) -- `EditGrid.morphological()` and `grow_region_queue` work on the lifted grid.

    votes=True also returns the (in, out) counts, uint16 [cascade * grid_size^3, 2] indexed like density_grid.
    -> grid uint8 [cascade * grid_size^3 / 8] (`out` when given; every byte is written), or (grid, votes)"""
    H, W, C, G = int(H), int(W), int(cascade), int(grid_size)
    if len(intrinsics) != 4:
        raise ValueError("lift_masks: intrinsics = (fx, fy, cx, cy)")
    if G < 2 or G > 128 or G & (G - 1):
        raise ValueError("lift_masks: grid_size must be a power of two in [2, 128]")
    if not torch.is_tensor(packed) or packed.dtype != torch.float32 or not packed.is_contiguous() or H < 1 or W < 1 or \
            packed.numel() == 0 or packed.numel() % (H * W):
        raise ValueError("lift_masks: packed must be a contiguous fp32 tensor of V x H x W values")
    V = packed.numel() // (H * W)
    n_bytes = C * G ** 3 // 8
    if not torch.is_tensor(poses) or poses.dtype != torch.float32 or poses.numel() != 16 * V or not poses.is_contiguous():
        raise ValueError(f"lift_masks: poses must be a contiguous fp32 tensor of {V} x 4 x 4 values")
    if out is None:
        out = torch.empty(n_bytes, dtype=torch.uint8, device=packed.device)
    for name, t in (("density_bitfield", density_bitfield), ("out", out)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.numel() != n_bytes or not t.is_contiguous():
            raise ValueError(f"lift_masks: {name} must be a contiguous uint8 tensor of {n_bytes} values")
    if int(min_views) < 0:
        raise ValueError("lift_masks: min_views must not be negative")
    counts = torch.empty(C * G ** 3, 2, dtype=torch.uint16, device=packed.device) if votes else None
    _lib.need_cuda(packed, poses, density_bitfield, out)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    _lib.check(_lib.load().lae_mask_lift(packed.data_ptr(), poses.data_ptr(), V, fx, fy, cx, cy, H, W, density_bitfield.data_ptr(), C, G,
                                        float(bound), float(depth_margin), int(min_views), float(min_share), out.data_ptr(),
                                        _lib.ptr(counts), _lib.stream()), "mask_lift")
    return (out, counts) if votes else out


def _compact_bits(x):
    x = x & 0x49249249
    x = (x | (x >> 2)) & 0xc30c30c3
    x = (x | (x >> 4)) & 0x0f00f00f
    x = (x | (x >> 8)) & 0xff0000ff
    return (x | (x >> 16)) & 0x0000ffff


def mask_lift_pack_numpy(depth, opacity, mask, min_opacity=0.5, dtype=np.float64):
    """lae_mask_lift_pack in `dtype`: |depth / opacity| where opacity >= min_opacity, else +inf, with the sign bit set iff the
    mask is set.  With dtype=np.float32 and fp32 inputs these are the kernel's bits (one division, one compare, one sign bit)."""
    dt = np.dtype(dtype).type
    d, a = np.asarray(depth).astype(dt), np.asarray(opacity).astype(dt)
    with np.errstate(all="ignore"):
        t = np.abs(np.where(a >= dt(min_opacity), d / a, dt(np.inf)))
    return np.where(np.asarray(mask) != 0, -t, t).astype(dt)              # negation sets the sign bit of 0, inf and NaN alike


def mask_lift_numpy(depths, opacities, masks, poses, intrinsics, H, W, density_bitfield, cascade, bound, grid_size=128,
                    min_opacity=0.5, depth_margin=2.0, min_views=1, min_share=0.5, dtype=np.float64):
    """numpy restatement of lae_mask_lift_pack and lae_mask_lift with every quantity in `dtype` (float64 by default; np.float32
    writes the kernels' statements in their order).  depths / opacities / masks [V, H, W], poses [V, 4, 4]; inputs are converted
    to `dtype` as they come.  -> dict:
      packed   [V, H, W] in `dtype`: the pack kernel's plane
      cells    int64 [n]: the occupied cells, as indices into density_grid (cascade * G^3 + Morton index), ascending
      centres  [n, 3] the cell centres
      outcome  uint8 [n, V]: BEHIND (q.z <= 0), OUTSIDE (the frame), OCCLUDED (or a NaN surface), IN, OUT -- the first that applies
      pixel    int64 [n, V, 2]: (column, row) gathered, -1 where the pair has none
      margin   float64 [n, V]: the distance of the nearest decision the pair took from its threshold, each in its own units:
               |q.z| (world units); for a pair outside the frame the distance it would have to move to come inside (pixels; the
               larger of the violated edges'); for a pair inside the distance of u and of v from the nearest pixel border
               (pixels; the frame's edges are pixel borders) and |t_cell - (t_surf + depth_margin * side)| (world units), which is
               inf where the surface is +inf or NaN: an undefined input decides there, not a threshold
      votes    uint16 [cascade * G^3, 2], grid uint8 [cascade * G^3 / 8]: lae_mask_lift's outputs"""
    dt = np.dtype(dtype).type
    H, W, C, G = int(H), int(W), int(cascade), int(grid_size)
    depths, opacities, masks = (np.asarray(a).reshape(-1, H, W) for a in (depths, opacities, masks))
    V = depths.shape[0]
    P = np.asarray(poses).reshape(V, 4, 4).astype(dt)
    fx, fy, cx, cy = (dt(v) for v in intrinsics)
    packed = mask_lift_pack_numpy(depths, opacities, masks, min_opacity, dt)
    t_surf, m_set = np.abs(packed), np.signbit(packed)
    bits = np.unpackbits(np.asarray(density_bitfield, dtype=np.uint8).reshape(-1), bitorder="little")
    assert bits.size == C * G ** 3, "density_bitfield must hold cascade * grid_size^3 bits"
    cells = np.flatnonzero(bits).astype(np.int64)
    n = cells.size
    cas, m = cells // G ** 3, (cells % G ** 3).astype(np.uint32)
    mip = np.minimum(np.ldexp(dt(1.0), cas.astype(np.int32)).astype(dt), dt(bound))
    rG = dt(1.0) / dt(G)
    coord = np.stack([_compact_bits(m), _compact_bits(m >> 1), _compact_bits(m >> 2)], -1).astype(dt)
    w = (((coord + dt(0.5)) * rG) * dt(2.0) - dt(1.0)) * mip[:, None]
    slack = dt(depth_margin) * ((dt(2.0) * mip) * rG)
    outcome = np.zeros((n, V), np.uint8)
    pixel = np.full((n, V, 2), -1, np.int64)
    margin = np.full((n, V), np.inf)
    inf = np.inf
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
            ts, ms = t_surf[v, py, px], m_set[v, py, px]
            t_cell = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            thr = ts + slack
            visible = inside & (t_cell <= thr)
            outcome[:, v] = np.select([~front, ~inside, ~visible, ms], [BEHIND, OUTSIDE, OCCLUDED, IN], OUT)
            pixel[:, v, 0], pixel[:, v, 1] = np.where(inside, px, -1), np.where(inside, py, -1)
            # margins, in float64 of the `dtype` values
            u64, v64, z64 = pu.astype(np.float64), pv.astype(np.float64), np.abs(q[2].astype(np.float64))
            viol = np.maximum(np.maximum(-u64, u64 - W), np.maximum(-v64, v64 - H))          # > 0 (or = 0 at u = W) outside
            to_border = np.minimum(np.abs(u64 - np.round(u64)), np.abs(v64 - np.round(v64)))
            depth_gap = np.abs(t_cell.astype(np.float64) - thr.astype(np.float64))
            depth_gap = np.where(np.isfinite(thr), depth_gap, inf)
            mg = np.where(inside, np.minimum(z64, np.minimum(to_border, depth_gap)), np.minimum(z64, np.abs(viol)))
            mg = np.where(front, mg, z64)
            margin[:, v] = np.where(np.isnan(mg), inf, mg)
    n_in = (outcome == IN).sum(1).astype(np.uint32)
    n_out = (outcome == OUT).sum(1).astype(np.uint32)
    f32 = np.float32
    sel = (n_in >= np.uint32(min_views)) & (n_in.astype(f32) >= f32(min_share) * (n_in + n_out).astype(f32))
    votes = np.zeros((C * G ** 3, 2), np.uint16)
    votes[cells, 0], votes[cells, 1] = n_in, n_out
    chosen = np.zeros(C * G ** 3, np.uint8)
    chosen[cells[sel]] = 1
    return {"packed": packed, "cells": cells, "centres": w, "outcome": outcome, "pixel": pixel, "margin": margin, "votes": votes,
            "grid": np.packbits(chosen, bitorder="little")}


def mask_iou(a, b):
    """intersection over union of two masks (nonzero = set; tensors or arrays of one shape) -> float; 1.0 when both are empty"""
    if torch.is_tensor(a) or torch.is_tensor(b):
        a, b = torch.as_tensor(a) != 0, torch.as_tensor(b) != 0
        b = b.to(a.device)
        union = int((a | b).sum())
        return float(int((a & b).sum()) / union) if union else 1.0
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    union = int((a | b).sum())
    return float((a & b).sum() / union) if union else 1.0


@torch.no_grad()
def selection_masks(renderer, edit_grid, poses, intrinsics, H, W, threshold=0.5, min_opacity=0.5):
    """the way back from a selection to 2D masks: every view is rendered with `render_distill` (perturb=False, fp16 autocast) and a
    pixel is marked where its opacity `weights` is at least `min_opacity` and the selected cells hold at least `threshold` of it
    (`weights_edit / weights >= threshold`, taken as weights_edit >= threshold * weights).  edit_grid: an EditGrid or its uint8
    bitfield; poses [V, 4, 4] on the device.  -> uint8 [V, H, W] (1 = selected) on the device"""
    from ..rays import get_rays
    grid = edit_grid.get_grid() if hasattr(edit_grid, "get_grid") else edit_grid
    poses = poses.reshape(-1, 4, 4)
    out = torch.empty(poses.shape[0], int(H), int(W), dtype=torch.uint8, device=grid.device)
    for i in range(poses.shape[0]):
        ray = get_rays(poses[i:i + 1], intrinsics, H, W)
        with torch.autocast("cuda", dtype=torch.float16):
            res = renderer.render_distill(ray["rays_o"][0], ray["rays_d"][0], grid, perturb=False)
        wd, we = res["weights"].float(), res["weights_edit"].float()
        out[i] = ((wd >= min_opacity) & (we >= threshold * wd)).reshape(int(H), int(W)).to(torch.uint8)
    return out
