"""Insert the selected object of one trained NeRF (the SOURCE) into another scene (the DESTINATION) (csrc/insert.hip, where the
rule is written down in full; DESIGN.md section 4c "Scene insert").  The reference has no counterpart.  This is the other half of
region_transform.py, which moves an object inside ONE field and pastes it over what it meets: here the object crosses from one
field into another, and the two fields' samples can be blended exactly.

Nothing is resampled.  `SceneInsert` holds a similarity x_dst = s R (x_src - pivot) + position of the cells selected in the
source's grid.  At render time the destination's marcher walks a bitfield composed of the destination's occupancy and the box image
of the selected, occupied source cells (`insert_occupancy`: lae_insert_occupancy); every sample it emits is tested for a pre-image
in a selected and occupied source cell, and the rows that pass are compacted (`insert_route`: lae_insert_route); the destination
field runs on all rows, the source field on the compacted ones, and `insert_blend` (lae_insert_blend) joins the two results per
sample before composite_rays: mode "replace" pastes the object over what stood there (the region transform's semantics), mode "add"
sums the densities and averages the colours by density -- the exact mixture of two participating media, for soft edges and overlaps.
`render_inserted` is the operator loop of `render_eval(frame_loop=False)` with these steps in it; `insert_views` renders frames,
depths and opacities in the shapes save_mesh_tsdf / save_mesh_textured / evaluate_consistency take; `bake_insert` fine-tunes the
destination NeRF on inserted renders, as bake_region_transform does for a move.  `insert_route_numpy` / `insert_blend_numpy` /
`insert_occupancy_numpy` restate the kernels; with dtype=np.float32 they give their bits.

THE ROUNDING MARGIN of the image boxes (`insert_margin`), region_transform.py's derivation with two bounds.  u = 2^-24; bound_s
and bound_d are the source's and the destination's.  F is the forward map and G its inverse as formed in float64 (taken as exact),
M = fp32(F), Minv = fp32(G), each entry off by a factor (1 + u) at most.  For a 3x4 matrix K and a bound b write
A(K, b) = max over rows of (|k0| + |k1| + |k2|) b + |k3|: it bounds every partial sum of K (x, 1) for |x_i| <= b.
 (a) the route computes p^ = fl(Minv (x, 1)) for a DESTINATION sample x, |x_i| <= bound_d (the marcher clamps its positions); a
     component passes through at most 4 roundings, so |p^ - Minv x| <= 4.01 u A(Minv, bound_d), and |Minv x - G x| <=
     u A(Minv, bound_d): |p^ - G x| <= 5.01 u A(Minv, bound_d) per component.
 (b) x = F(G x) = F p^ - sR (p^ - G x); a row of sR has absolute sum <= s sqrt(3) < 3.47: |x - F p^| < 17.4 u A(Minv, bound_d).
 (c) the route only inserts |p^_i| <= bound_s, and bit(p^) names the SOURCE cell S through the marcher's coordinate statement on the
     source grid, whose one inexact operation (q / mip_bound + 1, a value below 2) is off by u 2 at most: p^ lies within
     2 u bound_s of S, its image within 3.47 * 2 u bound_s < 7 u bound_s of F(S).
 (d) F(S) lies in the box of F's corner images (a cube's image is convex); the corners are source points, |c_i| <= bound_s, and the
     kernel has fl(M corner) instead, off by 4.01 u A(M, bound_s) + u A(M, bound_s) = 5.01 u A(M, bound_s).
 (e) box end -+ margin is one more rounding, <= 1.01 u A(M, bound_s).
 (f) the DESTINATION cell range of the box comes from the very statement that gives x its cell in the destination grid, and that
     statement is monotone: nothing to add, whatever the destination's cascade and grid size.
Needed: u (6.02 A(M, bound_s) + 17.4 A(Minv, bound_d) + 7 bound_s).  Used: u (8 A(M, bound_s) + 32 A(Minv, bound_d) + 16 bound_s),
rounded up to fp32 -- a small fraction of a destination cell; a map whose margin reaches a quarter of one (0.5 / H_d) is refused.

OUT OF SCOPE: the fused frame loop (lae_render_frame); more than one insert per render; non-uniform scale and shear; relighting
the object to the new scene; shadows the object would cast or receive; grids of more than two cascades."""
import types

import numpy as np
import torch

from .. import raymarching
from ..backend import insert_backend as _backend
from .region_transform import (RegionTransform, _affine, _cell_coord, _compact_bits, _grid_shape, cell_index_numpy, morton_numpy,
                               own_cell_mask, seed_occupancy, unpack_bits)

MODES = {"replace": 0, "add": 1}                        # include/laenerf.h LAE_INSERT_*
SRC_ALIGN = 128                                         # rows the source field is called with: a multiple of the marcher's own alignment


def _A(K, bound):
    K = np.asarray(K, dtype=np.float64)
    return float((np.abs(K[:, :3]).sum(1) * float(bound) + np.abs(K[:, 3])).max())


def insert_margin_needed(M, Minv, bound_s, bound_d):
    """the bound the module docstring derives: u (6.02 A(M, bound_s) + 17.4 A(Minv, bound_d) + 7 bound_s)"""
    return 2.0 ** -24 * (6.02 * _A(M, bound_s) + 17.4 * _A(Minv, bound_d) + 7.0 * float(bound_s))


def insert_margin(M, Minv, bound_s, bound_d):
    """the image boxes' rounding allowance: u (8 A(M, bound_s) + 32 A(Minv, bound_d) + 16 bound_s), u = 2^-24, rounded up to fp32.
    M, Minv: the fp32 maps [3, 4]"""
    m = 2.0 ** -24 * (8.0 * _A(M, bound_s) + 32.0 * _A(Minv, bound_d) + 16.0 * float(bound_s))
    return float(np.nextafter(np.float32(m), np.float32(np.inf)))


def _grid_pair(grid, what):
    try:
        C, H = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError(f"SceneInsert: {what} must be (cascade, grid_size)") from None
    if C < 1 or C > 2:
        raise ValueError(f"SceneInsert: {what} has {C} cascades (1 and 2 are served)")
    return _grid_shape(C * H ** 3 // 8 if H >= 2 else 0, H, C)


class SceneInsert:
    """x_dst = s R (x_src - pivot) + position of the source cells selected in `src_sel`.

    src_sel    the selection, uint8 [C_s * H_s^3 / 8] in the SOURCE's density_bitfield layout (EditGrid.get_grid() /
               new_from_masks on the source scene; a tensor on the device or a numpy array).  Kept as given: `sel`.
    src_grid   (C_s, H_s) of the source renderer: cascade and grid_size; bound_s = 2^(C_s - 1)
    dst_grid   (C_d, H_d) of the destination renderer; the two grids may differ
    rotation   3x3 proper rotation (orthonormal to 1e-6, determinant +1)
    scale      uniform, in [0.5, 2]; anything else is refused
    pivot      3 numbers in SOURCE coordinates; default: the centroid of the centres of the selected cells of their own cascade
    position   3 numbers in DESTINATION coordinates: where the pivot lands; default: pivot
    mode       "replace" (the object is pasted over what stands there) or "add" (the two media are mixed exactly)
    The inverse map is formed in float64 and rounded once: Minv [3,4] for positions, Rt [3,3] = R^T for directions, inv_scale =
    fp32(1 / s); the forward map M [3,4] likewise; margin = insert_margin(M, Minv, bound_s, bound_d)."""

    def __init__(self, src_sel, src_grid=(1, 128), dst_grid=(1, 128), rotation=None, scale=1.0, pivot=None, position=None, mode="replace"):
        if mode not in MODES:
            raise ValueError(f"SceneInsert: mode must be one of {sorted(MODES)} (got {mode!r})")
        is_t = torch.is_tensor(src_sel)
        n_bytes = int(src_sel.numel()) if is_t else int(np.asarray(src_sel).size)
        if (src_sel.dtype != torch.uint8) if is_t else (np.asarray(src_sel).dtype != np.uint8):
            raise ValueError("SceneInsert: src_sel must be uint8")
        self.src_cascade, self.src_grid_size, self.src_bound = _grid_pair(src_grid, "src_grid")
        self.dst_cascade, self.dst_grid_size, self.dst_bound = _grid_pair(dst_grid, "dst_grid")
        if n_bytes != self.src_cascade * self.src_grid_size ** 3 // 8:
            raise ValueError(f"SceneInsert: src_sel holds {n_bytes} bytes, the source grid {self.src_cascade * self.src_grid_size ** 3 // 8}")
        self.sel = src_sel
        self.mode, self.mode_id = mode, MODES[mode]
        R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
        s = float(scale)
        if not (0.5 <= s <= 2.0):
            raise ValueError(f"SceneInsert: scale must lie in [0.5, 2] (got {scale})")
        if not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
            raise ValueError("SceneInsert: rotation must be a proper rotation (orthonormal, determinant +1)")
        if pivot is None:
            pivot = self.selection_centroid()
        p = np.asarray(pivot, dtype=np.float64).reshape(3)
        if not np.isfinite(p).all():
            raise ValueError("SceneInsert: pivot must be finite")
        q = p.copy() if position is None else np.asarray(position, dtype=np.float64).reshape(3)
        if not np.isfinite(q).all():
            raise ValueError("SceneInsert: position must be finite")
        self.rotation, self.scale, self.pivot, self.position = R, s, p, q
        F = np.concatenate([s * R, (q - s * R @ p)[:, None]], 1)                    # x_dst = sR x_src + (position - sR pivot)
        G = np.concatenate([R.T / s, (-(R.T / s) @ F[:, 3])[:, None]], 1)
        self.M = np.ascontiguousarray(F, dtype=np.float32)
        self.Minv = np.ascontiguousarray(G, dtype=np.float32)
        self.Rt = np.ascontiguousarray(R.T, dtype=np.float32)
        self.inv_scale = float(np.float32(1.0 / s))
        self.margin = insert_margin(self.M, self.Minv, self.src_bound, self.dst_bound)
        if not self.margin < 0.5 / self.dst_grid_size:
            raise ValueError("SceneInsert: the placement is so far out that fp32 no longer resolves a quarter of a destination cell")

    @property
    def src_grid(self):
        return self.src_bound, self.src_cascade, self.src_grid_size

    @property
    def dst_grid(self):
        return self.dst_bound, self.dst_cascade, self.dst_grid_size

    @property
    def src_bytes(self):
        return self.src_cascade * self.src_grid_size ** 3 // 8

    @property
    def dst_bytes(self):
        return self.dst_cascade * self.dst_grid_size ** 3 // 8

    def sel_numpy(self):
        return self.sel.detach().cpu().numpy() if torch.is_tensor(self.sel) else np.asarray(self.sel)

    def selection_centroid(self):
        """RegionTransform.selection_centroid on the source grid (float64 [3]); zeros for an empty selection"""
        return RegionTransform.selection_centroid(types.SimpleNamespace(cascade=self.src_cascade, grid_size=self.src_grid_size,
                                                                        sel_numpy=self.sel_numpy))

    def sel_on(self, device):
        """the selection as a contiguous uint8 tensor on `device` (cached)"""
        cache = getattr(self, "_sel_dev", None)
        if cache is None or cache.device != torch.device(device):
            src = self.sel if torch.is_tensor(self.sel) else torch.from_numpy(np.ascontiguousarray(self.sel))
            cache = self._sel_dev = src.to(device).contiguous()
        return cache


# ------------------------------------------------------------------------------------------------------------ kernel wrappers
def _same_storage(a, b):
    return a.numel() > 0 and b.numel() > 0 and a.data_ptr() == b.data_ptr()


def _check_bitfield(name, what, t, n_bytes):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != n_bytes:
        raise ValueError(f"{name}: {what} must be a contiguous uint8 tensor of {n_bytes} values")


def insert_route(ins, xyzs, dirs, src_occ, deltas=None, out=None):
    """lae_insert_route on the destination marcher's rows xyzs, dirs fp32 [M, 3] (deltas fp32 [M, 2] or None) on the device; src_occ:
    the SOURCE's density_bitfield -> (slot int32 [M], xyzs_src [M, 3], dirs_src [M, 3], count int32 [1]); the first count rows of
    xyzs_src / dirs_src are the inserted rows' pre-images, the rest is left as it was.  out: these four buffers of the caller's;
    without it this wrapper allocates them with torch (the two row arrays zeroed).  The entry itself reads nothing back and
    allocates nothing, so the call can be captured -- after one eager call of the same size, which sizes the backend's scratch."""
    for name, t in (("xyzs", xyzs), ("dirs", dirs)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError(f"insert_route: {name} must be a contiguous fp32 [M, 3] tensor")
    M = xyzs.shape[0]
    if dirs.shape[0] != M:
        raise ValueError("insert_route: xyzs and dirs must have one row count")
    if deltas is not None and (not torch.is_tensor(deltas) or deltas.dtype != torch.float32 or deltas.shape != (M, 2) or
                               not deltas.is_contiguous()):
        raise ValueError("insert_route: deltas must be a contiguous fp32 [M, 2] tensor")
    _check_bitfield("insert_route", "src_occ", src_occ, ins.src_bytes)
    if out is None:
        out = (torch.empty(M, dtype=torch.int32, device=xyzs.device), torch.zeros_like(xyzs), torch.zeros_like(dirs),
               torch.empty(1, dtype=torch.int32, device=xyzs.device))
    try:
        slot, xs, ds, count = out
    except (TypeError, ValueError):
        raise ValueError("insert_route: out must hold (slot, xyzs_src, dirs_src, count)") from None
    if not all(torch.is_tensor(t) and t.is_contiguous() for t in out) or slot.dtype != torch.int32 or slot.shape != (M,) or \
            count.dtype != torch.int32 or count.numel() != 1 or any(t.dtype != torch.float32 or t.shape != (M, 3) for t in (xs, ds)):
        raise ValueError("insert_route: out must hold contiguous int32 [M], fp32 [M, 3], fp32 [M, 3] and int32 [1] tensors")
    if _same_storage(xs, ds) or any(_same_storage(o, i) for o in (xs, ds) for i in (xyzs, dirs)):
        raise ValueError("insert_route: out must not alias xyzs, dirs or itself (the rows are compacted, not rewritten in place)")
    _backend.route(xyzs, dirs, deltas, ins.sel_on(xyzs.device), src_occ, ins.Minv, ins.Rt, ins.src_grid, slot, xs, ds, count)
    return slot, xs, ds, count


def insert_blend(ins, sigma_d, rgb_d, sigma_s, rgb_s, slot, out=None, inplace=False):
    """lae_insert_blend: the destination field's sigma_d [M], rgb_d [M, 3] and the source field's sigma_s [n], rgb_s [n, 3] on the
    compacted rows (each fp16 or fp32), joined through slot int32 [M] by ins.mode with ins.inv_scale -> (sigma fp32 [M], rgb fp32
    [M, 3]).  out: the two buffers of the caller's; inplace=True writes into sigma_d / rgb_d, which must then be fp32."""
    M = slot.shape[0] if torch.is_tensor(slot) and slot.dim() == 1 else -1
    ok = lambda t, shape: torch.is_tensor(t) and t.dtype in (torch.float16, torch.float32) and tuple(t.shape) == shape and t.is_contiguous()
    if M < 0 or slot.dtype != torch.int32 or not slot.is_contiguous():
        raise ValueError("insert_blend: slot must be a contiguous int32 [M] tensor")
    if not ok(sigma_d, (M,)) or not ok(rgb_d, (M, 3)):
        raise ValueError("insert_blend: sigma_d / rgb_d must be contiguous fp16 or fp32 [M] / [M, 3] tensors")
    n = sigma_s.shape[0] if torch.is_tensor(sigma_s) and sigma_s.dim() == 1 else -1
    if n < 0 or not ok(sigma_s, (n,)) or not ok(rgb_s, (n, 3)):
        raise ValueError("insert_blend: sigma_s / rgb_s must be contiguous fp16 or fp32 [n] / [n, 3] tensors")
    if inplace:
        if out is not None or sigma_d.dtype != torch.float32 or rgb_d.dtype != torch.float32:
            raise ValueError("insert_blend: inplace=True takes fp32 sigma_d / rgb_d and no out")
        out = (sigma_d, rgb_d)
    elif out is None:
        out = (torch.empty(M, dtype=torch.float32, device=slot.device), torch.empty(M, 3, dtype=torch.float32, device=slot.device))
    try:
        sigma, rgb = out
    except (TypeError, ValueError):
        raise ValueError("insert_blend: out must hold (sigma, rgb)") from None
    if not ok(sigma, (M,)) or not ok(rgb, (M, 3)) or sigma.dtype != torch.float32 or rgb.dtype != torch.float32:
        raise ValueError("insert_blend: out must hold contiguous fp32 [M] and [M, 3] tensors")
    if _same_storage(sigma, rgb) or any(_same_storage(o, i) for o in (sigma, rgb) for i in (sigma_s, rgb_s, slot)) or \
            _same_storage(sigma, rgb_d) or _same_storage(rgb, sigma_d) or \
            (_same_storage(sigma, sigma_d) and sigma_d.dtype != torch.float32) or (_same_storage(rgb, rgb_d) and rgb_d.dtype != torch.float32):
        raise ValueError("insert_blend: out may be the fp32 sigma_d / rgb_d it replaces and must alias nothing else")
    _backend.blend(sigma_d, rgb_d, sigma_s, rgb_s, slot, ins.inv_scale, ins.mode_id, sigma, rgb)
    return sigma, rgb


def insert_occupancy(ins, dst_occ, src_occ, out=None):
    """lae_insert_occupancy: the bitfield the destination's marcher walks for `ins` -- dst_occ (the destination's occupancy) plus the
    box image of every selected, occupied source cell (src_occ: the source's occupancy); uint8, density_bitfield's layout, on the
    device -> uint8 of dst_occ's size (`out` when given; every byte is written; not dst_occ itself)"""
    _check_bitfield("insert_occupancy", "dst_occ", dst_occ, ins.dst_bytes)
    _check_bitfield("insert_occupancy", "src_occ", src_occ, ins.src_bytes)
    if out is None:
        out = torch.empty_like(dst_occ)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.numel() != dst_occ.numel() or not out.is_contiguous() or \
            _same_storage(out, dst_occ) or _same_storage(out, src_occ):
        raise ValueError("insert_occupancy: out must be another contiguous uint8 tensor of dst_occ's size")
    _backend.occupancy(dst_occ, ins.sel_on(dst_occ.device), src_occ, ins.M, ins.margin, ins.src_grid, ins.dst_grid, out)
    return out


# ------------------------------------------------------------------------------------------------------------ numpy restatements
def insert_route_numpy(ins, xyzs, dirs, src_occ, deltas=None, dtype=np.float64):
    """lae_insert_route in `dtype` (np.float32: the kernel's statements in its order, hence its bits) -> dict: slot int32 [M], count,
    xyzs_src, dirs_src [count, 3] in `dtype`, inserted bool [M], p [M, 3] (every row's pre-image)"""
    dt = np.dtype(dtype).type
    C, H, bound = ins.src_cascade, ins.src_grid_size, dt(ins.src_bound)
    x = np.asarray(xyzs).astype(dt).reshape(-1, 3)
    d = np.asarray(dirs).astype(dt).reshape(-1, 3)
    both = unpack_bits(ins.sel_numpy()) & unpack_bits(src_occ)
    assert both.size == C * H ** 3, "src_occ and the selection must hold the source grid's bits"
    Minv, Rt = ins.Minv.astype(dt), ins.Rt.astype(dt)
    p = np.stack([_affine(Minv[k], x[:, 0], x[:, 1], x[:, 2]) for k in range(3)], -1)
    with np.errstate(all="ignore"):
        inside = (np.abs(p) <= bound).all(-1)
        q = np.stack([(Rt[k, 0] * d[:, 0] + Rt[k, 1] * d[:, 1]) + Rt[k, 2] * d[:, 2] for k in range(3)], -1)
    inserted = inside & both[cell_index_numpy(np.where(inside[:, None], p, dt(0)), C, H, dt)[0]]
    if deltas is not None:
        inserted &= np.asarray(deltas).reshape(-1, 2)[:, 0] != 0
    slot = np.where(inserted, np.cumsum(inserted) - 1, -1).astype(np.int32)
    return {"slot": slot, "count": int(inserted.sum()), "xyzs_src": p[inserted], "dirs_src": q[inserted], "inserted": inserted, "p": p}


def insert_blend_numpy(ins, sigma_d, rgb_d, sigma_s, rgb_s, slot, dtype=np.float64):
    """lae_insert_blend in `dtype` (np.float32: the kernel's bits) -> (sigma [M], rgb [M, 3]); the inputs are converted exactly"""
    dt = np.dtype(dtype).type
    sd, rd = np.asarray(sigma_d).astype(dt).reshape(-1), np.asarray(rgb_d).astype(dt).reshape(-1, 3)
    ss_all, rs_all = np.asarray(sigma_s).astype(dt).reshape(-1), np.asarray(rgb_s).astype(dt).reshape(-1, 3)
    slot = np.asarray(slot).reshape(-1)
    hit = (slot >= 0) & (slot < ss_all.shape[0])
    k = np.where(hit, slot, 0)
    if ss_all.shape[0] == 0:
        return sd.copy(), rd.copy()
    ss = ss_all[k] * dt(np.float32(ins.inv_scale))
    rs = rs_all[k]
    if ins.mode == "replace":
        return np.where(hit, ss, sd), np.where(hit[:, None], rs, rd)
    with np.errstate(all="ignore"):
        sigma = sd + ss
        w = ss / sigma
        mixed = rd + w[:, None] * (rs - rd)
    rgb = np.where((hit & (sigma > 0))[:, None], mixed, rd)
    return np.where(hit, sigma, sd), rgb


def insert_occupancy_numpy(ins, dst_occ, src_occ, dtype=np.float64):
    """lae_insert_occupancy in `dtype` (np.float32: the kernel's bits) -> uint8 bitfield of dst_occ's size"""
    dt = np.dtype(dtype).type
    Cs, Hs, Cd, Hd = ins.src_cascade, ins.src_grid_size, ins.dst_cascade, ins.dst_grid_size
    Hs3, Hd3 = Hs ** 3, Hd ** 3
    out = unpack_bits(dst_occ).copy()
    occ_b, sel_b = unpack_bits(src_occ), unpack_bits(ins.sel_numpy())
    assert out.size == Cd * Hd3 and occ_b.size == Cs * Hs3 and sel_b.size == Cs * Hs3, "the bitfields must hold their grids' bits"
    src = np.flatnonzero(occ_b & sel_b & own_cell_mask(Cs, Hs, layer=True))
    if src.size == 0:
        return np.packbits(out, bitorder="little")
    cas, m = src // Hs3, (src % Hs3).astype(np.uint32)
    n = [_compact_bits(m), _compact_bits(m >> np.uint32(1)), _compact_bits(m >> np.uint32(2))]
    mb = np.ldexp(dt(1.0), cas.astype(np.int32)).astype(dt)
    rH = dt(1.0) / dt(Hs)
    face = [[(((n[a] + k).astype(dt) * rH) * dt(2.0) - dt(1.0)) * mb for k in (0, 1)] for a in range(3)]
    M, margin = ins.M.astype(dt), dt(np.float32(ins.margin))
    lo = hi = None
    for k in range(8):
        v = np.stack([_affine(M[a], face[0][k & 1], face[1][(k >> 1) & 1], face[2][k >> 2]) for a in range(3)], -1)
        lo = v if lo is None else np.minimum(lo, v)
        hi = v if hi is None else np.maximum(hi, v)
    lo, hi = lo - margin, hi + margin
    for t in range(Cd):
        tb, trb = dt(2.0 ** t), dt(2.0 ** -t)
        with np.errstate(all="ignore"):
            live = ~((lo > tb).any(-1) | (hi < -tb).any(-1))
        if not live.any():
            continue
        i0 = [_cell_coord(lo[live, a], trb, Hd, dt) for a in range(3)]
        i1 = [_cell_coord(hi[live, a], trb, Hd, dt) for a in range(3)]
        ext = [int((i1[a] - i0[a]).max()) + 1 for a in range(3)]
        for dz in range(ext[2]):
            z = i0[2] + dz
            for dy in range(ext[1]):
                y = i0[1] + dy
                for dx in range(ext[0]):
                    x = i0[0] + dx
                    ok = (x <= i1[0]) & (y <= i1[1]) & (z <= i1[2])
                    out[t * Hd3 + morton_numpy(x[ok], y[ok], z[ok])] = True
    return np.packbits(out, bitorder="little")


# ------------------------------------------------------------------------------------------------------------ rendering
def _check_renderers(name, dst, src, ins):
    if dst.density_bitfield.device != src.density_bitfield.device:
        raise ValueError(f"{name}: both renderers must sit on one device")
    for r, grid, which in ((src, ins.src_grid, "source"), (dst, ins.dst_grid, "destination")):
        if (float(r.bound), int(r.cascade), int(r.grid_size)) != (float(grid[0]), int(grid[1]), int(grid[2])):
            raise ValueError(f"{name}: the insert was made for another {which} grid (bound, cascade, grid_size)")


@torch.no_grad()
def render_inserted(dst_renderer, src_renderer, ins, rays_o, rays_d, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4,
                    scale_depth=True, dens_grid=None, device_compaction=True, frame_loop=False, want_stats=False, row_budget=0,
                    image_hw=None, tile_hw=(8, 4), max_n_step=8):
    """render_eval(frame_loop=False) of the destination scene with the source's selected object in it: the operator loop, marching
    insert_occupancy(ins, the destination's bitfield, src_renderer.density_bitfield); per iteration march_rays, insert_route, the
    destination model on all rows, the source model on the first `count` compacted rows (rounded up to a multiple of 128 rows, as
    the marcher pads its own: the padding is zeros or rows routed earlier), the source's density_scale, insert_blend and
    composite_rays.  `count` is read on the host: ONE more host read per iteration than render_eval's operator loop makes, and the
    source model is not called at all while it is 0.  Arguments and the returned dict are render_eval's; dens_grid replaces
    dst_renderer.density_bitfield as the DESTINATION's occupancy; frame_loop is accepted and ignored (the device-resident frame
    loop does not know the insert); image_hw keeps render_eval's image-tile ray order; want_stats adds "inserted_rows" and
    "source_calls" to render_eval's stats."""
    if image_hw is not None and rays_o.numel() == 3 * image_hw[0] * image_hw[1] and image_hw[0] % tile_hw[0] == 0 and \
            image_hw[1] % tile_hw[1] == 0 and not (torch.is_tensor(bg_color) and bg_color.numel() > 3):
        idx, inv = dst_renderer._tile_perm(image_hw[0], image_hw[1], tile_hw[0], tile_hw[1], rays_o.device)
        res = render_inserted(dst_renderer, src_renderer, ins, rays_o.reshape(-1, 3)[idx], rays_d.reshape(-1, 3)[idx], bg_color, perturb,
                              dt_gamma, max_steps, T_thresh, scale_depth, dens_grid, device_compaction, False, want_stats, row_budget,
                              max_n_step=max_n_step)
        return {k: (v[inv] if torch.is_tensor(v) and v.shape[:1] == inv.shape else v) for k, v in res.items()}
    _check_renderers("render_inserted", dst_renderer, src_renderer, ins)
    r = dst_renderer
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    occ = r.density_bitfield if dens_grid is None else dens_grid
    src_occ = src_renderer.density_bitfield.contiguous()
    grid = insert_occupancy(ins, occ.contiguous(), src_occ)
    N, device = rays_o.shape[0], rays_o.device
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, r.aabb_infer, r.min_near)
    weights_sum = torch.zeros(N, dtype=torch.float32, device=device)
    depth = torch.zeros(N, dtype=torch.float32, device=device)
    image = torch.zeros(N, 3, dtype=torch.float32, device=device)
    n_alive = N
    rays_alive = torch.arange(n_alive, dtype=torch.int32, device=device)
    rays_t = nears.clone()
    step = 0
    iterations = rows = inserted_rows = source_calls = 0
    budget = max(N, int(row_budget))
    while step < max_steps and n_alive > 0:
        n_step = max(min(budget // n_alive, max_n_step), 1)
        iterations += 1; rows += n_alive * n_step
        xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, r.bound, grid, r.cascade,
                                                    r.grid_size, nears, fars, 128, perturb if step == 0 else False, dt_gamma, max_steps)
        slot, xyzs_src, dirs_src, count = insert_route(ins, xyzs, dirs, src_occ, deltas=deltas)
        sigmas, rgbs = r.model(xyzs, dirs)
        sigmas = r.density_scale * sigmas
        n_src = int(count.item())                                             # the one host read the insert adds
        if n_src > 0:
            n_pad = min(-(-n_src // SRC_ALIGN) * SRC_ALIGN, xyzs_src.shape[0])
            sigmas_s, rgbs_s = src_renderer.model(xyzs_src[:n_pad], dirs_src[:n_pad])
            sigmas_s = src_renderer.density_scale * sigmas_s
            inserted_rows += n_src; source_calls += 1
        else:
            sigmas_s, rgbs_s = sigmas.new_empty(0), rgbs.new_empty(0, 3)
        sigmas, rgbs = insert_blend(ins, sigmas.contiguous().view(-1), rgbs.contiguous().view(-1, 3), sigmas_s.contiguous().view(-1),
                                    rgbs_s.contiguous().view(-1, 3), slot)
        raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh)
        if device_compaction:
            rays_alive, n_out = raymarching.compact_rays_alive(rays_alive, n_alive)
            n_alive = int(n_out.item())
        else:
            rays_alive = rays_alive[rays_alive >= 0]
            n_alive = rays_alive.shape[0]
        step += n_step
    image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
    if scale_depth:
        depth = torch.clamp(depth - nears, min=0) / (fars - nears)
    out = {"image": image, "depth": depth, "weights_sum": weights_sum}
    if want_stats:
        out["stats"] = {"iterations": iterations, "rows": rows, "steps": step, "alive_at_end": n_alive, "inserted_rows": inserted_rows,
                        "source_calls": source_calls}
    return out


@torch.no_grad()
def insert_views(dst_renderer, src_renderer, ins, poses, intrinsics, H, W, bg_color=1.0, **render_kw):
    """the composed scene from every pose [n, 4, 4] (cam2world, on the device) -> (frames uint8 [n, H, W, 3] by lae_eval_view's byte
    rule, depths fp32 [n, H*W] = the raw `sum w t`, opacities fp32 [n, H*W] = weights_sum): transform_views' shapes, what
    save_mesh_tsdf / save_mesh_textured(frames=, depths=, opacities=) and evaluate_consistency(frames=) take.  Rendered as
    render_packed_views renders: perturb=False, scale_depth=False, over white, fp16 autocast, both models in eval mode."""
    from .. import metrics as M
    from ..rays import get_rays
    H, W = int(H), int(W)
    poses = poses.reshape(-1, 4, 4)
    n, dev = poses.shape[0], dst_renderer.density_bitfield.device
    frames = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    depths = torch.empty(n, H * W, dtype=torch.float32, device=dev)
    opacities = torch.empty(n, H * W, dtype=torch.float32, device=dev)
    scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    was_training = (dst_renderer.model.training, src_renderer.model.training)
    dst_renderer.model.eval(); src_renderer.model.eval()
    try:
        for i in range(n):
            ray = get_rays(poses[i:i + 1], intrinsics, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = render_inserted(dst_renderer, src_renderer, ins, ray["rays_o"][0], ray["rays_d"][0], bg_color=bg_color, perturb=False,
                                      scale_depth=False, image_hw=(H, W), **render_kw)
            M.eval_view(res["image"].float().contiguous(), None, rgb_u8=frames[i], scratch=scratch)
            depths[i], opacities[i] = res["depth"].float(), res["weights_sum"].float()
    finally:
        src_renderer.model.train(was_training[1])
        dst_renderer.model.train(was_training[0])
    return frames, depths, opacities


def bake_insert(dst_renderer, optimizer, data, src_renderer, ins, steps=3000, lr=1e-2, depth_sup=False, trainer_kw=None, depth_weight=1e-3,
                seed=True, render_kw=None):
    """bake the insert into the DESTINATION NeRF, step for step as bake_region_transform bakes a move: every training pose of `data`
    (the destination's) is rendered with the object in it (render_inserted over black, fp16 autocast, eval mode), a NEW
    ResidentImages is built from the RGBA frames (straight colour, alpha = the rendered opacity; fp16; poses, intrinsics, bound,
    mode, bg and colour space of `data`), the student's occupancy is seeded with the composed bitfield (seed_occupancy; seed=False
    leaves it out -- the first groups then never march the object's place), and the existing Trainer runs `steps` steps on the
    destination (distill_steps rounds them to whole groups); the source renderer is only read.  depth_sup=True: the new data carries
    depth planes (`sum w t / opacity` where the opacity exceeds 0.5, else 0 = unsupervised) and the Trainer gets depth_weight.
    -> (data_new, trainer)"""
    from ..data import ResidentImages
    from ..rays import get_rays
    from ..trainer import Trainer
    from .distill import distill_steps
    _check_renderers("bake_insert", dst_renderer, src_renderer, ins)
    H, W, n = data.H, data.W, data.n_img
    dev = data.images.device
    images = torch.empty(n, H, W, 4, dtype=torch.float16, device=dev)
    plane = torch.zeros(n, H, W, dtype=torch.float32, device=dev) if depth_sup else None
    was_training = (dst_renderer.model.training, src_renderer.model.training)
    dst_renderer.model.eval(); src_renderer.model.eval()
    try:
        with torch.no_grad():
            for i in range(n):
                ray = get_rays(data.poses[i:i + 1], data.intrinsics, H, W)
                with torch.autocast("cuda", dtype=torch.float16):
                    res = render_inserted(dst_renderer, src_renderer, ins, ray["rays_o"][0], ray["rays_d"][0], bg_color=0, perturb=False,
                                          scale_depth=False, image_hw=(H, W), **(render_kw or {}))
                ws = res["weights_sum"].float().clamp(0, 1)
                img = res["image"].float()
                rgb = torch.where(ws[:, None] > 0, img / ws.clamp(min=1e-6)[:, None], torch.zeros_like(img)).clamp(0, 1)
                images[i] = torch.cat([rgb, ws[:, None]], 1).reshape(H, W, 4).to(torch.float16)
                if depth_sup:
                    plane[i] = torch.where(ws > 0.5, res["depth"].float() / ws.clamp(min=1e-6), torch.zeros_like(ws)).reshape(H, W)
            if seed:
                seed_occupancy(dst_renderer, insert_occupancy(ins, dst_renderer.density_bitfield.contiguous(),
                                                              src_renderer.density_bitfield.contiguous()))
    finally:
        src_renderer.model.train(was_training[1])
        dst_renderer.model.train(was_training[0])
    data_new = ResidentImages(images, data.poses, data.intrinsics, bound=data.bound, min_near=data.min_near, mode=data.mode, bg=data.bg,
                              color_space=data.color_space, seed=data.seed, device=dev)
    kw = dict(trainer_kw or {})
    if depth_sup:
        data_new.set_depths(plane)
        kw.setdefault("depth_weight", depth_weight)
    tr = Trainer(dst_renderer, optimizer, data_new, iters=steps, lr=lr, **kw)
    tr.train(distill_steps(steps))
    return data_new, tr
