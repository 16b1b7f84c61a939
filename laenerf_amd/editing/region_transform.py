"""Move, rotate, scale, copy or delete the selected region of a trained NeRF (csrc/region.hip, where the rule is written down
in full; DESIGN.md section 4c "Region transform").  The reference has no counterpart: every editing stage it has changes
appearance, none changes where the selected object is.

Nothing is resampled.  `RegionTransform` holds a similarity x_new = s R (x - pivot) + pivot + t of the selection; at render time
every sample the marcher emits is looked up where the object CAME FROM (`region_warp`: lae_region_warp), the marcher walks a
bitfield composed of the kept scene and the box image of the selection (`region_occupancy`: lae_region_occupancy), and the
density is scaled per sample.  `render_transformed` is the operator loop of `render_eval(frame_loop=False)` with these two steps
in it -- the device-resident frame loop (lae_render_frame) is not touched, so a transformed preview costs what the operator loop
costs.  `transform_views` renders frames, depths and opacities in the shapes save_mesh_tsdf / save_mesh_textured /
evaluate_consistency take, and `bake_region_transform` fine-tunes the NeRF on transformed renders, as distill_nerf does for a
recolouring.  `region_warp_numpy` / `region_occupancy_numpy` restate the kernels; with dtype=np.float32 they give their bits.

THE ROUNDING MARGIN of the image boxes (`rounding_margin`).  u = 2^-24.  F is the forward map and G its inverse as formed in
float64 (taken as exact), M = fp32(F), Minv = fp32(G), each entry off by a factor (1 + u) at most.  For a 3x4 matrix K write
A(K) = max over rows of (|k0| + |k1| + |k2|) bound + |k3|: it bounds every partial sum of K (x, 1) for |x_i| <= bound.
 (a) the warp computes p^ = fl(Minv (x, 1)); a component passes through at most 4 roundings, so |p^ - Minv x| <= 4.01 u A(Minv),
     and |Minv x - G x| <= u A(Minv): |p^ - G x| <= 5.01 u A(Minv) per component.
 (b) x = F(G x) = F p^ - sR (p^ - G x); a row of sR has absolute sum <= s sqrt(3) < 3.47: |x - F p^| < 17.4 u A(Minv).
 (c) sel(p^) names cell S through the marcher's coordinate statement, whose one inexact operation (q / mip_bound + 1, a value
     below 2) is off by u 2 at most: p^ lies within 2 u bound of S, its image within 3.47 * 2 u bound < 7 u bound of F(S).
 (d) F(S) lies in the box of F's corner images (a cube's image is convex); the kernel has fl(M corner) instead, off by
     4.01 u A(M) + u A(M) = 5.01 u A(M).
 (e) box end -+ margin is one more rounding, <= 1.01 u A(M).
 (f) the cell range of the box comes from the very statement that gives x its cell, and that statement is monotone: nothing to add.
Needed: u (6.02 A(M) + 17.4 A(Minv) + 7 bound).  Used: u (8 A(M) + 32 A(Minv) + 16 bound), rounded up to fp32 -- about 7e-6 at
bound 1 against a cell side of 1.6e-2: a small fraction of a cell, never a whole one (the kernel refuses a quarter cell).

OUT OF SCOPE: non-uniform scale and shear; more than one transform per render; the fused frame loop (lae_render_frame);
inpainting what was behind a removed object (the hole shows whatever the NeRF holds there); blending where the moved object
overlaps other content (the moved object is pasted over it)."""
import numpy as np
import torch

from .. import raymarching
from ..backend import region_backend as _backend

MODES = {"move": 0, "copy": 1, "delete": 2}            # include/laenerf.h LAE_REGION_*
MOVED, VACATED, KEPT = 0, 1, 2                          # region_warp_numpy's branch of a row


# ------------------------------------------------------------------------------------------------------------ grid helpers (numpy)
def _spread10(v):
    v = v.astype(np.uint32)
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return v


def morton_numpy(x, y, z):
    """raymarch_common.h morton_encode on integer arrays -> int64"""
    return (_spread10(x) | (_spread10(y) << np.uint32(1)) | (_spread10(z) << np.uint32(2))).astype(np.int64)


def _compact_bits(x):
    x = x.astype(np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xc30c30c3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0f00f00f)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xff0000ff)
    return ((x | (x >> np.uint32(16))) & np.uint32(0x0000ffff)).astype(np.int64)


def _grid_shape(n_bytes, grid_size, cascade=None, bound=None):
    """-> (C, H, bound) of a bitfield of n_bytes; ValueError unless H is a power of two in [4, 128], C is 1 or 2 and
    bound = 2^(C-1) (the grids lae_region_* serve)"""
    H = int(grid_size)
    if H < 4 or H > 128 or H & (H - 1):
        raise ValueError("region transform: grid_size must be a power of two in [4, 128]")
    if n_bytes * 8 % H ** 3:
        raise ValueError(f"region transform: a bitfield of {n_bytes} bytes holds no whole number of {H}^3 cascades")
    C = n_bytes * 8 // H ** 3
    if C < 1 or C > 2 or (cascade is not None and int(cascade) != C):
        raise ValueError(f"region transform: the bitfield holds {C} cascades (cascade={cascade}; 1 and 2 are served)")
    if bound is not None and float(bound) != float(2 ** (C - 1)):
        raise ValueError(f"region transform: bound must be 2^(cascade - 1) = {2 ** (C - 1)} (got {bound})")
    return C, H, float(2 ** (C - 1))


def coords_table(H):
    m = np.arange(H ** 3, dtype=np.uint32)
    return _compact_bits(m), _compact_bits(m >> np.uint32(1)), _compact_bits(m >> np.uint32(2))


def own_cell_mask(C, H, layer=False):
    """bool [C * H^3] in the bitfield's bit order: the cells of their own cascade (cascade 0; at c > 0 not all three coordinates in
    [H/4, 3H/4)).  layer=True: the image part's source cells, which add the layer with a coordinate equal to H/4."""
    nx, ny, nz = coords_table(H)
    lo, hi = H // 4 + (1 if layer else 0), 3 * (H // 4)
    inner = ((nx >= lo) & (nx < hi)) & ((ny >= lo) & (ny < hi)) & ((nz >= lo) & (nz < hi))
    out = np.ones((C, H ** 3), bool)
    out[1:] = ~inner
    return out.reshape(-1)


def unpack_bits(bitfield):
    return np.unpackbits(np.asarray(bitfield, dtype=np.uint8).reshape(-1), bitorder="little").astype(bool)


def _cascade_of(amax, C):
    """raymarch_common.h cascade_of: frexp's exponent clamped to [0, C - 1]"""
    with np.errstate(all="ignore"):
        e = np.frexp(amax)[1]
    return np.clip(e, 0, C - 1).astype(np.int64)


def _cell_coord(v, rb, H, dt):
    """probe_at's coordinate statement (int)clamp((0.5 * fma(v, rb, 1)) * H, 0, H - 1); rb is a power of two, so the fma is one
    rounded addition"""
    with np.errstate(all="ignore"):
        c = (dt(0.5) * (v * rb + dt(1.0))) * dt(H)
        c = np.minimum(dt(H - 1), np.maximum(dt(0.0), c))            # fmaxf / fminf: a NaN gives 0
        c = np.where(np.isnan(c), dt(0.0), c)
    return c.astype(np.int64)


def cell_index_numpy(q, C, H, dtype=np.float32):
    """bit index (cascade * H^3 + Morton) of the cell of q [n, 3] at q's own cascade -> (index int64 [n], level int64 [n])"""
    dt = np.dtype(dtype).type
    q = np.asarray(q).astype(dt)
    level = _cascade_of(np.abs(q).max(-1), C)
    rb = np.ldexp(dt(1.0), -level.astype(np.int32)).astype(dt)
    n = [_cell_coord(q[:, k], rb, H, dt) for k in range(3)]
    return level * H ** 3 + morton_numpy(n[0], n[1], n[2]), level


def _affine(m, x, y, z):
    """((m0 x + m1 y) + m2 z) + m3 in the arrays' dtype, one rounding per operation"""
    with np.errstate(all="ignore"):
        return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


# ------------------------------------------------------------------------------------------------------------ the transform
def rounding_margin(M, Minv, bound):
    """the image boxes' rounding allowance (the module docstring derives it): u (8 A(M) + 32 A(Minv) + 16 bound), u = 2^-24,
    rounded up to fp32.  M, Minv: the fp32 maps [3, 4]"""
    A = lambda K: float((np.abs(K[:, :3].astype(np.float64)).sum(1) * bound + np.abs(K[:, 3].astype(np.float64))).max())
    m = 2.0 ** -24 * (8.0 * A(np.asarray(M)) + 32.0 * A(np.asarray(Minv)) + 16.0 * float(bound))
    return float(np.nextafter(np.float32(m), np.float32(np.inf)))


class RegionTransform:
    """x_new = s R (x - pivot) + pivot + t of the cells selected in `edit_bitfield`.

    edit_bitfield  the selection, uint8 [cascade * grid_size^3 / 8] in density_bitfield's layout (EditGrid.get_grid(); a tensor on
                   the device or a numpy array).  Kept as given: `sel`.
    rotation       3x3 proper rotation (orthonormal to 1e-6, determinant +1)
    translation    3 numbers, world units
    scale          uniform, in [0.5, 2]; anything else is refused
    pivot          3 numbers; default: the centroid of the centres of the selected cells of their own cascade
    mode           "move" (the object leaves its place), "copy" (it stays and appears a second time), "delete" (it leaves and
                   appears nowhere: the transform is ignored, there is no image)
    The inverse map is formed in float64 and rounded once: Minv [3,4] for positions, Rt [3,3] = R^T for directions, inv_scale =
    fp32(1 / s); the forward map M [3,4] likewise; margin = rounding_margin(M, Minv, bound)."""

    def __init__(self, edit_bitfield, rotation=None, translation=None, scale=1.0, pivot=None, mode="move", grid_size=128, cascade=None,
                 bound=None):
        if mode not in MODES:
            raise ValueError(f"RegionTransform: mode must be one of {sorted(MODES)} (got {mode!r})")
        n_bytes = int(edit_bitfield.numel()) if torch.is_tensor(edit_bitfield) else int(np.asarray(edit_bitfield).size)
        if (edit_bitfield.dtype != torch.uint8) if torch.is_tensor(edit_bitfield) else (np.asarray(edit_bitfield).dtype != np.uint8):
            raise ValueError("RegionTransform: edit_bitfield must be uint8")
        self.cascade, self.grid_size, self.bound = _grid_shape(n_bytes, grid_size, cascade, bound)
        self.sel = edit_bitfield
        self.mode, self.mode_id = mode, MODES[mode]
        R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
        t = np.zeros(3) if translation is None else np.asarray(translation, dtype=np.float64).reshape(3)
        s = float(scale)
        if not (0.5 <= s <= 2.0):
            raise ValueError(f"RegionTransform: scale must lie in [0.5, 2] (got {scale})")
        if not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
            raise ValueError("RegionTransform: rotation must be a proper rotation (orthonormal, determinant +1)")
        if not np.isfinite(t).all():
            raise ValueError("RegionTransform: translation must be finite")
        if pivot is None:
            pivot = self.selection_centroid()
        p = np.asarray(pivot, dtype=np.float64).reshape(3)
        if not np.isfinite(p).all():
            raise ValueError("RegionTransform: pivot must be finite")
        self.rotation, self.translation, self.scale, self.pivot = R, t, s, p
        F = np.concatenate([s * R, (p + t - s * R @ p)[:, None]], 1)                # x_new = sR x + (pivot + t - sR pivot)
        G = np.concatenate([R.T / s, (-(R.T / s) @ F[:, 3])[:, None]], 1)
        self.M = np.ascontiguousarray(F, dtype=np.float32)
        self.Minv = np.ascontiguousarray(G, dtype=np.float32)
        self.Rt = np.ascontiguousarray(R.T, dtype=np.float32)
        self.inv_scale = float(np.float32(1.0 / s))
        self.margin = rounding_margin(self.M, self.Minv, self.bound)
        if mode != "delete" and not self.margin < 0.5 / self.grid_size:
            raise ValueError("RegionTransform: the translation is so large that fp32 no longer resolves a quarter of a cell")

    def sel_numpy(self):
        return self.sel.detach().cpu().numpy() if torch.is_tensor(self.sel) else np.asarray(self.sel)

    def selection_centroid(self):
        """the mean of the centres of the selected cells of their own cascade (float64 [3]); zeros for an empty selection"""
        C, H = self.cascade, self.grid_size
        cells = np.flatnonzero(unpack_bits(self.sel_numpy()) & own_cell_mask(C, H))
        if cells.size == 0:
            return np.zeros(3)
        cas, m = cells // H ** 3, (cells % H ** 3).astype(np.uint32)
        coord = np.stack([_compact_bits(m), _compact_bits(m >> np.uint32(1)), _compact_bits(m >> np.uint32(2))], -1).astype(np.float64)
        return ((((coord + 0.5) / H) * 2 - 1) * np.ldexp(1.0, cas)[:, None]).mean(0)

    def sel_on(self, device):
        """the selection as a contiguous uint8 tensor on `device` (cached)"""
        cache = getattr(self, "_sel_dev", None)
        if cache is None or cache.device != torch.device(device):
            src = self.sel if torch.is_tensor(self.sel) else torch.from_numpy(np.ascontiguousarray(self.sel))
            cache = self._sel_dev = src.to(device).contiguous()
        return cache


# ------------------------------------------------------------------------------------------------------------ kernel wrappers
def region_warp(rt, xyzs, dirs, inplace=False, out=None):
    """lae_region_warp on sample rows xyzs, dirs fp32 [M, 3] on the device -> (xyzs_out, dirs_out, sigma_scale [M]); inplace=True
    writes the rows back into xyzs / dirs.  out: (xyzs_out, dirs_out, sigma_scale) buffers of the caller's, or with inplace=True
    the sigma_scale buffer alone; without it this wrapper allocates them with torch (the kernel entry itself reads nothing back
    and allocates nothing, so the call can be captured -- with `out` it touches no allocator at all)."""
    for name, t in (("xyzs", xyzs), ("dirs", dirs)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError(f"region_warp: {name} must be a contiguous fp32 [M, 3] tensor")
    if dirs.shape[0] != xyzs.shape[0]:
        raise ValueError("region_warp: xyzs and dirs must have one row count")
    if out is not None and inplace:
        xo, do, scale = xyzs, dirs, out
    elif out is not None:
        xo, do, scale = out
    else:
        xo, do = (xyzs, dirs) if inplace else (torch.empty_like(xyzs), torch.empty_like(dirs))
        scale = torch.empty(xyzs.shape[0], dtype=torch.float32, device=xyzs.device)
    if xo.shape != xyzs.shape or do.shape != dirs.shape or scale.shape != xyzs.shape[:1] or \
            any(t.dtype != torch.float32 or not t.is_contiguous() for t in (xo, do, scale)):
        raise ValueError("region_warp: out must hold contiguous fp32 [M, 3], [M, 3] and [M] tensors")
    _backend.warp(xyzs, dirs, rt.sel_on(xyzs.device), rt.Minv, rt.Rt, rt.inv_scale, rt.mode_id, rt.bound, rt.cascade, rt.grid_size,
                  xo, do, scale)
    return xo, do, scale


def region_occupancy(rt, occ, out=None):
    """lae_region_occupancy: the bitfield the marcher walks for `rt` over the scene's occupancy `occ` (uint8, density_bitfield's
    layout, on the device) -> uint8 of the same size (`out` when given; every byte is written; not occ itself)"""
    if not torch.is_tensor(occ) or occ.dtype != torch.uint8 or not occ.is_contiguous() or \
            occ.numel() != rt.cascade * rt.grid_size ** 3 // 8:
        raise ValueError(f"region_occupancy: occ must be a contiguous uint8 tensor of {rt.cascade * rt.grid_size ** 3 // 8} values")
    if out is None:
        out = torch.empty_like(occ)
    if out.dtype != torch.uint8 or out.numel() != occ.numel() or not out.is_contiguous() or out.data_ptr() == occ.data_ptr():
        raise ValueError("region_occupancy: out must be another contiguous uint8 tensor of occ's size")
    _backend.occupancy(occ, rt.sel_on(occ.device), None if rt.mode == "delete" else rt.M, rt.margin, rt.mode_id, rt.bound, rt.cascade,
                       rt.grid_size, out)
    return out


# ------------------------------------------------------------------------------------------------------------ numpy restatements
def region_warp_numpy(rt, xyzs, dirs, dtype=np.float64):
    """lae_region_warp in `dtype` (np.float32: the kernel's statements in its order, hence its bits) -> dict: xyzs, dirs [M, 3],
    sigma_scale [M] in `dtype`, branch uint8 [M] (MOVED, VACATED, KEPT)"""
    dt = np.dtype(dtype).type
    C, H, bound = rt.cascade, rt.grid_size, dt(rt.bound)
    x = np.asarray(xyzs).astype(dt).reshape(-1, 3)
    d = np.asarray(dirs).astype(dt).reshape(-1, 3)
    sel = unpack_bits(rt.sel_numpy())
    Minv, Rt = rt.Minv.astype(dt), rt.Rt.astype(dt)
    p = np.stack([_affine(Minv[k], x[:, 0], x[:, 1], x[:, 2]) for k in range(3)], -1)
    with np.errstate(all="ignore"):
        inside = (np.abs(p) <= bound).all(-1)
        q = np.stack([(Rt[k, 0] * d[:, 0] + Rt[k, 1] * d[:, 1]) + Rt[k, 2] * d[:, 2] for k in range(3)], -1)
    moved = (rt.mode != "delete") & inside & sel[cell_index_numpy(np.where(inside[:, None], p, dt(0)), C, H, dt)[0]]
    vacated = ~moved & (rt.mode != "copy") & sel[cell_index_numpy(x, C, H, dt)[0]]
    branch = np.where(moved, MOVED, np.where(vacated, VACATED, KEPT)).astype(np.uint8)
    scale = np.where(moved, dt(np.float32(rt.inv_scale)), np.where(vacated, dt(0), dt(1))).astype(dt)
    return {"xyzs": np.where(moved[:, None], p, x), "dirs": np.where(moved[:, None], q, d), "sigma_scale": scale, "branch": branch}


def region_occupancy_numpy(rt, occ, dtype=np.float64):
    """lae_region_occupancy in `dtype` (np.float32: the kernel's bits) -> uint8 bitfield of occ's size"""
    dt = np.dtype(dtype).type
    C, H = rt.cascade, rt.grid_size
    H3 = H ** 3
    occ_b, sel_b = unpack_bits(occ), unpack_bits(rt.sel_numpy())
    assert occ_b.size == C * H3 and sel_b.size == C * H3, "occ and the selection must hold cascade * grid_size^3 bits"
    out = occ_b.copy()
    if rt.mode != "copy":
        out &= ~(sel_b & own_cell_mask(C, H))
    if rt.mode != "delete":
        src = np.flatnonzero(occ_b & sel_b & own_cell_mask(C, H, layer=True))
        cas, m = src // H3, (src % H3).astype(np.uint32)
        n = [_compact_bits(m), _compact_bits(m >> np.uint32(1)), _compact_bits(m >> np.uint32(2))]
        mb = np.ldexp(dt(1.0), cas.astype(np.int32)).astype(dt)
        rH = dt(1.0) / dt(H)
        face = [[(((n[a] + k).astype(dt) * rH) * dt(2.0) - dt(1.0)) * mb for k in (0, 1)] for a in range(3)]
        M, margin = rt.M.astype(dt), dt(np.float32(rt.margin))
        lo = hi = None
        for k in range(8):
            v = np.stack([_affine(M[a], face[0][k & 1], face[1][(k >> 1) & 1], face[2][k >> 2]) for a in range(3)], -1)
            lo = v if lo is None else np.minimum(lo, v)
            hi = v if hi is None else np.maximum(hi, v)
        lo, hi = lo - margin, hi + margin
        for t in range(C):
            tb, trb = dt(2.0 ** t), dt(2.0 ** -t)
            with np.errstate(all="ignore"):
                live = ~((lo > tb).any(-1) | (hi < -tb).any(-1))
            if not live.any():
                continue
            i0 = [_cell_coord(lo[live, a], trb, H, dt) for a in range(3)]
            i1 = [_cell_coord(hi[live, a], trb, H, dt) for a in range(3)]
            ext = [int((i1[a] - i0[a]).max()) + 1 for a in range(3)]
            for dz in range(ext[2]):
                z = i0[2] + dz
                for dy in range(ext[1]):
                    y = i0[1] + dy
                    for dx in range(ext[0]):
                        x = i0[0] + dx
                        ok = (x <= i1[0]) & (y <= i1[1]) & (z <= i1[2])
                        out[t * H3 + morton_numpy(x[ok], y[ok], z[ok])] = True
    return np.packbits(out, bitorder="little")


# ------------------------------------------------------------------------------------------------------------ rendering
@torch.no_grad()
def render_transformed(renderer, rt, rays_o, rays_d, bg_color=1, perturb=False, dt_gamma=0, max_steps=1024, T_thresh=1e-4,
                       scale_depth=True, dens_grid=None, device_compaction=True, frame_loop=False, want_stats=False, row_budget=0,
                       image_hw=None, tile_hw=(8, 4), max_n_step=8):
    """render_eval(frame_loop=False) of the scene with `rt` applied: the operator loop, with dens_grid = region_occupancy(rt, the
    scene's bitfield), the warp between march_rays and the field, and `sigmas *= sigma_scale` before composite_rays.  Arguments
    and the returned dict are render_eval's; dens_grid replaces renderer.density_bitfield as the SCENE's occupancy; frame_loop is
    accepted and ignored (the device-resident frame loop does not know the transform: a transformed render costs what the
    operator loop costs).  image_hw keeps render_eval's image-tile ray order."""
    if image_hw is not None and rays_o.numel() == 3 * image_hw[0] * image_hw[1] and image_hw[0] % tile_hw[0] == 0 and \
            image_hw[1] % tile_hw[1] == 0 and not (torch.is_tensor(bg_color) and bg_color.numel() > 3):
        idx, inv = renderer._tile_perm(image_hw[0], image_hw[1], tile_hw[0], tile_hw[1], rays_o.device)
        res = render_transformed(renderer, rt, rays_o.reshape(-1, 3)[idx], rays_d.reshape(-1, 3)[idx], bg_color, perturb, dt_gamma,
                                 max_steps, T_thresh, scale_depth, dens_grid, device_compaction, False, want_stats, row_budget,
                                 max_n_step=max_n_step)
        return {k: (v[inv] if torch.is_tensor(v) and v.shape[:1] == inv.shape else v) for k, v in res.items()}
    if (rt.cascade, rt.grid_size) != (renderer.cascade, renderer.grid_size) or float(rt.bound) != float(renderer.bound):
        raise ValueError("render_transformed: the transform was made for another grid (cascade, grid_size, bound)")
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    occ = renderer.density_bitfield if dens_grid is None else dens_grid
    grid = region_occupancy(rt, occ.contiguous())
    N, device = rays_o.shape[0], rays_o.device
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, renderer.aabb_infer, renderer.min_near)
    weights_sum = torch.zeros(N, dtype=torch.float32, device=device)
    depth = torch.zeros(N, dtype=torch.float32, device=device)
    image = torch.zeros(N, 3, dtype=torch.float32, device=device)
    n_alive = N
    rays_alive = torch.arange(n_alive, dtype=torch.int32, device=device)
    rays_t = nears.clone()
    step = 0
    iterations = rows = 0
    budget = max(N, int(row_budget))
    while step < max_steps and n_alive > 0:
        n_step = max(min(budget // n_alive, max_n_step), 1)
        iterations += 1; rows += n_alive * n_step
        xyzs, dirs, deltas = raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, renderer.bound, grid,
                                                    renderer.cascade, renderer.grid_size, nears, fars, 128,
                                                    perturb if step == 0 else False, dt_gamma, max_steps)
        xyzs, dirs, sigma_scale = region_warp(rt, xyzs, dirs, inplace=True)
        sigmas, rgbs = renderer.model(xyzs, dirs)
        sigmas = renderer.density_scale * sigmas
        sigmas = sigmas.float() * sigma_scale.view(sigmas.shape)              # fp32, as composite_rays reads it
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
        out["stats"] = {"iterations": iterations, "rows": rows, "steps": step, "alive_at_end": n_alive}
    return out


@torch.no_grad()
def transform_views(renderer, rt, poses, intrinsics, H, W, bg_color=1.0, **render_kw):
    """the transformed scene from every pose [n, 4, 4] (cam2world, on the device) -> (frames uint8 [n, H, W, 3] by lae_eval_view's
    byte rule, depths fp32 [n, H*W] = the raw `sum w t`, opacities fp32 [n, H*W] = weights_sum): what save_mesh_tsdf /
    save_mesh_textured(frames=, depths=, opacities=) and evaluate_consistency(frames=) take.  Rendered as
    render_packed_views renders: perturb=False, scale_depth=False, over white, fp16 autocast, the model in eval mode."""
    from .. import metrics as M
    from ..rays import get_rays
    H, W = int(H), int(W)
    poses = poses.reshape(-1, 4, 4)
    n, dev = poses.shape[0], renderer.density_bitfield.device
    frames = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    depths = torch.empty(n, H * W, dtype=torch.float32, device=dev)
    opacities = torch.empty(n, H * W, dtype=torch.float32, device=dev)
    scratch = torch.empty(M.EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    was_training = renderer.model.training
    renderer.model.eval()
    try:
        for i in range(n):
            ray = get_rays(poses[i:i + 1], intrinsics, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = render_transformed(renderer, rt, ray["rays_o"][0], ray["rays_d"][0], bg_color=bg_color, perturb=False,
                                         scale_depth=False, image_hw=(H, W), **render_kw)
            M.eval_view(res["image"].float().contiguous(), None, rgb_u8=frames[i], scratch=scratch)
            depths[i], opacities[i] = res["depth"].float(), res["weights_sum"].float()
    finally:
        renderer.model.train(was_training)
    return frames, depths, opacities


SEED_REFRESHES = 8            # occupancy refreshes (of 16 steps each) a seeded cell survives without density: 0.95^-8 = 1.51


@torch.no_grad()
def seed_occupancy(renderer, composed, refreshes=SEED_REFRESHES):
    """make the student march where the composed bitfield says the edited scene has density: every cell whose composed bit is set
    and whose density_grid value is below the seed is raised to it, then density_bitfield is repacked with the threshold
    update_extra_state uses, min(mean_density, density_thresh).  The seed is threshold / 0.95^refreshes: packbits sets a bit
    for values ABOVE the threshold, and a refresh decays a sampled cell by 0.95 when the field has no density there yet, so a
    cell raised to the threshold itself would be gone before the first step.  -> the number of cells raised (one host read)"""
    thr = min(float(renderer.mean_density), float(renderer.density_thresh))
    seed = max(thr, 1e-6) / 0.95 ** int(refreshes)
    shifts = torch.arange(8, dtype=torch.uint8, device=composed.device)
    bits = ((composed[:, None] >> shifts) & 1).bool().reshape(-1)
    flat = renderer.density_grid.view(-1)
    raise_ = bits & (flat < seed)
    flat[raise_] = seed
    renderer.density_bitfield = raymarching.packbits(renderer.density_grid, thr, renderer.density_bitfield)
    return int(raise_.sum().item())


def bake_region_transform(renderer, optimizer, data, rt, steps=3000, lr=1e-2, depth_sup=False, trainer_kw=None, depth_weight=1e-3,
                          seed=True, render_kw=None):
    """bake the transform into the NeRF, as distill_nerf bakes a recolouring: every training pose of `data` is rendered transformed
    (render_transformed over black, fp16 autocast, eval mode), a NEW ResidentImages is built from the RGBA frames (straight colour,
    alpha = the rendered opacity; fp16; poses, intrinsics, bound, mode, bg and colour space of `data`), the student's occupancy is
    seeded with the composed bitfield (seed_occupancy; seed=False leaves it out -- the first groups then never march the object's
    new place), and the existing Trainer runs `steps` steps (distill_steps rounds them to whole groups).  depth_sup=True: the new
    data carries depth planes (`sum w t / opacity` where the opacity exceeds 0.5, else 0 = unsupervised) and the Trainer gets
    depth_weight.  -> (data_new, trainer)"""
    from ..data import ResidentImages
    from ..rays import get_rays
    from ..trainer import Trainer
    from .distill import distill_steps
    H, W, n = data.H, data.W, data.n_img
    dev = data.images.device
    images = torch.empty(n, H, W, 4, dtype=torch.float16, device=dev)
    plane = torch.zeros(n, H, W, dtype=torch.float32, device=dev) if depth_sup else None
    was_training = renderer.model.training
    renderer.model.eval()
    try:
        with torch.no_grad():
            for i in range(n):
                ray = get_rays(data.poses[i:i + 1], data.intrinsics, H, W)
                with torch.autocast("cuda", dtype=torch.float16):
                    res = render_transformed(renderer, rt, ray["rays_o"][0], ray["rays_d"][0], bg_color=0, perturb=False, scale_depth=False,
                                             image_hw=(H, W), **(render_kw or {}))
                ws = res["weights_sum"].float().clamp(0, 1)
                img = res["image"].float()
                rgb = torch.where(ws[:, None] > 0, img / ws.clamp(min=1e-6)[:, None], torch.zeros_like(img)).clamp(0, 1)
                images[i] = torch.cat([rgb, ws[:, None]], 1).reshape(H, W, 4).to(torch.float16)
                if depth_sup:
                    plane[i] = torch.where(ws > 0.5, res["depth"].float() / ws.clamp(min=1e-6), torch.zeros_like(ws)).reshape(H, W)
            if seed:
                seed_occupancy(renderer, region_occupancy(rt, renderer.density_bitfield.contiguous()))
    finally:
        renderer.model.train(was_training)
    data_new = ResidentImages(images, data.poses, data.intrinsics, bound=data.bound, min_near=data.min_near, mode=data.mode, bg=data.bg,
                              color_space=data.color_space, seed=data.seed, device=dev)
    kw = dict(trainer_kw or {})
    if depth_sup:
        data_new.set_depths(plane)
        kw.setdefault("depth_weight", depth_weight)
    tr = Trainer(renderer, optimizer, data_new, iters=steps, lr=lr, **kw)
    tr.train(distill_steps(steps))
    return data_new, tr
