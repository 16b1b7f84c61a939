"""Textured mesh export: a per-triangle texture atlas baked on the device (csrc/atlas.hip, where the layout and the rules are
written down in full).

    atlas_layout(T, cell=8, texture_size=None)   the closed-form layout: cells, cells per row, the image side S
    atlas_uv(layout)                             per-corner file UVs [T, 3, 2] float64
    atlas_owner_numpy(layout)                    the triangle of every texel, cell-major (-1: unused)
    atlas_texels(verts, tris, normals, cell)     per texel: position, face normal, view direction, owner (lae_atlas_texels)
    atlas_fuse_views(packed, poses, ...)         the views' colours fused into the texels (lae_atlas_fuse_views)
    atlas_pack(rgb, owner, layout)               cell-major colours -> the image uint8 [S, S, 3] (lae_atlas_pack)
    atlas_texels_numpy / atlas_fuse_views_numpy / atlas_pack_numpy     the three kernels restated in a chosen dtype
    sample_texture_numpy(texture, uv)            a bilinear lookup with texel centres at half-integers
    write_obj / read_obj                         name.obj + name.mtl + name.png

The layout.  Triangles are packed two to a square cell of n x n texels (n = cell >= 4): cells = ceil(T / 2), cpr = ceil(sqrt(cells))
cells per row, S = cpr * n; triangle t lives in cell t // 2, half t & 1; cell c has its origin at texel ((c % cpr) * n, (c // cpr) * n).
In texel-centre coordinates of the cell, with m = n - 3, half 0 has the UV corners (0, 0), (m, 0), (0, m) and owns the texels with
i + j <= n - 1; half 1 is its point mirror, corners (n-1, n-1), (n-1-m, n-1), (n-1, n-1-m), and owns i + j >= n.  A bilinear lookup
at a point with x + y <= m has weight only on texels with i + j <= m + 1 = n - 2, so the halves never read each other's texels.
Every owned texel, gutter included, is baked at the point the affine extension of the half's UV -> triangle map gives: a colour
affine in position is reproduced by a bilinear lookup anywhere in the UV triangle, with no dilation pass.  The file UV of the
absolute texel-centre coordinates (X, Y) is u = (X + 0.5) / S, v = 1 - (Y + 0.5) / S; image row 0 is the top."""
import collections
import math
import os

import numpy as np
import torch

from . import _lib

MAX_SIDE = 16384                    # the largest texture side lae_atlas_* accept
MIN_CELL = 4
DEFAULT_MIN_COS = 0.25              # extract_mesh_textured's default (DESIGN.md section 4h records what was measured)

Layout = collections.namedtuple("Layout", "T cell cells cpr S n_texels")


def atlas_layout(T, cell=8, texture_size=None):
    """the layout of T triangles.  texture_size: the largest cell whose S = cpr * cell fits into it is chosen (cell is ignored).
    S > 16384 or cell < 4: ValueError naming the largest cell that fits.  T == 0: one empty cell (nothing is baked)."""
    T = int(T)
    if T < 0:
        raise ValueError("atlas_layout: T must not be negative")
    cells = (T + 1) // 2
    r = math.isqrt(cells)
    cpr = max(1, r if r * r == cells else r + 1)                             # ceil(sqrt(cells))
    limit = MAX_SIDE if texture_size is None else min(int(texture_size), MAX_SIDE)
    fits = limit // cpr
    if texture_size is not None:
        cell = fits
    cell = int(cell)
    if cell < MIN_CELL or cpr * cell > limit:
        raise ValueError(f"atlas_layout: {T} triangles need {cpr} cells per row; the largest cell that fits a texture of side {limit} "
                         f"is {fits} (asked for {cell}, the least is {MIN_CELL})")
    return Layout(T, cell, cells, cpr, cpr * cell, cells * cell * cell)


def _corners(layout):
    """cell-relative UV corners [2, 3, 2] of the two halves"""
    n, m = layout.cell, layout.cell - 3
    h0 = np.array([[0, 0], [m, 0], [0, m]], np.float64)
    return np.stack([h0, (n - 1) - h0])


def atlas_corner_texels(layout):
    """absolute texel-centre coordinates (X, Y) of every triangle's three UV corners, [T, 3, 2] float64"""
    t = np.arange(layout.T)
    c = t // 2
    origin = np.stack([(c % layout.cpr) * layout.cell, (c // layout.cpr) * layout.cell], -1).astype(np.float64)
    return origin[:, None, :] + _corners(layout)[t & 1]


def atlas_uv(layout):
    """file UVs [T, 3, 2] float64: u = (X + 0.5) / S, v = 1 - (Y + 0.5) / S"""
    xy = atlas_corner_texels(layout)
    return np.stack([(xy[..., 0] + 0.5) / layout.S, 1.0 - (xy[..., 1] + 0.5) / layout.S], -1)


def _texel_ij(layout):
    """per cell-major texel id: (cell, i, j)"""
    n = layout.cell
    ids = np.arange(layout.n_texels)
    c, r = ids // (n * n), ids % (n * n)
    return c, r % n, r // n


def atlas_owner_numpy(layout):
    """int32 [cells * cell^2], cell-major (id = c * cell^2 + j * cell + i): the triangle that owns the texel, -1 for the unused
    half of an odd T's last cell"""
    c, i, j = _texel_ij(layout)
    t = 2 * c + (i + j >= layout.cell)
    return np.where(t < layout.T, t, -1).astype(np.int32)


def atlas_image_index(layout):
    """per cell-major texel id: its (Y, X) in the S x S image"""
    c, i, j = _texel_ij(layout)
    return (c // layout.cpr) * layout.cell + j, (c % layout.cpr) * layout.cell + i


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements

def _len3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def atlas_texels_numpy(verts, tris, normals=None, cell=8, dtype=np.float32):
    """numpy restatement of lae_atlas_texels in `dtype` (np.float32 with fp32 inputs: the kernel's statements in their order, so
    the kernel's bits).  -> dict pos, nrm, dirs [n_texels, 3] in `dtype`, owner int32 [n_texels], layout"""
    f = np.dtype(dtype).type
    v = np.asarray(verts).reshape(-1, 3).astype(f)
    tr = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    lay = atlas_layout(len(tr), cell)
    n, N = lay.cell, lay.n_texels
    owner = atlas_owner_numpy(lay)
    _, i, j = _texel_ij(lay)
    live = owner >= 0
    t = np.where(live, owner, 0)
    half = (t & 1).astype(bool)
    idx = tr[t] if len(tr) else np.zeros((N, 3), np.int64)
    valid = live & ((idx >= 0) & (idx < len(v))).all(1)
    idx = np.where(valid[:, None], idx, 0)
    fm = f(n - 3)
    with np.errstate(all="ignore"):
        b1 = (np.where(half, n - 1 - i, i).astype(f) / fm)[:, None]
        b2 = (np.where(half, n - 1 - j, j).astype(f) / fm)[:, None]
        v0 = v[idx[:, 0]]
        e1, e2 = v[idx[:, 1]] - v0, v[idx[:, 2]] - v0
        pos = (v0 + b1 * e1) + b2 * e2
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        ln = _len3(c[:, 0], c[:, 1], c[:, 2])
        ok = valid & (ln > 0) & (ln <= f(3.0e38))
        nrm = np.where(ok[:, None], c / np.where(ok, ln, f(1))[:, None], f(0)).astype(f)
        if normals is not None:
            g = np.asarray(normals).reshape(-1, 3).astype(f)
            g0 = g[idx[:, 0]]
            gi = (g0 + b1 * (g[idx[:, 1]] - g0)) + b2 * (g[idx[:, 2]] - g0)
        else:
            gi = np.zeros((N, 3), f)
        gl = _len3(gi[:, 0], gi[:, 1], gi[:, 2])
        gok = valid & (gl > 0) & (gl <= f(3.0e38))
        dirs = np.where(gok[:, None], -(gi / np.where(gok, gl, f(1))[:, None]), np.where(ok[:, None], -nrm, np.array([0, 0, 1], f)[None, :]))
    pos = np.where(valid[:, None] & np.isfinite(pos), pos, f(0)).astype(f)
    dirs = np.where(live[:, None], dirs, f(0)).astype(f)
    return {"pos": pos, "nrm": nrm, "dirs": dirs, "owner": owner, "layout": lay}


def atlas_fuse_views_numpy(packed, poses, intrinsics, H, W, frames, pos, nrm, owner, trunc, min_cos, dtype=np.float64):
    """numpy restatement of lae_atlas_fuse_views with every quantity in `dtype` (np.float32 writes the kernel's statements in
    their order: with fp32 inputs the kernel's bits; trunc and min_cos go through fp32, the values the kernel receives).  -> dict:
      rgb      [N, 3] in `dtype`; counts uint16 [N]; n_grey int
      counted  bool [N, V]: the pairs that were summed
      margin   float64 [N, V]: the distance of the nearest decision the pair took from its threshold, each in its own units, as
               tsdf_numpy gives it: |q.z|; outside the frame the distance to come inside (pixels); inside the distance of u and
               of v from the nearest pixel border (pixels), ||s| - trunc| (world units; inf where the surface is inf or NaN) and,
               where |s| <= trunc holds, |cos - min_cos|.  Unowned texels: inf"""
    dt = np.dtype(dtype).type
    H, W = int(H), int(W)
    pk = np.asarray(packed).reshape(-1, H, W).astype(dt)
    V = pk.shape[0]
    P = np.asarray(poses).reshape(V, 4, 4).astype(dt)
    fr = np.asarray(frames, dtype=np.uint8).reshape(V, H, W, 3)
    fx, fy, cx, cy = (dt(v) for v in intrinsics)
    tr, mc = dt(np.float32(trunc)), dt(np.float32(min_cos))
    w, nr = np.asarray(pos).reshape(-1, 3).astype(dt), np.asarray(nrm).reshape(-1, 3).astype(dt)
    live = np.asarray(owner).reshape(-1) >= 0
    N = len(w)
    t_all = np.abs(pk)
    counted = np.zeros((N, V), bool)
    margin = np.full((N, V), np.inf)
    cnt = np.zeros(N, np.uint32)
    sums = np.zeros((N, 3), np.uint32)
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
            t_tex = _len3(d[:, 0], d[:, 1], d[:, 2])
            s = ts - t_tex
            near = seen & (np.abs(s) <= tr)
            cosv = (-((nr[:, 0] * d[:, 0] + nr[:, 1] * d[:, 1]) + nr[:, 2] * d[:, 2])) / t_tex
            take = live & near & (cosv > mc)
            counted[:, v] = take
            cnt += take
            sums += np.where(take[:, None], fr[v, py, px].astype(np.uint32), np.uint32(0))
            u64, v64, z64 = pu.astype(np.float64), pv.astype(np.float64), np.abs(q[2].astype(np.float64))
            viol = np.maximum(np.maximum(-u64, u64 - W), np.maximum(-v64, v64 - H))
            to_border = np.minimum(np.abs(u64 - np.round(u64)), np.abs(v64 - np.round(v64)))
            gap = np.abs(np.abs(s.astype(np.float64)) - float(tr))
            gap = np.where(np.isfinite(ts), gap, np.inf)
            cgap = np.where(near, np.abs(cosv.astype(np.float64) - float(mc)), np.inf)
            mg = np.where(inside, np.minimum(np.minimum(z64, to_border), np.minimum(gap, cgap)), np.minimum(z64, np.abs(viol)))
            mg = np.where(front, mg, z64)
            margin[:, v] = np.where(np.isnan(mg) | ~live, np.inf, mg)
        has = cnt > 0
        rgb = np.where(has[:, None], sums.astype(dt) / np.where(has, cnt, 1).astype(dt)[:, None] / dt(255.0), dt(0.5))
        rgb = np.where(live[:, None], rgb, dt(0.0)).astype(dt)
    return {"rgb": rgb, "counts": cnt.astype(np.uint16), "n_grey": int((live & ~has).sum()), "counted": counted, "margin": margin}


def atlas_pack_numpy(rgb, owner, layout):
    """numpy restatement of lae_atlas_pack: cell-major colours [n_texels, 3] -> the image uint8 [S, S, 3]; unowned texels are 0"""
    from .mesh import color_bytes_numpy
    img = np.zeros((layout.S, layout.S, 3), np.uint8)
    Y, X = atlas_image_index(layout)
    own = np.asarray(owner).reshape(-1) >= 0
    img[Y, X] = np.where(own[:, None], color_bytes_numpy(np.asarray(rgb).reshape(-1, 3)), np.uint8(0))
    return img


def atlas_image_numpy(values, layout, fill=0.0):
    """cell-major per-texel values [n_texels, C] -> the image [S, S, C] in their dtype (no byte quantisation)"""
    values = np.asarray(values)
    img = np.full((layout.S, layout.S) + values.shape[1:], fill, values.dtype)
    Y, X = atlas_image_index(layout)
    img[Y, X] = values
    return img


def bilinear_taps(x, y, S):
    """the four taps of a bilinear lookup at texel-centre coordinates (x, y) (texel (X, Y)'s centre is at (X, Y)), indices clamped
    to the image -> (X [.., 4], Y [.., 4], weight [.., 4]) in float64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    X = np.stack([x0, x0 + 1, x0, x0 + 1], -1)
    Y = np.stack([y0, y0, y0 + 1, y0 + 1], -1)
    wgt = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1)
    return np.clip(X, 0, S - 1).astype(np.int64), np.clip(Y, 0, S - 1).astype(np.int64), wgt


def sample_texture_numpy(texture, uv):
    """a bilinear lookup in texture [S, S, C] (row 0 on top; uint8 is scaled to [0, 1]) at file UVs [..., 2], texel centres at
    half-integers: x = u S - 0.5, y = (1 - v) S - 0.5 -> [..., C] float64"""
    tex = np.asarray(texture)
    tex = tex.astype(np.float64) / 255.0 if tex.dtype == np.uint8 else tex.astype(np.float64)
    S = tex.shape[0]
    uv = np.asarray(uv, np.float64)
    X, Y, wgt = bilinear_taps(uv[..., 0] * S - 0.5, (1.0 - uv[..., 1]) * S - 0.5, S)
    return (tex[Y, X] * wgt[..., None]).sum(-2)


# ---------------------------------------------------------------------------------------------------------------------------
# device entry points

def _f32(t, shape_tail, who, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != shape_tail or \
            not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous fp32 tensor [n, {', '.join(str(s) for s in shape_tail)}]")


def atlas_texels(verts, tris, normals=None, cell=8, texture_size=None):
    """the texels of a mesh's atlas (lae_atlas_texels).  verts fp32 [V, 3] in the box, tris int32 [T, 3], normals optional fp32
    [V, 3], all on the device.  -> dict pos, nrm, dirs fp32 [n_texels, 3], owner int32 [n_texels] (cell-major), layout.  Triangle
    indices are range-checked first (one host read; ValueError as in pack_ply)."""
    _f32(verts, (3,), "atlas_texels", "verts")
    if normals is not None:
        _f32(normals, (3,), "atlas_texels", "normals")
        if normals.shape[0] != verts.shape[0]:
            raise ValueError("atlas_texels: one normal per vertex")
    if not torch.is_tensor(tris) or tris.dtype != torch.int32 or tris.dim() != 2 or tris.shape[1] != 3 or not tris.is_contiguous():
        raise ValueError("atlas_texels: tris must be a contiguous int32 tensor [T, 3]")
    V, T = verts.shape[0], tris.shape[0]
    if T == 0 or V == 0:
        raise ValueError("atlas_texels: an empty mesh has no texels")
    lay = atlas_layout(T, cell, texture_size)
    _lib.need_cuda(verts, tris, normals)
    if bool(((tris < 0) | (tris >= V)).any()):
        raise ValueError("atlas_texels: a triangle index is out of range")
    dev = verts.device
    out = {k: torch.empty(lay.n_texels, 3, dtype=torch.float32, device=dev) for k in ("pos", "nrm", "dirs")}
    out["owner"] = torch.empty(lay.n_texels, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().lae_atlas_texels(verts.data_ptr(), V, tris.data_ptr(), T, _lib.ptr(normals), lay.cell, out["pos"].data_ptr(),
                                           out["nrm"].data_ptr(), out["dirs"].data_ptr(), out["owner"].data_ptr(), _lib.stream()),
               "atlas_texels")
    out["layout"] = lay
    return out


def atlas_fuse_views(packed, poses, intrinsics, H, W, frames, pos, nrm, owner, trunc, min_cos=DEFAULT_MIN_COS, counts=False):
    """the colours of V views fused into texels (lae_atlas_fuse_views).  packed fp32 [V, H, W] (tsdf.render_packed_views), poses
    fp32 [V, 4, 4] cam2world, intrinsics (fx, fy, cx, cy), frames [V, H, W, 3] uint8 or fp32 (converted to bytes by lae_eval_view's
    rule first), pos / nrm / owner as atlas_texels returns them, trunc > 0 in world units, 0 <= min_cos < 1.  A view counts for a
    texel where its surface lies within trunc of the texel along the pixel's ray and the texel's face normal meets the ray at a
    cosine above min_cos.  -> dict rgb fp32 [n_texels, 3] (0.5 where no view counts), counts uint16 [n_texels] or None, n_grey
    int32 [1] on the device (the owned texels no view counted for)."""
    from .tsdf import _frame_bytes
    H, W = int(H), int(W)
    if len(intrinsics) != 4:
        raise ValueError("atlas_fuse_views: intrinsics = (fx, fy, cx, cy)")
    if not torch.is_tensor(packed) or packed.dtype != torch.float32 or not packed.is_contiguous() or H < 1 or W < 1 or \
            packed.numel() == 0 or packed.numel() % (H * W):
        raise ValueError("atlas_fuse_views: packed must be a contiguous fp32 tensor of V x H x W values")
    V = packed.numel() // (H * W)
    if V > 65535:
        raise ValueError("atlas_fuse_views: at most 65535 views")
    if not torch.is_tensor(poses) or poses.dtype != torch.float32 or poses.numel() != 16 * V or not poses.is_contiguous():
        raise ValueError(f"atlas_fuse_views: poses must be a contiguous fp32 tensor of {V} x 4 x 4 values")
    _f32(pos, (3,), "atlas_fuse_views", "pos")
    _f32(nrm, (3,), "atlas_fuse_views", "nrm")
    N = pos.shape[0]
    if N == 0 or nrm.shape[0] != N or not torch.is_tensor(owner) or owner.dtype != torch.int32 or tuple(owner.shape) != (N,) or \
            not owner.is_contiguous():
        raise ValueError("atlas_fuse_views: pos, nrm [n, 3] and owner int32 [n] describe the same n >= 1 texels")
    if not float(trunc) > 0.0 or not np.isfinite(float(trunc)):
        raise ValueError("atlas_fuse_views: trunc must be positive and finite")
    if not 0.0 <= float(min_cos) < 1.0:
        raise ValueError("atlas_fuse_views: min_cos must lie in [0, 1)")
    dev = packed.device
    fb = _frame_bytes(frames, V, H, W, dev, "atlas_fuse_views")
    _lib.need_cuda(packed, poses, pos, nrm, owner, fb)
    rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
    cnt = torch.empty(N, dtype=torch.uint16, device=dev) if counts else None
    n_grey = torch.empty(1, dtype=torch.int32, device=dev)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    _lib.check(_lib.load().lae_atlas_fuse_views(packed.data_ptr(), poses.data_ptr(), V, fx, fy, cx, cy, H, W, fb.data_ptr(), pos.data_ptr(),
                                               nrm.data_ptr(), owner.data_ptr(), N, float(trunc), float(min_cos), rgb.data_ptr(),
                                               _lib.ptr(cnt), n_grey.data_ptr(), _lib.stream()), "atlas_fuse_views")
    return {"rgb": rgb, "counts": cnt, "n_grey": n_grey}


def atlas_pack(rgb, owner, layout):
    """cell-major fp32 colours [n_texels, 3] -> the image uint8 [S, S, 3] on the device (lae_atlas_pack; lae_eval_view's byte rule,
    unowned texels 0)"""
    _f32(rgb, (3,), "atlas_pack", "rgb")
    if rgb.shape[0] != layout.n_texels or not torch.is_tensor(owner) or owner.dtype != torch.int32 or \
            tuple(owner.shape) != (layout.n_texels,) or not owner.is_contiguous() or layout.T < 1:
        raise ValueError(f"atlas_pack: rgb [n, 3] and owner int32 [n] must hold the layout's {layout.n_texels} texels")
    _lib.need_cuda(rgb, owner)
    img = torch.empty(layout.S, layout.S, 3, dtype=torch.uint8, device=rgb.device)
    _lib.check(_lib.load().lae_atlas_pack(rgb.data_ptr(), owner.data_ptr(), layout.T, layout.cell, img.data_ptr(), _lib.stream()), "atlas_pack")
    return img


# ---------------------------------------------------------------------------------------------------------------------------
# files

def _rows(fmt, arr):
    """one line per row of arr, formatted in one pass"""
    arr = np.asarray(arr)
    return (fmt * len(arr)) % tuple(arr.reshape(-1).tolist()) if len(arr) else ""


def obj_text(vertices, triangles, uv, mtl_name, normals=None):
    """the text of an OBJ with per-corner texture coordinates: `mtllib`, `v`, optional `vn`, three `vt` per triangle and
    `f a/ta[/na] b/tb[/nb] c/tc[/nc]` (1-based; corner k of triangle t uses vt 3 t + k + 1, vertex a its own vn)"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    if len(uv) != 3 * len(t):
        raise ValueError("write_obj: uv must hold three corners per triangle")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_obj: a triangle index is out of range")
    parts = [f"mtllib {mtl_name}\nusemtl atlas\n", _rows("v %.9g %.9g %.9g\n", v)]
    a = t + 1
    ta = (3 * np.arange(len(t))[:, None] + np.arange(3)[None, :]) + 1
    if normals is not None:
        nr = np.asarray(normals, np.float64).reshape(-1, 3)
        if len(nr) != len(v):
            raise ValueError("write_obj: one normal per vertex")
        parts.append(_rows("vn %.9g %.9g %.9g\n", nr))
        faces = np.stack([a, ta, a], -1).reshape(len(t), 9)
        ffmt = "f %d/%d/%d %d/%d/%d %d/%d/%d\n"
    else:
        faces = np.stack([a, ta], -1).reshape(len(t), 6)
        ffmt = "f %d/%d %d/%d %d/%d\n"
    parts.append(_rows("vt %.12g %.12g\n", uv))
    parts.append(_rows(ffmt, faces))
    return "".join(parts)


def _atomic_write(path, data):
    tmp = f"{path}.{os.getpid()}.tmp"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)


def png_bytes(texture):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(texture, dtype=np.uint8), "RGB").save(buf, format="PNG")
    return buf.getvalue()


def write_obj(path, vertices, triangles, uv, texture, normals=None):
    """name.obj (obj_text), name.mtl (`newmtl atlas`, `map_Kd name.png`) and name.png (texture uint8 [S, S, 3], row 0 on top) next to
    each other; each file is written under a temporary name and renamed.  uv [T, 3, 2] as atlas_uv gives them."""
    path = os.fspath(path)
    stem = path[:-4] if path.lower().endswith(".obj") else path
    d = os.path.dirname(os.path.abspath(stem))
    os.makedirs(d, exist_ok=True)
    name = os.path.basename(stem)
    text = obj_text(vertices, triangles, uv, name + ".mtl", normals)
    mtl = f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n"
    _atomic_write(stem + ".png", png_bytes(texture))
    _atomic_write(stem + ".mtl", mtl.encode("ascii"))
    _atomic_write(stem + ".obj", text.encode("ascii"))
    return stem + ".obj"


def read_obj(path):
    """an OBJ as write_obj writes it -> dict vertices [V, 3] float64, normals [V, 3] float64 or None, triangles [T, 3] int32,
    uv [T, 3, 2] float64 (per corner), mtllib, map_kd (the names the files give) and texture uint8 [S, S, 3] (None if the image
    is missing)"""
    path = os.fspath(path)
    groups = {"v": [], "vn": [], "vt": [], "f": []}
    mtllib = None
    with open(path, "r") as f:
        for ln in f:
            k, _, rest = ln.partition(" ")
            if k in groups:
                groups[k].append(rest)
            elif k == "mtllib":
                mtllib = rest.strip()
    def table(key, cols):
        return np.array(" ".join(groups[key]).split(), np.float64).reshape(-1, cols)
    v, vn, vt = table("v", 3), table("vn", 3), table("vt", 2)
    T = len(groups["f"])
    corners = np.array(" ".join(groups["f"]).replace("/", " ").split(), np.int64).reshape(T, 3, -1) if T else np.zeros((0, 3, 2), np.int64)
    tris = (corners[..., 0] - 1).astype(np.int32)
    uv = vt[corners[..., 1] - 1] if T else np.zeros((0, 3, 2))
    out = {"vertices": v, "normals": vn if len(vn) else None, "triangles": tris, "uv": uv, "mtllib": mtllib, "map_kd": None, "texture": None}
    d = os.path.dirname(os.path.abspath(path))
    if mtllib and os.path.exists(os.path.join(d, mtllib)):
        for ln in open(os.path.join(d, mtllib)):
            if ln.startswith("map_Kd "):
                out["map_kd"] = ln[7:].strip()
        if out["map_kd"] and os.path.exists(os.path.join(d, out["map_kd"])):
            from PIL import Image
            out["texture"] = np.asarray(Image.open(os.path.join(d, out["map_kd"])).convert("RGB"))
    return out
