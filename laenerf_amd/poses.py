"""Training-camera pose refinement: float64 restatements of its three kernels, and SO(3) helpers.

The kernels (include/laenerf.h): `lae_grid_input_grad` (d loss / d x of the samples from the level-major feature gradients, without a
dy_dx buffer), `lae_pose_ray_grad` (per ray: sum g and sum (x - o) x g) and `lae_pose_step` (per-image reduction, a sparse Adam step in
the world-frame tangent space, composition onto an fp64 master, the fp32 matrices the sampler reads).  The identity behind them: moving
a camera (R, T) to (Exp(w) R, T + t) moves every sample x of its rays to T + t + Exp(w)(x - T), so at w = t = 0
d loss / d t = sum g and d loss / d w = sum (x - T) x g.  Not part of the gradient: the view direction (SH -> colour MLP input), nears /
fars, and the occupancy decisions of the march.

`pose_numpy` bundles the three restatements (`pose_numpy.grid_input_grad`, `.ray_grad`, `.step`); none of this touches the GPU.
"""
import ctypes
import ctypes.util
import types

import numpy as np

__all__ = ["exp_so3", "pose_error", "perturb_poses", "grid_level_scales", "grid_forward_numpy", "grid_input_grad_numpy",
           "pose_ray_grad_numpy", "pose_step_numpy", "pose_numpy"]

_PRIMES = (1, 2654435761, 805459861)
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- SO(3)
def exp_so3(w):
    """Rodrigues' formula in float64: w [3] -> Exp(w) [3, 3] = I + A K + B K^2, A = sin t / t, B = (1 - cos t) / t^2, t = |w|; the
    series A = 1 - t^2 / 6, B = 1 / 2 - t^2 / 24 for t^2 < 1e-12 (Exp(0) is the identity exactly)"""
    w = np.asarray(w, dtype=np.float64).reshape(3)
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if t2 < 1e-12:
        A, B = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        t = np.sqrt(t2)
        A, B = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            k2 = K[i, 0] * K[0, j] + K[i, 1] * K[1, j] + K[i, 2] * K[2, j]
            E[i, j] = (1.0 if i == j else 0.0) + (A * K[i, j] + B * k2)
    return E


def pose_error(a, b):
    """a, b [n, 4, 4] (or [n, 3, 4]) camera-to-world matrices -> (angle [n] of Ra Rb^T in radians, distance [n] of the origins)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    rel = np.einsum("nij,nkj->nik", a[:, :3, :3], b[:, :3, :3])
    # the angle from the antisymmetric part and the trace: accurate near zero, where arccos of the trace alone is not
    s = 0.5 * np.sqrt((rel[:, 2, 1] - rel[:, 1, 2]) ** 2 + (rel[:, 0, 2] - rel[:, 2, 0]) ** 2 + (rel[:, 1, 0] - rel[:, 0, 1]) ** 2)
    c = 0.5 * (np.trace(rel, axis1=1, axis2=2) - 1.0)
    return np.arctan2(s, c), np.linalg.norm(a[:, :3, 3] - b[:, :3, 3], axis=1)


def perturb_poses(poses, deg, dist, seed=0):
    """poses [n, 4, 4] -> float32 copies with every camera rotated about its own origin by `deg` degrees about a random axis and moved
    by `dist` in a random direction (the form the refinement undoes: R <- Exp(w) R, T <- T + t)"""
    rng = np.random.default_rng(seed)
    out = np.array(poses, dtype=np.float64, copy=True)
    for i in range(out.shape[0]):
        ax, tr = rng.standard_normal(3), rng.standard_normal(3)
        out[i, :3, :3] = exp_so3(ax / np.linalg.norm(ax) * np.deg2rad(deg)) @ out[i, :3, :3]
        out[i, :3, 3] += tr / np.linalg.norm(tr) * dist
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the grid
def _exp2f(v):
    """the C library's exp2f, which the host side of the HIP library (and the oracle) evaluates the level scales with"""
    name = ctypes.util.find_library("m")
    if name:
        fn = ctypes.CDLL(name).exp2f
        fn.argtypes, fn.restype = [ctypes.c_float], ctypes.c_float
        return np.float32(fn(float(v)))
    return np.exp2(np.float32(v))


def grid_level_scales(L, S, H):
    """float32 [L]: scale_l = fmaf(exp2f(l * S), H, -1) (gridencoder.cu:138); S = log2(per_level_scale) as float32"""
    S = np.float32(S)
    # exp2f's float32 result times a small integer minus one is exact in float64: one rounding, like the fused multiply-add
    return np.array([np.float32(np.float64(_exp2f(np.float32(l) * S)) * np.float64(H) - 1.0) for l in range(L)], dtype=np.float32)


def _level_index(pg, scale, size, gridtype, align_corners):
    """gridencoder.cu:66-84 on integer corners pg [..., 3] (uint64 holding uint32 values) -> entry index inside the level"""
    res = np.uint64(int(np.ceil(scale)) + 1)
    side = res if align_corners else res + np.uint64(1)
    stride, index = np.uint64(1), np.zeros(pg.shape[:-1], np.uint64)
    for d in range(3):
        if stride <= np.uint64(size):
            index = (index + pg[..., d] * stride) & _M32
            stride = (stride * side) & _M32                                  # uint32 arithmetic, as the kernels'
    if gridtype == 0 and stride > np.uint64(size):
        index = np.zeros(pg.shape[:-1], np.uint64)
        for d in range(3):
            index ^= (pg[..., d] * np.uint64(_PRIMES[d])) & _M32
    return index % np.uint64(size)


class _Table:
    """the fp16 table [n, 2] (float16, uint16 bits, or any float array holding fp16 values), gathered rows widened to float64"""

    def __init__(self, table):
        t = np.asarray(table)
        self.t = (t.view(np.float16) if t.dtype == np.uint16 else t).reshape(-1, 2)

    def __getitem__(self, rows):
        return self.t[rows].astype(np.float64)


def _corners(pg, idx):
    return pg + np.array([idx & 1, (idx >> 1) & 1, idx >> 2], dtype=np.uint64)


def grid_forward_numpy(x, table, offsets, S, H, gridtype=0, align_corners=False, in_map=(0.0, 1.0)):
    """the encoder's forward in float64 throughout (positions included), for finite differences: x [M, 3] float64, table fp16 values
    [n, 2] (float16 or uint16 bits) -> features [L, M, 2] float64; a row outside [0, 1]^3 after the map gives zeros"""
    x = np.asarray(x, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    L = offsets.shape[0] - 1
    tab = _Table(table)
    x01 = (x + np.float64(np.float32(in_map[0]))) * np.float64(np.float32(in_map[1]))
    inside = np.all((x01 >= 0) & (x01 <= 1), axis=1)
    out = np.zeros((L, x.shape[0], 2))
    for l, scale in enumerate(grid_level_scales(L, S, H)):
        pos = x01 * np.float64(scale) + (0.0 if align_corners else 0.5)
        fl = np.floor(pos)
        fr = pos - fl
        pg = np.where(inside[:, None], fl, 0).astype(np.uint64)
        size = int(offsets[l + 1] - offsets[l])
        for idx in range(8):
            w = np.ones(x.shape[0])
            for d in range(3):
                w = w * (fr[:, d] if (idx >> d) & 1 else 1.0 - fr[:, d])
            v = tab[offsets[l] + _level_index(_corners(pg, idx), scale, size, gridtype, align_corners).astype(np.int64)]
            out[l] += np.where(inside, w, 0.0)[:, None] * v
    return out


def grid_cells_f32(x, L, S, H, align_corners=False, in_map=(0.0, 1.0)):
    """the forward's float32 cell computation -> (inside [M] bool, pg [L, M, 3] uint64, frac [L, M, 3] float32, scales [L] float32)"""
    x = np.asarray(x, dtype=np.float32)
    x01 = (x + np.float32(in_map[0])) * np.float32(in_map[1])
    inside = np.all((x01 >= 0) & (x01 <= 1), axis=1)
    scales = grid_level_scales(L, S, H)
    pgs, frs = [], []
    for scale in scales:
        # fmaf(x01, scale, 0 or 0.5): the float32 product is exact in float64, so is the sum for every position a table can hold
        pos = (x01.astype(np.float64) * np.float64(scale) + (0.0 if align_corners else 0.5)).astype(np.float32)
        fl = np.floor(pos)
        pgs.append(np.where(inside[:, None], fl, 0).astype(np.uint64))
        frs.append((pos - fl).astype(np.float32))
    return inside, np.stack(pgs), np.stack(frs), scales


def grid_input_grad_numpy(x, table, offsets, grad_feats, S, H, gridtype=0, align_corners=False, in_map=(0.0, 1.0), full=False):
    """float64 restatement of lae_grid_input_grad: the cell and the fractional position from the float32 computation, as the kernel
    takes them, everything after that in float64.  x [M, 3] float32, table fp16 [n, 2], grad_feats fp16 [L, M, 2] -> grad_x [M, 3]
    float64; full=True: also A [M, 3], the sum of the absolute values of the 8 L terms of every output (times |in_scale|), and its
    per-level parts [L, M, 3]"""
    offsets = np.asarray(offsets, dtype=np.int64)
    L = offsets.shape[0] - 1
    g = np.asarray(grad_feats)
    if g.dtype == np.uint16:
        g = g.view(np.float16)
    g = g.reshape(L, -1, 2).astype(np.float64)
    M = g.shape[1]
    tab = _Table(table)
    inside, pgs, frs, scales = grid_cells_f32(x, L, S, H, align_corners, in_map)
    out, absl = np.zeros((M, 3)), np.zeros((L, M, 3))
    for l in range(L):
        size = int(offsets[l + 1] - offsets[l])
        fr = frs[l].astype(np.float64)
        v = [tab[offsets[l] + _level_index(_corners(pgs[l], idx), scales[l], size, gridtype, align_corners).astype(np.int64)] for idx in range(8)]
        for gd in range(3):
            da, db = (1 if gd == 0 else 0), (1 if gd == 2 else 2)
            for pr in range(4):
                wa = fr[:, da] if pr & 1 else 1.0 - fr[:, da]
                wb = fr[:, db] if pr & 2 else 1.0 - fr[:, db]
                il = ((pr & 1) << da) | (((pr >> 1) & 1) << db)
                ir = il | (1 << gd)
                w = np.where(inside, np.float64(scales[l]) * wa * wb, 0.0)
                for ch in range(2):
                    term = w * (v[ir][:, ch] - v[il][:, ch]) * g[l, :, ch]
                    out[:, gd] += term
                    absl[l, :, gd] += np.abs(term)
    k = np.float64(np.float32(in_map[1]))
    if full:
        return out * k, absl.sum(0) * abs(k), absl * abs(k)
    return out * k


# ---------------------------------------------------------------------------------------------------------------- the pose kernels
def pose_ray_grad_numpy(rays, xyzs, grad_x, rays_o, full=False):
    """float64 restatement of lae_pose_ray_grad: rays int32 [N, 3] (ray id, offset, count), xyzs / grad_x [M, 3], rays_o [N, 3] ->
    out [N, 6] = (sum g, sum (x - o) x g) at the ray id's row; a ray with count 0 or offset + count > M gives zeros.
    full=True: also the sums of the absolute values of the terms"""
    rays = np.asarray(rays, dtype=np.int64)
    x, g, o = (np.asarray(a, dtype=np.float64) for a in (xyzs, grad_x, rays_o))
    N, M = rays.shape[0], x.shape[0]
    out, A = np.zeros((N, 6)), np.zeros((N, 6))
    for idx, off, cnt in rays:
        if cnt == 0 or off + cnt > M or not 0 <= idx < N:
            continue
        gg = g[off:off + cnt]
        r = x[off:off + cnt] - o[idx]
        out[idx, :3] = gg.sum(0)
        A[idx, :3] = np.abs(gg).sum(0)
        for c, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
            out[idx, 3 + c] = (r[:, i] * gg[:, j] - r[:, j] * gg[:, i]).sum()
            A[idx, 3 + c] = (np.abs(r[:, i] * gg[:, j]) + np.abs(r[:, j] * gg[:, i])).sum()
    return (out, A) if full else out


def pose_step_numpy(ray_grads, inds, hw, master, m, v, counts, inv_scale=1.0, skip=False, lr=1e-3, betas=(0.9, 0.99), eps=1e-15):
    """float64 restatement of lae_pose_step on copies -> (master [n, 12], m [n, 6], v [n, 6], counts [n] int32, train rows [n, 12]
    float32).  inv_scale: the float of the optimizer's state word 7; lr: the float32 the kernel reads"""
    master, m, v = (np.array(a, dtype=np.float64, copy=True) for a in (master, m, v))
    master = master.reshape(-1, 12)
    counts = np.array(counts, dtype=np.int32, copy=True)
    img = np.asarray(inds, dtype=np.int64) // int(hw)
    rg = np.asarray(ray_grads, dtype=np.float64).reshape(-1, 6)
    b1, b2 = float(betas[0]), float(betas[1])
    for i in range(master.shape[0]):
        sel = img == i
        if not sel.any() or skip:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            g = rg[sel].sum(0) * np.float64(np.float32(inv_scale))
        if not np.all(np.isfinite(g)):
            continue
        counts[i] += 1
        t = float(counts[i])
        m[i] = b1 * m[i] + (1.0 - b1) * g
        v[i] = b2 * v[i] + (1.0 - b2) * (g * g)
        d = -((np.float64(np.float32(lr)) / (1.0 - b1 ** t)) * (m[i] / (np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t) + eps)))
        P = master[i].reshape(3, 4)
        if np.any(d[3:] != 0):
            P[:, :3] = exp_so3(d[3:]) @ P[:, :3]
        for c in range(3):
            if d[c] != 0:                                  # a zero step keeps the operand's bits (-0.0 + 0.0 would not)
                P[c, 3] += d[c]
    return master, m, v, counts, master.astype(np.float32)


pose_numpy = types.SimpleNamespace(grid_input_grad=grid_input_grad_numpy, grid_forward=grid_forward_numpy, ray_grad=pose_ray_grad_numpy,
                                   step=pose_step_numpy, exp_so3=exp_so3)
