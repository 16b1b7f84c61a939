"""shared by tests/test_insert_cpu.py and tests/test_gpu_insert.py: random source / destination grids and placements for the scene
insert (laenerf_amd/editing/scene_insert.py), sample rows that meet every branch, and the small analytic `Blobs` field of
tests/test_gpu_region.py restated (a test file cannot be imported): its density sum and density-weighted colour of several blobs
ARE the `add` mixture of the blobs taken one by one."""
import copy
import functools

import numpy as np
import torch

import region_util as U
from laenerf_amd.editing import region_transform as RT
from laenerf_amd.editing.scene_insert import SceneInsert

F32 = np.float32


def random_insert(rng, sel, src_grid, dst_grid, mode="replace", scale=None, rotation=None, shift=0.3):
    """a placement of the selection's centroid at a random spot of the destination's inner part"""
    s = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0)))) if scale is None else scale
    R = U.random_rotation(rng) if rotation is None else rotation
    bound_d = 2.0 ** (dst_grid[0] - 1)
    return SceneInsert(sel, src_grid, dst_grid, rotation=R, scale=s, position=rng.uniform(-shift, shift, 3) * bound_d, mode=mode)


def with_mode(ins, mode):
    other = copy.copy(ins)
    other.mode, other.mode_id = mode, {"replace": 0, "add": 1}[mode]
    return other


def forward64(ins, p):
    return (ins.scale * (ins.rotation @ (np.asarray(p, np.float64) - ins.pivot).T)).T + ins.position


def inverse64(ins, x):
    return ((ins.rotation.T @ (np.asarray(x, np.float64) - ins.position).T) / ins.scale).T + ins.pivot


def image_points(rng, ins, src_occ, n):
    """destination points whose pre-image lies in selected, occupied source cells of their own cascade: F(p) for p uniform inside
    randomly chosen cells (float64 map, rounded to fp32), those inside the destination's bound -- most of them are inserted rows"""
    C, H = ins.src_cascade, ins.src_grid_size
    cells = np.flatnonzero(RT.unpack_bits(ins.sel_numpy()) & RT.unpack_bits(src_occ) & RT.own_cell_mask(C, H))
    if cells.size == 0:
        return np.zeros((0, 3), F32)
    pick = cells[rng.integers(0, cells.size, n)]
    cas, m = pick // H ** 3, pick % H ** 3
    p = (((U.coords(H)[m] + rng.random((n, 3))) / H) * 2 - 1) * (2.0 ** cas)[:, None]
    x = forward64(ins, p)
    return x[(np.abs(x) <= ins.dst_bound).all(-1)].astype(F32)


def rows(rng, ins, src_occ, n):
    """n sample rows that meet every branch: uniform in the destination's box, images of selected cells, rows of zeros (the
    marcher's padding, with a zero step), rows with dirs zero -> (xyzs, dirs, deltas)"""
    x = np.concatenate([rng.uniform(-ins.dst_bound, ins.dst_bound, (n, 3)).astype(F32), image_points(rng, ins, src_occ, n)])
    x = x[rng.permutation(len(x))][:n]
    d = rng.standard_normal(x.shape).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    deltas = rng.uniform(0.01, 0.02, (len(x), 2)).astype(F32)
    x[3::17] = 0.0
    d[3::17] = 0.0
    deltas[3::17] = 0.0
    d[5::19] = 0.0
    deltas[7::23, 0] = 0.0                                   # a zero step on a row that is not zeros: skipped all the same
    return x, d, deltas


def clear_of_boundaries(ins, x, eps=1e-4):
    """rows whose float64 pre-image sits at least eps from every decision boundary of the route: the source's bound faces, the
    cascade faces and the cell faces of the source grid at the pre-image's own cascade -> bool [n]"""
    p = inverse64(ins, x)
    C, H = ins.src_cascade, ins.src_grid_size
    ok = (np.abs(np.abs(p) - ins.src_bound) >= eps).all(-1)
    for c in range(C):                                        # the faces |p_i| = 2^c are cell faces of every level as well
        side = 2.0 ** c * 2.0 / H
        g = (p + 2.0 ** c) / side
        ok &= (np.abs(g - np.round(g)) * side >= eps).all(-1)
    return ok


# ---------------------------------------------------------------- an analytic scene: smooth blobs (tests/test_gpu_region.py's)
G = 128
CELL = 2.0 / G
WIDTH = 1.5 * CELL                 # the sigmoid's width: a few cells from full density to none
MARGIN = 12 * CELL                 # occupancy and selection reach this far beyond a blob's radius: 8 widths, sigmoid(-8) = 3e-4
SIGMA0 = 60.0
FREQ = 9.0                         # colour frequency in object-local coordinates
A_C, A_R = np.array([-0.45, 0.05, -0.1]), 0.1         # the blob of the source scene
B_C, B_R = np.array([0.6, -0.55, 0.5]), 0.12          # the blob of the destination scene


class Blobs(torch.nn.Module):
    """model(xyzs, dirs) -> (sigmas [M], rgbs [M, 3]).  A blob: centre c, radius r, object-to-world rotation R and scale s; in its
    local frame p = R^T (x - c) / s the density is SIGMA0 sigmoid((r - |p|) / WIDTH) / s (the rule's density of a scaled object) and
    the colour 0.5 + 0.25 sin(FREQ p + phase) + 0.2 R^T d.  Several blobs: the densities add and the colours average by density.
    Every statement is elementwise over the rows -- the rotations are written out, no matmul and no reduction kernel, whose
    blocking follows the row count -- so a row's result does not depend on which other rows share the call: the property the
    bit-for-bit render tests rest on, which a library GEMM does not promise."""

    def __init__(self, blobs, device="cuda:0"):
        super().__init__()
        self.device = device
        self.blobs = [dict(c=[float(v) for v in np.asarray(b["c"], F32)], r=float(b["r"]),
                           Rt=[[float(v) for v in row] for row in np.asarray(b.get("R", np.eye(3)), F32).T], s=float(b.get("s", 1.0)),
                           phase=float(b["phase"])) for b in blobs]

    @staticmethod
    def _rot(Rt, v):
        """R^T v, component by component: (r0 v0 + r1 v1) + r2 v2"""
        return [(Rt[k][0] * v[0] + Rt[k][1] * v[1]) + Rt[k][2] * v[2] for k in range(3)]

    def forward(self, x, d):
        x, d = x.float(), d.float()
        dv = [d[:, k] for k in range(3)]
        sig, col = [], []
        for b in self.blobs:
            p = [c / b["s"] for c in self._rot(b["Rt"], [x[:, k] - b["c"][k] for k in range(3)])]
            dist = torch.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
            sig.append(SIGMA0 * torch.sigmoid((b["r"] - dist) / WIDTH) / b["s"])
            dl = self._rot(b["Rt"], dv)
            col.append(torch.stack([(0.5 + 0.25 * torch.sin(FREQ * p[k] + b["phase"]) + 0.2 * dl[k]).clamp(0, 1) for k in range(3)], -1))
        total = sig[0]
        for s in sig[1:]:
            total = total + s
        den = total.clamp(min=1e-30)
        rgb = (sig[0] / den)[:, None] * col[0]
        for s, c in zip(sig[1:], col[1:]):
            rgb = rgb + (s / den)[:, None] * c
        return total, rgb


@functools.lru_cache(None)
def cell_centres(C):
    return U.centres(C, G)


def ball_bits(c, r, C=1):
    """the analytic occupancy of a blob on a grid of C cascades of G^3 cells: cells whose centre lies within r of c (at cascade
    k > 0: within r plus half the cell's diagonal, so the coarse cells cover the ball) -> bool [C * G^3]"""
    ctr = cell_centres(C)
    out = [((ctr[k] - np.asarray(c)) ** 2).sum(-1) < (r + (0.0 if k == 0 else 0.5 * 3 ** 0.5 * CELL * 2 ** k)) ** 2 for k in range(C)]
    return np.concatenate(out)


def dilate(bits):
    """one cell in each direction (the 3 x 3 x 3 neighbourhood) of a bool [G^3] set in the bitfield's order"""
    co = U.coords(G)
    g = np.zeros((G, G, G), bool)
    g[co[:, 0], co[:, 1], co[:, 2]] = bits
    pad = np.pad(g, 1)
    out = np.zeros_like(g)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out |= pad[a:a + G, b:b + G, c:c + G]
    return out[co[:, 0], co[:, 1], co[:, 2]]


def placed(A, rot_deg, t, s):
    """blob A rotated by rot_deg about z through its centre, scaled by s about it and shifted by t"""
    return dict(A, c=np.asarray(A["c"]) + np.asarray(t), R=U.rot_z(rot_deg), s=s)
