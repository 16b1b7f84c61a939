"""shared by tests/test_region_cpu.py and tests/test_gpu_region.py: random grids, selections and transforms for the region
transform (laenerf_amd/editing/region_transform.py), and dense views of a bitfield"""
import numpy as np

from laenerf_amd.editing import region_transform as RT


def coords(H):
    """cell coordinates of the Morton indices 0 .. H^3 - 1 -> int64 [H^3, 3]"""
    return np.stack(RT.coords_table(H), -1)


def centres(C, H):
    """cell centres [C, H^3, 3] float64 in the bitfield's order"""
    c = ((coords(H) + 0.5) / H) * 2 - 1
    return np.stack([c * 2.0 ** k for k in range(C)])


def pack(bits):
    return np.packbits(np.asarray(bits, bool).reshape(-1), bitorder="little")


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


ROT90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])       # exact in fp32


def random_scene(rng, C, H, fill=0.02):
    """-> (occ, sel) bitfields: a few blobs and a sprinkle of single cells as occupancy; the selection is one blob's cells, thinned
    at random, a subset of the occupancy.  Cells of every cascade take part (the inner half of cascade 1 too: the rule must ignore it)."""
    ctr = centres(C, H)
    bound = 2.0 ** (C - 1)
    occ = rng.random((C, H ** 3)) < fill
    blobs = [(rng.uniform(-0.6, 0.6, 3) * bound, rng.uniform(0.15, 0.35) * bound) for _ in range(3)]
    for c0, r in blobs:
        occ |= ((ctr - c0) ** 2).sum(-1) < r * r
    c0, r = blobs[0]
    sel = occ & (((ctr - c0) ** 2).sum(-1) < (1.2 * r) ** 2) & (rng.random((C, H ** 3)) < 0.8)
    return pack(occ), pack(sel)


def random_transform(rng, sel, H, mode, scale=None, rotation=None, shift=0.4):
    C = sel.size * 8 // H ** 3
    bound = 2.0 ** (C - 1)
    s = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0)))) if scale is None else scale
    R = random_rotation(rng) if rotation is None else rotation
    return RT.RegionTransform(sel, rotation=R, translation=rng.uniform(-shift, shift, 3) * bound, scale=s, mode=mode, grid_size=H)


def cell_at_level(x, level, H, dtype=np.float32):
    """bit index of x's cell at cascade `level` (the marcher's statement) -> int64 [n]"""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    rb = dt(2.0 ** -level)
    n = [RT._cell_coord(x[:, k], rb, H, dt) for k in range(3)]
    return level * H ** 3 + RT.morton_numpy(n[0], n[1], n[2])


def image_points(rng, rt, n):
    """points whose pre-image lies in selected own-cascade cells: F(p) for p uniform inside randomly chosen cells (float64 map,
    rounded to fp32) -- most of them are rows the warp moves"""
    C, H = rt.cascade, rt.grid_size
    cells = np.flatnonzero(RT.unpack_bits(rt.sel_numpy()) & RT.own_cell_mask(C, H))
    if cells.size == 0:
        return np.zeros((0, 3), np.float32)
    pick = cells[rng.integers(0, cells.size, n)]
    cas, m = pick // H ** 3, pick % H ** 3
    p = (((coords(H)[m] + rng.random((n, 3))) / H) * 2 - 1) * (2.0 ** cas)[:, None]
    s, R = rt.scale, rt.rotation
    x = (s * (R @ (p - rt.pivot).T)).T + rt.pivot + rt.translation
    return x[(np.abs(x) <= rt.bound).all(-1)].astype(np.float32)
