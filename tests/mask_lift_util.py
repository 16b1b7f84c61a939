"""The scene of the mask-lift tests, built in float64 and handed over as fp32.

A sphere of radius 0.45 around the origin in a bound-2 box with two cascades of 32^3 cells.  Occupied are the cells of either
cascade whose centre lies in the shell R - side <= |w| <= R (side: the cell side of the cell's own cascade), so that no occupied
cell floats in front of the surface.  The masks mark the cap AXIS . X >= CAP of the sphere's surface.  The views are analytic:
depth = 0.97 t and opacity 0.97 where the pixel's ray hits the sphere at distance t, both 0 elsewhere; 40 x 56 pixels, focal 100,
principal point (30.5, 18.25).

Cameras: view 0 is CLOSE -- 0.62 from the centre (0.17 above the surface), looking along the tangent tilted towards the sphere, so
that some of the shell is behind it, most of it outside its frame and a few cells inside.  The others stand on a ring of radius 3
around AXIS, at most 4 degrees off the plane through the origin normal to AXIS, each with its own azimuth (golden-angle steps),
roll and a small offset of its look-at point: generic rotations (AXIS is not a coordinate axis; axis-aligned views would put whole
planes of cell centres on pixel borders), and rays that meet the sphere nearly parallel to the cap's plane (|AXIS . dir| <= sin(4 +
8.6 + 1 degrees) = 0.24).  The geometric property of tests/test_gpu_mask_lift.py rests on that: a visible cell lies at most
depth_margin sides behind the surface point of its pixel ALONG THE RAY, which moves it by at most 0.24 of that across the cap's
plane, and no occupied cell lies in front of the surface."""
import functools

import numpy as np

G, C, BOUND = 32, 2, 2.0
H, W = 40, 56
INTRINSICS = (100.0, 100.0, 30.5, 18.25)
RADIUS, OPACITY = 0.45, 0.97
AXIS = np.array([0.36, 0.48, 0.8])
CAP = 0.15
EPS = 1e-4                 # the exclusion band of the comparisons with float64, in the units of mask_lift_numpy's margin
EPS_CAP = 0.005            # at most this share of the (occupied cell, view) pairs may lie inside it
VIEWS = (5, 65)            # 65: one more than the kernel's LDS pose chunk


def _frame(fwd, roll):
    """a right-handed camera frame (columns right, down, forward) looking along `fwd`, rolled about it"""
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.13, 0.97, 0.21]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c, s = np.cos(roll), np.sin(roll)
    return np.stack([c * right + s * down, c * down - s * right, fwd], -1)


def poses(V):
    """[V, 4, 4] float64 cam2world"""
    a = AXIS / np.linalg.norm(AXIS)
    e1 = np.cross(a, np.array([1.0, 0.0, 0.0]))
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    P = np.tile(np.eye(4), (V, 1, 1))
    # the close camera: on e1, looking along e2 (tangentially), tilted a little towards the sphere
    P[0, :3, 3] = 0.62 * e1 + 0.05 * a
    P[0, :3, :3] = _frame(e2 - 0.8 * e1, 0.4)
    for v in range(1, V):
        az = 2.399963 * v + 0.3
        el = np.deg2rad(4.0) * np.sin(1.7 * v)
        o = 3.0 * (np.cos(el) * (np.cos(az) * e1 + np.sin(az) * e2) + np.sin(el) * a)
        look = 0.04 * np.array([np.sin(2.1 * v), np.cos(1.3 * v), np.sin(0.7 * v + 1.0)])
        P[v, :3, 3] = o
        P[v, :3, :3] = _frame(look - o, 0.9 * np.sin(2.9 * v + 0.5))
    return P


def occupancy():
    """uint8 bitfield [C * G^3 / 8] (Morton order, cascade-major) of the shell, and the bool [C * G^3] it packs"""
    from laenerf_amd.editing.mask_lift import _compact_bits
    m = np.arange(G ** 3, dtype=np.uint32)
    coord = np.stack([_compact_bits(m), _compact_bits(m >> 1), _compact_bits(m >> 2)], -1).astype(np.float64)
    occ = np.zeros((C, G ** 3), bool)
    for c in range(C):
        mip = min(2.0 ** c, BOUND)
        r = np.linalg.norm((((coord + 0.5) / G) * 2 - 1) * mip, axis=-1)
        side = 2 * mip / G
        occ[c] = (r >= RADIUS - side) & (r <= RADIUS)
    occ = occ.reshape(-1)
    return np.packbits(occ, bitorder="little"), occ


def render(P):
    """one analytic view in float64 -> depth = OPACITY * t, opacity, mask (uint8), each [H, W]"""
    fx, fy, cx, cy = INTRINSICS
    a = AXIS / np.linalg.norm(AXIS)
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(gx + 0.5 - cx) / fx, (gy + 0.5 - cy) / fy, np.ones_like(gx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d @ P[:3, :3].T
    o = P[:3, 3]
    b = d @ o
    disc = b * b - (o @ o - RADIUS * RADIUS)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    hit = (disc > 0) & (t > 0)
    X = o + t[..., None] * d
    mask = hit & (X @ a >= CAP)
    return np.where(hit, OPACITY * t, 0.0), np.where(hit, OPACITY, 0.0), mask.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fixture(V):
    """-> dict: depths, opacities fp32 [V, H, W], masks uint8 [V, H, W], poses fp32 [V, 4, 4], bits uint8 [C G^3 / 8], occ bool
    [C G^3].  Cached: do not write into the arrays."""
    P = poses(V)
    planes = [render(p) for p in P]
    bits, occ = occupancy()
    out = {"depths": np.stack([p[0] for p in planes]).astype(np.float32), "opacities": np.stack([p[1] for p in planes]).astype(np.float32),
           "masks": np.stack([p[2] for p in planes]), "poses": P.astype(np.float32), "bits": bits, "occ": occ}
    for arr in out.values():
        arr.setflags(write=False)
    return out


def numpy_args(f):
    """the positional arguments of mask_lift_numpy"""
    return f["depths"], f["opacities"], f["masks"], f["poses"], INTRINSICS, H, W, f["bits"], C, BOUND, G


@functools.lru_cache(maxsize=None)
def restated(V, dtype="float64", depth_margin=2.0, min_views=1, min_share=0.5):
    """mask_lift_numpy on the fixture, computed once per setting"""
    from laenerf_amd.editing.mask_lift import mask_lift_numpy
    return mask_lift_numpy(*numpy_args(fixture(V)), depth_margin=depth_margin, min_views=min_views, min_share=min_share,
                           dtype=np.dtype(dtype))


def sides_of(cells):
    """the cell side of each cell index (cascade * G^3 + Morton)"""
    return 2 * np.minimum(2.0 ** (np.asarray(cells) // G ** 3), BOUND) / G


def geometric_violations(cells, centres, depth_margin):
    """the selected cells that break the property the rule promises on this scene, independent of any restatement: a selected
    cell's centre lies within (depth_margin + 1) sides of the sphere's surface and on the masked side of the cap's plane, within
    one side -> (indices off the surface, indices across the plane)"""
    a = AXIS / np.linalg.norm(AXIS)
    side = sides_of(cells)
    centres = np.asarray(centres, np.float64)
    off = np.abs(np.linalg.norm(centres, axis=-1) - RADIUS) > (depth_margin + 1) * side
    across = centres @ a < CAP - side
    return np.flatnonzero(off), np.flatnonzero(across)
