"""The scene of the TSDF tests, built in float64 and handed over as fp32.

The sphere of tests/mask_lift_util.py (radius 0.45, opacity 0.97, depth = 0.97 t; 40 x 56 pixels, focal 100, principal point
(30.5, 18.25)) seen from cameras on a Fibonacci sphere of radius 3 -- not that file's ring, which never looks down the axis: view v
of V stands at height z = 1 - (2 v + 1) / V and azimuth 2.399963 v + 0.3, with the look-at offset and roll of mask_lift_util.poses.
`close=True` appends that file's view 0: a camera 0.62 from the centre looking along the tangent, so that whole bricks of the
lattice are behind it or outside its frame.  The lattice is linspace(-0.75, 0.75, R) per axis (or per-axis sizes), the truncation
three voxel sides.  Frames: the byte colour of the hit point X, rgb = 0.5 + 0.5 X / 0.45, white elsewhere."""
import functools

import numpy as np

import mask_lift_util as MU

H, W, INTRINSICS, RADIUS, OPACITY = MU.H, MU.W, MU.INTRINSICS, MU.RADIUS, MU.OPACITY
HALF = 0.75                # the lattice spans [-HALF, HALF]^3
TRUNC_VOXELS = 3.0
EPS = MU.EPS               # the exclusion band of the comparisons with float64, in the units of tsdf_numpy's margin
PAIR_CAP = 0.005           # at most this share of the (voxel, view) pairs may lie inside it
VOXEL_CAP = 0.05           # at most this share of the voxels may have such a pair
U_TOL = 2e-5               # |u32 - u64| outside the band: s carries about four roundings at magnitude <= 3.3 (<= 1e-6); divided
#                            by trunc = 0.145 that is 7e-6, a mean of such terms stays below it; times three
SIDE_TOL = 0.75            # every vertex lies within this many voxel sides of the sphere
# (V, lattice, with the close camera appended): no axis a multiple of the kernel's brick (4 x 4 x 16); one view more than its LDS
# pose chunk; whole bricks behind the close camera or outside its frame
GPU_CASES = ((24, (19, 24, 32), False), (65, 24, False), (24, (19, 24, 32), True))
COLOR_TOL = 0.087          # twice the largest vertex-colour error measured on the float64 restatement (0.0435; test_tsdf_cpu.py)


def poses(V, close=False):
    """[V (+ 1), 4, 4] float64 cam2world"""
    P = np.tile(np.eye(4), (V, 1, 1))
    for v in range(V):
        z = 1.0 - (2 * v + 1) / V
        az = 2.399963 * v + 0.3
        rho = np.sqrt(max(1.0 - z * z, 0.0))
        o = 3.0 * np.array([rho * np.cos(az), rho * np.sin(az), z])
        look = 0.04 * np.array([np.sin(2.1 * v), np.cos(1.3 * v), np.sin(0.7 * v + 1.0)])
        P[v, :3, 3] = o
        P[v, :3, :3] = MU._frame(look - o, 0.9 * np.sin(2.9 * v + 0.5))
    if close:
        P = np.concatenate([P, MU.poses(1)], 0)
    return P


def render(P):
    """one analytic view in float64 -> packed plane [H, W] (t where the ray hits, +inf elsewhere: depth / opacity = t), frame uint8 [H, W, 3]"""
    fx, fy, cx, cy = INTRINSICS
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
    rgb = np.where(hit[..., None], 0.5 + 0.5 * X / RADIUS, 1.0)
    depth, opacity = np.where(hit, OPACITY * t, 0.0).astype(np.float32), np.where(hit, OPACITY, 0.0).astype(np.float32)
    with np.errstate(all="ignore"):
        plane = np.abs(np.where(opacity >= np.float32(0.5), depth / opacity, np.float32(np.inf))).astype(np.float32)   # lae_mask_lift_pack
    return plane, (np.clip(rgb, 0.0, 1.0).astype(np.float32) * np.float32(255)).astype(np.uint8)


def axes(shape):
    shape = (shape,) * 3 if np.isscalar(shape) else tuple(shape)
    return [np.linspace(-HALF, HALF, n).astype(np.float32) for n in shape]


def trunc(shape):
    """TRUNC_VOXELS x the largest axis spacing, from the fp32 axes"""
    return float(TRUNC_VOXELS * max(float(a[1] - a[0]) for a in axes(shape)))


@functools.lru_cache(maxsize=None)
def fixture(V, close=False):
    """-> dict packed fp32 [V', H, W], frames uint8 [V', H, W, 3], poses fp32 [V', 4, 4].  Cached: do not write into the arrays."""
    P = poses(V, close)
    views = [render(p) for p in P]
    out = {"packed": np.stack([v[0] for v in views]), "frames": np.stack([v[1] for v in views]), "poses": P.astype(np.float32)}
    for arr in out.values():
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(V, shape, dtype="float64", close=False, min_views=1, frames=True):
    """tsdf_numpy on the fixture, computed once per setting.  Cached: do not write into the arrays."""
    from laenerf_amd.tsdf import tsdf_numpy
    f = fixture(V, close)
    return tsdf_numpy(f["packed"], f["poses"], INTRINSICS, H, W, axes(shape), trunc(shape), frames=f["frames"] if frames else None,
                      min_views=min_views, dtype=np.dtype(dtype))


def band(r):
    """-> (bool [n, V]: the pairs inside the exclusion band, bool [n]: the voxels with such a pair), the caps asserted"""
    pairs = r["margin"] < EPS
    voxels = pairs.any(1)
    print("band: pairs", pairs.mean(), "voxels", voxels.mean())
    assert pairs.mean() <= PAIR_CAP and voxels.mean() <= VOXEL_CAP
    return pairs, voxels


def mesh_report(verts, tris, shape):
    """-> dict: closed (every edge in exactly two triangles), euler (V - E + F), off (the largest distance of a vertex from the
    sphere, in voxel sides; verts in index space), X (the vertices in world space, float64)"""
    verts, tris = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3)
    shape = (shape,) * 3 if np.isscalar(shape) else tuple(shape)
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    step = np.array([2 * HALF / (n - 1) for n in shape])
    X = verts * step - HALF
    off = float(np.abs(np.linalg.norm(X, axis=1) - RADIUS).max() / step.max()) if len(X) else 0.0
    return {"closed": bool(len(cnt)) and bool((cnt == 2).all()), "euler": len(verts) - len(uniq) + len(tris), "off": off, "X": X}
