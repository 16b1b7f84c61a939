"""The scenes of the texture-atlas tests, built on tests/tsdf_util.py: its sphere (radius 0.45), cameras, packed views and
frames (`fixture(V, close)`, colour 0.5 + 0.5 X / 0.45), and the marching-cubes mesh of its restated float64 TSDF field.

    mesh(case)              the mesh of tsdf_util's case (V, lattice, close): positions in the box, triangles, vertex normals
    texels(case, dtype)     atlas_texels_numpy on it (cell = CELL)
    fused(case, dtype, kind)    atlas_fuse_views_numpy of the case's views into the float32 texels; kind "affine": the fixture's
                            frames; "pattern": PATTERN frames
    band(r)                 the exclusion band of the float64 comparisons (tsdf_util's eps and caps), asserted
    surface_points(case)    10 000 random points on the mesh: triangle, barycentric weights, position
    pattern(X)              the detail pattern: 0.5 + 0.4 sin(2 pi X / PERIOD) per axis, evaluated at X moved onto the sphere

PERIOD = 0.115 lies between four image pixels (a pixel covers 2.55 / 100 = 0.0255 at the nearest surface point: 0.102) and two
lattice cells of the DETAIL case's lattice (2 x 1.5 / 23 = 0.130): the views resolve it, the lattice does not."""
import functools

import numpy as np

import tsdf_util as U

CELL = 8
MIN_COS = 0.25                     # the tests' own value, whatever the default is
EPS, PAIR_CAP, TEXEL_CAP = U.EPS, U.PAIR_CAP, U.VOXEL_CAP
CASES = U.GPU_CASES                # (24, (19, 24, 32), False), (65, 24, False), (24, (19, 24, 32), True)
DETAIL_CASE = U.GPU_CASES[1]       # the cubic lattice of 24 points, 65 views
PERIOD = 0.115
N_POINTS = 10000
# twice the largest error of the texture, sampled at surface_points, against 0.5 + 0.5 X / 0.45 on the float64 restatement
# with MIN_COS (0.0723 / 0.0265 / 0.0723 on the three cases: the 19-point axis and 24 views make the first and third coarse;
# test_atlas_cpu.py test_affine_scene_error prints and bounds them).  A pixel of the views covers 0.028 of the colour range.
COLOR_TOL = 0.145


def bounds(shape):
    return np.full(3, -U.HALF, np.float32), np.full(3, U.HALF, np.float32)


@functools.lru_cache(maxsize=None)
def mesh(case):
    """-> dict pos fp32 [V, 3] (in the box), tris int32 [T, 3], normals fp32 [V, 3], index_verts fp32 [V, 3], u fp32 (the field).
    Cached: do not write into the arrays."""
    from laenerf_amd.mesh import marching_cubes_numpy, vertex_attributes_numpy
    V, shape, close = case
    u = U.restated(V, shape, close=close)["u"].astype(np.float32)
    verts, tris = marching_cubes_numpy(u, 0.0)
    lo, hi = bounds(shape)
    a = vertex_attributes_numpy(u, verts, lo, hi)
    out = {"pos": a["pos"].astype(np.float32), "tris": tris, "normals": a["normals"].astype(np.float32), "index_verts": verts, "u": u}
    for arr in out.values():
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def texels(case, dtype="float32", cell=CELL):
    from laenerf_amd.atlas import atlas_texels_numpy
    m = mesh(case)
    return atlas_texels_numpy(m["pos"], m["tris"], m["normals"], cell=cell, dtype=np.dtype(dtype))


def pattern(X):
    """the detail colour of a point: X is moved onto the sphere along its radius first"""
    X = np.asarray(X, np.float64)
    X = X * (U.RADIUS / np.linalg.norm(X, axis=-1, keepdims=True))
    return 0.5 + 0.4 * np.sin(2.0 * np.pi * X / PERIOD)


def affine(X):
    return 0.5 + 0.5 * np.asarray(X, np.float64) / U.RADIUS


def _hits(P):
    """tsdf_util.render's ray / sphere intersection: -> (hit [H, W], X [H, W, 3])"""
    fx, fy, cx, cy = U.INTRINSICS
    gx, gy = np.meshgrid(np.arange(U.W, dtype=np.float64), np.arange(U.H, dtype=np.float64))
    d = np.stack([(gx + 0.5 - cx) / fx, (gy + 0.5 - cy) / fy, np.ones_like(gx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d @ P[:3, :3].T
    o = P[:3, 3]
    b = d @ o
    disc = b * b - (o @ o - U.RADIUS * U.RADIUS)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return (disc > 0) & (t > 0), o + t[..., None] * d


@functools.lru_cache(maxsize=None)
def pattern_frames(V, close=False):
    """uint8 [V', H, W, 3]: the pattern at every pixel's hit point, white elsewhere (lae_eval_view's byte rule)"""
    out = []
    for P in U.poses(V, close):
        hit, X = _hits(P)
        with np.errstate(all="ignore"):
            rgb = np.where(hit[..., None], pattern(np.where(hit[..., None], X, 1.0)), 1.0)
        out.append((np.clip(rgb, 0.0, 1.0).astype(np.float32) * np.float32(255)).astype(np.uint8))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def frames_of(case, kind):
    V, shape, close = case
    return U.fixture(V, close)["frames"] if kind == "affine" else pattern_frames(V, close)


@functools.lru_cache(maxsize=None)
def fused(case, dtype="float64", kind="affine", min_cos=MIN_COS):
    """atlas_fuse_views_numpy of the case's views into its float32 texels (the kernel's inputs), computed once per setting"""
    from laenerf_amd.atlas import atlas_fuse_views_numpy
    V, shape, close = case
    f = U.fixture(V, close)
    t = texels(case)
    return atlas_fuse_views_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, frames_of(case, kind), t["pos"], t["nrm"], t["owner"],
                                  U.trunc(shape), min_cos, dtype=np.dtype(dtype))


def band(r, owner):
    """-> (bool [N, V]: the pairs inside the exclusion band, bool [N]: the texels with such a pair); the shares are taken over the
    owned texels and asserted against tsdf_util's caps"""
    live = np.asarray(owner) >= 0
    pairs = r["margin"] < EPS
    tex = pairs.any(1)
    print("band: pairs", pairs[live].mean(), "texels", tex[live].mean())
    assert pairs[live].mean() <= PAIR_CAP and tex[live].mean() <= TEXEL_CAP
    return pairs, tex


@functools.lru_cache(maxsize=None)
def surface_points(case, n=N_POINTS, seed=5):
    """n random points on the mesh, triangles drawn by area -> (t [n], bary [n, 3], X [n, 3] float64)"""
    m = mesh(case)
    p = m["pos"].astype(np.float64)[m["tris"]]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    rng = np.random.default_rng(seed)
    t = rng.choice(len(area), n, p=area / area.sum())
    r = rng.uniform(size=(n, 2))
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    bary = np.stack([1 - r.sum(1), r[:, 0], r[:, 1]], -1)
    return t, bary, (p[t] * bary[..., None]).sum(1)


def sample_texture(texture, case, cell=CELL):
    """the texture ([S, S, 3] uint8 or float) looked up at surface_points -> [n, 3] float64"""
    from laenerf_amd.atlas import atlas_uv, sample_texture_numpy
    lay = texels(case, cell=cell)["layout"]
    t, bary, _ = surface_points(case)
    uv = (atlas_uv(lay)[t] * bary[..., None]).sum(1)
    return sample_texture_numpy(texture, uv)


def sample_vertex_colors(colors, case):
    """per-vertex colours interpolated over the triangles at surface_points -> [n, 3] float64"""
    t, bary, _ = surface_points(case)
    return (np.asarray(colors, np.float64)[mesh(case)["tris"][t]] * bary[..., None]).sum(1)


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
