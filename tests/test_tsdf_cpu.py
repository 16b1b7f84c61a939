"""The TSDF rule on the CPU: tsdf.tsdf_numpy / tsdf_vertex_colors_numpy on the scene of tests/tsdf_util.py.  These tests assert
the figures tests/test_gpu_tsdf.py relies on, for the very inputs it uses.

Measured (float64 against float32 restatement; V views, lattice):
  V = 24, 32^3         pairs inside the band 0.038 %, voxels with such a pair 0.91 %, max |u32 - u64| outside 1.4e-6
  V = 65, 24^3         0.034 %, 2.3 %, 9.2e-7
  V = 24, 19 x 24 x 32 0.033 %, 0.81 %, 8.5e-7
  count mismatches outside the band: none.  The band eps = 1e-4 (mask_lift_util.EPS) is an exclusion band, not a tolerance; the
  caps are 0.5 % of the pairs and 5 % of the voxels; the bound on u is derived in tsdf_util.U_TOL.
Meshes of the float64 field (marching_cubes_numpy at 0): closed, Euler characteristic 2, the largest vertex distance from the
sphere 0.39 / 0.33 / 0.35 voxel sides (bound 0.75).
Vertex colours of the float64 restatement against 0.5 + 0.5 X / 0.45 at the vertex: largest error 0.027 / 0.021 / 0.0435; the
bound is twice the largest, tsdf_util.COLOR_TOL = 0.087 (the frames are bytes of the colour at the pixel's hit point, fused over
the truncation band of three voxel sides).
The fill rule: 12 views at 32^3 leave a second solid component (Euler characteristic 3 in all), which the components filter
removes."""
import numpy as np
import pytest

import tsdf_util as U
from laenerf_amd.components import filter_components_numpy
from laenerf_amd.mesh import marching_cubes_numpy
from laenerf_amd.tsdf import FREE, NEAR, OCCLUDED, OUTSIDE, UNSEEN, tsdf_numpy, tsdf_vertex_colors_numpy

CASES = U.GPU_CASES + ((24, 32, False),)


@pytest.mark.parametrize("V,shape,close", CASES)
def test_float32_restatement_against_float64(V, shape, close):
    r64, r32 = U.restated(V, shape, close=close), U.restated(V, shape, "float32", close=close)
    _, v64 = U.band(r64)
    _, v32 = U.band(r32)
    ok = ~(v64 | v32)
    c64, c32 = r64["counts"].reshape(-1, 4), r32["counts"].reshape(-1, 4)
    assert (c64[ok] == c32[ok]).all()
    du = np.abs(r32["u"].astype(np.float64) - r64["u"]).reshape(-1)[ok].max()
    print("max |u32 - u64| outside the band", du)
    assert du <= U.U_TOL
    assert r32["u"].dtype == np.float32 and r32["rgb"].dtype == np.float32 and (np.abs(r64["u"]) <= 1).all()
    # the outcome table and the counts say the same
    for code, col in ((NEAR, 0), (FREE, 1), (OCCLUDED, 2)):
        assert ((r64["outcome"] == code).sum(1) == c64[:, col]).all()


@pytest.mark.parametrize("V,shape,close", CASES)
def test_mesh_is_one_closed_surface_on_the_sphere_with_its_colours(V, shape, close):
    r = U.restated(V, shape, close=close)
    verts, tris = marching_cubes_numpy(r["u"].astype(np.float32), 0.0)
    m = U.mesh_report(verts, tris, shape)
    print("vertices", len(verts), "triangles", len(tris), "euler", m["euler"], "off", m["off"])
    assert m["closed"] and m["euler"] == 2 and m["off"] <= U.SIDE_TOL
    col, n_grey = tsdf_vertex_colors_numpy(r["rgb"], r["counts"], verts)
    err = np.abs(col - (0.5 + 0.5 * m["X"] / U.RADIUS)).max()
    print("largest vertex colour error", err)
    assert n_grey == 0 and err <= U.COLOR_TOL


def test_fill_rule_leaves_a_blob_that_the_components_filter_removes():
    r = U.restated(12, 32)
    u = r["u"].astype(np.float32)
    verts, tris = marching_cubes_numpy(u, 0.0)
    m = U.mesh_report(verts, tris, 32)
    assert m["off"] > U.SIDE_TOL                                     # something far from the sphere
    kept, info = filter_components_numpy(u, 0.0, largest=True)
    assert info["n_components"] >= 2
    v2, t2 = marching_cubes_numpy(kept, 0.0)
    m2 = U.mesh_report(v2, t2, 32)
    assert m2["closed"] and m2["euler"] == 2 and m2["off"] <= U.SIDE_TOL
    # the blob is what no view sees empty: every voxel of it is seen occluded and by fewer than min_views as near or free
    c = r["counts"].reshape(-1, 4)
    gone = ((u > 0) & ~(kept > 0)).reshape(-1)
    assert gone.any() and (c[gone, 2] > 0).all() and (c[gone, 0] + c[gone, 1] == 0).all()


def test_special_values():
    f = U.fixture(24)
    ax, tr = U.axes(12), U.trunc(12)
    base = tsdf_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, ax, tr, frames=f["frames"])
    # min_views = 2: a voxel with one observation falls back to the fill rule
    two = tsdf_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, ax, tr, frames=f["frames"], min_views=2)
    c = base["counts"].reshape(-1, 4).astype(np.int64)
    n_obs = c[:, 0] + c[:, 1]
    want = np.where(n_obs >= 2, base["u"].reshape(-1), np.where(c[:, 2] > 0, 1.0, -1.0))
    assert (two["counts"] == base["counts"]).all() and (two["u"].reshape(-1) == want).all()
    big = tsdf_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, ax, tr, min_views=25)
    assert set(np.unique(big["u"])) <= {-1.0, 1.0} and big["rgb"] is None
    # a view of all +inf: every voxel in its frame is free (the others are never seen), u = -1 everywhere, the mesh is empty
    inf = np.full((1, U.H, U.W), np.inf, np.float32)
    r = tsdf_numpy(inf, f["poses"][:1], U.INTRINSICS, U.H, U.W, ax, tr)
    assert np.isin(r["outcome"], (FREE, OUTSIDE)).all() and (r["outcome"] == FREE).any() and (r["u"] == -1.0).all()
    verts, tris = marching_cubes_numpy(r["u"].astype(np.float32), 0.0)
    assert len(verts) == 0 and len(tris) == 0
    # a NaN plane changes nothing; the sign bit is ignored
    pk = np.concatenate([f["packed"], np.full((1, U.H, U.W), np.nan, np.float32)])
    po = np.concatenate([f["poses"], f["poses"][:1]])
    fr = np.concatenate([f["frames"], f["frames"][:1]])
    r = tsdf_numpy(pk, po, U.INTRINSICS, U.H, U.W, ax, tr, frames=fr)
    assert np.isin(r["outcome"][:, -1], (UNSEEN, OUTSIDE)).all() and (r["outcome"][:, -1] == UNSEEN).any()
    neg = tsdf_numpy(-f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, ax, tr, frames=f["frames"])
    for k in ("u", "counts", "rgb"):
        assert np.array_equal(r[k], base[k]) and np.array_equal(neg[k], base[k])


def test_vertex_colour_cases_by_hand():
    rgb = np.zeros((2, 2, 2, 3), np.float32)
    counts = np.zeros((2, 2, 2, 4), np.uint16)
    rgb[0, 0, 0], rgb[1, 0, 0], rgb[0, 1, 0] = (0.2, 0.4, 0.6), (1.0, 0.0, 0.5), (0.9, 0.8, 0.7)
    counts[0, 0, 0, 0], counts[1, 0, 0, 0] = 3, 1                                    # (0,1,0) holds a colour but no near view
    verts = np.array([[0.25, 0, 0], [0, 0.5, 0], [0, 1, 0.5], [0, 0, 0], [1, 0.75, 0]], np.float32)
    col, n_grey = tsdf_vertex_colors_numpy(rgb, counts, verts)
    want = [[0.2 + 0.25 * 0.8, 0.4 - 0.25 * 0.4, 0.6 - 0.25 * 0.1], [0.2, 0.4, 0.6], [0.5, 0.5, 0.5], [0.2, 0.4, 0.6], [1.0, 0.0, 0.5]]
    assert n_grey == 1 and np.allclose(col, want, atol=1e-7)


def test_package_exports_and_binding():
    import laenerf_amd
    from laenerf_amd import _lib, build
    assert laenerf_amd.tsdf_fuse is laenerf_amd.tsdf.tsdf_fuse and laenerf_amd.tsdf_numpy is tsdf_numpy
    assert "lae_tsdf_fuse" in _lib.SIGNATURES and "lae_tsdf_vertex_colors" in _lib.SIGNATURES and "tsdf.hip" in build.SOURCES
    with pytest.raises(AttributeError):
        laenerf_amd.no_such_thing


def test_entry_points_reject_bad_arguments_before_any_launch(hip_lib):
    import ctypes
    from laenerf_amd import _lib
    for name in ("lae_tsdf_fuse", "lae_tsdf_vertex_colors"):
        getattr(hip_lib, name).argtypes = _lib.SIGNATURES[name]
    one = ctypes.c_void_p(64)

    def fuse(p=one, po=one, v=3, fx=100.0, fy=100.0, h=40, w=56, xs=one, ys=one, zs=one, n=(8, 8, 8), fr=None, tr=0.1, mv=1, u=one, c=None, rgb=None):
        return hip_lib.lae_tsdf_fuse(p, po, v, fx, fy, 30.5, 18.25, h, w, xs, ys, zs, n[0], n[1], n[2], fr, tr, mv, u, c, rgb, None)
    for kw in (dict(p=None), dict(po=None), dict(xs=None), dict(ys=None), dict(zs=None), dict(u=None), dict(rgb=one)):
        assert fuse(**kw) == -3, kw
    for kw in (dict(v=0), dict(v=65536), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15), dict(n=(1, 8, 8)), dict(n=(8, 8, 513)), dict(tr=0.0),
               dict(tr=-1.0), dict(tr=float("nan")), dict(tr=float("inf")), dict(fx=0.0), dict(fy=-2.0), dict(mv=0), dict(c=ctypes.c_void_p(68))):
        assert fuse(**kw) == -1, kw
    vc = hip_lib.lae_tsdf_vertex_colors
    assert vc(one, one, 1, 8, 8, one, 4, one, None, None) == -1 and vc(one, one, 8, 8, 600, one, 4, one, None, None) == -1
    assert vc(None, one, 8, 8, 8, one, 4, one, None, None) == -3 and vc(one, None, 8, 8, 8, one, 4, one, None, None) == -3
    assert vc(one, one, 8, 8, 8, None, 4, one, None, None) == -3 and vc(one, one, 8, 8, 8, one, 4, None, None, None) == -3
    assert vc(None, None, 8, 8, 8, None, 0, None, None, None) == 0
