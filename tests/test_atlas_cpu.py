"""The texture atlas without a GPU: the closed-form layout, the numpy restatements of the three kernels (laenerf_amd/atlas.py),
the OBJ writer and reader, and the new entry points' argument checks."""
import ctypes
import os

import numpy as np
import pytest

import atlas_util as AU
import tsdf_util as U
from laenerf_amd import atlas as A

CELLS, TS = (4, 5, 8), (1, 2, 3, 7, 50)
WEIGHT_EPS = 1e-9          # a bilinear weight below this is the rounding of the lookup's coordinate (float64, S <= 40), not a tap


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("T", TS)
def test_layout_owners_partition_and_lookups_stay_inside(cell, T):
    lay = A.atlas_layout(T, cell)
    cells = (T + 1) // 2
    cpr = int(np.ceil(np.sqrt(cells)))
    assert (lay.cells, lay.cpr, lay.S, lay.n_texels) == (cells, cpr, cpr * cell, cells * cell * cell)
    owner = A.atlas_owner_numpy(lay)
    # the owners partition the used texels: every triangle owns n (n + 1) / 2 (half 0) or n (n - 1) / 2 (half 1) texels, the rest
    # (the last half of an odd T) is unused, and every texel has its own pixel of the image
    count = np.bincount(owner[owner >= 0], minlength=T)
    assert np.array_equal(count, np.where(np.arange(T) & 1, cell * (cell - 1) // 2, cell * (cell + 1) // 2))
    assert (owner < 0).sum() == (cell * (cell - 1) // 2 if T & 1 else 0)
    Y, X = A.atlas_image_index(lay)
    assert len(set(zip(Y.tolist(), X.tolist()))) == lay.n_texels and Y.max() < lay.S and X.max() < lay.S
    uv = A.atlas_uv(lay)
    assert uv.shape == (T, 3, 2) and uv.min() >= 0 and uv.max() <= 1
    # a dense barycentric grid, edges and corners included: every tap with weight belongs to the triangle
    owner_img = A.atlas_image_numpy(owner, lay, fill=-1)
    G = 12
    a, b = np.meshgrid(np.arange(G + 1), np.arange(G + 1))
    keep = a + b <= G
    bary = np.stack([G - a[keep] - b[keep], a[keep], b[keep]], -1) / G                  # [P, 3]
    xy = np.einsum("pk,tkc->tpc", bary, A.atlas_corner_texels(lay))                     # [T, P, 2]
    TX, TY, wgt = A.bilinear_taps(xy[..., 0], xy[..., 1], lay.S)
    foreign = (owner_img[TY, TX] != np.arange(T)[:, None, None]) & (wgt > WEIGHT_EPS)
    assert not foreign.any()
    # and the file UVs are those corners: u = (X + 0.5) / S, v = 1 - (Y + 0.5) / S
    back = np.stack([uv[..., 0] * lay.S - 0.5, (1 - uv[..., 1]) * lay.S - 0.5], -1)
    assert np.abs(back - A.atlas_corner_texels(lay)).max() < 1e-9


def test_layout_limits():
    assert A.atlas_layout(220000, texture_size=4096).cell == 12 and A.atlas_layout(220000, texture_size=4096).S <= 4096
    with pytest.raises(ValueError, match="largest cell that fits.* is 7 "):
        A.atlas_layout(10 ** 7, 16)                                   # 2237 cells per row: S = 35792
    with pytest.raises(ValueError, match="largest cell"):
        A.atlas_layout(50, 3)
    with pytest.raises(ValueError, match="largest cell that fits.* is 3 "):
        A.atlas_layout(50, texture_size=16)                           # 5 cells per row: cell 3
    assert A.atlas_layout(0).n_texels == 0 and A.atlas_layout(0).S == 8
    assert A.atlas_layout(2 * 4096 * 4096, 4).S == 16384              # the largest atlas there is


def _random_mesh(T, seed):
    rng = np.random.default_rng(seed)
    V = T + 2
    verts = rng.uniform(-0.5, 0.5, (V, 3)).astype(np.float32)
    tris = np.stack([rng.permutation(V)[:3] for _ in range(T)]).astype(np.int32)
    normals = rng.normal(size=(V, 3)).astype(np.float32)
    return verts, tris, normals


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("T", (7, 50))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_affine_colours_are_reproduced_by_a_bilinear_lookup(cell, T, dtype):
    verts, tris, normals = _random_mesh(T, 10 * T + cell)
    t = A.atlas_texels_numpy(verts, tris, normals, cell=cell, dtype=dtype)
    lay = t["layout"]
    M = np.array([[0.3, -0.2, 0.1], [-0.1, 0.25, 0.3], [0.2, 0.2, -0.3]])

    def colour(X):                                                    # affine in position, within [0.05, 0.95] on the box
        return 0.5 + np.asarray(X, np.float64) @ M
    tex = A.atlas_image_numpy(colour(t["pos"]).astype(np.float32), lay)                  # fp32 texels, no byte quantisation
    rng = np.random.default_rng(1)
    r = rng.uniform(size=(T, 40, 2))
    flip = r.sum(-1) > 1
    r[flip] = 1 - r[flip]
    bary = np.concatenate([1 - r.sum(-1, keepdims=True), r], -1)                         # [T, 40, 3]
    bary = np.concatenate([bary, np.tile(np.eye(3)[None], (T, 1, 1)), np.tile([[0.5, 0.5, 0], [0, 0.5, 0.5]], (T, 1, 1))], 1)
    uv = np.einsum("tpk,tkc->tpc", bary, A.atlas_uv(lay))
    X = np.einsum("tpk,tkc->tpc", bary, verts.astype(np.float64)[tris])
    err = np.abs(A.sample_texture_numpy(tex, uv) - colour(X)).max()
    print("largest error", err)
    assert err <= 1e-6


def test_degenerate_triangles_give_finite_outputs():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.inf, 0, 0]], np.float32)
    normals = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]], np.float32)
    normals[1] = 0
    normals[0] = 0
    # a proper triangle whose vertex normals are all zero, a zero-area one (collinear), a repeated vertex, an index out of range,
    # a non-finite vertex
    tris = np.array([[0, 1, 2], [0, 1, 3], [1, 1, 2], [0, 1, 7], [0, 1, 4]], np.int32)
    for dtype in (np.float32, np.float64):
        t = A.atlas_texels_numpy(verts, tris, normals, cell=5, dtype=dtype)
        for k in ("pos", "nrm", "dirs"):
            assert np.isfinite(t[k]).all(), k
        own = t["owner"]
        assert np.allclose(t["nrm"][own == 0], [0, 0, 1]) and np.allclose(t["dirs"][own == 0], [0, 0, -1])     # the face normal steps in
        for k in (1, 2, 3, 4):
            assert (t["nrm"][own == k] == 0).all(), k
        assert (t["pos"][own == 3] == 0).all() and (t["pos"][own == -1] == 0).all() and (t["dirs"][own == -1] == 0).all()
        assert (t["dirs"][own == 3] == [0, 0, 1]).all()
    # and a flagged texel is seen by no view: grey, counted
    f = U.fixture(24)
    r = A.atlas_fuse_views_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, f["frames"], t["pos"], t["nrm"], t["owner"], 0.2, 0.0)
    flagged = (t["owner"] >= 1)
    assert (r["counts"][flagged] == 0).all() and (r["rgb"][flagged] == 0.5).all() and r["n_grey"] >= flagged.sum()
    assert (r["rgb"][t["owner"] < 0] == 0).all() and np.isfinite(r["rgb"]).all()


def test_the_face_normals_of_the_marching_cubes_sphere_point_outward():
    for case in AU.CASES[:2]:
        t = AU.texels(case)
        live = t["owner"] >= 0
        length = np.linalg.norm(t["nrm"][live].astype(np.float64), axis=1)
        ok = length > 0
        assert ok.mean() > 0.99 and np.abs(length[ok] - 1).max() < 1e-6
        radial = t["pos"][live][ok].astype(np.float64)
        radial /= np.linalg.norm(radial, axis=1, keepdims=True)
        cosine = (radial * t["nrm"][live][ok]).sum(1)
        print("least cosine between the face normal and the radius", cosine.min())
        assert cosine.min() > 0.5
        # dirs: minus the interpolated vertex normal, unit
        assert ((t["dirs"][live][ok] * radial).sum(1) < -0.5).all()
        assert np.abs(np.linalg.norm(t["dirs"][live].astype(np.float64), axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("case", AU.CASES)
def test_float32_and_float64_fuse_agree_outside_the_band(case):
    """the float32 restatement (the kernel's statements) against float64, wherever no decision of the pair lies within eps = 1e-4
    of its threshold (in-frame tests, pixel floors, |s| = trunc, the min_cos test).  Measured shares inside the band on the three
    cases: pairs 0.00060 / 0.00064 / 0.00059, texels 0.014 / 0.041 / 0.015 (caps 0.005 and 0.05)."""
    t = AU.texels(case)
    r32, r64 = AU.fused(case, "float32"), AU.fused(case, "float64")
    pairs, tex = AU.band(r64, t["owner"])
    assert np.array_equal(r32["counted"][~pairs], r64["counted"][~pairs])
    ok = ~tex
    assert np.array_equal(r32["counts"][ok], r64["counts"][ok])
    d = np.abs(r32["rgb"].astype(np.float64) - r64["rgb"])[ok].max()
    print("max |rgb32 - rgb64| outside the band", d, "grey", r32["n_grey"], r64["n_grey"])
    assert d <= 1e-6                                                  # two fp32 divisions of exact integers: 2 * 2^-24 of at most 1
    assert r64["counts"].max() > 1 and (r64["counts"][t["owner"] >= 0] > 0).mean() > 0.99


@pytest.mark.parametrize("case", AU.CASES)
def test_affine_scene_error(case):
    """the texture of the affine scene, looked up at 10 000 surface points, against 0.5 + 0.5 X / 0.45: the largest error on the
    float64 restatement is 0.0723 / 0.0265 / 0.0723; atlas_util.COLOR_TOL is twice the largest of them, rounded up"""
    t = AU.texels(case)
    r = AU.fused(case, "float64")
    tex = A.atlas_image_numpy(r["rgb"], t["layout"])
    _, _, X = AU.surface_points(case)
    err = np.abs(AU.sample_texture(tex, case) - AU.affine(X)).max()
    print("largest error", err, "grey", r["n_grey"])
    assert err <= AU.COLOR_TOL / 2 and r["n_grey"] == 0


def test_the_texture_keeps_detail_the_vertex_colours_lose():
    """pattern frames (period 0.115: above four pixels, below two lattice cells) on the 24^3 lattice with 65 views, float64
    restatements, 10 000 surface points: RMS error of the baked texture 0.0754, of tsdf_vertex_colors_numpy's colours interpolated
    over the triangles 0.2390 (the pattern's own RMS about its mean is 0.286)."""
    from laenerf_amd.tsdf import tsdf_numpy, tsdf_vertex_colors_numpy
    case = AU.DETAIL_CASE
    V, shape, close = case
    t = AU.texels(case)
    r = AU.fused(case, "float64", "pattern")
    tex = A.atlas_image_numpy(r["rgb"], t["layout"])
    _, _, X = AU.surface_points(case)
    want = AU.pattern(X)
    e_tex = AU.rms(AU.sample_texture(tex, case), want)
    f = U.fixture(V, close)
    v = tsdf_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, U.axes(shape), U.trunc(shape), frames=AU.pattern_frames(V, close))
    col, _ = tsdf_vertex_colors_numpy(v["rgb"], v["counts"], AU.mesh(case)["index_verts"])
    e_vert = AU.rms(AU.sample_vertex_colors(col, case), want)
    print("RMS error: texture", e_tex, "vertex colours", e_vert, "pattern RMS", AU.rms(want, want.mean(0)))
    assert e_tex < e_vert


def test_pack_restated():
    lay = A.atlas_layout(5, 5)                                        # three cells in a 2 x 2 atlas, the last one half used
    owner = A.atlas_owner_numpy(lay)
    rng = np.random.default_rng(0)
    rgb = rng.uniform(-0.2, 1.2, (lay.n_texels, 3)).astype(np.float32)
    rgb[3] = np.nan
    img = A.atlas_pack_numpy(rgb, owner, lay)
    Y, X = A.atlas_image_index(lay)
    from laenerf_amd.mesh import color_bytes_numpy
    assert img.shape == (lay.S, lay.S, 3) and img.dtype == np.uint8
    assert np.array_equal(img[Y[owner >= 0], X[owner >= 0]], color_bytes_numpy(rgb[owner >= 0])) and (img[Y[3], X[3]] == 0).all()
    assert (img[Y[owner < 0], X[owner < 0]] == 0).all()
    used = np.zeros((lay.S, lay.S), bool)
    used[Y, X] = True
    assert (img[~used] == 0).all() and (~used).any()                  # the cell past `cells`


@pytest.mark.parametrize("with_normals", (True, False))
def test_obj_round_trip(tmp_path, with_normals):
    verts, tris, normals = _random_mesh(7, 3)
    lay = A.atlas_layout(len(tris), 5)
    uv = A.atlas_uv(lay)
    tex = np.random.default_rng(1).integers(0, 256, (lay.S, lay.S, 3), dtype=np.uint8)
    path = A.write_obj(str(tmp_path / "sub" / "thing.obj"), verts, tris, uv, tex, normals=normals if with_normals else None)
    assert sorted(os.listdir(tmp_path / "sub")) == ["thing.mtl", "thing.obj", "thing.png"]
    o = A.read_obj(path)
    assert o["mtllib"] == "thing.mtl" and o["map_kd"] == "thing.png"
    assert o["vertices"].shape == (9, 3) and np.array_equal(o["vertices"].astype(np.float32), verts)
    assert np.array_equal(o["triangles"], tris) and o["uv"].shape == (7, 3, 2) and np.abs(o["uv"] - uv).max() < 1e-11
    assert (o["normals"] is None) if not with_normals else np.array_equal(o["normals"].astype(np.float32), normals)
    assert o["texture"].shape == (lay.S, lay.S, 3) and np.array_equal(o["texture"], tex)
    text = open(path).read().split("\n")
    assert text[0] == "mtllib thing.mtl" and sum(ln.startswith("vt ") for ln in text) == 21
    assert sum(ln.startswith("f ") for ln in text) == 7 and text[-2].count("/") == (6 if with_normals else 3)
    # the stem alone names the same three files; an empty mesh writes valid empty files
    A.write_obj(str(tmp_path / "empty"), np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3, 2)), np.zeros((8, 8, 3), np.uint8),
                normals=np.zeros((0, 3)) if with_normals else None)
    e = A.read_obj(str(tmp_path / "empty.obj"))
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3) and e["uv"].shape == (0, 3, 2) and e["texture"].shape == (8, 8, 3)
    with pytest.raises(ValueError, match="write_obj"):
        A.write_obj(str(tmp_path / "bad.obj"), verts, tris + 5, uv, tex)
    with pytest.raises(ValueError, match="write_obj"):
        A.write_obj(str(tmp_path / "bad.obj"), verts, tris, uv[:-1], tex)


def test_entry_points_check_their_arguments_before_any_launch(hip_lib):
    one = ctypes.c_void_p(16)
    c, r, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    ref = ctypes.byref
    assert hip_lib.lae_atlas_layout(7, 5, ref(c), ref(r), ref(s)) == 0 and (c.value, r.value, s.value) == (4, 2, 10)
    for T in (1, 2, 3, 50, 220000, 2 * 4096 * 4096):
        lay = A.atlas_layout(T, 4)
        assert hip_lib.lae_atlas_layout(T, 4, ref(c), ref(r), ref(s)) == 0 and (c.value, r.value, s.value) == (lay.cells, lay.cpr, lay.S)
    assert hip_lib.lae_atlas_layout(7, 5, None, ref(r), ref(s)) == -3
    for T, cell in ((0, 8), (7, 3), (10 ** 7, 16), (2 * 4096 * 4096 + 1, 4), (1, 16385)):
        assert hip_lib.lae_atlas_layout(T, cell, ref(c), ref(r), ref(s)) == -1, (T, cell)

    def texels(v=one, V=9, t=one, T=7, n=one, cell=5, pos=one, nrm=one, dirs=one, owner=one):
        return hip_lib.lae_atlas_texels(v, V, t, T, n, cell, pos, nrm, dirs, owner, None)
    for kw in (dict(v=None), dict(t=None), dict(pos=None), dict(nrm=None), dict(dirs=None), dict(owner=None)):
        assert texels(**kw) == -3, kw
    for kw in (dict(V=0), dict(T=0), dict(cell=3), dict(T=10 ** 7, cell=16)):
        assert texels(**kw) == -1, kw

    def fuse(p=one, po=one, V=24, fx=100.0, fy=100.0, cx=30.5, cy=18.25, H=40, W=56, fr=one, pos=one, nrm=one, owner=one, N=64, tr=0.2,
             mc=0.25, rgb=one, counts=None, grey=None):
        return hip_lib.lae_atlas_fuse_views(p, po, V, fx, fy, cx, cy, H, W, fr, pos, nrm, owner, N, tr, mc, rgb, counts, grey, None)
    for kw in (dict(p=None), dict(po=None), dict(fr=None), dict(pos=None), dict(nrm=None), dict(owner=None), dict(rgb=None)):
        assert fuse(**kw) == -3, kw
    nan = float("nan")
    for kw in (dict(V=0), dict(V=65536), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(N=0), dict(N=16384 * 16384 + 1), dict(fx=0.0),
               dict(fy=-2.0), dict(fx=nan), dict(cx=nan), dict(cy=nan), dict(tr=0.0), dict(tr=-0.3), dict(tr=nan), dict(tr=float("inf")),
               dict(mc=-0.1), dict(mc=1.0), dict(mc=nan)):
        assert fuse(**kw) == -1, kw

    def pack(rgb=one, owner=one, T=7, cell=5, img=one):
        return hip_lib.lae_atlas_pack(rgb, owner, T, cell, img, None)
    assert pack(rgb=None) == -3 and pack(owner=None) == -3 and pack(img=None) == -3
    assert pack(T=0) == -1 and pack(cell=3) == -1 and pack(T=10 ** 7, cell=16) == -1
