"""lae_atlas_texels / lae_atlas_fuse_views / lae_atlas_pack (through laenerf_amd.atlas) against their numpy restatements on the scenes
of tests/atlas_util.py, and NeRFRenderer.extract_mesh_textured / save_mesh_textured / Trainer.save_mesh_textured on a small randomly
initialised renderer.

What is compared, and how closely (tests/test_atlas_cpu.py asserts the figures on the CPU, for these very inputs):
  texels    pos, nrm, dirs bit for bit and owner equal against atlas_texels_numpy(dtype=float32).
  float32   counts equal on every texel and rgb bit for bit against atlas_fuse_views_numpy(dtype=float32); n_grey equal.
  float64   counts equal on every texel without a (texel, view) pair whose nearest decision lies within eps = 1e-4 of its
            threshold, rgb within 1e-6 there; the shares inside that band are capped (0.5 % of the pairs, 5 % of the texels).
  cull      the same bytes with LAE_ATLAS_CULL=0 and from two calls; one camera stands 0.62 from the centre.
  scene     the baked texture keeps a pattern the vertex colours lose; on the affine scene it stays within atlas_util.COLOR_TOL."""
import numpy as np
import pytest
import torch

import atlas_util as AU
import tsdf_util as U
from gpu_util import DEV, N
from gpu_util import T as _T

pytestmark = pytest.mark.gpu


def T(a):
    return _T(np.array(a))                                           # the fixtures are read-only: hand torch a copy


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tetrahedron():
    verts = np.array([[0.3, 0.3, 0.3], [-0.3, -0.3, 0.3], [-0.3, 0.3, -0.3], [0.3, -0.3, -0.3]], np.float32)
    tris = np.array([[0, 1, 3], [0, 2, 1], [0, 3, 2], [1, 2, 3]], np.int32)
    return verts, tris, (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(np.float32), 4


def _seven():
    rng = np.random.default_rng(7)
    verts = rng.uniform(-0.5, 0.5, (9, 3)).astype(np.float32)
    tris = np.stack([rng.permutation(9)[:3] for _ in range(7)]).astype(np.int32)
    tris[3] = (2, 2, 5)                                              # a zero-area triangle
    normals = rng.normal(size=(9, 3)).astype(np.float32)
    normals[tris[1]] = 0                                             # a triangle without vertex normals
    return verts, tris, normals, 5


def _sphere():
    m = AU.mesh(AU.CASES[0])
    return m["pos"], m["tris"], m["normals"], AU.CELL


@pytest.mark.parametrize("make", (_tetrahedron, _seven, _sphere))
@pytest.mark.parametrize("with_normals", (True, False))
def test_texels_bit_for_bit(make, with_normals):
    from laenerf_amd.atlas import atlas_texels, atlas_texels_numpy
    verts, tris, normals, cell = make()
    normals = normals if with_normals else None
    g = atlas_texels(T(verts), T(tris), None if normals is None else T(normals), cell=cell)
    r = atlas_texels_numpy(verts, tris, normals, cell=cell, dtype=np.float32)
    assert g["layout"] == r["layout"] and np.array_equal(N(g["owner"]), r["owner"])
    for k in ("pos", "nrm", "dirs"):
        print(k, "mismatches", (_bits(N(g[k])) != _bits(r[k])).sum())
        assert np.array_equal(_bits(N(g[k])), _bits(r[k])), k
    assert (r["owner"] >= 0).sum() > 0 and ((r["owner"] < 0).any() == bool(len(tris) & 1))


def _fuse(case, kind="affine", **kw):
    from laenerf_amd.atlas import atlas_fuse_views
    V, shape, close = case
    f = U.fixture(V, close)
    t = AU.texels(case)
    return atlas_fuse_views(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, T(AU.frames_of(case, kind)), T(t["pos"]), T(t["nrm"]),
                            T(t["owner"]), U.trunc(shape), AU.MIN_COS, counts=True, **kw)


@pytest.fixture(scope="module")
def fused():
    """case -> atlas_fuse_views' dict of device tensors, one launch per case"""
    return {case: _fuse(case) for case in AU.CASES}


@pytest.mark.parametrize("case", AU.CASES)
def test_fuse_bit_for_bit_against_the_float32_restatement(fused, case):
    r = AU.fused(case, "float32")
    g = fused[case]
    print("mismatches: counts", (N(g["counts"]) != r["counts"]).sum(), "rgb", (_bits(N(g["rgb"])) != _bits(r["rgb"])).sum())
    assert np.array_equal(N(g["counts"]), r["counts"]) and np.array_equal(_bits(N(g["rgb"])), _bits(r["rgb"]))
    assert int(g["n_grey"]) == r["n_grey"] and r["counts"].max() > 1


@pytest.mark.parametrize("case", AU.CASES)
def test_fuse_against_float64_outside_the_band(fused, case):
    r = AU.fused(case, "float64")
    _, in_band = AU.band(r, AU.texels(case)["owner"])
    ok = ~in_band
    g = fused[case]
    assert np.array_equal(N(g["counts"])[ok], r["counts"][ok])
    d = np.abs(N(g["rgb"]).astype(np.float64) - r["rgb"])[ok].max()
    print("max |rgb - rgb64| outside the band", d)
    assert d <= 1e-6                                                 # two fp32 divisions of exact integers: 2 * 2^-24 of at most 1


def test_cull_switch_and_two_calls_give_the_same_bytes(fused, monkeypatch):
    for case in (AU.CASES[2], AU.CASES[1]):                          # the close camera; the pose chunk crossed
        g = fused[case]
        again = _fuse(case)
        monkeypatch.setenv("LAE_ATLAS_CULL", "0")
        plain = _fuse(case)
        monkeypatch.delenv("LAE_ATLAS_CULL")
        for k in ("rgb", "counts", "n_grey"):
            assert torch.equal(g[k], again[k]) and torch.equal(g[k], plain[k]), (case, k)


def test_a_texel_no_view_sees_is_grey_and_counted():
    """the sphere's texels plus one at the centre of the sphere (behind the surface for every camera) and one unowned"""
    from laenerf_amd.atlas import atlas_fuse_views, atlas_fuse_views_numpy
    case = AU.CASES[0]
    V, shape, close = case
    f, t = U.fixture(V, close), AU.texels(case)
    live = np.nonzero(t["owner"] >= 0)[0][:300]                      # more than one workgroup
    pos = np.concatenate([t["pos"][live], np.zeros((2, 3), np.float32)])
    nrm = np.concatenate([t["nrm"][live], np.array([[0, 0, 1], [0, 0, 1]], np.float32)])
    owner = np.concatenate([t["owner"][live], np.array([5, -1], np.int32)])
    g = atlas_fuse_views(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, T(f["frames"]), T(pos), T(nrm), T(owner), U.trunc(shape),
                         AU.MIN_COS, counts=True)
    r = atlas_fuse_views_numpy(f["packed"], f["poses"], U.INTRINSICS, U.H, U.W, f["frames"], pos, nrm, owner, U.trunc(shape), AU.MIN_COS,
                               dtype=np.float32)
    assert int(g["n_grey"]) == r["n_grey"] == 1
    assert (N(g["rgb"])[300] == 0.5).all() and (N(g["rgb"])[301] == 0).all() and N(g["counts"])[300] == 0 and N(g["counts"])[:300].min() > 0
    assert np.array_equal(_bits(N(g["rgb"])), _bits(r["rgb"])) and np.array_equal(N(g["counts"]), r["counts"])


@pytest.mark.parametrize("T_cell", ((5, 5), (7, 4), (50, 8)))
def test_pack_equals_its_restatement(T_cell):
    from laenerf_amd.atlas import atlas_layout, atlas_owner_numpy, atlas_pack, atlas_pack_numpy, atlas_image_index
    lay = atlas_layout(*T_cell)
    owner = atlas_owner_numpy(lay)
    rng = np.random.default_rng(0)
    rgb = rng.uniform(-0.2, 1.2, (lay.n_texels, 3)).astype(np.float32)
    rgb[3], rgb[5, 1] = np.nan, np.inf
    img = N(atlas_pack(T(rgb), T(owner), lay))
    assert np.array_equal(img, atlas_pack_numpy(rgb, owner, lay))
    Y, X = atlas_image_index(lay)
    assert (img[Y[owner < 0], X[owner < 0]] == 0).all() and img.max() == 255


def test_scene_detail_and_affine_colour():
    """the device's texture against the device's vertex colours on the pattern frames (RMS error at 10 000 surface points), and the
    affine scene's texture against 0.5 + 0.5 X / 0.45"""
    from laenerf_amd.atlas import atlas_pack
    from laenerf_amd.tsdf import tsdf_fuse, tsdf_vertex_colors
    case = AU.DETAIL_CASE
    V, shape, close = case
    t, f = AU.texels(case), U.fixture(V, close)
    _, _, X = AU.surface_points(case)
    owner = T(t["owner"])
    tex = N(atlas_pack(_fuse(case, "pattern")["rgb"], owner, t["layout"]))
    want = AU.pattern(X)
    e_tex = AU.rms(AU.sample_texture(tex, case), want)
    ax = [torch.from_numpy(a) for a in U.axes(shape)]
    v = tsdf_fuse(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, ax, U.trunc(shape), frames=T(AU.pattern_frames(V, close)))
    col, _ = tsdf_vertex_colors(v["rgb"], v["counts"], T(AU.mesh(case)["index_verts"]))
    e_vert = AU.rms(AU.sample_vertex_colors(N(col), case), want)
    print("RMS error: texture", e_tex, "vertex colours", e_vert)
    assert e_tex < e_vert
    for c in AU.CASES:
        tc = AU.texels(c)
        img = N(atlas_pack(_fuse(c)["rgb"], T(tc["owner"]), tc["layout"]))
        err = np.abs(AU.sample_texture(img, c) - AU.affine(AU.surface_points(c)[2])).max()
        print(c, "largest colour error", err)
        assert err <= AU.COLOR_TOL


def test_python_operators_refuse_what_the_entry_points_would_misread():
    from laenerf_amd import atlas as A
    verts, tris, normals, cell = _seven()
    with pytest.raises(ValueError, match="atlas_texels"):
        A.atlas_texels(T(verts).double(), T(tris))
    with pytest.raises(ValueError, match="atlas_texels"):
        A.atlas_texels(T(verts), T(tris).long())
    with pytest.raises(ValueError, match="out of range"):
        A.atlas_texels(T(verts), T(tris + 4))
    with pytest.raises(ValueError, match="atlas_texels"):
        A.atlas_texels(T(verts), T(tris[:0]))
    with pytest.raises(ValueError, match="largest cell"):
        A.atlas_texels(T(verts), T(tris), cell=3)
    with pytest.raises(RuntimeError):
        A.atlas_texels(torch.from_numpy(verts), torch.from_numpy(tris))
    f = U.fixture(24)
    t = A.atlas_texels(T(verts), T(tris), cell=cell)
    good = dict(packed=T(f["packed"]), poses=T(f["poses"]), intrinsics=U.INTRINSICS, H=U.H, W=U.W, frames=T(f["frames"]), pos=t["pos"],
                nrm=t["nrm"], owner=t["owner"], trunc=0.2)
    for bad in (dict(packed=good["packed"].double()), dict(poses=good["poses"][:-1].contiguous()), dict(trunc=0.0), dict(min_cos=1.0),
                dict(min_cos=-0.5), dict(frames=good["frames"][:-1]), dict(intrinsics=(1.0, 2.0)), dict(nrm=t["nrm"][:-1].contiguous()),
                dict(owner=t["owner"].long())):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError, match="atlas_fuse_views"):
            A.atlas_fuse_views(**kw)
    with pytest.raises(ValueError, match="atlas_pack"):
        A.atlas_pack(t["pos"][:-1].contiguous(), t["owner"], t["layout"])
    assert A.atlas_fuse_views(**good)["counts"] is None


# ---------------------------------------------------------------- extract_mesh_textured / save_mesh_textured on a renderer
RES = 32
INTR_R = (50.0, 50.0, 27.5, 20.25)


@pytest.fixture(scope="module")
def scene():
    """the small randomly initialised renderer of tests/test_gpu_tsdf.py and four cameras"""
    from laenerf_amd import synthetic as S
    from test_gpu_frame import make
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0
    poses = T(S.lookat_poses(4, radius=3.2, seed=4))
    r.threshold = _threshold(r)
    return net, r, poses


def _threshold(r):
    """a level the random density crosses: the 0.7 quantile of the lattice's values, as tests/test_gpu_mesh_attrs.py takes it"""
    from laenerf_amd import mesh

    def query(pts):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return r.model.density_sigma(pts)
    u = mesh.extract_fields(r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu(), RES, query)
    return float(np.quantile(u.cpu().numpy(), 0.7))


def _views(poses):
    return dict(poses=poses, intrinsics=INTR_R, H=U.H, W=U.W)


def test_field_texels_equal_the_model_queried_directly(scene):
    from laenerf_amd.atlas import atlas_pack, atlas_texels, atlas_uv
    net, r, poses = scene
    thr = r.threshold
    ref = r.extract_mesh_attributes(resolution=RES, threshold=thr, colors=False)
    m = r.extract_mesh_textured(resolution=RES, threshold=thr, cell=5, color_chunk=1000)
    Tn = m["triangles"].shape[0]
    print("triangles", Tn, "texture", tuple(m["texture"].shape))
    assert Tn > 0 and torch.equal(m["vertices"], ref["vertices"]) and torch.equal(m["triangles"], ref["triangles"])
    assert torch.equal(m["normals"], ref["normals"]) and int(m["n_grey"]) == 0
    lay = m["layout"]
    assert lay.T == Tn and lay.cell == 5 and tuple(m["texture"].shape) == (lay.S, lay.S, 3) and m["texture"].dtype == torch.uint8
    assert np.array_equal(N(m["uv"]), atlas_uv(lay))
    tx = atlas_texels(ref["vertices"], ref["triangles"], ref["normals"], cell=5)
    for k in ("pos", "dirs", "owner"):
        assert torch.equal(m["texels"][k], tx[k]), k
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        direct = torch.cat([r.model(tx["pos"][i:i + 1000], tx["dirs"][i:i + 1000])[1].float() for i in range(0, lay.n_texels, 1000)])
    assert torch.equal(m["texels"]["rgb"], direct)
    assert torch.equal(m["texture"], atlas_pack(direct, tx["owner"], lay))
    again = r.extract_mesh_textured(resolution=RES, threshold=thr, cell=5, color_chunk=1000)
    assert torch.equal(again["texture"], m["texture"])
    with pytest.raises(ValueError, match="extract_mesh_textured"):
        r.extract_mesh_textured(resolution=RES, source="views")
    with pytest.raises(ValueError, match="extract_mesh_textured"):
        r.extract_mesh_textured(resolution=RES, source="colours")


def test_views_source_on_both_geometries_and_the_field_fallback(scene):
    net, r, poses = scene
    ref = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, colors=False)
    a = r.extract_mesh_textured(resolution=RES, source="views", geometry="tsdf", **_views(poses))
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(a[k], ref[k]), k
    Tn = a["triangles"].shape[0]
    n_owned = int((a["texels"]["owner"] >= 0).sum())
    grey = int(a["n_grey"])
    print("triangles", Tn, "owned texels", n_owned, "grey", grey)
    assert Tn > 0 and 0 <= grey < n_owned and tuple(a["texture"].shape) == (a["layout"].S,) * 2 + (3,)
    # a constant frame: every texel is that constant or grey
    flat = torch.full((4, U.H, U.W, 3), 127, dtype=torch.uint8, device=DEV)
    flat[..., 1] = 40
    b = r.extract_mesh_textured(resolution=RES, source="views", geometry="tsdf", frames=flat, **_views(poses))
    rgb = N(b["texels"]["rgb"])[N(b["texels"]["owner"]) >= 0]
    one = np.array([np.float32(127) / np.float32(255), np.float32(40) / np.float32(255), np.float32(127) / np.float32(255)], np.float32)
    is_flat, is_grey = (np.abs(rgb - one) <= 1e-7).all(1), (rgb == 0.5).all(1)
    assert (is_flat | is_grey).all() and is_grey.sum() == int(b["n_grey"]) == grey and is_flat.any()
    # the fallback replaces exactly the grey texels, by the field's colour there
    c = r.extract_mesh_textured(resolution=RES, source="views", geometry="tsdf", frames=flat, fallback="field", **_views(poses))
    rgb_c = N(c["texels"]["rgb"])[N(c["texels"]["owner"]) >= 0]
    assert int(c["n_grey"]) == grey and np.array_equal(rgb_c[is_flat], rgb[is_flat])
    if grey:
        pos, dirs = (c["texels"][k][c["texels"]["owner"] >= 0][torch.from_numpy(is_grey).to(DEV)].contiguous() for k in ("pos", "dirs"))
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert np.array_equal(rgb_c[is_grey], N(r.model(pos, dirs)[1].float()))
    # the density's level set with the views' colours
    d = r.extract_mesh_textured(resolution=RES, threshold=r.threshold, source="views", geometry="density", **_views(poses))
    assert d["triangles"].shape[0] > 0 and d["texture"].shape[0] == d["layout"].S and r.model.training is False


def test_files_and_the_older_exports_keep_their_bytes(scene, tmp_path):
    from laenerf_amd.atlas import read_obj
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.trainer import Trainer
    net, r, poses = scene

    def older(tag):
        p = [str(tmp_path / f"{tag}_{k}.ply") for k in range(3)]
        r.save_mesh(p[0], resolution=RES, threshold=r.threshold)
        r.save_mesh(p[1], resolution=RES, threshold=r.threshold, normals=True, colors=True)
        r.save_mesh_tsdf(p[2], poses, INTR_R, U.H, U.W, resolution=RES)
        return [open(q, "rb").read() for q in p]
    before = older("before")
    a = str(tmp_path / "a.obj")
    v, t = r.save_mesh_textured(a, resolution=RES, threshold=r.threshold)
    m = r.extract_mesh_textured(resolution=RES, threshold=r.threshold)
    o = read_obj(a)
    Tn = m["triangles"].shape[0]
    assert Tn > 0 and o["triangles"].shape == (Tn, 3) and np.array_equal(o["triangles"], N(m["triangles"])) and np.array_equal(t, o["triangles"])
    assert np.array_equal(o["vertices"].astype(np.float32), N(m["vertices"])) and v.dtype == np.float64
    assert np.array_equal(o["normals"].astype(np.float32), N(m["normals"])) and np.abs(o["uv"] - N(m["uv"])).max() < 1e-11
    assert np.array_equal(o["texture"], N(m["texture"])) and o["mtllib"] == "a.mtl" and o["map_kd"] == "a.png"
    # the Trainer's method on the same cameras, no EMA kept: the same files
    img = np.full((4, U.H, U.W, 4), 255, np.uint8)
    data = ResidentImages.from_arrays(img, N(poses), INTR_R, device=DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    tr = Trainer(r, opt, data, 100, 1e-2, num_rays=1024, graph=False)
    b = str(tmp_path / "b.obj")
    tr.save_mesh_textured(b, resolution=RES, source="views", geometry="tsdf")
    c = str(tmp_path / "c.obj")
    r.save_mesh_textured(c, resolution=RES, source="views", geometry="tsdf", **_views(poses))
    ob, oc = read_obj(b), read_obj(c)
    assert ob["triangles"].shape[0] > 0 and np.array_equal(ob["triangles"], oc["triangles"]) and np.array_equal(ob["texture"], oc["texture"])
    assert open(b, "rb").read().replace(b"b.mtl", b"c.mtl") == open(c, "rb").read()
    # an empty mesh writes valid empty files
    e = str(tmp_path / "e.obj")
    v0, t0 = r.save_mesh_textured(e, resolution=RES, threshold=1e9)
    oe = read_obj(e)
    assert len(v0) == 0 and len(t0) == 0 and oe["vertices"].shape == (0, 3) and oe["triangles"].shape == (0, 3) and oe["texture"].shape == (8, 8, 3)
    assert older("after") == before
