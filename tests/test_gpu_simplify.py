"""simplify.simplify_mesh (csrc/simplify.hip) against simplify.simplify_numpy on the inputs of tests/simplify_util.py, and the
`simplify=` argument of the renderer's and the Trainer's export entry points on the small randomly initialised renderer of
tests/test_gpu_atlas.py.

The comparison.  Integers (vertex_map, triangles, V', T') are exact.  Positions, normals and colours are fp64 results rounded once
to fp32 on both sides; the two fp64 results differ by summation order only (test_simplify_cpu.py test_summation_order: below
1e-9 cell, measured 4e-14), so the rounded values differ by at most one fp32 spacing:
|got - want| <= spacing_fp32(|want|) + 1e-9 cell per component (+ 1e-9 for the unit normals and the colours).  Normals are compared
only where normal_margin = |N| / sum |n| >= 1e-6, and the test asserts that no cluster of these inputs falls below that."""
import numpy as np
import pytest
import torch

import simplify_util as SU
import tsdf_util as U
from gpu_util import DEV, N
from gpu_util import T as _T

pytestmark = pytest.mark.gpu
MARGIN = 1e-6


def T(a, dtype=None):
    return _T(np.ascontiguousarray(a), dtype)


def _device_args(name):
    m, kw = SU.arguments(name)
    kw = dict(kw)
    if "colors" in kw:
        kw["colors"] = T(kw["colors"])
    return T(m["verts"]), T(m["tris"]), kw


def _compare(got, want, cell, what):
    assert torch.is_tensor(got["vertices"]) and got["vertices"].is_cuda
    Vo, To = len(want["vertices"]), len(want["triangles"])
    assert tuple(got["vertices"].shape) == (Vo, 3) and tuple(got["triangles"].shape) == (To, 3) and tuple(got["normals"].shape) == (Vo, 3)
    assert got["vertices"].dtype == torch.float32 and got["triangles"].dtype == torch.int32 and got["vertex_map"].dtype == torch.int32
    assert np.array_equal(N(got["vertex_map"]), want["vertex_map"]), what
    assert np.array_equal(N(got["triangles"]), want["triangles"]), what
    differ = 0
    gv = N(got["vertices"]).astype(np.float64)
    tol = SU.spacing32(want["vertices"]) + 1e-9 * cell
    err = np.abs(gv - want["vertices"].astype(np.float64))
    differ += int((N(got["vertices"]) != want["vertices"]).sum())
    print(what, "V'", Vo, "T'", To, "positions: largest error / tolerance", float((err / tol).max()) if Vo else 0.0)
    assert (err <= tol).all(), what
    assert (want["normal_margin"] >= MARGIN).all(), "the guard below would hide clusters"     # 0 clusters below it on these inputs
    ok = want["normal_margin"] >= MARGIN
    gn = N(got["normals"])
    errn = np.abs(gn.astype(np.float64) - want["normals"].astype(np.float64))
    assert (errn[ok] <= SU.spacing32(want["normals"])[ok] + 1e-9).all(), what
    differ += int((gn != want["normals"])[ok].sum())
    if "colors" in want:
        gc = N(got["colors"])
        assert gc.shape == want["colors"].shape and (np.abs(gc.astype(np.float64) - want["colors"]) <= SU.spacing32(want["colors"]) + 1e-9).all()
        differ += int((gc != want["colors"]).sum())
    else:
        assert "colors" not in got
    print(what, "values not bit-identical:", differ, "of", gv.size + gn.size)


@pytest.mark.parametrize("name", sorted(SU.CASES))
def test_against_the_restatement(name):
    from laenerf_amd.simplify import simplify_mesh
    v, t, kw = _device_args(name)
    got = simplify_mesh(v, t, **kw)
    _compare(got, SU.want(name), float(np.float32(kw["cell"])), name)
    again = simplify_mesh(v, t, **kw)
    for k in got:
        assert torch.equal(got[k], again[k]), k                                  # two calls, the same bytes


@pytest.mark.parametrize("lanes", [1, 16, 64])
def test_lane_mappings(lanes):
    """every mapping of lanes to clusters passes the same comparison (they differ by summation order only)"""
    from laenerf_amd.simplify import simplify_mesh
    for name in ("random12_c2.5", "sphere24_c4", "hand"):
        v, t, kw = _device_args(name)
        got = simplify_mesh(v, t, lanes=lanes, **kw)
        _compare(got, SU.want(name), float(np.float32(kw["cell"])), f"{name} lanes {lanes}")
        assert torch.equal(got["vertices"], simplify_mesh(v, t, lanes=lanes, **kw)["vertices"])


def test_errors_and_empty_inputs():
    from laenerf_amd.simplify import simplify_mesh
    h = SU.hand()
    o = h["origin"]
    bad = h["verts"].copy()
    bad[4, 1] = np.nan
    for origin in (o, None):
        with pytest.raises(ValueError):
            simplify_mesh(T(bad), T(h["tris"]), SU.HAND_CELL, origin=origin)
    low = h["verts"].copy()
    low[5, 0] = -0.01
    with pytest.raises(ValueError):
        simplify_mesh(T(low), T(h["tris"]), SU.HAND_CELL, origin=o)
    with pytest.raises(ValueError):
        simplify_mesh(T(h["verts"]), T(h["tris"]), SU.HAND_CELL, origin=o, dims=(2, 2, 2))
    wrong = h["tris"].copy()
    wrong[2, 1] = 9
    with pytest.raises(ValueError):
        simplify_mesh(T(h["verts"]), T(wrong), SU.HAND_CELL, origin=o)
    with pytest.raises(ValueError):
        simplify_mesh(T(h["verts"]), T(h["tris"]), SU.HAND_CELL, origin=o, placement="median")
    # T = 0: the vertices alone; V = 0: nothing
    from laenerf_amd.simplify import simplify_numpy
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    e = simplify_mesh(T(h["verts"]), none, SU.HAND_CELL, origin=o, colors=T(h["colors"]))
    _compare(e, simplify_numpy(h["verts"], np.zeros((0, 3), np.int32), SU.HAND_CELL, origin=o, colors=h["colors"]), SU.HAND_CELL, "T = 0")
    assert e["triangles"].shape == (0, 3) and e["vertices"].shape == (7, 3)
    z = simplify_mesh(torch.zeros(0, 3, device=DEV), none, 1.0)
    assert z["vertices"].shape == (0, 3) and z["triangles"].shape == (0, 3) and z["normals"].shape == (0, 3) and z["vertex_map"].shape == (0,)
    assert z["vertices"].is_cuda and z["triangles"].dtype == torch.int32


# ---------------------------------------------------------------- the exports' simplify= on a renderer
RES = 32
INTR_R = (50.0, 50.0, 27.5, 20.25)
CELL = 2.5


@pytest.fixture(scope="module")
def scene():
    from laenerf_amd import synthetic as S
    from test_gpu_atlas import _threshold
    from test_gpu_frame import make
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0
    poses = _T(S.lookat_poses(4, radius=3.2, seed=4))
    r.threshold = _threshold(r)
    return net, r, poses


def test_attributes_equal_simplify_mesh_on_the_unsimplified_mesh(scene):
    from laenerf_amd.simplify import simplify_mesh
    net, r, poses = scene
    full = r.extract_mesh_attributes(resolution=RES, threshold=r.threshold, colors=False)
    cell, origin, dims = r.simplify_grid(RES, CELL)
    want = simplify_mesh(full["vertices"], full["triangles"], cell, origin=origin, dims=dims)
    got = r.extract_mesh_attributes(resolution=RES, threshold=r.threshold, simplify=CELL, color_chunk=100)
    print("V", full["vertices"].shape[0], "->", got["vertices"].shape[0], "T", full["triangles"].shape[0], "->", got["triangles"].shape[0])
    assert 0 < got["triangles"].shape[0] < full["triangles"].shape[0]
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(got[k], want[k]), k
    dirs = torch.where((want["normals"] == 0).all(1, keepdim=True), torch.tensor([0.0, 0.0, 1.0], device=DEV), -want["normals"]).contiguous()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        direct = torch.cat([r.model(want["vertices"][i:i + 100], dirs[i:i + 100])[1].float() for i in range(0, dirs.shape[0], 100)])
    assert torch.equal(got["colors"], direct)
    v, t = r.extract_mesh(resolution=RES, threshold=r.threshold, simplify=CELL)
    assert v.dtype == np.float64 and np.array_equal(v, N(want["vertices"]).astype(np.float64)) and np.array_equal(t, N(want["triangles"]))


def test_saved_files_hold_the_simplified_mesh(scene, tmp_path):
    from laenerf_amd.atlas import read_obj
    from laenerf_amd.mesh import read_ply
    net, r, poses = scene
    views = dict(poses=poses, intrinsics=INTR_R, H=U.H, W=U.W)
    full = {"density": r.extract_mesh(resolution=RES, threshold=r.threshold)[1].shape[0],
            "tsdf": r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, colors=False)["triangles"].shape[0]}
    p = [str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply", "d.obj")]
    out = [r.save_mesh(p[0], resolution=RES, threshold=r.threshold, simplify=CELL),
           r.save_mesh(p[1], resolution=RES, threshold=r.threshold, normals=True, colors=True, simplify=CELL),
           r.save_mesh_tsdf(p[2], poses, INTR_R, U.H, U.W, resolution=RES, simplify=CELL),
           r.save_mesh_textured(p[3], resolution=RES, threshold=r.threshold, simplify=CELL)]
    for path, (v, t), kind in zip(p, out, ("density", "density", "tsdf", "density")):
        f = read_obj(path) if path.endswith(".obj") else read_ply(path)
        print(path.rsplit("/", 1)[1], "V'", len(v), "T'", len(t), "of", full[kind])
        assert v.dtype == np.float64 and f["vertices"].shape == (len(v), 3) and f["triangles"].shape == (len(t), 3)
        assert 0 < len(t) < full[kind] and np.array_equal(f["triangles"], t)
        assert np.array_equal(np.asarray(f["vertices"], np.float32), v.astype(np.float32)) and np.array_equal(v, v.astype(np.float32).astype(np.float64))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[3][1])
    assert "colors" in read_ply(p[1]) and "colors" in read_ply(p[2]) and "normals" in read_ply(p[2])
    # TSDF colours: the member means of the fused vertex colours; n_grey counts before simplification
    a = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES)
    b = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, simplify=CELL)
    from laenerf_amd.simplify import simplify_mesh
    cell, origin, dims = r.simplify_grid(RES, CELL)
    s = simplify_mesh(a["vertices"], a["triangles"], cell, origin=origin, dims=dims, colors=a["colors"])
    assert torch.equal(b["colors"], s["colors"]) and torch.equal(b["vertices"], s["vertices"]) and int(b["n_grey"]) == int(a["n_grey"])
    assert b["colors"].shape[0] == b["vertices"].shape[0] < a["vertices"].shape[0]


def test_textured_layout_gets_larger_cells(scene):
    net, r, poses = scene
    S = 1024                                         # 66 261 triangles are 183 cells a row: cells of 5 texels; a tenth of them: 18
    a = r.extract_mesh_textured(resolution=RES, threshold=r.threshold, texture_size=S)
    b = r.extract_mesh_textured(resolution=RES, threshold=r.threshold, texture_size=S, simplify=CELL)
    print("layout cell", a["layout"].cell, "->", b["layout"].cell, "T", a["layout"].T, "->", b["layout"].T)
    assert b["layout"].cell >= a["layout"].cell and 0 < b["layout"].T < a["layout"].T
    assert b["uv"].shape[0] == b["triangles"].shape[0] == b["layout"].T and b["texture"].shape[0] <= S
    g = r.extract_mesh_textured(resolution=RES, source="views", geometry="tsdf", simplify=CELL, poses=poses, intrinsics=INTR_R, H=U.H, W=U.W)
    assert g["triangles"].shape[0] > 0 and g["vertices"].shape[0] == g["normals"].shape[0]


def test_none_changes_no_byte(scene, tmp_path):
    """simplify=None against a call that omits the argument, entry point by entry point"""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.trainer import Trainer
    net, r, poses = scene
    kw = dict(resolution=RES, threshold=r.threshold)
    views = dict(poses=poses, intrinsics=INTR_R, H=U.H, W=U.W)

    def same(a, b):
        if isinstance(a, dict):
            assert a.keys() == b.keys()
            return all(same(a[k], b[k]) for k in a)
        if isinstance(a, (tuple, list)):
            return all(same(x, y) for x, y in zip(a, b))
        if torch.is_tensor(a):
            return a.dtype == b.dtype and torch.equal(a, b)
        if isinstance(a, np.ndarray):
            return a.dtype == b.dtype and np.array_equal(a, b)
        return a == b or a is b or type(a) is type(b)

    assert same(r.extract_mesh(**kw), r.extract_mesh(simplify=None, **kw))
    assert same(r.extract_mesh_attributes(**kw), r.extract_mesh_attributes(simplify=None, **kw))
    assert same(r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES), r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, simplify=None))
    ta, tb = r.extract_mesh_textured(**kw), r.extract_mesh_textured(simplify=None, **kw)
    for k in ("vertices", "triangles", "normals", "uv", "texture", "n_grey"):
        assert torch.equal(ta[k], tb[k]), k
    files = []
    for tag, extra in (("a", {}), ("b", {"simplify": None})):
        p = [str(tmp_path / f"{tag}{i}") for i in range(4)]
        r.save_mesh(p[0] + ".ply", **kw, **extra)
        r.save_mesh(p[1] + ".ply", normals=True, colors=True, **kw, **extra)
        r.save_mesh_tsdf(p[2] + ".ply", poses, INTR_R, U.H, U.W, resolution=RES, **extra)
        r.save_mesh_textured(p[3] + ".obj", **kw, **extra)
        files.append([open(q, "rb").read() for q in (p[0] + ".ply", p[1] + ".ply", p[2] + ".ply", p[3] + ".png")]
                     + [open(p[3] + ".obj", "rb").read().replace(tag.encode() + b"3.mtl", b"x3.mtl")])
    assert files[0] == files[1]
    # the Trainer's three methods forward the argument
    img = np.full((4, U.H, U.W, 4), 255, np.uint8)
    data = ResidentImages.from_arrays(img, N(poses), INTR_R, device=DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    tr = Trainer(r, opt, data, 100, 1e-2, num_rays=1024, graph=False)
    full = tr.save_mesh(str(tmp_path / "t0.ply"), **kw)[1].shape[0]
    for i, (fn, args) in enumerate(((tr.save_mesh, kw), (tr.save_mesh, dict(normals=True, **kw)), (tr.save_mesh_tsdf, dict(resolution=RES)),
                                    (tr.save_mesh_textured, kw))):
        v, t = fn(str(tmp_path / f"t{i + 1}") + (".obj" if fn == tr.save_mesh_textured else ".ply"), simplify=CELL, **args)
        assert 0 < len(t) and (fn == tr.save_mesh_tsdf or len(t) < full) and np.array_equal(v, v.astype(np.float32).astype(np.float64))
