"""The component rule and `simplify` TOGETHER through every export entry point of NeRFRenderer (laenerf_amd/export.py), bit for bit
against the public operators composed by hand: the order of the pipeline's steps -- floaters out of the field, marching cubes,
positions from the UNFILTERED field, simplification, then the colours -- and the field each step reads."""
import numpy as np
import pytest
import torch

import tsdf_util as U
from gpu_util import DEV, N
from gpu_util import T as _T

pytestmark = pytest.mark.gpu
CELL = 2.5
CHUNK = 100                                                            # the colour loop runs many chunks
RULE = dict(keep_largest=True, simplify=CELL)


def _simplify_by_hand(r, R, pos, tris, colors=None):
    from laenerf_amd.simplify import simplify_mesh
    cell, origin, dims = r.simplify_grid(R, CELL)
    return simplify_mesh(pos, tris, cell, origin=origin, dims=dims, colors=colors)


def test_density_entry_points_equal_the_operators_composed_by_hand(tmp_path):
    """the scene of test_save_mesh_without_floaters_and_the_default_path: more than one component at the 0.7 quantile of R = 64"""
    from laenerf_amd import components, mesh
    from test_gpu_components import _network
    r = _network()
    R = 64
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return r.model.density(pts)["sigma"]

    with torch.no_grad():
        u = mesh.extract_fields(bmin, bmax, R, query, device=DEV)
        thr = float(np.quantile(u.cpu().numpy(), 0.7))
        f, info = components.filter_components(u, thr, largest=True, info=True)
        vi, ti = mesh.marching_cubes(f, thr)
        pos = mesh.vertex_attributes(u, vi, bmin, bmax, want=("pos",))["pos"]         # from the unfiltered field
        s = _simplify_by_hand(r, R, pos, ti)
        dirs = torch.where((s["normals"] == 0).all(1, keepdim=True), torch.tensor([0.0, 0.0, 1.0], device=DEV), -s["normals"]).contiguous()
        with torch.autocast("cuda", dtype=torch.float16):
            rgb = torch.cat([r.model(s["vertices"][i:i + CHUNK], dirs[i:i + CHUNK])[1].float() for i in range(0, dirs.shape[0], CHUNK)])
        T_all = mesh.marching_cubes(u, thr)[1].shape[0]
    T_kept, T_s, V_s = ti.shape[0], s["triangles"].shape[0], s["vertices"].shape[0]
    print("components", info["n_components"], "removed", info["n_removed"], "T", T_all, "->", T_kept, "->", T_s, "V'", V_s, "chunks", -(-V_s // CHUNK))
    assert info["n_removed"] >= 1 and 0 < T_s < T_kept < T_all and V_s > 3 * CHUNK
    want_v, want_t = N(s["vertices"]).astype(np.float64), N(s["triangles"])
    kw = dict(resolution=R, threshold=thr, **RULE)

    v, t = r.extract_mesh(**kw)
    assert v.dtype == np.float64 and t.dtype == np.int32 and np.array_equal(v, want_v) and np.array_equal(t, want_t)

    m = r.extract_mesh_attributes(color_chunk=CHUNK, **kw)
    assert set(m) == {"vertices", "triangles", "normals", "colors"}
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(m[k], s[k]), k
    assert torch.equal(m["colors"], rgb)
    bare = r.extract_mesh_attributes(normals=False, colors=False, **kw)
    assert set(bare) == {"vertices", "triangles"} and torch.equal(bare["vertices"], s["vertices"]) and torch.equal(bare["triangles"], s["triangles"])
    only_colors = r.extract_mesh_attributes(normals=False, color_chunk=CHUNK, **kw)
    assert set(only_colors) == {"vertices", "triangles", "colors"} and torch.equal(only_colors["colors"], rgb)

    plain, full = str(tmp_path / "plain.ply"), str(tmp_path / "full.ply")
    v, t = r.save_mesh(plain, **kw)
    ply = mesh.read_ply(plain)
    assert np.array_equal(v, want_v) and np.array_equal(t, want_t)
    assert np.array_equal(ply["vertices"], N(s["vertices"])) and np.array_equal(ply["triangles"], want_t)
    assert "normals" not in ply and "colors" not in ply
    v, t = r.save_mesh(full, normals=True, colors=True, color_chunk=CHUNK, **kw)
    ply = mesh.read_ply(full)
    assert np.array_equal(v, want_v) and np.array_equal(t, want_t)
    assert np.array_equal(ply["vertices"], N(s["vertices"])) and np.array_equal(ply["triangles"], want_t)
    assert np.array_equal(ply["normals"], N(s["normals"])) and np.array_equal(ply["colors"], mesh.color_bytes_numpy(N(rgb)))

    # textured: the same geometry under the same rule and simplify
    tex = r.extract_mesh_textured(geometry="density", color_chunk=CHUNK * 100, **kw)
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(tex[k], m[k]), k
    assert tex["layout"].T == T_s and tex["uv"].shape[0] == T_s and int(tex["n_grey"]) == 0
    assert r.model.training is False


def test_tsdf_entry_points_equal_the_operators_composed_by_hand(tmp_path, monkeypatch):
    """the scene of tests/test_gpu_tsdf.py (four views of the small renderer) with that file's planted blob, so that the component
    rule has something to drop from the fused field"""
    import torch.nn.functional as F
    from laenerf_amd import mesh, tsdf
    from laenerf_amd import synthetic as S
    from test_gpu_frame import make
    from test_gpu_tsdf import INTR_R, RES
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0
    poses = _T(S.lookat_poses(4, radius=3.2, seed=4))
    real = tsdf.tsdf_fuse

    def planted(*a, **kw):
        out = real(*a, **kw)
        empty = F.avg_pool3d((out["u"] < 0).float()[None, None], 5, stride=1)[0, 0] == 1      # 5^3 windows of empty space
        i, j, k = (int(x) for x in empty.nonzero()[0])
        out["u"][i + 1:i + 4, j + 1:j + 4, k + 1:k + 4] = 1.0         # a 3^3 blob with empty space all around it
        return out
    monkeypatch.setattr(tsdf, "tsdf_fuse", planted)

    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()
    axes = mesh.lattice(bmin, bmax, RES)
    trunc = 3.0 * max(float(a[1] - a[0]) for a in axes)
    packed, frames = tsdf.render_packed_views(r, poses, INTR_R, U.H, U.W, return_frames=True)
    fused = tsdf.tsdf_fuse(packed, poses, INTR_R, U.H, U.W, axes, trunc, frames=frames, min_views=1)
    vi, ti = mesh.marching_cubes(mesh.drop_components(fused["u"], 0.0, keep_largest=True), 0.0)
    pos = mesh.vertex_attributes(fused["u"], vi, bmin, bmax, want=("pos",))["pos"]
    colors, n_grey = tsdf.tsdf_vertex_colors(fused["rgb"], fused["counts"], vi)
    s = _simplify_by_hand(r, RES, pos, ti, colors=colors)
    T_all = mesh.marching_cubes(fused["u"], 0.0)[1].shape[0]
    T_kept, T_s = ti.shape[0], s["triangles"].shape[0]
    print("T", T_all, "->", T_kept, "->", T_s, "grey", n_grey)
    assert 0 < T_s < T_kept < T_all

    unsimplified = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, keep_largest=True)
    assert torch.equal(unsimplified["triangles"], ti) and torch.equal(unsimplified["colors"], colors)
    m = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, **RULE)
    assert set(m) == {"vertices", "triangles", "normals", "colors", "n_grey"}
    for k in ("vertices", "triangles", "normals", "colors"):
        assert torch.equal(m[k], s[k]), k
    assert m["n_grey"] == unsimplified["n_grey"] == n_grey
    bare = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, normals=False, colors=False, **RULE)
    assert set(bare) == {"vertices", "triangles"} and torch.equal(bare["vertices"], s["vertices"]) and torch.equal(bare["triangles"], s["triangles"])

    path = str(tmp_path / "t.ply")
    v, t = r.save_mesh_tsdf(path, poses, INTR_R, U.H, U.W, resolution=RES, **RULE)
    ply = mesh.read_ply(path)
    assert v.dtype == np.float64 and np.array_equal(v, N(s["vertices"]).astype(np.float64)) and np.array_equal(t, N(s["triangles"]))
    assert np.array_equal(ply["vertices"], N(s["vertices"])) and np.array_equal(ply["triangles"], N(s["triangles"]))
    assert np.array_equal(ply["normals"], N(s["normals"])) and np.array_equal(ply["colors"], mesh.color_bytes_numpy(N(s["colors"])))
    assert r.model.training is False
