"""lae_tsdf_fuse / lae_tsdf_vertex_colors (through tsdf.tsdf_fuse / tsdf_vertex_colors) against the restatement tsdf.tsdf_numpy on
the scene of tests/tsdf_util.py, and NeRFRenderer.extract_mesh_tsdf / save_mesh_tsdf / Trainer.save_mesh_tsdf on a small randomly
initialised renderer.

What is compared, and how closely (tests/test_tsdf_cpu.py asserts the figures on the CPU, for these very inputs):
  float32   counts equal on every voxel; u and rgb bit for bit against tsdf_numpy(dtype=float32), which writes the kernel's
            statements in their order; the vertex colours bit for bit against tsdf_vertex_colors_numpy(dtype=float32).
  float64   a (voxel, view) pair is compared wherever its margin -- the distance of its nearest decision from the threshold -- is
            at least eps = 1e-4: counts equal on every voxel without a pair inside that band, u within 2e-5 there (derived in
            tsdf_util.U_TOL; measured 1.4e-6).  The pairs inside the band may be at most 0.5 % of all, the voxels with such a
            pair at most 5 % (measured 0.04 % and 0.8 - 2.3 %): an exclusion band, not a tolerance.
  cull      the same bytes with LAE_TSDF_CULL=0, and from two calls; one camera stands 0.62 from the centre, so whole bricks are
            behind it or outside its frame.
  scene     properties that need no restatement: the mesh is closed, has Euler characteristic 2, every vertex lies within 0.75
            voxel sides of the sphere, and its colour within tsdf_util.COLOR_TOL of 0.5 + 0.5 X / 0.45."""
import numpy as np
import pytest
import torch

import tsdf_util as U
from gpu_util import DEV, N
from gpu_util import T as _T

pytestmark = pytest.mark.gpu


def T(a):
    return _T(np.array(a))                                           # the fixtures are read-only: hand torch a copy


def _fuse(V, shape, close, frames=True, **kw):
    from laenerf_amd.tsdf import tsdf_fuse
    f = U.fixture(V, close)
    ax = [torch.from_numpy(a) for a in U.axes(shape)]                # host tensors, as mesh.lattice returns them
    return tsdf_fuse(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, ax, U.trunc(shape), frames=T(f["frames"]) if frames else None,
                     counts=True, **kw)


@pytest.fixture(scope="module")
def fused():
    """case -> tsdf_fuse's dict of device tensors, one launch per case"""
    return {case: _fuse(*case) for case in U.GPU_CASES}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("case", U.GPU_CASES)
def test_bit_for_bit_against_the_float32_restatement(fused, case):
    V, shape, close = case
    r = U.restated(V, shape, "float32", close=close)
    g = fused[case]
    print("mismatches: counts", (N(g["counts"]) != r["counts"]).sum(), "u", (_bits(N(g["u"])) != _bits(r["u"])).sum(), "rgb",
          (_bits(N(g["rgb"])) != _bits(r["rgb"])).sum())
    assert np.array_equal(N(g["counts"]), r["counts"])
    assert np.array_equal(_bits(N(g["u"])), _bits(r["u"])) and np.array_equal(_bits(N(g["rgb"])), _bits(r["rgb"]))
    assert N(g["counts"])[..., 0].max() > 0 and N(g["counts"])[..., 2].max() > 0


@pytest.mark.parametrize("case", U.GPU_CASES)
def test_counts_and_field_against_float64(fused, case):
    V, shape, close = case
    r = U.restated(V, shape, close=close)
    _, in_band = U.band(r)
    ok = ~in_band
    g = fused[case]
    assert np.array_equal(N(g["counts"]).reshape(-1, 4)[ok], r["counts"].reshape(-1, 4)[ok])
    du = np.abs(N(g["u"]).astype(np.float64) - r["u"]).reshape(-1)[ok].max()
    print("max |u - u64| outside the band", du)
    assert du <= U.U_TOL
    drgb = np.abs(N(g["rgb"]).astype(np.float64) - r["rgb"]).reshape(-1, 3)[ok].max()
    print("max |rgb - rgb64| outside the band", drgb)
    assert drgb <= 1e-6                                              # two fp32 divisions of exact integers: 2 * 2^-24 of at most 1


def test_cull_switch_two_calls_and_the_output_flavours(fused, monkeypatch):
    case = U.GPU_CASES[2]
    assert case[2]                                                   # the case with the close camera
    g = fused[case]
    again = _fuse(*case)
    monkeypatch.setenv("LAE_TSDF_CULL", "0")
    plain = _fuse(*case)
    monkeypatch.delenv("LAE_TSDF_CULL")
    for k in ("u", "counts", "rgb"):
        assert torch.equal(g[k], again[k]) and torch.equal(g[k], plain[k]), k
    # without frames: the same field and counts, no colours; fp32 frames go through lae_eval_view's byte rule
    from laenerf_amd.mesh import color_bytes_numpy
    from laenerf_amd.tsdf import tsdf_fuse
    bare = _fuse(*case, frames=False)
    assert bare["rgb"] is None and torch.equal(bare["u"], g["u"]) and torch.equal(bare["counts"], g["counts"])
    f = U.fixture(case[0], case[2])
    rng = np.random.default_rng(3)
    ff = rng.uniform(-0.2, 1.2, f["frames"].shape).astype(np.float32)
    ax = [torch.from_numpy(a) for a in U.axes(case[1])]
    a = tsdf_fuse(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, ax, U.trunc(case[1]), frames=T(ff))
    b = tsdf_fuse(T(f["packed"]), T(f["poses"]), U.INTRINSICS, U.H, U.W, ax, U.trunc(case[1]), frames=T(color_bytes_numpy(ff)))
    assert torch.equal(a["rgb"], b["rgb"]) and a["counts"] is not None


@pytest.mark.parametrize("case", U.GPU_CASES[:2])
def test_vertex_colours_and_the_mesh_of_the_fused_field(fused, case):
    from laenerf_amd.mesh import marching_cubes
    from laenerf_amd.tsdf import tsdf_vertex_colors, tsdf_vertex_colors_numpy
    V, shape, close = case
    g = fused[case]
    verts, tris = marching_cubes(g["u"], 0.0)
    col, n_grey = tsdf_vertex_colors(g["rgb"], g["counts"], verts)
    want, want_grey = tsdf_vertex_colors_numpy(N(g["rgb"]), N(g["counts"]), N(verts), dtype=np.float32)
    assert np.array_equal(_bits(N(col)), _bits(want)) and n_grey == want_grey == 0
    m = U.mesh_report(N(verts), N(tris), shape)
    err = np.abs(N(col) - (0.5 + 0.5 * m["X"] / U.RADIUS)).max()
    print("vertices", len(verts), "euler", m["euler"], "off", m["off"], "colour error", err)
    assert m["closed"] and m["euler"] == 2 and m["off"] <= U.SIDE_TOL and err <= U.COLOR_TOL


def test_vertex_colour_cases_by_hand():
    from laenerf_amd.tsdf import tsdf_vertex_colors, tsdf_vertex_colors_numpy
    rgb = np.zeros((2, 3, 2, 3), np.float32)
    counts = np.zeros((2, 3, 2, 4), np.uint16)
    rgb[0, 0, 0], rgb[1, 0, 0], rgb[0, 1, 0] = (0.2, 0.4, 0.6), (1.0, 0.0, 0.5), (0.9, 0.8, 0.7)
    rgb[1, 1, 0] = (0.1, 0.3, 0.8)
    counts[0, 0, 0, 0], counts[1, 0, 0, 0], counts[1, 1, 0, 0] = 3, 1, 2     # (0, 1, 0) holds a colour but no near view
    # both / one (the lower end) / neither / on a lattice point / one (the upper end) / neither, 300 times: more than one workgroup
    verts = np.array([[0.25, 0, 0], [0, 0.5, 0], [0, 1, 0.5], [0, 0, 0], [0.5, 1, 0]] + [[0, 2, 0.5]] * 300, np.float32)
    col, n_grey = tsdf_vertex_colors(T(rgb), T(counts), T(verts))
    want, want_grey = tsdf_vertex_colors_numpy(rgb, counts, verts, dtype=np.float32)
    assert n_grey == want_grey == 301 and np.array_equal(_bits(N(col)), _bits(want))
    assert np.allclose(N(col)[:5], [[0.4, 0.3, 0.575], [0.2, 0.4, 0.6], [0.5, 0.5, 0.5], [0.2, 0.4, 0.6], [0.1, 0.3, 0.8]], atol=1e-6)
    empty, none = tsdf_vertex_colors(T(rgb), T(counts), torch.empty(0, 3, device=DEV))
    assert tuple(empty.shape) == (0, 3) and none == 0


def test_special_values_in_one_small_launch():
    from laenerf_amd.tsdf import tsdf_fuse, tsdf_numpy
    f = U.fixture(24)
    use = [0, 7, 13]
    pk = np.array(f["packed"][use])
    pk[0, ::2] = -pk[0, ::2]                                         # the sign bit is ignored
    pk[0, 5, :8], pk[0, 6, :8], pk[0, 20:24, 20:30] = -0.0, np.nan, 0.3     # zero and a wall in front of the lattice
    pk[1] = np.inf                                                   # a transparent view
    pk[2, :, ::3] = np.nan                                           # no observation
    pk[2, :, 1::3] = -np.inf
    po, fr = np.array(f["poses"][use]), np.array(f["frames"][use])
    ax, tr = U.axes(8), U.trunc(8)
    for mv in (1, 2):
        g = tsdf_fuse(T(pk), T(po), U.INTRINSICS, U.H, U.W, [torch.from_numpy(a) for a in ax], tr, frames=T(fr), min_views=mv)
        r = tsdf_numpy(pk, po, U.INTRINSICS, U.H, U.W, ax, tr, frames=fr, min_views=mv, dtype=np.float32)
        assert np.array_equal(N(g["counts"]), r["counts"]), mv
        assert np.array_equal(_bits(N(g["u"])), _bits(r["u"])) and np.array_equal(_bits(N(g["rgb"])), _bits(r["rgb"])), mv
        c = r["counts"].reshape(-1, 4)
        assert (c[:, 1] > 0).any() and (c[:, 2] > 0).any() and not np.isnan(r["u"]).any()
    # a view of all +inf alone: u = -1 everywhere, no vertex
    from laenerf_amd.mesh import marching_cubes
    g = tsdf_fuse(T(pk[1:2]), T(po[1:2]), U.INTRINSICS, U.H, U.W, [torch.from_numpy(a) for a in ax], tr, counts=True)
    assert (N(g["u"]) == -1.0).all() and N(g["counts"])[..., 1].max() == 1 and g["rgb"] is None
    verts, tris = marching_cubes(g["u"], 0.0)
    assert verts.shape[0] == 0 and tris.shape[0] == 0


def test_invalid_arguments_leave_the_outputs_untouched():
    from laenerf_amd import _lib
    from laenerf_amd.tsdf import tsdf_fuse, tsdf_vertex_colors
    f = U.fixture(24)
    lib = _lib.load()
    V, n = 24, 8
    packed, poses, frames = T(f["packed"]), T(f["poses"]), T(f["frames"])
    ax = [T(a) for a in U.axes(n)]
    u = torch.full((n, n, n), 7.0, device=DEV)
    counts = torch.full((n, n, n, 4), 0x7777, dtype=torch.uint16, device=DEV)
    rgb = torch.full((n, n, n, 3), 7.0, device=DEV)
    fx, fy, cx, cy = U.INTRINSICS

    def fuse(p=packed.data_ptr(), po=poses.data_ptr(), v=V, fx=fx, fy=fy, h=U.H, w=U.W, xs=ax[0].data_ptr(), ys=ax[1].data_ptr(),
             zs=ax[2].data_ptr(), nn=(n, n, n), fr=frames.data_ptr(), tr=0.3, mv=1, out=u.data_ptr(), c=counts.data_ptr(), col=rgb.data_ptr()):
        return lib.lae_tsdf_fuse(p, po, v, fx, fy, cx, cy, h, w, xs, ys, zs, nn[0], nn[1], nn[2], fr, tr, mv, out, c, col, None)
    for kw in (dict(p=None), dict(po=None), dict(xs=None), dict(ys=None), dict(zs=None), dict(out=None), dict(fr=None)):
        assert fuse(**kw) == -3, kw
    for kw in (dict(v=0), dict(v=65536), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15), dict(nn=(1, n, n)), dict(nn=(n, n, 513)), dict(tr=0.0),
               dict(tr=-0.3), dict(tr=float("nan")), dict(fx=0.0), dict(fy=-2.0), dict(mv=0), dict(c=counts.data_ptr() + 4)):
        assert fuse(**kw) == -1, kw
    verts = torch.zeros(4, 3, device=DEV)
    col = torch.full((4, 3), 7.0, device=DEV)
    vc = lambda r=rgb.data_ptr(), c=counts.data_ptr(), nn=(n, n, n), v=verts.data_ptr(), out=col.data_ptr(): \
        lib.lae_tsdf_vertex_colors(r, c, nn[0], nn[1], nn[2], v, 4, out, None, None)
    assert vc(r=None) == -3 and vc(c=None) == -3 and vc(v=None) == -3 and vc(out=None) == -3 and vc(nn=(n, 1, n)) == -1 and vc(nn=(600, n, n)) == -1
    torch.cuda.synchronize()
    assert (N(u) == 7.0).all() and (N(counts) == 0x7777).all() and (N(rgb) == 7.0).all() and (N(col) == 7.0).all()
    # and the Python operators refuse what the entry points would misread
    tr = U.trunc(n)
    host = [torch.from_numpy(a) for a in U.axes(n)]
    for bad in (dict(packed=packed.double()), dict(poses=poses[:-1].contiguous()), dict(axes=host[:2]), dict(axes=[a.double() for a in host]),
                dict(trunc=0.0), dict(min_views=0), dict(frames=frames[:-1]), dict(frames=frames.to(torch.float16)), dict(intrinsics=(1.0, 2.0))):
        kw = dict(packed=packed, poses=poses, intrinsics=U.INTRINSICS, H=U.H, W=U.W, axes=host, trunc=tr)
        kw.update(bad)
        with pytest.raises(ValueError, match="tsdf_fuse"):
            tsdf_fuse(**kw)
    with pytest.raises(RuntimeError):
        tsdf_fuse(packed.cpu(), poses, U.INTRINSICS, U.H, U.W, host, tr)
    with pytest.raises(ValueError, match="tsdf_vertex_colors"):
        tsdf_vertex_colors(rgb, counts[..., :3].contiguous(), verts)
    with pytest.raises(ValueError, match="tsdf_vertex_colors"):
        tsdf_vertex_colors(rgb, counts, verts.double())
    assert fuse() == 0                                               # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert not (N(u) == 7.0).any() and not (N(counts)[..., :3] == 0x7777).any() and not (N(rgb) == 7.0).any()


# ---------------------------------------------------------------- extract_mesh_tsdf / save_mesh_tsdf on a renderer
RES = 32
INTR_R = (50.0, 50.0, 27.5, 20.25)


@pytest.fixture(scope="module")
def scene():
    """the small randomly initialised renderer of tests/test_gpu_mask_lift.py (the sphere preset as its occupancy, opaque
    surfaces), four cameras, and the mesh extract_mesh_tsdf makes of them"""
    from laenerf_amd import synthetic as S
    from test_gpu_frame import make
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0
    poses = T(S.lookat_poses(4, radius=3.2, seed=4))
    m = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES)
    return net, r, poses, m


def test_extract_mesh_tsdf_is_a_valid_mesh_and_repeats(scene):
    net, r, poses, m = scene
    V, Tn = m["vertices"].shape[0], m["triangles"].shape[0]
    print("vertices", V, "triangles", Tn, "grey", m["n_grey"])
    assert V > 0 and Tn > 0 and int(m["triangles"].min()) >= 0 and int(m["triangles"].max()) < V
    length = N(m["normals"]).astype(np.float64)
    length = np.sqrt((length * length).sum(1))
    assert (np.abs(length - 1) < 1e-5)[length > 0].all() and (length > 0).any()
    col = N(m["colors"])
    assert col.shape == (V, 3) and col.min() >= 0 and col.max() <= 1 + 1e-6 and 0 <= m["n_grey"] < V
    lo, hi = N(r.aabb_infer[:3]), N(r.aabb_infer[3:])
    assert (N(m["vertices"]) >= lo - 1e-6).all() and (N(m["vertices"]) <= hi + 1e-6).all()
    again = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES)
    for k in ("vertices", "triangles", "normals", "colors"):
        assert torch.equal(m[k], again[k]), k
    assert r.model.training is False and "index_vertices" not in m
    bare = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, normals=False, colors=False)
    assert set(bare) == {"vertices", "triangles"} and torch.equal(bare["vertices"], m["vertices"])


def test_frames_change_the_colours_only(scene):
    net, r, poses, m = scene
    grey = torch.full((4, U.H, U.W, 3), 127, dtype=torch.uint8, device=DEV)
    grey[..., 1] = 40
    g = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, frames=grey)
    for k in ("vertices", "triangles", "normals"):
        assert torch.equal(m[k], g[k]), k
    assert not torch.equal(m["colors"], g["colors"])
    col = N(g["colors"])
    one = (np.float32(127) / np.float32(255), np.float32(40) / np.float32(255), np.float32(127) / np.float32(255))
    flat = (np.abs(col - np.array(one, np.float32)) <= 1e-7).all(1) | (col == 0.5).all(1)     # the constant, or no view coloured it
    assert flat.all() and g["n_grey"] == m["n_grey"] == int((col == 0.5).all(1).sum())
    # fp32 frames go through the byte rule: 0.5 -> 127
    half = torch.full((4, U.H, U.W, 3), 0.5, device=DEV)
    half[..., 1] = 40.5 / 255
    h = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, frames=half)
    assert torch.equal(h["colors"], g["colors"])
    # given depths bypass the geometry render
    from laenerf_amd.tsdf import render_packed_views
    far = [torch.full((U.H * U.W,), 9.0, device=DEV)] * 4
    ones = torch.ones(4, U.H * U.W, device=DEV)
    plane = render_packed_views(r, poses, INTR_R, U.H, U.W, depths=far, opacities=ones)
    assert plane.shape == (4, U.H, U.W) and (plane == 9.0).all()
    empty = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, depths=far, opacities=ones, colors=False)
    assert empty["vertices"].shape[0] == 0 and empty["triangles"].shape[0] == 0      # every seen voxel is free
    with pytest.raises(ValueError, match="render_packed_views"):
        render_packed_views(r, poses, INTR_R, U.H, U.W, depths=far)


def test_save_mesh_tsdf_round_trips_and_the_trainer_writes_the_same_file(scene, tmp_path):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.mesh import color_bytes_numpy, read_ply
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.trainer import Trainer
    net, r, poses, m = scene
    a = str(tmp_path / "a.ply")
    v, t = r.save_mesh_tsdf(a, poses, INTR_R, U.H, U.W, resolution=RES)
    ply = read_ply(a)
    assert np.array_equal(ply["vertices"], N(m["vertices"])) and np.array_equal(ply["triangles"], N(m["triangles"]))
    assert np.array_equal(ply["normals"], N(m["normals"])) and np.array_equal(ply["colors"], color_bytes_numpy(N(m["colors"])))
    assert v.dtype == np.float64 and np.allclose(v, N(m["vertices"]), atol=1e-6) and np.array_equal(t, N(m["triangles"]))
    # the Trainer's method on the same cameras, no EMA kept: the same bytes
    img = np.full((4, U.H, U.W, 4), 255, np.uint8)
    data = ResidentImages.from_arrays(img, N(poses), INTR_R, device=DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    tr = Trainer(r, opt, data, 100, 1e-2, num_rays=1024, graph=False)
    assert tr.ema is None
    b = str(tmp_path / "b.ply")
    tr.save_mesh_tsdf(b, resolution=RES)
    assert open(a, "rb").read() == open(b, "rb").read()
    # an empty result is a valid PLY with zero elements
    c = str(tmp_path / "c.ply")
    far = torch.full((4, U.H * U.W), 9.0, device=DEV)
    v0, t0 = r.save_mesh_tsdf(c, poses, INTR_R, U.H, U.W, resolution=RES, depths=far, opacities=torch.ones_like(far))
    ply = read_ply(c)
    assert len(v0) == 0 and len(t0) == 0 and ply["vertices"].shape == (0, 3) and ply["triangles"].shape == (0, 3) and ply["colors"].shape == (0, 3)


def test_keep_largest_drops_a_planted_blob(scene, monkeypatch):
    """a second solid blob planted into the fused field (what the fill rule leaves of a region seen only as occluded)"""
    from laenerf_amd import tsdf
    import torch.nn.functional as F
    net, r, poses, m = scene
    base = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, keep_largest=True)
    real = tsdf.tsdf_fuse

    def planted(*a, **kw):
        out = real(*a, **kw)
        empty = F.avg_pool3d((out["u"] < 0).float()[None, None], 5, stride=1)[0, 0] == 1      # 5^3 windows of empty space
        i, j, k = (int(x) for x in empty.nonzero()[0])
        out["u"][i + 1:i + 4, j + 1:j + 4, k + 1:k + 4] = 1.0         # a 3^3 blob with empty space all around it
        return out
    monkeypatch.setattr(tsdf, "tsdf_fuse", planted)
    both = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES)
    kept = r.extract_mesh_tsdf(poses, INTR_R, U.H, U.W, resolution=RES, keep_largest=True)
    assert both["vertices"].shape[0] > m["vertices"].shape[0]
    for k in ("vertices", "triangles", "colors"):
        assert torch.equal(kept[k], base[k]), k
