"""Mesh export with per-vertex attributes on the MI355X: lae_mesh_vertex_attrs against its numpy restatement (positions bit for
bit, normals against a float64 evaluation of the same formulas), lae_mesh_pack_ply against numpy structured arrays byte for byte,
and save_mesh(normals=, colors=) end to end on a seeded network."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, T
from test_mesh_attrs_cpu import LAYOUTS, field

pytestmark = pytest.mark.gpu

BMIN, BMAX = (-1.0, -0.5, -2.0), (1.0, 1.5, 1.0)                      # a non-cubic box
SHAPES = [(9, 12, 17), (16, 16, 16), (5, 3, 130)]
# normals / dirs against float64: the interpolated gradient carries under ten fp32 roundings relative to
# M = max(|d(base)|, |d(q)|), about 5e-7 M; compared only where |g| >= 1e-2 M, so the direction's relative error stays below
# 5e-5 plus the normalisation's few ulp
NORMAL_TOL = 1e-4
MIN_RATIO = 1e-2
MAX_EXCLUDED = 0.01


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_vertex_attrs_match_the_restatement(name, shape):
    from laenerf_amd import mesh
    u = field(name, shape)
    v, _ = mesh.marching_cubes_numpy(u, 0.0)
    assert 200 <= len(v) <= 6000
    du, dv = T(u), T(v)
    got = mesh.vertex_attributes(du, dv, BMIN, BMAX)
    assert sorted(got) == ["dirs", "normals", "pos"]
    assert all(x.is_cuda and x.dtype == torch.float32 and x.shape == (len(v), 3) for x in got.values())
    ref32 = mesh.vertex_attributes_numpy(u, v, BMIN, BMAX)
    ref64 = mesh.vertex_attributes_numpy(u, v, BMIN, BMAX, dtype=np.float64)
    assert np.array_equal(got["pos"].cpu().numpy().view(np.uint32), ref32["pos"].view(np.uint32))
    g0, g1, t = mesh.edge_gradients_numpy(u, v, dtype=np.float64)
    g = g0 + t[:, None] * (g1 - g0)
    M = np.maximum(np.linalg.norm(g0, axis=1), np.linalg.norm(g1, axis=1))
    keep = np.linalg.norm(g, axis=1) >= MIN_RATIO * M
    assert (~keep).mean() <= MAX_EXCLUDED
    for k in ("normals", "dirs"):
        err = np.abs(got[k].cpu().numpy().astype(np.float64) - ref64[k])[keep].max()
        print(f"{name} {shape} {k}: V {len(v)}, excluded {(~keep).sum()}, max |device - float64| {err:.3e}")
        assert err <= NORMAL_TOL
    again = mesh.vertex_attributes(du, dv, BMIN, BMAX)
    assert all(torch.equal(got[k], again[k]) for k in got)
    only = mesh.vertex_attributes(du, dv, BMIN, BMAX, want=("normals",))
    assert list(only) == ["normals"] and torch.equal(only["normals"], got["normals"])


def test_vertex_attrs_clamp_garbage_vertices():
    from laenerf_amd import mesh
    u = np.random.default_rng(1).standard_normal((4, 4, 4)).astype(np.float32)
    verts = np.array([[np.nan, 1, 1], [-3.5, 2, 2], [1, -0.25, 7], [100.5, 2, 1], [2, 3, 3.75], [3, 3, 3], [np.inf, -np.inf, 2],
                      [1.5, 2.5, 0.5], [-100, -100, -100], [0, 0, 1e6]], np.float32)
    got = {k: x.cpu().numpy() for k, x in mesh.vertex_attributes(T(u), T(verts), BMIN, BMAX).items()}
    torch.cuda.synchronize()
    ref = mesh.vertex_attributes_numpy(u, verts, BMIN, BMAX)
    assert np.array_equal(got["pos"].view(np.uint32), ref["pos"].view(np.uint32)) and np.isfinite(got["pos"]).all()
    assert np.isfinite(got["normals"]).all() and np.isfinite(got["dirs"]).all()
    length = np.linalg.norm(got["dirs"], axis=1)
    assert np.allclose(length, 1.0, atol=1e-5)
    fallback = (got["normals"] == 0).all(axis=1)
    assert np.array_equal(got["dirs"][fallback], np.tile(np.float32([0, 0, 1]), (fallback.sum(), 1)))
    assert np.array_equal(got["dirs"][~fallback], -got["normals"][~fallback])


def test_vertex_attrs_abi_rejects_bad_sizes_and_null_pointers():
    from laenerf_amd import _lib
    lib = _lib.load()
    u = torch.zeros(4, 4, 4, device=DEV)
    v = torch.ones(5, 3, device=DEV)
    out = torch.full((5, 3), 7.0, device=DEV)
    box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    up, vp, op = u.data_ptr(), v.data_ptr(), out.data_ptr()
    assert lib.lae_mesh_vertex_attrs(up, 4, 4, 1, vp, 5, *box, op, None, None, None) == -1
    assert lib.lae_mesh_vertex_attrs(up, 513, 4, 4, vp, 5, *box, op, None, None, None) == -1
    assert lib.lae_mesh_vertex_attrs(None, 4, 4, 4, vp, 5, *box, op, None, None, None) == -3
    assert lib.lae_mesh_vertex_attrs(up, 4, 4, 4, None, 5, *box, op, None, None, None) == -3
    assert lib.lae_mesh_vertex_attrs(None, 4, 4, 4, None, 0, *box, None, None, None, None) == 0     # V = 0: nothing to do
    assert lib.lae_mesh_vertex_attrs(up, 4, 4, 4, vp, 5, *box, None, None, None, None) == 0         # no output asked for
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                          # nothing was launched
    from laenerf_amd import mesh
    empty = mesh.vertex_attributes(u, torch.empty(0, 3, device=DEV), box[:3], box[3:])
    assert all(x.shape == (0, 3) for x in empty.values())
    with pytest.raises(RuntimeError):
        mesh.vertex_attributes(torch.zeros(4, 4, 1, device=DEV), v, box[:3], box[3:])


COUNTS = [1, 3, 63, 64, 65, 255, 256, 257, 1000]


def _pack_inputs(V, Tn):
    rng = np.random.default_rng(1000 * V + Tn)
    pos = rng.standard_normal((V, 3)).astype(np.float32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    special = np.array([-0.5, -0.0, 0.0, 1.0, 1.5, np.nan, np.inf, -np.inf, 0.999999, 1e-9], np.float32)
    levels = (np.arange(256, dtype=np.float32) / np.float32(255))      # exact multiples of 1/255
    rgb = rng.uniform(-0.2, 1.2, (V, 3)).astype(np.float32)
    flat = rgb.reshape(-1)
    pool = np.concatenate([special, levels])
    where = rng.choice(flat.size, size=max(1, flat.size // 2), replace=False)
    flat[where] = pool[rng.integers(0, len(pool), len(where))]
    flat[:min(flat.size, len(special))] = special[:min(flat.size, len(special))]
    tris = rng.integers(0, V, (Tn, 3)).astype(np.int32)
    return pos, nrm, rgb, tris


@pytest.mark.parametrize("n", COUNTS)
def test_pack_ply_bytes_equal_numpy_structured_arrays(n):
    from laenerf_amd import mesh
    V, Tn = n, COUNTS[(COUNTS.index(n) + 4) % len(COUNTS)]             # V and T both walk the list, in different pairs
    pos, nrm, rgb, tris = _pack_inputs(V, Tn)
    faces = np.zeros(Tn, mesh.FACE_DTYPE)
    faces["n"] = 3
    faces["i"] = tris
    dpos, dnrm, drgb, dtris = T(pos), T(nrm), T(rgb), T(tris)
    for normals, colors in LAYOUTS:
        verts = np.zeros(V, mesh.vertex_dtype(normals, colors))
        verts["pos"] = pos
        if normals:
            verts["normals"] = nrm
        if colors:
            verts["colors"] = mesh.color_bytes_numpy(rgb)
        head, vb, fb = mesh.pack_ply(dpos, dtris, normals=dnrm if normals else None, colors=drgb if colors else None)
        assert head == mesh.ply_header(V, Tn, normals, colors)
        assert vb.is_cuda and vb.dtype == torch.uint8 and fb.is_cuda and fb.dtype == torch.uint8
        assert vb.cpu().numpy().tobytes() == verts.tobytes()
        assert fb.cpu().numpy().tobytes() == faces.tobytes()


def test_pack_ply_writes_nothing_past_its_buffers_and_either_half_alone():
    from laenerf_amd import _lib, mesh
    lib = _lib.load()
    V, Tn = 257, 65
    pos, nrm, rgb, tris = _pack_inputs(V, Tn)
    dpos, dnrm, drgb, dtris = T(pos), T(nrm), T(rgb), T(tris)
    verts = np.zeros(V, mesh.vertex_dtype(True, True))
    verts["pos"], verts["normals"], verts["colors"] = pos, nrm, mesh.color_bytes_numpy(rgb)
    faces = np.zeros(Tn, mesh.FACE_DTYPE)
    faces["n"], faces["i"] = 3, tris
    pad = 64
    vb = torch.full((V * 27 + pad,), 0xAB, dtype=torch.uint8, device=DEV)
    fb = torch.full((Tn * 13 + pad,), 0xAB, dtype=torch.uint8, device=DEV)
    assert lib.lae_mesh_pack_ply(dpos.data_ptr(), dnrm.data_ptr(), drgb.data_ptr(), V, None, 0, vb.data_ptr(), None, None) == 0
    assert vb[:V * 27].cpu().numpy().tobytes() == verts.tobytes() and (vb[V * 27:] == 0xAB).all() and (fb == 0xAB).all()
    assert lib.lae_mesh_pack_ply(None, None, None, 0, dtris.data_ptr(), Tn, None, fb.data_ptr(), None) == 0
    assert fb[:Tn * 13].cpu().numpy().tobytes() == faces.tobytes() and (fb[Tn * 13:] == 0xAB).all()
    # a 4-byte aligned base that is not 16-byte aligned takes the dword stores
    vb4 = torch.full((4 + V * 27 + pad,), 0xAB, dtype=torch.uint8, device=DEV)
    assert vb4.data_ptr() % 16 == 0
    assert lib.lae_mesh_pack_ply(dpos.data_ptr(), dnrm.data_ptr(), drgb.data_ptr(), V, None, 0, vb4.data_ptr() + 4, None, None) == 0
    assert vb4[4:4 + V * 27].cpu().numpy().tobytes() == verts.tobytes() and (vb4[:4] == 0xAB).all() and (vb4[4 + V * 27:] == 0xAB).all()


def test_pack_ply_rejects_misaligned_bases_null_inputs_and_bad_indices():
    from laenerf_amd import _lib, mesh
    lib = _lib.load()
    pos = torch.zeros(8, 3, device=DEV)
    tris = torch.zeros(8, 3, dtype=torch.int32, device=DEV)
    vb = torch.full((8 * 12 + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    fb = torch.full((8 * 13 + 8,), 0xAB, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        assert lib.lae_mesh_pack_ply(pos.data_ptr(), None, None, 8, tris.data_ptr(), 8, vb.data_ptr() + off, fb.data_ptr(), None) == -1
        assert lib.lae_mesh_pack_ply(pos.data_ptr(), None, None, 8, tris.data_ptr(), 8, vb.data_ptr(), fb.data_ptr() + off, None) == -1
    assert lib.lae_mesh_pack_ply(None, None, None, 8, tris.data_ptr(), 8, vb.data_ptr(), fb.data_ptr(), None) == -3
    assert lib.lae_mesh_pack_ply(pos.data_ptr(), None, None, 8, None, 8, vb.data_ptr(), fb.data_ptr(), None) == -3
    torch.cuda.synchronize()
    assert (vb == 0xAB).all() and (fb == 0xAB).all()                    # nothing was launched
    for bad in (-1, 8):
        t = tris.clone()
        t[5, 1] = bad
        with pytest.raises(ValueError):
            mesh.pack_ply(pos, t)
    head, v0, f0 = mesh.pack_ply(torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV))
    assert head == mesh.ply_header(0, 0) and v0.numel() == 0 and f0.numel() == 0


# ---- end to end on the seeded network of test_gpu_mesh.py

R = 48
COLOR_CHUNK = 4096


def _network(seed=11):
    """a structured random network, set up like tools/train_loop.py's teacher"""
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=1).to(DEV).eval()
    net.encoder.embeddings.data.uniform_(-1.0, 1.0)
    net.sigma_net.weights.data.mul_(1.5)
    return NeRFRenderer(net, bound=1, density_thresh=10).to(DEV).eval()


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """the renderer, its field and threshold, the geometry-only file and the device mesh with attributes (computed once)"""
    from laenerf_amd import mesh
    r = _network()
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    def query(pts):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return r.model.density_sigma(pts)

    u = mesh.extract_fields(bmin, bmax, R, query)
    thr = float(np.quantile(u.cpu().numpy(), 0.7))
    d = tmp_path_factory.mktemp("mesh_attrs")
    plain = str(d / "plain.ply")
    v, t = r.save_mesh(plain, resolution=R, threshold=thr)
    m = r.extract_mesh_attributes(resolution=R, threshold=thr, color_chunk=COLOR_CHUNK)
    return dict(r=r, u=u, thr=thr, dir=d, plain=plain, v=v, t=t, m=m, bmin=bmin, bmax=bmax)


def test_extract_mesh_attributes_returns_device_tensors(exported):
    from laenerf_amd import mesh
    m, V, Tn = exported["m"], len(exported["v"]), len(exported["t"])
    assert sorted(m) == ["colors", "normals", "triangles", "vertices"]
    assert V > COLOR_CHUNK and V % COLOR_CHUNK != 0 and Tn > 1000
    assert all(x.is_cuda for x in m.values())
    assert m["vertices"].shape == (V, 3) and m["normals"].shape == (V, 3) and m["colors"].shape == (V, 3)
    assert m["colors"].dtype == torch.float32 and 0.0 <= float(m["colors"].min()) and float(m["colors"].max()) <= 1.0
    assert np.array_equal(m["triangles"].cpu().numpy(), exported["t"])
    assert np.array_equal(m["vertices"].cpu().numpy(), exported["v"].astype(np.float32))
    iv, it = mesh.marching_cubes(exported["u"], exported["thr"])
    a = mesh.vertex_attributes(exported["u"], iv, exported["bmin"], exported["bmax"])
    assert torch.equal(a["normals"], m["normals"]) and torch.equal(a["pos"], m["vertices"])
    geometry = exported["r"].extract_mesh_attributes(resolution=R, threshold=exported["thr"], normals=False, colors=False)
    assert sorted(geometry) == ["triangles", "vertices"] and torch.equal(geometry["vertices"], m["vertices"])


def test_save_mesh_with_normals_and_colors(exported):
    from laenerf_amd import mesh
    r, m = exported["r"], exported["m"]
    path = str(exported["dir"] / "full.ply")
    v, t = r.save_mesh(path, resolution=R, threshold=exported["thr"], normals=True, colors=True, color_chunk=COLOR_CHUNK)
    assert v.dtype == np.float64 and np.array_equal(v, exported["v"]) and np.array_equal(t, exported["t"])
    got, plain = mesh.read_ply(path), mesh.read_ply(exported["plain"])
    assert sorted(got) == ["colors", "normals", "triangles", "vertices"] and sorted(plain) == ["triangles", "vertices"]
    assert np.array_equal(got["vertices"].view(np.uint32), plain["vertices"].view(np.uint32))
    assert np.array_equal(got["triangles"], plain["triangles"])
    iv, _ = mesh.marching_cubes(exported["u"], exported["thr"])
    a = mesh.vertex_attributes(exported["u"], iv, exported["bmin"], exported["bmax"])
    assert np.array_equal(got["normals"].view(np.uint32), a["normals"].cpu().numpy().view(np.uint32))
    V = len(v)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        chunks = [r.model(a["pos"][i:i + COLOR_CHUNK], a["dirs"][i:i + COLOR_CHUNK])[1].float() for i in range(0, V, COLOR_CHUNK)]
        whole = r.model(a["pos"], a["dirs"])[1].float()
    chunked = mesh.color_bytes_numpy(torch.cat(chunks).cpu().numpy())
    assert np.array_equal(got["colors"], chunked)
    assert np.array_equal(mesh.color_bytes_numpy(m["colors"].cpu().numpy()), chunked)
    # one call over every vertex instead: truncation can flip a level on a last-bit difference
    single = mesh.color_bytes_numpy(whole.cpu().numpy())
    diff = np.abs(single.astype(np.int32) - chunked.astype(np.int32))
    print(f"V {V}: single call against {COLOR_CHUNK}-row chunks: {int((diff > 0).sum())} of {diff.size} bytes differ, max {int(diff.max())} level(s)")
    assert diff.max() <= 1
    assert len(np.unique(got["colors"])) > 16                          # colours, not a constant

@pytest.mark.parametrize("normals,colors", [(True, False), (False, True)])
def test_save_mesh_other_layouts(exported, normals, colors):
    from laenerf_amd import mesh
    path = str(exported["dir"] / f"n{int(normals)}c{int(colors)}.ply")
    exported["r"].save_mesh(path, resolution=R, threshold=exported["thr"], normals=normals, colors=colors)
    got, plain = mesh.read_ply(path), mesh.read_ply(exported["plain"])
    assert sorted(got) == sorted(["triangles", "vertices"] + ["normals"] * normals + ["colors"] * colors)
    assert np.array_equal(got["vertices"].view(np.uint32), plain["vertices"].view(np.uint32))
    assert np.array_equal(got["triangles"], plain["triangles"])
    if normals:
        assert np.array_equal(got["normals"].view(np.uint32), exported["m"]["normals"].cpu().numpy().view(np.uint32))
    if colors:
        want = mesh.color_bytes_numpy(exported["m"]["colors"].cpu().numpy())
        assert np.abs(got["colors"].astype(np.int32) - want.astype(np.int32)).max() <= 1


def test_save_mesh_without_flags_writes_todays_bytes(exported):
    from laenerf_amd import mesh
    r = exported["r"]
    a, b = str(exported["dir"] / "flags_false.ply"), str(exported["dir"] / "write_ply.ply")
    r.save_mesh(a, resolution=R, threshold=exported["thr"], normals=False, colors=False)
    mesh.write_ply(b, *r.extract_mesh(resolution=R, threshold=exported["thr"]))
    data = [open(p, "rb").read() for p in (a, b, exported["plain"])]
    assert data[0] == data[1] == data[2]
    # and the packed writer gives the same file for the geometry-only layout
    head, vb, fb = mesh.pack_ply(exported["m"]["vertices"], exported["m"]["triangles"])
    c = str(exported["dir"] / "packed_plain.ply")
    mesh.write_ply_packed(c, head, vb, fb)
    assert open(c, "rb").read() == data[0]
