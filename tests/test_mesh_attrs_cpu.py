"""Per-vertex mesh attributes and the PLY layouts, on the host: the numpy restatement of lae_mesh_vertex_attrs (sign convention,
positions, lattice-point and constant-field cases) and read_ply over every vertex layout."""
import numpy as np
import pytest

from laenerf_amd import mesh

SHAPES = [(9, 12, 17), (16, 16, 16)]
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]


def field(name, shape):
    """the test fields on linspace(-1, 1) per axis; every one is cut at threshold 0"""
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing="ij")
    if name == "sphere":
        return (0.7 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    if name == "torus":
        return (0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z)).astype(np.float32)
    assert name == "noise"
    return np.random.default_rng(0).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_agree_with_the_faces_right_hand_normals(name, shape):
    u = field(name, shape)
    v, t = mesh.marching_cubes_numpy(u, 0.0)
    assert ((v - np.floor(v) > 0).sum(axis=1) == 1).all()             # every vertex sits inside one lattice edge
    a = mesh.vertex_attributes_numpy(u, v, BMIN, BMAX)
    p = a["pos"].astype(np.float64)
    face = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    summed = a["normals"].astype(np.float64)[t].sum(axis=1)
    assert len(t) > 100 and ((face * summed).sum(axis=1) > 0).all()
    assert np.array_equal(a["dirs"], -a["normals"])
    assert np.allclose(np.linalg.norm(a["normals"], axis=1), 1.0, atol=1e-6)


def test_positions_are_the_float64_scaling_rounded_once():
    shape = (16, 16, 16)
    bmin, bmax = (-1.0, -0.5, -2.0), (1.0, 1.5, 1.0)
    for name in ("sphere", "noise"):
        v, _ = mesh.marching_cubes_numpy(field(name, shape), 0.0)
        a = mesh.vertex_attributes_numpy(field(name, shape), v, bmin, bmax)
        want = mesh.scale_vertices(v, bmin, bmax, shape[0]).astype(np.float32)
        assert a["pos"].dtype == np.float32 and np.array_equal(a["pos"].view(np.uint32), want.view(np.uint32))
        same = mesh.vertex_attributes_numpy(field(name, shape), v, bmin, bmax, dtype=np.float64)["pos"]
        assert np.array_equal(same.view(np.uint32), want.view(np.uint32))


def test_a_vertex_on_a_lattice_point_gets_that_points_gradient():
    rng = np.random.default_rng(5)
    u = rng.standard_normal((6, 7, 8)).astype(np.float32)
    thr = np.float32(0.25)
    u[3, 3, 3] = thr                                                   # outside, exactly at the threshold
    u[2, 3, 3] = u[3, 2, 3] = u[3, 3, 2] = 1.5                        # edges ending there: t = 1
    u[4, 3, 3] = u[3, 4, 3] = u[3, 3, 4] = 2.5                        # edges starting there: t = 0
    v, _ = mesh.marching_cubes_numpy(u, thr)
    at = np.nonzero((v == np.float32(3)).all(axis=1))[0]
    assert len(at) == 6                                                # one vertex per edge, all at the same place
    bmin, bmax = (-1.0, -0.5, -2.0), (1.0, 1.5, 1.0)
    a = mesh.vertex_attributes_numpy(u, v, bmin, bmax)
    g = np.array([u[4, 3, 3] - u[2, 3, 3], u[3, 4, 3] - u[3, 2, 3], u[3, 3, 4] - u[3, 3, 2]], np.float32) * np.float32(0.5)
    w = g * (np.array(u.shape, np.float32) - 1) / (np.array(bmax, np.float32) - np.array(bmin, np.float32))
    want = -(w / np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])).astype(np.float32)
    for i in at:
        assert np.array_equal(a["normals"][i], want) and np.array_equal(a["dirs"][i], -want)
    # and a border point takes the one-sided differences
    b = mesh.vertex_attributes_numpy(u, np.array([[0, 6, 2]], np.float32), BMIN, BMAX, dtype=np.float64)
    gb = np.array([u[1, 6, 2] - u[0, 6, 2], u[0, 6, 2] - u[0, 5, 2], (u[0, 6, 3] - u[0, 6, 1]) * 0.5], np.float64) * \
        (np.array(u.shape) - 1.0) / 2.0
    assert np.allclose(b["dirs"][0], gb / np.linalg.norm(gb), atol=1e-12)


def test_a_constant_patch_gives_zero_normals_and_the_fallback_direction():
    u = np.full((5, 6, 7), 3.25, np.float32)
    verts = np.array([[1.5, 1, 1], [0, 0, 0], [4, 5, 5.75], [2, 2.25, 3]], np.float32)
    a = mesh.vertex_attributes_numpy(u, verts, BMIN, BMAX)
    assert np.array_equal(a["normals"], np.zeros((4, 3), np.float32))
    assert np.array_equal(a["dirs"], np.tile(np.array([0, 0, 1], np.float32), (4, 1)))
    u[0, 0, 0] = np.nan                                                # a non-finite gradient falls back too
    a = mesh.vertex_attributes_numpy(u, verts, BMIN, BMAX)
    assert np.array_equal(a["normals"][1], [0, 0, 0]) and np.array_equal(a["dirs"][1], [0, 0, 1])


def test_color_bytes_follow_the_rgb_u8_rule():
    x = np.array([-0.5, 0.0, 1.0 / 255, 0.999, 1.0, 7.0, np.nan, np.inf, -np.inf, 128 / 255], np.float32)
    want = [0, 0, int(np.float32(1.0 / 255) * np.float32(255)), 254, 255, 255, 0, 255, 0, int(np.float32(128 / 255) * np.float32(255))]
    assert mesh.color_bytes_numpy(x).tolist() == want


def _records(V, T, normals, colors, seed=0):
    rng = np.random.default_rng(seed)
    verts = np.zeros(V, mesh.vertex_dtype(normals, colors))
    verts["pos"] = rng.standard_normal((V, 3))
    if normals:
        verts["normals"] = rng.standard_normal((V, 3))
    if colors:
        verts["colors"] = rng.integers(0, 256, (V, 3))
    faces = np.zeros(T, mesh.FACE_DTYPE)
    faces["n"] = 3
    faces["i"] = rng.integers(0, max(V, 1), (T, 3))
    return verts, faces


@pytest.mark.parametrize("normals,colors", LAYOUTS)
def test_read_ply_round_trips_every_layout(tmp_path, normals, colors):
    assert mesh.vertex_dtype(normals, colors).itemsize == 12 + 12 * normals + 3 * colors and mesh.FACE_DTYPE.itemsize == 13
    for V, T in ((0, 0), (1, 1), (37, 61)):
        verts, faces = _records(V, T, normals, colors, seed=V)
        path = tmp_path / f"m{V}.ply"
        with open(path, "wb") as f:
            f.write(mesh.ply_header(V, T, normals, colors) + verts.tobytes() + faces.tobytes())
        got = mesh.read_ply(str(path))
        assert sorted(got) == sorted(["vertices", "triangles"] + ["normals"] * normals + ["colors"] * colors)
        assert got["vertices"].shape == (V, 3) and got["vertices"].dtype == np.float32
        assert got["triangles"].shape == (T, 3) and got["triangles"].dtype == np.int32
        assert np.array_equal(got["vertices"], verts["pos"]) and np.array_equal(got["triangles"], faces["i"])
        if normals:
            assert np.array_equal(got["normals"], verts["normals"])
        if colors:
            assert got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], verts["colors"])


def test_read_ply_reads_what_write_ply_writes(tmp_path):
    verts, faces = _records(20, 30, False, False)
    path = tmp_path / "plain.ply"
    mesh.write_ply(str(path), verts["pos"], faces["i"])
    got = mesh.read_ply(str(path))
    assert sorted(got) == ["triangles", "vertices"]
    assert np.array_equal(got["vertices"], verts["pos"]) and np.array_equal(got["triangles"], faces["i"])
    with open(path, "rb") as f:
        assert f.read().startswith(mesh.ply_header(20, 30))             # the same header as the packed writer's
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError):
        mesh.read_ply(str(path))


@pytest.mark.parametrize("normals,colors", LAYOUTS)
def test_header_text_matches_the_layout(normals, colors):
    lines = mesh.ply_header(5, 9, normals, colors).decode("ascii").split("\n")
    want = ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x", "property float y", "property float z"]
    if normals:
        want += ["property float nx", "property float ny", "property float nz"]
    if colors:
        want += ["property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face 9", "property list uchar int vertex_indices", "end_header", ""]
    assert lines == want
