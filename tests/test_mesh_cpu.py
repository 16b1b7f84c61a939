"""Marching cubes without a GPU: the generated case table, the numpy restatement of the kernels' specification on analytic
and random fields (closed, consistently oriented 2-manifolds), the PLY writer and extract_geometry's scaling."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT


def _gen():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_generated_table_matches_committed_file():
    g = _gen()
    assert g.render() == open(os.path.join(ROOT, "laenerf_amd", "csrc", "mc_table.inc")).read()


def test_every_crossed_edge_lies_in_exactly_one_loop():
    g = _gen()
    from laenerf_amd.mesh import mc_table
    tb = mc_table()
    for case in range(256):
        loops, crossed = g.case_loops(case)
        used = sorted(e for loop in loops for e in loop)
        assert used == crossed, case
        assert all(len(loop) >= 3 for loop in loops), case
        assert tb["edge_mask"][case] == sum(1 << e for e in crossed)
        assert tb["tri_count"][case] == sum(len(loop) - 2 for loop in loops)
    assert tb["max_tris"] == max(tb["tri_count"])


def _edge_uses(tris):
    """undirected edge -> (uses, signed directions sum): a closed consistently oriented manifold has (2, 0) everywhere"""
    d = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    lo, hi = d.min(1), d.max(1)
    sign = np.where(d[:, 0] < d[:, 1], 1, -1)
    key = lo.astype(np.int64) * (1 << 32) + hi
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    s = np.zeros(len(uk), np.int64)
    np.add.at(s, inv, sign)
    return cnt, s, len(uk)


def _closed_manifold(v, t):
    cnt, s, n_edges = _edge_uses(t)
    assert (cnt == 2).all() and (s == 0).all()
    assert len(np.unique(t)) == len(v)                           # every vertex is used
    return len(v) - n_edges + len(t)                             # Euler characteristic


def _volume(v, t):
    a, b, c = (v[t[:, q]].astype(np.float64) for q in range(3))
    return np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0


def _grid(n):
    return np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")


def test_sphere_is_a_closed_oriented_manifold():
    from laenerf_amd.mesh import marching_cubes_numpy
    n, r = 64, 20.0
    x, y, z = _grid(n)
    c = (n - 1) / 2
    u = (r - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)).astype(np.float32)    # inside = positive (density-like)
    v, t = marching_cubes_numpy(u, 0.0)
    assert v.dtype == np.float32 and t.dtype == np.int32 and len(t) > 1000
    assert _closed_manifold(v, t) == 2
    # the outward orientation gives a positive divergence-theorem volume
    vol = _volume(v, t)
    assert abs(vol - 4.0 / 3.0 * np.pi * r ** 3) < 0.01 * 4.0 / 3.0 * np.pi * r ** 3
    # normals point from inside to outside: against the gradient of the field (which grows towards the centre)
    a, b, cc = (v[t[:, q]].astype(np.float64) for q in range(3))
    nrm = np.cross(b - a, cc - a)
    grad = c - (a + b + cc) / 3.0
    assert (np.einsum("ij,ij->i", nrm, grad) < 0).all()
    # vertices lie on the sphere (linear interpolation of a distance field)
    rad = np.linalg.norm(v.astype(np.float64) - c, axis=1)
    assert np.abs(rad - r).max() < 0.05


def test_torus_has_euler_characteristic_zero():
    from laenerf_amd.mesh import marching_cubes_numpy
    n = 48
    x, y, z = _grid(n)
    c = (n - 1) / 2
    q = np.sqrt((x - c) ** 2 + (y - c) ** 2) - 14.0
    u = (5.0 - np.sqrt(q ** 2 + (z - c) ** 2)).astype(np.float32)
    v, t = marching_cubes_numpy(u, 0.0)
    assert _closed_manifold(v, t) == 0
    assert _volume(v, t) > 0


@pytest.mark.parametrize("seed", range(6))
def test_random_fields_with_an_outside_border_are_closed_manifolds(seed):
    """only a face rule that neighbouring cubes share gives this on fields full of ambiguous faces"""
    from laenerf_amd.mesh import marching_cubes_numpy
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((16, 16, 16)).astype(np.float32)
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = (-1.0,) * 6
    v, t = marching_cubes_numpy(u, 0.0)
    assert len(t) > 500
    _closed_manifold(v, t)
    assert _volume(v, t) > 0


def test_specification_details_of_the_numpy_restatement():
    from laenerf_amd.mesh import marching_cubes_numpy
    u = np.zeros((2, 2, 3), np.float32)
    u[0, 0, 0] = 3.0                                            # one inside corner, threshold 1: t = (1 - 3) / (0 - 3)
    v, t = marching_cubes_numpy(u, 1.0)
    tt = np.float32(np.float32(-2.0) / np.float32(-3.0))
    # vertices by (point, axis): the three edges owned by point 0
    assert np.array_equal(v, np.array([[tt, 0, 0], [0, tt, 0], [0, 0, tt]], np.float32))
    assert np.array_equal(t, [[0, 1, 2]])
    # a value exactly at the threshold is outside; NaN is outside; inf gives t = 0.5 when (thr - a) / (b - a) is not finite
    u = np.array([[[1.0, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]], np.float32)
    assert marching_cubes_numpy(u, 1.0)[0].shape == (0, 3)
    u[0, 0, 0] = np.inf
    u[1, 1, 1] = np.nan
    v, t = marching_cubes_numpy(u, 1.0)
    assert np.array_equal(v, [[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]]) and len(t) == 1
    with pytest.raises(RuntimeError):
        marching_cubes_numpy(np.zeros((1, 4, 4), np.float32), 0.0)
    with pytest.raises(RuntimeError):
        marching_cubes_numpy(np.zeros((513, 2, 2), np.float32), 0.0)


def read_ply(path):
    """a small parser of the binary little-endian PLY write_ply produces"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int(next(h for h in head if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in head if h.startswith("element face")).split()[-1])
    assert "property list uchar int vertex_indices" in head
    v = np.frombuffer(data, "<f4", nv * 3, end).reshape(nv, 3)
    f = np.frombuffer(data, [("n", "u1"), ("i", "<i4", (3,))], nf, end + 12 * nv)
    assert (f["n"] == 3).all() and len(data) == end + 12 * nv + 13 * nf
    return v, f["i"]


def test_write_ply_round_trips(tmp_path):
    from laenerf_amd.mesh import marching_cubes_numpy, write_ply
    x, y, z = _grid(12)
    u = (4.0 - np.sqrt((x - 5.5) ** 2 + (y - 5.5) ** 2 + (z - 5.5) ** 2)).astype(np.float32)
    v, t = marching_cubes_numpy(u, 0.0)
    p = tmp_path / "sub" / "m.ply"
    write_ply(str(p), v.astype(np.float64), t)
    v2, t2 = read_ply(str(p))
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    write_ply(str(p), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    v2, t2 = read_ply(str(p))
    assert v2.shape == (0, 3) and t2.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(str(p), v, t + len(v))


def test_extract_geometry_scaling_equals_the_reference_expression():
    import torch
    from laenerf_amd.mesh import lattice, scale_vertices
    rng = np.random.default_rng(0)
    for bound, R in ((1.0, 256), (2.0, 129), (0.37, 64)):
        bmin = torch.tensor([-bound, -bound * 0.5, -bound], dtype=torch.float32)
        bmax = torch.tensor([bound, bound, bound * 0.75], dtype=torch.float32)
        v = (rng.random((1000, 3)) * (R - 1)).astype(np.float32).astype(np.float64)
        b_max_np, b_min_np = bmax.numpy(), bmin.numpy()
        ref = v / (R - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]          # nerf/utils.py:214-217
        assert np.abs(scale_vertices(v, bmin, bmax, R) - ref).max() <= 1e-6 * bound
        # lattice points are index-space points mapped the same way
        X = lattice(bmin, bmax, R)
        assert all(x.dtype == torch.float32 and len(x) == R for x in X)
        assert np.array_equal(X[0].numpy(), torch.linspace(bmin[0], bmax[0], R).numpy())


def test_marching_cubes_rejects_cpu_tensors_and_bad_shapes():
    import torch
    from laenerf_amd.mesh import marching_cubes
    with pytest.raises(RuntimeError):
        marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(TypeError):
        marching_cubes([[[0.0]]], 0.0)


def test_abi_rejects_bad_sizes_and_null_pointers(hip_lib):
    import ctypes
    one = ctypes.c_void_p(256)
    assert hip_lib.lae_marching_cubes_scratch_bytes(1, 4, 4) == 0
    assert hip_lib.lae_marching_cubes_scratch_bytes(4, 513, 4) == 0
    assert hip_lib.lae_marching_cubes_scratch_bytes(2, 2, 2) >= 4 * 8
    assert hip_lib.lae_marching_cubes_scratch_bytes(512, 512, 512) >= 4 * 512 ** 3
    assert hip_lib.lae_marching_cubes_count(one, 1, 4, 4, 0.0, one, one, None) == -1
    assert hip_lib.lae_marching_cubes_count(one, 4, 4, 600, 0.0, one, one, None) == -1
    assert hip_lib.lae_marching_cubes_count(None, 4, 4, 4, 0.0, one, one, None) == -3
    assert hip_lib.lae_marching_cubes_count(one, 4, 4, 4, 0.0, None, one, None) == -3
    assert hip_lib.lae_marching_cubes_count(one, 4, 4, 4, 0.0, one, None, None) == -3
    assert hip_lib.lae_marching_cubes_emit(one, 4, 0, 4, 0.0, one, one, one, None) == -1
    assert hip_lib.lae_marching_cubes_emit(one, 4, 4, 4, 0.0, one, None, one, None) == -3
    assert hip_lib.lae_marching_cubes_emit(one, 4, 4, 4, 0.0, one, one, None, None) == -3
    assert hip_lib.lae_marching_cubes_emit(one, 4, 4, 4, 0.0, None, one, one, None) == -3


def test_trainer_save_mesh_delegates_to_the_renderer():
    from laenerf_amd.trainer import Trainer
    calls = []

    class R:
        def save_mesh(self, path, resolution=256, threshold=10):
            calls.append((path, resolution, threshold))
            return "mesh"

    tr = Trainer.__new__(Trainer)
    tr.r = R()
    assert tr.save_mesh("a.ply") == "mesh" and tr.save_mesh("b.ply", resolution=64, threshold=2.5) == "mesh"
    assert calls == [("a.ply", 256, 10), ("b.ply", 64, 2.5)]
