"""Marching cubes on the MI355X against the numpy restatement of its specification (triangles exactly, vertices bit for bit),
and mesh extraction from a network against the reference-shaped field loop (nerf/utils.py:189-219)."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, T

pytestmark = pytest.mark.gpu


def _same(u, thr):
    from laenerf_amd.mesh import marching_cubes, marching_cubes_numpy
    v, t = marching_cubes(T(u), thr)
    v0, t0 = marching_cubes_numpy(u, thr)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert np.array_equal(t.cpu().numpy(), t0)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), v0.view(np.uint32))
    return v0, t0


def test_every_single_cube_case():
    for case in range(256):
        u = np.array([[[((case >> (dx + 2 * dy + 4 * dz)) & 1) * 2.0 - 0.25 * (dx + dy + dz) for dz in range(2)]
                       for dy in range(2)] for dx in range(2)], np.float32)
        v, t = _same(u, 0.5)
        assert (len(t) == 0) == (case in (0, 255))


def test_sphere():
    n = 96
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    u = (30.0 - np.sqrt((x - 47.3) ** 2 + (y - 46.9) ** 2 + (z - 48.1) ** 2)).astype(np.float32)
    v, t = _same(u, 0.0)
    assert len(t) > 10000


@pytest.mark.parametrize("shape", [(17, 33, 9), (2, 2, 2), (64, 64, 64), (5, 3, 130), (33, 17, 68)])
def test_random_fields(shape):
    rng = np.random.default_rng(sum(shape))
    u = rng.standard_normal(shape).astype(np.float32)
    flat = u.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 10), replace=False)
    flat[idx[0::4]] = 0.25                                            # exactly at the threshold (outside)
    flat[idx[1::4]] = np.inf
    flat[idx[2::4]] = -np.inf
    flat[idx[3::4]] = np.nan
    _same(u, 0.25)
    _same(u, -1.0)


def test_unaligned_field_takes_the_scalar_path():
    rng = np.random.default_rng(3)
    base = torch.from_numpy(rng.standard_normal(1 + 20 * 12 * 16).astype(np.float32)).to(DEV)
    u = base[1:].view(20, 12, 16)                                     # contiguous, 4 bytes past a 16-byte boundary
    from laenerf_amd.mesh import marching_cubes, marching_cubes_numpy
    v, t = marching_cubes(u, 0.1)
    v0, t0 = marching_cubes_numpy(u.cpu().numpy(), 0.1)
    assert np.array_equal(t.cpu().numpy(), t0) and np.array_equal(v.cpu().numpy().view(np.uint32), v0.view(np.uint32))


def test_empty_and_full_fields():
    from laenerf_amd.mesh import marching_cubes
    for val in (-1.0, 3.0):
        v, t = marching_cubes(torch.full((9, 10, 11), val, device=DEV), 0.5)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_numpy_in_numpy_out_and_two_runs_are_identical():
    from laenerf_amd.mesh import marching_cubes, marching_cubes_numpy
    rng = np.random.default_rng(7)
    u = rng.standard_normal((48, 40, 56)).astype(np.float32)
    v, t = marching_cubes(u, 0.3)
    assert isinstance(v, np.ndarray) and v.dtype == np.float64 and isinstance(t, np.ndarray)
    v0, t0 = marching_cubes_numpy(u, 0.3)
    assert np.array_equal(v, v0.astype(np.float64)) and np.array_equal(t, t0)
    a = marching_cubes(T(u), 0.3)
    b = marching_cubes(T(u), 0.3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_abi_rejects_bad_sizes_and_null_pointers():
    from laenerf_amd import _lib
    lib = _lib.load()
    u = torch.zeros(4, 4, 4, device=DEV)
    s = torch.empty(int(lib.lae_marching_cubes_scratch_bytes(4, 4, 4)), dtype=torch.uint8, device=DEV)
    c = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    assert lib.lae_marching_cubes_count(u.data_ptr(), 4, 4, 1, 0.0, s.data_ptr(), c.data_ptr(), None) == -1
    assert lib.lae_marching_cubes_count(u.data_ptr(), 4, 513, 4, 0.0, s.data_ptr(), c.data_ptr(), None) == -1
    assert lib.lae_marching_cubes_count(None, 4, 4, 4, 0.0, s.data_ptr(), c.data_ptr(), None) == -3
    assert lib.lae_marching_cubes_emit(u.data_ptr(), 4, 4, 4, 0.0, s.data_ptr(), None, c.data_ptr(), None) == -3
    torch.cuda.synchronize()
    assert c.tolist() == [7, 7]                                       # nothing was launched
    with pytest.raises(RuntimeError):
        from laenerf_amd.mesh import marching_cubes
        marching_cubes(torch.zeros(4, 4, 1, device=DEV), 0.0)


def _network(seed=11):
    """a structured random network, set up like tools/train_loop.py's teacher"""
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=1).to(DEV).eval()
    net.encoder.embeddings.data.uniform_(-1.0, 1.0)
    net.sigma_net.weights.data.mul_(1.5)
    return NeRFRenderer(net, bound=1, density_thresh=10).to(DEV).eval()


def _reference_fields(bound_min, bound_max, resolution, query_func, S=128):
    """nerf/utils.py:189-204 as written: host lattice, meshgrid per chunk, a host copy per chunk"""
    X = torch.linspace(bound_min[0], bound_max[0], resolution).split(S)
    Y = torch.linspace(bound_min[1], bound_max[1], resolution).split(S)
    Z = torch.linspace(bound_min[2], bound_max[2], resolution).split(S)
    u = np.zeros([resolution, resolution, resolution], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


def _ref_query(model):
    def query_func(pts):                                              # nerf/utils.py:731-735
        with torch.no_grad():
            with torch.autocast("cuda", dtype=torch.float16):
                return model.density(pts.to(DEV))["sigma"]
    return query_func


def test_extract_fields_equals_the_reference_loop():
    from laenerf_amd.mesh import extract_fields
    r = _network()
    bmin, bmax = r.aabb_infer[:3], r.aabb_infer[3:]
    for R, S in ((80, 32), (131, 128)):
        ref = _reference_fields(bmin.cpu(), bmax.cpu(), R, _ref_query(r.model), S=S)
        u = extract_fields(bmin, bmax, R, _ref_query(r.model), S=S)
        assert u.is_cuda and np.array_equal(u.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_extract_mesh_and_save_mesh_match_numpy_over_the_reference_field(tmp_path):
    from laenerf_amd.mesh import marching_cubes_numpy, scale_vertices
    from test_mesh_cpu import read_ply
    r = _network()
    R = 96
    bmin, bmax = r.aabb_infer[:3], r.aabb_infer[3:]
    ref = _reference_fields(bmin.cpu(), bmax.cpu(), R, _ref_query(r.model), S=128)
    thr = float(np.quantile(ref, 0.7))                                # a surface through a good part of the box
    v, t = r.extract_mesh(resolution=R, threshold=thr)
    v0, t0 = marching_cubes_numpy(ref, thr)
    assert len(t0) > 1000
    assert np.array_equal(t, t0)
    ref_v = v0.astype(np.float64) / (R - 1.0) * (bmax.cpu().numpy() - bmin.cpu().numpy())[None, :] + bmin.cpu().numpy()[None, :]
    assert v.dtype == np.float64 and np.array_equal(v, ref_v) and np.array_equal(v, scale_vertices(v0, bmin, bmax, R))
    path = tmp_path / "mesh.ply"
    v2, t2 = r.save_mesh(str(path), resolution=R, threshold=thr)
    pv, pt = read_ply(str(path))
    assert np.array_equal(pv, v.astype(np.float32)) and np.array_equal(pt, t) and np.array_equal(v2, v)
