"""Mesh extraction from a trained NeRF: the reference's `extract_fields` / `extract_geometry` / `Trainer.save_mesh`
(nerf/utils.py:189-219, 722-741) with marching cubes on the device (csrc/mesh.hip) instead of PyMCubes, and a PLY writer
instead of trimesh.

    marching_cubes(u, threshold)        the contract of mcubes.marching_cubes: vertices in index space, triangles
    marching_cubes_numpy(u, threshold)  the same specification restated in numpy (what the tests compare against)
    extract_fields / extract_geometry   the reference's lattice sweep and scaling, with the field kept on the device
    write_ply(path, vertices, triangles)

The specification (include/laenerf.h, lae_marching_cubes_*): corner inside iff value > threshold (NaN outside); one vertex
per crossed lattice edge, ordered by (lower point's linear index, axis x < y < z), at lower + t along the axis with
t = (thr - a) / (b - a) in fp32 (non-finite -> 0.5, clamped to [0, 1]); triangles ordered by (cube linear index, table
order) with welded vertex ids; the case table is tools/gen_mc_table.py's (csrc/mc_table.inc).
"""
import os
import re

import numpy as np
import torch

from . import _lib
from ._lib import check, need_contig, need_cuda, ptr, stream

MAX_SIDE = 512
_TABLE = None


def mc_table():
    """-> dict(edge_corner [12], edge_axis [12], edge_mask [256], tri_count [256], tri_edges [256, MC_MAX_TRIS, 3]) read from
    csrc/mc_table.inc, the table the kernels are compiled with"""
    global _TABLE
    if _TABLE is None:
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.inc")).read()
        max_tris = int(re.search(r"#define MC_MAX_TRIS (\d+)", src).group(1))

        def arr(name):
            body = re.search(r"__constant__ \w+ " + name + r"\[[^=]*=\s*\{(.*?)\};", src, re.S).group(1)
            body = re.sub(r"//[^\n]*", "", body)
            return np.array([int(v, 0) for v in re.findall(r"-?(?:0x)?[0-9a-fA-F]+", body)], np.int64)

        _TABLE = dict(edge_corner=arr("MC_EDGE_CORNER"), edge_axis=arr("MC_EDGE_AXIS"), edge_mask=arr("MC_EDGE_MASK"),
                      tri_count=arr("MC_TRI_COUNT"), tri_edges=arr("MC_TRI_EDGES").reshape(256, max_tris, 3), max_tris=max_tris)
    return _TABLE


def _check_shape(shape):
    if len(shape) != 3 or any(not 2 <= n <= MAX_SIDE for n in shape):
        raise RuntimeError(f"laenerf_amd.marching_cubes: field must be [Nx, Ny, Nz] with 2 <= N <= {MAX_SIDE} (got {tuple(shape)})")


def marching_cubes_numpy(u, threshold):
    """numpy restatement of lae_marching_cubes_*: -> vertices [V,3] fp32 (index space), triangles [T,3] int32"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    _check_shape(u.shape)
    nx, ny, nz = u.shape
    thr = np.float32(threshold)
    b = u > thr
    crossed = np.zeros(u.shape + (3,), bool)
    crossed[:-1, :, :, 0] = b[:-1] != b[1:]
    crossed[:, :-1, :, 1] = b[:, :-1] != b[:, 1:]
    crossed[:, :, :-1, 2] = b[:, :, :-1] != b[:, :, 1:]
    flat = crossed.reshape(-1)
    vid = np.full(flat.size, -1, np.int64)
    vid[flat] = np.arange(int(flat.sum()))
    pa = np.nonzero(flat)[0]
    p, axis = pa // 3, pa % 3
    i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
    step = np.array([ny * nz, nz, 1])[axis]
    uf = u.reshape(-1)
    a, bb = uf[p], uf[p + step]
    with np.errstate(all="ignore"):
        t = (thr - a) / (bb - a)
    t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
    t = np.clip(t, np.float32(0), np.float32(1))
    verts = np.stack([i, j, k], 1).astype(np.float32)
    verts[np.arange(len(p)), axis] += t

    tb = mc_table()
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= b[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(tb["tri_count"][case] > 0)                     # C order = cube linear index order
    cases = case[ci, cj, ck]
    cube = (ci * ny + cj) * nz + ck
    n = tb["tri_count"][cases]
    cube_r, case_r = np.repeat(cube, n), np.repeat(cases, n)
    slot = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    e = tb["tri_edges"][case_r, slot]                                       # [T, 3] cube-local edge ids
    c = tb["edge_corner"][e]
    owner = cube_r[:, None] + (c & 1) * (ny * nz) + ((c >> 1) & 1) * nz + ((c >> 2) & 1)
    tris = vid[owner * 3 + tb["edge_axis"][e]]
    assert (tris >= 0).all()
    return verts, tris.astype(np.int32).reshape(-1, 3)


def marching_cubes(u, threshold):
    """mcubes.marching_cubes on the device.  u: a CUDA fp32 tensor [Nx,Ny,Nz] -> (vertices [V,3] fp32, triangles [T,3] int32) on
    the same device; a numpy array -> uploaded, run on the device, (vertices float64, triangles int64) numpy.  A CPU tensor is an
    error (there is no CPU fallback)."""
    if isinstance(u, np.ndarray):
        v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda(), threshold)
        return v.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.int64)
    if not isinstance(u, torch.Tensor):
        raise TypeError("laenerf_amd.marching_cubes: u must be a torch tensor or a numpy array")
    need_cuda(u)
    if u.dtype != torch.float32:
        raise RuntimeError("laenerf_amd.marching_cubes: field must be float32")
    need_contig(u)
    _check_shape(u.shape)
    nx, ny, nz = u.shape
    lib = _lib.load()
    scratch = torch.empty(int(lib.lae_marching_cubes_scratch_bytes(nx, ny, nz)), dtype=torch.uint8, device=u.device)
    counts = torch.empty(2, dtype=torch.int32, device=u.device)
    thr = float(threshold)
    check(lib.lae_marching_cubes_count(ptr(u), nx, ny, nz, thr, ptr(scratch), ptr(counts), stream()), "marching_cubes_count")
    V, T = (int(x) for x in counts.cpu())                                  # the one host read: sizes the outputs
    verts = torch.empty(V, 3, dtype=torch.float32, device=u.device)
    tris = torch.empty(T, 3, dtype=torch.int32, device=u.device)
    if V:
        check(lib.lae_marching_cubes_emit(ptr(u), nx, ny, nz, thr, ptr(scratch), ptr(verts), ptr(tris), stream()), "marching_cubes_emit")
    return verts, tris


def lattice(bound_min, bound_max, resolution):
    """the reference's sample coordinates per axis (nerf/utils.py:191-193): torch.linspace on the host, fp32"""
    return [torch.linspace(float(bound_min[a]), float(bound_max[a]), resolution) for a in range(3)]


@torch.no_grad()
def extract_fields(bound_min, bound_max, resolution, query_func, S=128, device=None):
    """nerf/utils.py:189-204 with the field on the device: the same lattice and S^3 chunks (so query_func sees the same
    points in the same batches), but the points are assembled on the device and each chunk's sigma is written straight into
    the device field u [R,R,R] fp32 -- no per-chunk host copy.  -> u (a CUDA tensor)"""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    X, Y, Z = (c.to(dev) for c in lattice(bound_min, bound_max, resolution))
    u = torch.empty(resolution, resolution, resolution, dtype=torch.float32, device=dev)
    for xi, xs in enumerate(X.split(S)):
        for yi, ys in enumerate(Y.split(S)):
            for zi, zs in enumerate(Z.split(S)):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
                val = query_func(pts).reshape(len(xs), len(ys), len(zs))
                u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


def scale_vertices(vertices, bound_min, bound_max, resolution):
    """index space -> the box (nerf/utils.py:214-217): v / (R - 1) * (bmax - bmin) + bmin, float64 with fp32 bounds"""
    b_max = np.asarray(torch.as_tensor(bound_max).detach().cpu(), dtype=np.float32)
    b_min = np.asarray(torch.as_tensor(bound_min).detach().cpu(), dtype=np.float32)
    return np.asarray(vertices, dtype=np.float64) / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, S=128):
    """nerf/utils.py:207-219: -> vertices [V,3] float64 in the box, triangles [T,3] int32 (numpy)"""
    u = extract_fields(bound_min, bound_max, resolution, query_func, S=S)
    v, t = marching_cubes(u, threshold)
    return scale_vertices(v.cpu().numpy(), bound_min, bound_max, resolution), t.cpu().numpy()


def write_ply(path, vertices, triangles):
    """binary little-endian PLY 1.0: `float x y z`, `property list uchar int vertex_indices`"""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: a triangle index is out of range")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())
