"""Mesh extraction from a trained NeRF: the reference's `extract_fields` / `extract_geometry` / `Trainer.save_mesh`
(nerf/utils.py:189-219, 722-741) with marching cubes on the device (csrc/mesh.hip) instead of PyMCubes, and a PLY writer
instead of trimesh.

    marching_cubes(u, threshold)        the contract of mcubes.marching_cubes: vertices in index space, triangles
    marching_cubes_numpy(u, threshold)  the same specification restated in numpy (what the tests compare against)
    extract_fields / extract_geometry   the reference's lattice sweep and scaling, with the field kept on the device
    drop_components(u, threshold, ...)  the field without its floaters (components.py), for marching cubes only
    write_ply(path, vertices, triangles)
    vertex_attributes(u, verts, bmin, bmax)  per-vertex position in the box, normal and view direction on the device
    vertex_attributes_numpy(...)             the same specification restated in numpy
    pack_ply / write_ply_packed              the PLY bodies assembled on the device; the file is a header plus two buffers
    read_ply(path)                           reads what write_ply and write_ply_packed write

The specification (include/laenerf.h, lae_marching_cubes_*): corner inside iff value > threshold (NaN outside); one vertex
per crossed lattice edge, ordered by (lower point's linear index, axis x < y < z), at lower + t along the axis with
t = (thr - a) / (b - a) in fp32 (non-finite -> 0.5, clamped to [0, 1]); triangles ordered by (cube linear index, table
order) with welded vertex ids; the case table is tools/gen_mc_table.py's (csrc/mc_table.inc).

Vertex attributes (include/laenerf.h, lae_mesh_vertex_attrs): position = v / (n - 1) * (bmax - bmin) + bmin in fp64 with fp32
bounds, rounded once to fp32; the normal is the central-difference lattice gradient (one-sided on a border), interpolated
along the vertex's lattice edge, moved to the box by (n - 1) / (bmax - bmin), normalised and negated (it points towards lower
density, like the faces' right-hand normals); dirs = -normal is the direction a camera looking straight at the surface sees
it along (fallback (0, 0, 1) where the gradient vanishes).
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


def has_component_rule(keep_largest=False, min_component=None, min_component_fraction=None):
    return bool(keep_largest) or min_component is not None or min_component_fraction is not None


def drop_components(u, threshold, keep_largest=False, min_component=None, min_component_fraction=None):
    """the field marching cubes should run on: u itself with no rule (nothing is labelled, nothing launched), else a filtered copy
    (components.filter_components: keep_largest keeps the largest connected component of {u > threshold}, min_component those of
    at least that many lattice points, min_component_fraction those of at least that fraction of the largest).  u is not
    modified: vertex normals are taken from it, so a removed blob next to a kept surface does not bend that surface's normals."""
    if not has_component_rule(keep_largest, min_component, min_component_fraction):
        return u
    from . import components
    return components.filter_components(u, threshold, largest=keep_largest, min_size=min_component, min_fraction=min_component_fraction)[0]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, S=128, keep_largest=False, min_component=None,
                     min_component_fraction=None):
    """nerf/utils.py:207-219: -> vertices [V,3] float64 in the box, triangles [T,3] int32 (numpy).  keep_largest / min_component /
    min_component_fraction: drop_components between the sweep and marching cubes (the kept surfaces keep their bits)"""
    u = extract_fields(bound_min, bound_max, resolution, query_func, S=S)
    v, t = marching_cubes(drop_components(u, threshold, keep_largest, min_component, min_component_fraction), threshold)
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


# ---------------------------------------------------------------------------------------------------------------------------
# export with per-vertex attributes: lae_mesh_vertex_attrs, lae_mesh_pack_ply

ATTRS = ("pos", "normals", "dirs")


def _bounds32(b):
    return np.asarray(torch.as_tensor(b).detach().cpu(), dtype=np.float32).reshape(3)


def vertex_attributes(u, verts, bound_min, bound_max, want=ATTRS):
    """u [nx,ny,nz] fp32 CUDA (the field marching cubes ran on), verts [V,3] fp32 CUDA in index space -> a dict with the entries
    of `want` ("pos", "normals", "dirs"), each [V,3] fp32 on the device"""
    need_cuda(u, verts)
    if u.dtype != torch.float32 or verts.dtype != torch.float32:
        raise RuntimeError("laenerf_amd.vertex_attributes: field and vertices must be float32")
    need_contig(u, verts)
    _check_shape(u.shape)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError("laenerf_amd.vertex_attributes: vertices must be [V, 3]")
    unknown = set(want) - set(ATTRS)
    if unknown:
        raise ValueError(f"laenerf_amd.vertex_attributes: unknown attribute(s) {sorted(unknown)}")
    bmin, bmax = _bounds32(bound_min), _bounds32(bound_max)
    V = verts.shape[0]
    out = {k: torch.empty(V, 3, dtype=torch.float32, device=u.device) for k in ATTRS if k in want}
    nx, ny, nz = u.shape
    check(_lib.load().lae_mesh_vertex_attrs(ptr(u), nx, ny, nz, ptr(verts), V, *(float(x) for x in bmin), *(float(x) for x in bmax),
                                            ptr(out.get("pos")), ptr(out.get("normals")), ptr(out.get("dirs")), stream()),
          "mesh_vertex_attrs")
    return out


def edge_gradients_numpy(u, verts, dtype=np.float32):
    """where lae_mesh_vertex_attrs looks for a vertex's gradient: -> (d(base) [V,3], d(q) [V,3], t [V]) in `dtype`, with base the
    vertex's lower lattice point, q the other end of its lattice edge and t its fraction along it (index space)"""
    u32 = np.ascontiguousarray(u, dtype=np.float32)
    _check_shape(u32.shape)
    f = np.dtype(dtype).type
    n = np.array(u32.shape)
    v = np.array(verts, dtype=np.float32).reshape(-1, 3)
    v[~np.isfinite(v)] = 0
    base_f = np.clip(np.floor(v), np.float32(0), (n - 1).astype(np.float32)[None, :])
    base = base_f.astype(np.int64)
    frac = v - base_f                                                        # fp32
    has = frac > 0
    on_edge = has.any(axis=1)
    axis = np.argmax(has, axis=1)                                            # the first axis with frac > 0
    rows = np.arange(len(v))
    t = np.where(on_edge, frac[rows, axis], np.float32(0)).astype(f)
    q = base.copy()
    q[rows[on_edge], axis[on_edge]] = np.minimum(base[on_edge, axis[on_edge]] + 1, n[axis[on_edge]] - 1)
    uu = u32.astype(f)

    def grad(p):
        g = np.empty((len(p), 3), f)
        for a in range(3):
            lo, hi = p.copy(), p.copy()
            lo[:, a] = np.maximum(p[:, a] - 1, 0)
            hi[:, a] = np.minimum(p[:, a] + 1, n[a] - 1)
            diff = uu[hi[:, 0], hi[:, 1], hi[:, 2]] - uu[lo[:, 0], lo[:, 1], lo[:, 2]]
            g[:, a] = np.where(hi[:, a] - lo[:, a] == 2, diff * f(0.5), diff)
        return g

    with np.errstate(all="ignore"):
        return grad(base), grad(q), t


def vertex_attributes_numpy(u, verts, bound_min, bound_max, dtype=np.float32):
    """numpy restatement of lae_mesh_vertex_attrs -> dict(pos, normals, dirs), each [V,3], with fp32 operations in the kernel's
    order.  dtype=np.float64 evaluates the gradient, normal and direction formulas in float64 instead (what the device's
    normals are compared against); pos is fp32 and the same either way."""
    f = np.dtype(dtype).type
    n = np.array(np.shape(u))
    bmin, bmax = _bounds32(bound_min), _bounds32(bound_max)
    ext = bmax - bmin                                                        # fp32
    g0, g1, t = edge_gradients_numpy(u, verts, dtype)
    v = np.array(verts, dtype=np.float32).reshape(-1, 3)
    v[~np.isfinite(v)] = 0
    pos = (v.astype(np.float64) / (n - 1.0)[None, :] * ext.astype(np.float64)[None, :] + bmin.astype(np.float64)[None, :]).astype(np.float32)
    with np.errstate(all="ignore"):
        g = g0 + t[:, None] * (g1 - g0)
        s = (n - 1).astype(np.float32).astype(f) / ext.astype(f)             # fp32: float(n - 1) / (bmax - bmin)
        w = g * s[None, :]
        length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
        ok = (length > 0) & np.isfinite(length)
        unit = w / length[:, None]
    dirs = np.where(ok[:, None], unit, np.array([0, 0, 1], f)[None, :]).astype(f)
    normals = np.where(ok[:, None], -unit, f(0)).astype(f)
    return dict(pos=pos, normals=normals, dirs=dirs)


def color_bytes_numpy(rgb):
    """lae_eval_view's rgb_u8 rule in numpy: clip(x, 0, 1) * 255 in fp32, truncated; NaN -> 0"""
    x = np.asarray(rgb, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1)))
    return (x * np.float32(255)).astype(np.uint8)


def vertex_dtype(normals=False, colors=False):
    """the packed numpy record of one PLY vertex"""
    fields = [("pos", "<f4", (3,))]
    if normals:
        fields.append(("normals", "<f4", (3,)))
    if colors:
        fields.append(("colors", "u1", (3,)))
    return np.dtype(fields)


FACE_DTYPE = np.dtype([("n", "u1"), ("i", "<i4", (3,))])


def ply_header(V, T, normals=False, colors=False):
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {V}\nproperty float x\nproperty float y\nproperty float z\n"
    if normals:
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    return (head + f"element face {T}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def pack_ply(pos, tris, normals=None, colors=None):
    """pos [V,3] fp32, tris [T,3] int32, optional normals [V,3] fp32 and colors [V,3] fp32 in [0, 1], all on the device ->
    (header bytes, vertex_bytes [V * stride] uint8, face_bytes [T * 13] uint8); the two buffers stay on the device.  Triangle
    indices are range-checked first (one host read; ValueError as in write_ply)."""
    need_cuda(pos, tris, normals, colors)
    need_contig(pos, tris, normals, colors)
    for name, x in (("pos", pos), ("normals", normals), ("colors", colors)):
        if x is not None and (x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3 or x.shape[0] != pos.shape[0]):
            raise RuntimeError(f"laenerf_amd.pack_ply: {name} must be float32 [V, 3]")
    if tris.dtype != torch.int32 or tris.dim() != 2 or tris.shape[1] != 3:
        raise RuntimeError("laenerf_amd.pack_ply: tris must be int32 [T, 3]")
    V, T = pos.shape[0], tris.shape[0]
    if T and bool(((tris < 0) | (tris >= V)).any()):
        raise ValueError("pack_ply: a triangle index is out of range")
    stride = vertex_dtype(normals is not None, colors is not None).itemsize
    vb = torch.empty(V * stride, dtype=torch.uint8, device=pos.device)
    fb = torch.empty(T * FACE_DTYPE.itemsize, dtype=torch.uint8, device=pos.device)
    check(_lib.load().lae_mesh_pack_ply(ptr(pos), ptr(normals), ptr(colors), V, ptr(tris), T, ptr(vb) if V else None,
                                        ptr(fb) if T else None, stream()), "mesh_pack_ply")
    return ply_header(V, T, normals is not None, colors is not None), vb, fb


def write_ply_packed(path, header, vertex_bytes, face_bytes):
    """one copy to the host and one write per buffer"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(header)
        for buf in (vertex_bytes, face_bytes):
            f.write(memoryview(buf.cpu().numpy()))


_PLY_PROPS = {("x", "y", "z"): ("vertices", "float", "<f4"), ("nx", "ny", "nz"): ("normals", "float", "<f4"),
              ("red", "green", "blue"): ("colors", "uchar", "u1")}


def read_ply(path):
    """a binary little-endian PLY as write_ply / write_ply_packed write it -> dict(vertices [V,3] fp32, triangles [T,3] int32,
    and normals [V,3] fp32 / colors [V,3] uint8 where the file has them)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("read_ply: not a binary little-endian PLY 1.0")
    V = T = None
    props, element = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                V = int(w[2])
            elif element == "face":
                T = int(w[2])
            else:
                raise ValueError(f"read_ply: unknown element {element}")
        elif w[:1] == ["property"]:
            if element == "vertex":
                props.append((w[1], w[2]))
            elif w[1:] != ["list", "uchar", "int", "vertex_indices"]:
                raise ValueError(f"read_ply: unsupported face property `{ln}`")
    if V is None or T is None or len(props) % 3:
        raise ValueError("read_ply: the header names no vertex / face element or an unknown vertex layout")
    fields = []
    for i in range(0, len(props), 3):
        names, types = tuple(n for _, n in props[i:i + 3]), {t for t, _ in props[i:i + 3]}
        if names not in _PLY_PROPS or types != {_PLY_PROPS[names][1]}:
            raise ValueError(f"read_ply: unknown vertex properties {names}")
        fields.append((_PLY_PROPS[names][0], _PLY_PROPS[names][2], (3,)))
    vdt = np.dtype(fields)
    if len(data) != end + V * vdt.itemsize + T * FACE_DTYPE.itemsize:
        raise ValueError("read_ply: the file's size does not match its header")
    verts = np.frombuffer(data, vdt, V, end)
    faces = np.frombuffer(data, FACE_DTYPE, T, end + V * vdt.itemsize)
    if T and not (faces["n"] == 3).all():
        raise ValueError("read_ply: a face is not a triangle")
    out = {name: np.ascontiguousarray(verts[name]) for name in vdt.names}
    out["triangles"] = np.ascontiguousarray(faces["i"]).astype(np.int32)
    return out
