"""Mesh simplification on the device: quadric vertex clustering (csrc/simplify.hip).  The reference exports
the marching-cubes mesh at the lattice's triangle count; it has no counterpart of this module.

    simplify_mesh(verts, tris, cell, ...)     device tensors in, a dict of device tensors out
    simplify_numpy(verts, tris, cell, ...)    the same specification restated in numpy (what the tests compare against)
    grid_of(cell, origin, dims, lo, hi)       the cluster lattice both use

The rule (include/laenerf.h, lae_simplify_*).  Vertices fall into the cells of a lattice of spacing `cell` anchored at `origin`:
ijk = floor(((double)p - (double)origin) / (double)cell), key = (i ny + j) nz + k.  Every non-empty cell is one output vertex, its
id the rank of its key; `vertex_map` [V] maps input to output vertices.  Per cluster, in fp64 and relative to the cell centre
origin + (ijk + 0.5) cell: the member vertices' mean position m and colour mean, and over every triangle with at least one corner
in the cluster (once per cluster, dropped and degenerate triangles included) n = (p1 - p0) x (p2 - p0), A += n n^T,
b += -(n . p0) n, N += n.  The output vertex sits at centre + clamp(x, +-cell / 2) with (A + lambda I) x = lambda m - b,
lambda = reg trace(A) / 3 + 1e-18 cell^4: the point closest to the planes of the faces around the cell (weighted by squared area),
pulled towards the members' mean where those planes leave it free -- on a flat patch it stays on the plane, at a corner it goes
to the corner, where the mean would cut it off.  placement="mean" takes x = m (the control).  Normals are N / |N| (zero where N
is zero; they point where the faces' right-hand normals point, the convention of mesh.vertex_attributes), colours the member
mean.  Triangles: corners through vertex_map; a triangle with two equal corners is dropped; survivors keep their corner order
and their input order; with dedup only the lowest input index of every vertex set stays.

Output vertices that no triangle references stay (an unreferenced input vertex, or a cluster whose triangles all collapsed):
vertex_map is total.  Vertex clustering does NOT preserve manifoldness: two sheets closer than a cell are welded, and a thin
feature can collapse to an edge or a point.

Ordering is torch's (a stable sort of the int64 vertex keys, a stable sort of the (cluster, triangle) pairs, a stable sort of the
dedup keys, running sums, searchsorted for the segment starts); the kernels do the rest.  No floating-point number is added
atomically anywhere, so two calls give the same bytes.  Host reads: (V', flag) and (T', flag), 16 bytes each, plus one of 24
bytes for the vertices' bounds where origin or dims is None.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, need_contig, need_cuda, ptr, stream

BAD_VERTEX, BAD_INDEX = 1, 2               # include/laenerf.h LAE_SIMPLIFY_BAD_*
DEDUP_MAX = 1 << 21                        # LAE_SIMPLIFY_DEDUP_MAX
PLACEMENTS = {"quadric": 0, "mean": 1}     # LAE_SIMPLIFY_QUADRIC / _MEAN
MAX_COLORS = 4


def grid_of(cell, origin, dims, lo=None, hi=None):
    """-> (cell fp32, origin fp32 [3], dims (nx, ny, nz)).  origin None: lo, the vertices' componentwise minimum; dims None: the
    cells up to hi, their maximum.  ValueError for a cell that is not a positive finite fp32 or bounds that are not finite."""
    c = np.float32(cell)
    if not (c > 0 and np.isfinite(c)):
        raise ValueError("simplify_mesh: cell must be positive and finite (as fp32)")
    o = np.asarray(lo if origin is None else origin, dtype=np.float32).reshape(3)
    if not np.isfinite(o).all():
        raise ValueError("simplify_mesh: a vertex (or the origin) is not finite")
    if dims is None:
        h = np.asarray(hi, dtype=np.float32).reshape(3)
        if not np.isfinite(h).all():
            raise ValueError("simplify_mesh: a vertex is not finite")
        d = np.floor((h.astype(np.float64) - o.astype(np.float64)) / np.float64(c)) + 1
        if (d < 1).any():
            raise ValueError("simplify_mesh: a vertex lies below the origin")
        if (d >= 2.0 ** 32).any():
            raise ValueError("simplify_mesh: more than 2^32 cells along an axis; use a larger cell")
        dims = d
    dims = tuple(int(x) for x in dims)
    if len(dims) != 3 or any(not 1 <= n < 2 ** 32 for n in dims) or dims[0] * dims[1] * dims[2] >= 4 * 10 ** 18:
        raise ValueError("simplify_mesh: dims must be three positive cell counts whose product stays below 4e18")
    return c, o, dims


def _check_args(C, reg, placement):
    if placement not in PLACEMENTS:
        raise ValueError("simplify_mesh: placement is 'quadric' or 'mean'")
    if not 0.0 < float(reg) <= 1e6:
        raise ValueError("simplify_mesh: reg must be positive")
    if C > MAX_COLORS:
        raise ValueError(f"simplify_mesh: colors may have at most {MAX_COLORS} channels")


def _dedup_error(V_out):
    return ValueError(f"simplify_mesh: {V_out} output vertices do not fit the 21-bit fields of the duplicate key; "
                      "pass dedup=False or use a larger cell")


def simplify_numpy(verts, tris, cell, origin=None, dims=None, colors=None, reg=1e-2, placement="quadric", dedup=True):
    """numpy restatement of lae_simplify_*: the arguments of simplify_mesh as arrays -> its dict as arrays (vertices fp32 [V',3],
    triangles int32 [T',3], normals fp32 [V',3], colors fp32 [V',C] when given, vertex_map int32 [V]) plus, before rounding,
    positions64 and normals64 [V',3], normal_margin [V'] = |N| / sum |n| (1 where a cluster has no area), and keys int64 [V'],
    centres [V',3], cond [V'] (the condition number of A + lambda I; 1 for placement "mean"), n_duplicates."""
    v32 = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
    V, T = len(v32), len(t)
    col = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(V, -1)
    C = 0 if col is None else col.shape[1]
    _check_args(C, reg, placement)
    empty = {"vertices": np.zeros((0, 3), np.float32), "triangles": np.zeros((0, 3), np.int32), "normals": np.zeros((0, 3), np.float32),
             "vertex_map": np.zeros(0, np.int32), "positions64": np.zeros((0, 3)), "normals64": np.zeros((0, 3)),
             "normal_margin": np.zeros(0), "keys": np.zeros(0, np.int64), "centres": np.zeros((0, 3)), "cond": np.zeros(0), "n_duplicates": 0}
    if V == 0:
        if T:
            raise ValueError("simplify_mesh: a triangle index is out of range")
        if col is not None:
            empty["colors"] = np.zeros((0, C), np.float32)
        return empty
    with np.errstate(all="ignore"):
        c32, o32, dims = grid_of(cell, origin, dims, v32.min(0), v32.max(0))
        c, o = np.float64(c32), o32.astype(np.float64)
        f = np.floor((v32.astype(np.float64) - o[None, :]) / c)
        ok = (f >= 0) & (f < np.array(dims, np.float64)[None, :])
    if not ok.all():
        raise ValueError("simplify_mesh: a vertex is not finite, lies below the origin or outside dims")
    if T and (t.min() < 0 or t.max() >= V):
        raise ValueError("simplify_mesh: a triangle index is out of range")
    ijk = f.astype(np.int64)
    keys = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    ukeys, vmap = np.unique(keys, return_inverse=True)
    vmap = vmap.reshape(-1)
    Vo = len(ukeys)
    uijk = np.stack([ukeys // (dims[1] * dims[2]), (ukeys // dims[2]) % dims[1], ukeys % dims[2]], 1)
    centre = o[None, :] + (uijk.astype(np.float64) + 0.5) * c

    def seg_sum(idx, w):
        return np.stack([np.bincount(idx, weights=w[:, a], minlength=Vo) for a in range(w.shape[1])], 1) if w.shape[1] else np.zeros((Vo, 0))

    count = np.bincount(vmap, minlength=Vo).astype(np.float64)
    m = seg_sum(vmap, v32.astype(np.float64) - centre[vmap]) / count[:, None]
    mt = vmap[t]                                                                  # [T, 3] clusters of the corners
    emit = np.stack([np.ones(T, bool), mt[:, 1] != mt[:, 0], (mt[:, 2] != mt[:, 0]) & (mt[:, 2] != mt[:, 1])], 1)
    tt, slot = np.nonzero(emit)
    pc = mt[tt, slot]                                                             # the pair's cluster
    p = v32.astype(np.float64)[t[tt]] - centre[pc][:, None, :]                    # [P, 3 corners, 3]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).reshape(-1, 3)
    d = -((n[:, 0] * p[:, 0, 0] + n[:, 1] * p[:, 0, 1]) + n[:, 2] * p[:, 0, 2])
    A6 = seg_sum(pc, np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2], n[:, 2] * n[:, 2]], 1))
    b = seg_sum(pc, d[:, None] * n)
    N = seg_sum(pc, n)
    area = np.bincount(pc, weights=np.sqrt((n * n).sum(1)), minlength=Vo)
    lenN = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    with np.errstate(all="ignore"):
        normals64 = np.where(lenN[:, None] > 0, N / lenN[:, None], 0.0)
        margin = np.where(area > 0, lenN / area, 1.0)
    cond = np.ones(Vo)
    x = m
    if placement == "quadric":
        A = A6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(Vo, 3, 3)
        lam = float(reg) * ((A6[:, 0] + A6[:, 3]) + A6[:, 5]) / 3.0 + 1e-18 * ((c * c) * (c * c))
        M = A + lam[:, None, None] * np.eye(3)[None]
        x = np.linalg.solve(M, (lam[:, None] * m - b)[:, :, None])[:, :, 0]
        cond = np.linalg.cond(M)
    h = 0.5 * c
    pos64 = centre + np.clip(x, -h, h)
    out = {"vertices": pos64.astype(np.float32), "normals": normals64.astype(np.float32), "vertex_map": vmap.astype(np.int32),
           "positions64": pos64, "normals64": normals64, "normal_margin": margin, "keys": ukeys, "centres": centre, "cond": cond}
    if col is not None:
        out["colors"] = (seg_sum(vmap, col.astype(np.float64)) / count[:, None]).astype(np.float32)
    alive = (mt[:, 0] != mt[:, 1]) & (mt[:, 1] != mt[:, 2]) & (mt[:, 0] != mt[:, 2])
    keep = alive.copy()
    if dedup:
        if Vo > DEDUP_MAX:
            raise _dedup_error(Vo)
        s = np.sort(mt.astype(np.int64), axis=1)
        tk = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
        idx = np.nonzero(alive)[0]
        first = idx[np.unique(tk[idx], return_index=True)[1]]                     # idx ascends: the first of a key is its lowest index
        keep = np.zeros(T, bool)
        keep[first] = True
    out["n_duplicates"] = int(alive.sum() - keep.sum())
    out["triangles"] = mt[keep].astype(np.int32).reshape(-1, 3)
    return out


@torch.no_grad()
def simplify_mesh(verts, tris, cell, origin=None, dims=None, colors=None, reg=1e-2, placement="quadric", dedup=True, lanes=0,
                  probe=None):
    """verts [V,3] fp32 and tris [T,3] int32 on the device (any frame), cell > 0; origin [3] (None: the vertices' componentwise
    minimum) and dims (nx, ny, nz) (None: up to their maximum) -- either None costs one more host read; optional colors [V,C]
    fp32, C <= 4.  -> a dict of device tensors: `vertices` [V',3] fp32, `triangles` [T',3] int32, `normals` [V',3] fp32, `colors`
    [V',C] when given, `vertex_map` [V] int32.  reg: the weight of the members' mean against the planes (the solve's condition
    number is at most 1 + 3 / reg); placement "quadric" or "mean"; dedup: drop triangles that repeat a vertex set (at most 2^21
    output vertices).  Output vertices no triangle references stay, and manifoldness is not preserved (the module's docstring).
    ValueError: a vertex that is not finite, below the origin or outside dims; a triangle index outside [0, V); too many output
    vertices for dedup.  V = 0 and T = 0 are legal.  lanes: 1, 16 or 64 lanes per cluster in the reduce kernel (0: the library's
    choice; the bytes differ by summation order only); probe(name): called after each stage (tools/simplify_bench.py)."""
    need_cuda(verts, tris, colors)
    need_contig(verts, tris, colors)
    if verts.dtype != torch.float32 or verts.dim() != 2 or verts.shape[1] != 3:
        raise RuntimeError("laenerf_amd.simplify_mesh: verts must be float32 [V, 3]")
    if tris.dtype != torch.int32 or tris.dim() != 2 or tris.shape[1] != 3:
        raise RuntimeError("laenerf_amd.simplify_mesh: tris must be int32 [T, 3]")
    V, T = verts.shape[0], tris.shape[0]
    if colors is not None and (colors.dtype != torch.float32 or colors.dim() != 2 or colors.shape[0] != V):
        raise RuntimeError("laenerf_amd.simplify_mesh: colors must be float32 [V, C]")
    C = 0 if colors is None else colors.shape[1]
    _check_args(C, reg, placement)
    if lanes not in (0, 1, 16, 64):
        raise ValueError("simplify_mesh: lanes is 0, 1, 16 or 64")
    dev = verts.device
    probe = probe or (lambda name: None)

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    if V == 0:
        if T:
            raise ValueError("simplify_mesh: a triangle index is out of range")
        out = {"vertices": new((0, 3), torch.float32), "triangles": new((0, 3), torch.int32), "normals": new((0, 3), torch.float32),
               "vertex_map": new((0,), torch.int32)}
        if colors is not None:
            out["colors"] = new((0, C), torch.float32)
        return out
    lo = hi = None
    if origin is None or dims is None:
        lo, hi = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy()       # the extra host read
    elif isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().numpy()
    cell32, o32, dims = grid_of(cell, origin, dims, lo, hi)
    grid = (*(float(x) for x in o32), float(cell32), *dims)
    lib = _lib.load()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    keys = new((V,), torch.int64)
    check(lib.lae_simplify_keys(ptr(verts), V, *grid, ptr(keys), ptr(flag), stream()), "simplify_keys")
    probe("keys")
    vkeys, vorder = torch.sort(keys, stable=True)
    head = torch.ones(V, dtype=torch.bool, device=dev)
    head[1:] = vkeys[1:] != vkeys[:-1]
    rank = torch.cumsum(head, 0) - 1                                              # the output vertex of each sorted position
    V_out, bad = (int(x) for x in torch.stack([rank[-1] + 1, flag[0].long()]).cpu())      # host read 1
    if bad & BAD_VERTEX:
        raise ValueError("simplify_mesh: a vertex is not finite, lies below the origin or outside dims")
    if dedup and V_out > DEDUP_MAX:
        raise _dedup_error(V_out)
    vmap = new((V,), torch.int32)
    vmap[vorder] = rank.to(torch.int32)
    vstart = torch.searchsorted(rank, torch.arange(V_out + 1, dtype=torch.int64, device=dev))
    probe("vertex_order")

    surv = new((T,), torch.uint8)
    tkey = new((T,), torch.int64) if dedup else None
    porder = None
    if T:
        pair_cluster = new((3 * T,), torch.int32)
        check(lib.lae_simplify_pairs(ptr(tris), T, ptr(vmap), V, V_out, ptr(pair_cluster), ptr(surv), ptr(tkey), ptr(flag), stream()),
              "simplify_pairs")
        probe("pairs")
        sorted_cluster, porder = torch.sort(pair_cluster, stable=True)
        pstart = torch.searchsorted(sorted_cluster, torch.arange(V_out + 1, dtype=torch.int32, device=dev))
        probe("pair_order")
    else:
        pstart = torch.zeros(V_out + 1, dtype=torch.int64, device=dev)

    out = {"vertices": new((V_out, 3), torch.float32), "normals": new((V_out, 3), torch.float32)}
    if colors is not None:
        out["colors"] = new((V_out, C), torch.float32)
    check(lib.lae_simplify_reduce(ptr(verts), V, ptr(colors), C, ptr(tris), T, ptr(vorder), ptr(vkeys), ptr(vstart), ptr(porder),
                                  ptr(pstart), V_out, *grid, float(reg), PLACEMENTS[placement], int(lanes), ptr(out["vertices"]),
                                  ptr(out["normals"]), ptr(out.get("colors")) if C else None, stream()), "simplify_reduce")
    probe("reduce")

    T_out = 0
    if T:
        keep = surv
        if dedup:
            sorted_key, torder = torch.sort(tkey, stable=True)
            keep = new((T,), torch.uint8)
            check(lib.lae_simplify_first(ptr(sorted_key), ptr(torder), T, ptr(keep), stream()), "simplify_first")
            probe("dedup_order")
        incl = torch.cumsum(keep, 0, dtype=torch.int64)
        T_out, bad = (int(x) for x in torch.stack([incl[-1], flag[0].long()]).cpu())      # host read 2
        if bad & BAD_INDEX:
            raise ValueError("simplify_mesh: a triangle index is out of range")
    out["triangles"] = new((T_out, 3), torch.int32)
    if T_out:
        check(lib.lae_simplify_compact(ptr(tris), T, ptr(vmap), ptr(keep), ptr(incl), T_out, ptr(out["triangles"]), stream()),
              "simplify_compact")
    probe("compact")
    out["vertex_map"] = vmap
    return out
