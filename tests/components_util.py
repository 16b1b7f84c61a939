"""fields for the connected-component tests (test_components_cpu.py, test_gpu_components.py): every builder returns an fp32 array
whose inside set at THR is the shape described; the numpy reference of a (shape, field) pair is computed once and shared"""
import numpy as np

THR = 0.5
TILE = (4, 4, 64)                                                     # csrc/components.hip CC_TX, CC_TY, CC_TZ
# the issue's shapes, plus one with three full tiles and a partial one along z (130 is two tiles of 64 and a partial one)
SHAPES = [(2, 2, 2), (3, 5, 7), (9, 17, 33), (33, 9, 17), (40, 24, 72), (5, 6, 130), (3, 6, 200)]


def _field(inside):
    return np.where(inside, np.float32(1.0), np.float32(0.0)).astype(np.float32)


def iid(shape, occupancy, seed):
    return _field(np.random.default_rng(seed).random(shape) < occupancy)


def checkerboard(shape):
    i, j, k = np.indices(shape)
    return _field((i + j + k) % 2 == 0)


def serpentine(shape, flip=False):
    """one path, one point wide: in every even x plane the even y rows, joined at alternating z ends by one point of the odd rows;
    the odd x planes hold one point, alternately over the plane path's end and over its start.  The path starts at linear index
    0; flip reverses every axis, which puts that end at the last index."""
    nx, ny, nz = shape
    b = np.zeros(shape, bool)
    plane = np.zeros((ny, nz), bool)
    plane[0::2] = True
    for j in range(1, ny - 1, 2):
        plane[j, nz - 1 if (j // 2) % 2 == 0 else 0] = True
    je = (ny - 1) - (ny - 1) % 2
    end = (je, nz - 1 if (je // 2) % 2 == 0 else 0)
    b[0::2] = plane
    for i in range(1, nx - 1, 2):
        b[(i,) + (end if (i // 2) % 2 == 0 else (0, 0))] = True
    return _field(b[::-1, ::-1, ::-1] if flip else b)


def comb(shape, thin=False):
    """parallel teeth (the even y planes; thin: their even z rows only, lines along x) joined only by the plane at the highest x:
    every tooth's smallest index is at x = 0, far from where the teeth meet"""
    i, j, k = np.indices(shape)
    teeth = (j % 2 == 0) & ((k % 2 == 0) if thin else True)
    return _field(teeth | (i == shape[0] - 1))


def _corner(shape):
    """a lattice point with a tile border through it on every axis that has one"""
    return tuple(t if n >= t + 2 else n // 2 for n, t in zip(shape, TILE))


def _box(shape, lo, hi):
    b = np.zeros(shape, bool)
    b[tuple(slice(max(l, 0), min(h, n)) for l, h, n in zip(lo, hi, shape))] = True
    return b


def touching_boxes(shape, far):
    """two boxes of up to 2^3 points on either side of a tile corner c: the first ends at c on every axis, the second begins at c on
    the axes in `far` (3 axes: the boxes meet at a corner; 2: along an edge) and ends there on the others.  Never face-adjacent."""
    c = _corner(shape)
    a = _box(shape, [x - 2 for x in c], c)
    b = _box(shape, [x if ax in far else x - 2 for ax, x in enumerate(c)], [x + 2 if ax in far else x for ax, x in enumerate(c)])
    return _field(a | b)


def linked_boxes(shape, axis):
    """two boxes on either side of the tile border across `axis`, shifted by one point along the other axes: exactly one pair of
    their points is face-adjacent, and it straddles the border"""
    c = _corner(shape)
    a = _box(shape, [x - 2 for x in c], c)
    b = _box(shape, [x if ax == axis else x - 1 for ax, x in enumerate(c)], [x + 2 if ax == axis else x + 1 for ax, x in enumerate(c)])
    return _field(a | b)


def special_values(shape, seed):
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal(shape) + THR).astype(np.float32)
    flat = u.reshape(-1)
    idx = rng.choice(flat.size, size=max(4, flat.size // 5), replace=False)
    flat[idx[0::4]] = THR                                             # exactly at the threshold: outside
    flat[idx[1::4]] = np.inf
    flat[idx[2::4]] = -np.inf
    flat[idx[3::4]] = np.nan
    return u


FIELDS = {
    "iid_0.2": lambda s: iid(s, 0.2, 1), "iid_0.3116": lambda s: iid(s, 0.3116, 2), "iid_0.5": lambda s: iid(s, 0.5, 3),
    "iid_0.9": lambda s: iid(s, 0.9, 4),
    "all_inside": lambda s: np.ones(s, np.float32), "all_outside": lambda s: np.zeros(s, np.float32),
    "checkerboard": checkerboard,
    "serpentine_from_first": lambda s: serpentine(s), "serpentine_from_last": lambda s: serpentine(s, flip=True),
    "comb": comb, "comb_thin": lambda s: comb(s, thin=True),
    "corner_contact": lambda s: touching_boxes(s, (0, 1, 2)),
    "edge_contact_x": lambda s: touching_boxes(s, (1, 2)), "edge_contact_y": lambda s: touching_boxes(s, (0, 2)),
    "edge_contact_z": lambda s: touching_boxes(s, (0, 1)),
    "face_link_x": lambda s: linked_boxes(s, 0), "face_link_y": lambda s: linked_boxes(s, 1), "face_link_z": lambda s: linked_boxes(s, 2),
    "special_values": lambda s: special_values(s, 5),
}

_CACHE = {}


def case(shape, name):
    """-> (u, labels, sizes, stats): the field and its numpy reference, computed once per session and never written to"""
    key = (tuple(shape), name)
    if key not in _CACHE:
        from laenerf_amd.components import components_numpy
        u = FIELDS[name](tuple(shape))
        out = (u,) + components_numpy(u, THR)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def sphere_and_blobs(R, radius=None, seed=0, n_blobs=3):
    """-> (u with a sphere and n_blobs small blobs, u with the sphere alone), fp32 [R,R,R], threshold 0: the blobs are at least two
    cells from the sphere and from each other, and smaller than it"""
    radius = 0.3 * R if radius is None else radius
    c = (R - 1) / 2.0 + np.array([0.3, -0.1, 0.2])
    x = np.stack(np.meshgrid(*(np.arange(R, dtype=np.float64),) * 3, indexing="ij"), -1)
    sphere = (radius - np.sqrt(((x - c) ** 2).sum(-1))).astype(np.float32)
    both = sphere.copy()
    rb = max(1.5, 0.04 * R)
    dirs = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]], np.float64)[:n_blobs] / np.sqrt(3.0)
    for d in dirs:
        cb = c + d * (radius + rb + 3.0)
        blob = (rb - np.sqrt(((x - cb) ** 2).sum(-1))).astype(np.float32)
        both = np.maximum(both, blob)
    return both, sphere
