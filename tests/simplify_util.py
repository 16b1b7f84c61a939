"""The inputs of the simplification tests (test_simplify_cpu.py, test_gpu_simplify.py): meshes built once through
marching_cubes_numpy, cached, read-only.

    sphere24()       r - |X - c| on 24^3, r = 8.3, c = 11.5 + (0.13, -0.21, 0.07): V 1278, T 2552, index space, origin 0
    atlas_case()     atlas_util.mesh(atlas_util.CASES[0]): the 19 x 24 x 32 lattice in the box, origin the box minimum
    random12()       standard_normal((12, 12, 12)) at threshold 0: V 2372, T 4258
    box20()          min(X - 4.3, 14.6 - X, ...) on 20^3
    hand()           9 vertices, 7 triangles: a repeated corner, a collinear triangle, an unreferenced vertex, vertices on
                     cell boundaries, colours with C = 3
    CASES            name -> (mesh function, cell, keyword arguments of simplify_*), every comparison case of the GPU file
    want(name, **kw) simplify_numpy of a case, cached
    topology(tris)   (number of duplicate vertex sets, edges not in exactly two triangles, Euler characteristic over used vertices)
"""
import functools

import numpy as np


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _mc(u):
    from laenerf_amd.mesh import marching_cubes_numpy
    v, t = marching_cubes_numpy(u.astype(np.float32), 0.0)
    return {"verts": v, "tris": t, "origin": np.zeros(3, np.float32)}


def _lattice(n):
    return np.meshgrid(*(np.arange(m, dtype=np.float64) for m in n), indexing="ij")


@functools.lru_cache(maxsize=None)
def sphere24():
    X, Y, Z = _lattice((24, 24, 24))
    c = 11.5 + np.array([0.13, -0.21, 0.07])
    return _frozen(_mc(8.3 - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)))


SPHERE_C, SPHERE_R = 11.5 + np.array([0.13, -0.21, 0.07]), 8.3


@functools.lru_cache(maxsize=None)
def random12():
    return _frozen(_mc(np.random.default_rng(0).standard_normal((12, 12, 12))))


BOX_LO, BOX_HI = 4.3, 14.6


@functools.lru_cache(maxsize=None)
def box20():
    X, Y, Z = _lattice((20, 20, 20))
    return _frozen(_mc(np.minimum.reduce([X - BOX_LO, BOX_HI - X, Y - BOX_LO, BOX_HI - Y, Z - BOX_LO, BOX_HI - Z])))


@functools.lru_cache(maxsize=None)
def atlas_case():
    import atlas_util
    case = atlas_util.CASES[0]
    m = atlas_util.mesh(case)
    lo, hi = atlas_util.bounds(case[1])
    import torch
    axes = [torch.linspace(float(lo[a]), float(hi[a]), case[1][a]) for a in range(3)]      # mesh.lattice's statement, per axis
    spacing = max(float(a[1] - a[0]) for a in axes)                          # the largest spacing, as the renderer takes it
    return _frozen({"verts": m["pos"], "tris": m["tris"], "origin": lo.copy(), "spacing": spacing})


HAND_CELL = 2.0


@functools.lru_cache(maxsize=None)
def hand():
    """cell 2: the vertices 0, 2 and 3 lie exactly on cell boundaries (coordinates that are multiples of the cell); vertex 8 is in no
    triangle; triangle 3 repeats a corner, triangle 4 is collinear (on the x axis), triangles 5 and 6 collapse to the vertex set
    of triangle 0.  Clusters: {0, 1}, {2, 4}, {3}, {5}, {6}, {7}, {8}"""
    v = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.75], [2.0, 0.0, 0.0], [2.0, 2.0, 4.0], [3.5, 0.0, 0.0], [0.25, 3.0, 0.5],
                  [1.0, 1.5, 5.0], [5.0, 5.0, 1.0], [7.5, 0.5, 6.5]], np.float32)
    t = np.array([[0, 2, 5], [2, 3, 5], [3, 6, 7], [4, 4, 7], [0, 2, 4], [1, 4, 5], [5, 1, 2]], np.int32)
    col = np.random.default_rng(3).uniform(size=(9, 3)).astype(np.float32)
    return _frozen({"verts": v, "tris": t, "origin": np.zeros(3, np.float32), "colors": col})


def _atlas_cell(k):
    return k * atlas_case()["spacing"]


# name -> (mesh, cell, keyword arguments)
CASES = {
    "sphere24_c1.5": (sphere24, 1.5, {}), "sphere24_c2": (sphere24, 2.0, {}), "sphere24_c3": (sphere24, 3.0, {}),
    "sphere24_c4": (sphere24, 4.0, {}),
    "atlas_c1.5": (atlas_case, lambda: _atlas_cell(1.5), {}), "atlas_c2.5": (atlas_case, lambda: _atlas_cell(2.5), {}),
    "random12_c1": (random12, 1.0, {}), "random12_c2.5": (random12, 2.5, {}),
    "box20_c3": (box20, 3.0, {}),
    "hand": (hand, HAND_CELL, {}), "hand_one_cluster": (hand, 64.0, {}),
    # the variants of the rule
    "random12_c2.5_nodedup": (random12, 2.5, {"dedup": False}), "atlas_c2.5_nodedup": (atlas_case, lambda: _atlas_cell(2.5), {"dedup": False}),
    "sphere24_c3_mean": (sphere24, 3.0, {"placement": "mean"}), "box20_c3_mean": (box20, 3.0, {"placement": "mean"}),
    "sphere24_c2_reg1e-3": (sphere24, 2.0, {"reg": 1e-3}), "random12_c1_reg1e-3": (random12, 1.0, {"reg": 1e-3}),
    "hand_auto_origin": (hand, HAND_CELL, {"origin": None}),
}
# what the restated rule gives (V', T', duplicates removed), checked on the CPU when the rule was written
COUNTS = {"sphere24_c1.5": (None, 872, 0), "sphere24_c2": (None, 546, 0), "sphere24_c3": (None, 250, 0), "sphere24_c4": (None, 132, 0),
          "atlas_c1.5": (207, 410, 0), "atlas_c2.5": (75, 147, 7), "random12_c1": (1458, 2920, 20), "random12_c2.5": (125, 458, 99)}
CLOSED = ("sphere24_c1.5", "sphere24_c2", "sphere24_c3", "sphere24_c4", "atlas_c1.5")


def arguments(name):
    """-> (mesh dict, keyword arguments of simplify_numpy / simplify_mesh past verts and tris)"""
    fn, cell, kw = CASES[name]
    m = fn()
    kw = dict(kw)
    kw.setdefault("origin", m["origin"])
    kw["cell"] = cell() if callable(cell) else cell
    if "colors" in m:
        kw["colors"] = m["colors"]
    return m, kw


@functools.lru_cache(maxsize=None)
def want(name):
    from laenerf_amd.simplify import simplify_numpy
    m, kw = arguments(name)
    return _frozen(simplify_numpy(m["verts"], m["tris"], **kw))


def topology(tris):
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    sets = np.sort(t, axis=1)
    dup = len(sets) - len(np.unique(sets, axis=0)) if len(sets) else 0
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True) if len(e) else (e, np.zeros(0, int))
    return dup, int((cnt != 2).sum()), len(np.unique(t)) - len(ue) + len(t)


def spacing32(x):
    """the distance from |x| to the next fp32 above it"""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)
