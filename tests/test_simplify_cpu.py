"""simplify.simplify_numpy, the restatement the device kernels are compared against (test_gpu_simplify.py), checked on its own:
the counts of tests/simplify_util.py's inputs, the triangle rules, and the properties of the quadric placement."""
import os
import re

import numpy as np
import pytest

import simplify_util as SU
from laenerf_amd.simplify import simplify_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lae_simplify_keys", "lae_simplify_pairs", "lae_simplify_reduce", "lae_simplify_first", "lae_simplify_compact")


def test_input_meshes():
    for fn, V, T in ((SU.sphere24, 1278, 2552), (SU.random12, 2372, 4258), (SU.atlas_case, 968, 1932)):
        m = fn()
        assert (len(m["verts"]), len(m["tris"])) == (V, T), fn.__name__
    assert SU.hand()["verts"].shape == (9, 3) and SU.hand()["tris"].shape == (7, 3)


@pytest.mark.parametrize("name", sorted(SU.COUNTS))
def test_counts(name):
    w = SU.want(name)
    Vo, To, dups = SU.COUNTS[name]
    dup_sets, open_edges, euler = SU.topology(w["triangles"])
    print(name, len(w["vertices"]), len(w["triangles"]), w["n_duplicates"], dup_sets, open_edges, euler)
    assert len(w["triangles"]) == To and w["n_duplicates"] == dups and dup_sets == 0
    assert Vo is None or len(w["vertices"]) == Vo
    if name in SU.CLOSED:
        assert open_edges == 0 and euler == 2
    if name.startswith("random12"):
        assert abs(SU.want("random12_c2.5")["normal_margin"].min() - 0.026) < 5e-4


def test_hand_mesh():
    w = SU.want("hand")
    # clusters {0, 1}, {2, 4}, {3}, {5}, {6}, {7}, {8} in key order (i, j, k): (0,0,0) (0,0,2) (0,1,0) (1,0,0) (1,1,2) (2,2,0) (3,0,3)
    assert w["vertex_map"].tolist() == [0, 0, 3, 4, 3, 2, 1, 5, 6]
    assert w["triangles"].tolist() == [[0, 3, 2], [3, 4, 2], [4, 1, 5]] and w["n_duplicates"] == 2
    assert len(w["vertices"]) == 7                                             # the unreferenced vertex 8 keeps its cluster
    c = SU.hand()["colors"].astype(np.float64)
    assert np.array_equal(w["colors"][0], ((c[0] + c[1]) / 2).astype(np.float32)) and np.array_equal(w["colors"][6], c[8].astype(np.float32))
    assert np.array_equal(w["vertices"][6], SU.hand()["verts"][8])             # no faces: x = m, the member itself
    nd = SU.want("random12_c2.5_nodedup")
    assert len(nd["triangles"]) == 458 + 99 and SU.topology(nd["triangles"])[0] == 99
    one = SU.want("hand_one_cluster")
    assert len(one["vertices"]) == 1 and one["triangles"].shape == (0, 3) and (one["vertex_map"] == 0).all()
    auto = SU.want("hand_auto_origin")
    assert np.array_equal(auto["triangles"], w["triangles"]) and np.array_equal(auto["vertices"], w["vertices"])


def test_degenerate_inputs():
    h = SU.hand()
    e = simplify_numpy(h["verts"], np.zeros((0, 3), np.int32), SU.HAND_CELL, origin=h["origin"], colors=h["colors"])
    assert e["triangles"].shape == (0, 3) and len(e["vertices"]) == 7 and (e["normals"] == 0).all() and e["colors"].shape == (7, 3)
    z = simplify_numpy(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert z["vertices"].shape == (0, 3) and z["triangles"].shape == (0, 3) and z["vertex_map"].shape == (0,)
    bad = h["verts"].copy()
    bad[4, 1] = np.nan
    for origin in (h["origin"], None):
        with pytest.raises(ValueError):
            simplify_numpy(bad, h["tris"], SU.HAND_CELL, origin=origin)
    low = h["verts"].copy()
    low[5, 0] = -0.01
    with pytest.raises(ValueError):
        simplify_numpy(low, h["tris"], SU.HAND_CELL, origin=h["origin"])
    with pytest.raises(ValueError):
        simplify_numpy(h["verts"], h["tris"], SU.HAND_CELL, origin=h["origin"], dims=(2, 2, 2))
    with pytest.raises(ValueError):
        simplify_numpy(h["verts"], h["tris"], SU.HAND_CELL, placement="median")


@pytest.mark.parametrize("name", ["sphere24_c2", "atlas_c2.5", "random12_c1", "random12_c2.5", "hand"])
def test_vertex_map_and_triangle_order(name):
    m, kw = SU.arguments(name)
    w = SU.want(name)
    vm = w["vertex_map"]
    assert vm.shape == (len(m["verts"]),) and vm.min() == 0 and np.array_equal(np.unique(vm), np.arange(len(w["vertices"])))
    # monotone in key: the keys of the output vertices ascend, and every vertex maps to the cluster that holds it
    assert (np.diff(w["keys"]) > 0).all()
    c = np.float64(np.float32(kw["cell"]))
    inside = np.abs(m["verts"].astype(np.float64) - w["centres"][vm]) <= c / 2
    assert inside.all()
    # survivors: the mapped input triangles with three distinct corners, in input order and corner order, first of each set
    mt = vm[m["tris"]]
    alive = (mt[:, 0] != mt[:, 1]) & (mt[:, 1] != mt[:, 2]) & (mt[:, 0] != mt[:, 2])
    seen, keep = set(), []
    for i in np.nonzero(alive)[0]:
        k = tuple(sorted(mt[i]))
        if k not in seen:
            seen.add(k)
            keep.append(i)
    assert np.array_equal(w["triangles"], mt[keep])


def test_planar_patch_stays_on_its_plane():
    # a jittered 9 x 9 patch of the plane z = 20 + x / 2 - y / 4 whose coordinates are multiples of 1 / 256: exact in fp32
    rng = np.random.default_rng(1)
    g = 9
    xy = np.stack(np.meshgrid(np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 2) + rng.integers(-19, 20, (g * g, 2)) / 64.0
    P = np.concatenate([5.0 + xy, 20.0 + xy[:, :1] / 2 - xy[:, 1:] / 4], 1)
    v32 = P.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), P)
    n = np.array([-0.5, 0.25, 1.0]) / np.linalg.norm([-0.5, 0.25, 1.0])
    idx = np.arange(g * g).reshape(g, g)
    q = np.stack([idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]], -1).reshape(-1, 4)
    tris = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int32)
    for cell in (2.0, 3.5):
        w = simplify_numpy(v32, tris, cell, origin=np.zeros(3, np.float32))
        d = np.abs((w["positions64"] - P[0]) @ n)
        # a cluster whose plane point lies outside its cell is clamped back into it, off the plane: none of these is
        free = (np.abs(w["positions64"] - w["centres"]) < cell / 2).all(1)
        print("cell", cell, "clusters", len(d), "unclamped", int(free.sum()), "off-plane", d[free].max())
        assert free.sum() > 4 and d[free].max() <= 1e-12 * cell


def test_box_corners_quadric_beats_mean():
    q, m = SU.want("box20_c3"), SU.want("box20_c3_mean")
    corners = np.array([[x, y, z] for x in (SU.BOX_LO, SU.BOX_HI) for y in (SU.BOX_LO, SU.BOX_HI) for z in (SU.BOX_LO, SU.BOX_HI)])
    dq = np.linalg.norm(q["positions64"][None] - corners[:, None], axis=2).min(1)
    dm = np.linalg.norm(m["positions64"][None] - corners[:, None], axis=2).min(1)
    print("quadric", np.round(dq, 3), "mean", np.round(dm, 3))
    assert (dq < dm).all()


@pytest.mark.parametrize("name", ["sphere24_c1.5", "sphere24_c4", "atlas_c2.5", "random12_c1", "random12_c2.5", "box20_c3", "hand",
                                  "sphere24_c2_reg1e-3", "random12_c1_reg1e-3"])
def test_inside_cell_and_condition(name):
    m, kw = SU.arguments(name)
    w = SU.want(name)
    c = np.float64(np.float32(kw["cell"]))
    assert (np.abs(w["positions64"] - w["centres"]) <= c / 2).all()
    reg = kw.get("reg", 1e-2)
    print(name, "cond", w["cond"].max(), "bound", 1 + 3 / reg)
    assert w["cond"].max() <= (1 + 3 / reg) * (1 + 1e-9)


@pytest.mark.parametrize("name", ["sphere24_c2", "random12_c2.5", "atlas_c1.5", "box20_c3"])
def test_summation_order(name):
    m, kw = SU.arguments(name)
    w = SU.want(name)
    perm = np.random.default_rng(7).permutation(len(m["tris"]))
    s = simplify_numpy(m["verts"], m["tris"][perm], **kw)
    c = float(np.float32(kw["cell"]))
    d = np.abs(s["positions64"] - w["positions64"]).max()
    print(name, "shuffled order moves positions by", d, "cell", c)
    assert d < 1e-9 * c and np.abs(s["normals64"] - w["normals64"]).max() < 1e-9
    assert np.array_equal(s["vertex_map"], w["vertex_map"])


def test_abi_lists_the_entries():
    from laenerf_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    assert re.search(r'#define\s+LAE_ABI_TAG\s+"(\w+)"', hdr).group(1) == "abi28" and _lib.ABI_TAG == b"abi28"
    sentence = re.search(r"added under abi28 without touching an existing prototype:([^)]*)\)", hdr).group(1)
    for name in SYMBOLS:
        assert name in sentence, name
        proto = re.search(r"LAE_API\s+int\s+" + name + r"\s*\(([^;]*)\);", hdr)
        assert proto and len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert "simplify.hip" in build.SOURCES
    import laenerf_amd
    assert "simplify_mesh" in laenerf_amd.__all__ and laenerf_amd.simplify_numpy is simplify_numpy
