"""The connected-component specification on the host: components_numpy / filter_components_numpy on cases with known answers,
against scipy where it is installed, the property that lets marching cubes run on a filtered field, and the C ABI of
lae_components_* (symbols, tag and the argument checks that return before any launch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from components_util import THR, sphere_and_blobs

NAMES = ["lae_components_label", "lae_components_sizes", "lae_components_filter"]


def _cc(u, thr=THR):
    from laenerf_amd.components import components_numpy
    return components_numpy(np.asarray(u, np.float32), thr)


def _lin(shape, i, j, k):
    return (i * shape[1] + j) * shape[2] + k


def test_all_inside_is_one_component_rooted_at_zero():
    labels, sizes, stats = _cc(np.ones((2, 2, 2)))
    assert labels.dtype == np.int32 and sizes.dtype == np.int32 and stats.dtype == np.int32
    assert (labels == 0).all() and sizes.tolist() == [8] + [0] * 7 and stats.tolist() == [1, 0, 8, 8]


def test_all_outside():
    labels, sizes, stats = _cc(np.zeros((3, 4, 5)))
    assert (labels == -1).all() and not sizes.any() and stats.tolist() == [0, -1, 0, 0]


def test_checkerboard_every_inside_point_is_its_own_component():
    i, j, k = np.indices((5, 4, 7))
    inside = (i + j + k) % 2 == 0
    labels, sizes, stats = _cc(inside.astype(np.float32))
    n = int(inside.sum())
    assert stats.tolist() == [n, 0, 1, n]
    assert np.array_equal(labels.reshape(-1)[inside.reshape(-1)], np.nonzero(inside.reshape(-1))[0])
    assert np.array_equal(sizes, inside.reshape(-1).astype(np.int32))


@pytest.mark.parametrize("second, n_comp", [
    ((slice(2, 4), slice(2, 4), slice(0, 2)), 2),      # touches the first cube along an edge only
    ((slice(2, 4), slice(2, 4), slice(2, 4)), 2),      # at a corner only
    ((slice(2, 4), slice(1, 3), slice(1, 3)), 1),      # shares one face link: (1,1,1) - (2,1,1)
])
def test_two_cubes(second, n_comp):
    shape = (5, 5, 5)
    u = np.zeros(shape, np.float32)
    u[0:2, 0:2, 0:2] = 1
    u[second] = 1
    labels, sizes, stats = _cc(u)
    assert stats[0] == n_comp and stats[3] == 16
    if n_comp == 2:
        root2 = _lin(shape, *(s.start for s in second))
        assert stats.tolist() == [2, 0, 8, 16] and sizes[0] == 8 and sizes[root2] == 8
        assert (labels[second] == root2).all() and (labels[0:2, 0:2, 0:2] == 0).all()
    else:
        assert stats.tolist() == [1, 0, 16, 16] and (labels[u > 0] == 0).all()


def test_nan_threshold_and_minus_inf_are_outside_plus_inf_is_inside():
    u = np.array([[[np.nan, 0.25], [-np.inf, np.inf]], [[0.25, np.nan], [np.inf, np.float32(0.25) + np.float32(1e-7)]]], np.float32)
    labels, sizes, stats = _cc(u, 0.25)
    assert np.array_equal(labels >= 0, np.array([[[0, 0], [0, 1]], [[0, 0], [1, 1]]], bool))
    assert stats.tolist() == [1, 3, 3, 3] and (labels[labels >= 0] == 3).all()
    # the threshold is the double cast once to fp32: 0.1 as fp32 is above 0.1, and a point holding fp32(0.1) is not above itself
    assert _cc(np.full((2, 2, 2), np.float32(0.1)), 0.1)[2].tolist() == [0, -1, 0, 0]


def test_against_scipy_on_random_fields():
    ndimage = pytest.importorskip("scipy.ndimage")
    for seed in range(10):
        rng = np.random.default_rng(seed)
        shape = tuple(int(x) for x in rng.integers(2, 14, 3))
        u = rng.random(shape).astype(np.float32)
        thr = float(rng.choice([0.3, 0.5, 0.6884, 0.8]))
        labels, sizes, stats = _cc(u, thr)
        lab, n = ndimage.label(u > np.float32(thr))                    # the default structure: 6-connectivity
        flat = lab.reshape(-1)
        first = np.full(n + 1, -1, np.int64)
        for p in range(flat.size - 1, -1, -1):
            first[flat[p]] = p                                         # the smallest index of each scipy label
        first[0] = -1
        assert np.array_equal(labels.reshape(-1), first[flat].astype(np.int32))
        assert stats[0] == n and stats[3] == int((flat > 0).sum())
        counts = np.bincount(flat, minlength=n + 1)[1:]
        assert stats[2] == (counts.max() if n else 0)
        assert np.array_equal(sizes[first[1:]], counts.astype(np.int32)) and int(sizes.sum()) == stats[3]


def _three_bars():
    """components of sizes 4, 6, 6 (roots 0, 30, 40) and a single point (root 79) in a [4, 2, 10] field"""
    u = np.zeros((4, 2, 10), np.float32)
    u[0, 0, 0:4] = 2.0
    u[1, 1, 0:6] = np.inf
    u[2, 0, 0:6] = 3.0
    u[3, 1, 9] = 7.0
    u[0, 1, 5] = np.nan
    u[0, 1, 6] = -4.0
    return u


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_filter(u, thr, out, removed_roots, labels):
    gone = np.isin(labels, removed_roots)
    assert np.array_equal(_bits(out)[~gone], _bits(u)[~gone])          # bitwise u, NaN payloads included
    assert (_bits(out)[gone] == _bits(np.float32(thr))).all()          # exactly float32(thr): not above it, so outside


def test_filter_largest_tie_goes_to_the_lower_root():
    from laenerf_amd.components import filter_components_numpy
    u = _three_bars()
    u.reshape(-1).view(np.uint32)[15] = 0x7fc00123                     # a NaN with a payload at (0, 1, 5)
    labels, sizes, stats = _cc(u, 1.0)
    assert stats.tolist() == [4, 30, 6, 17] and sizes[[0, 30, 40, 79]].tolist() == [4, 6, 6, 1]
    out, info = filter_components_numpy(u, 1.0, largest=True)
    assert info == dict(n_components=4, largest_root=30, largest_size=6, n_inside=17, min_size=0, keep_root=30)
    _check_filter(u, 1.0, out, [0, 40, 79], labels)
    assert _cc(out, 1.0)[2].tolist() == [1, 30, 6, 6]


def test_filter_min_size_boundary_and_fraction_ceiling():
    from laenerf_amd.components import filter_components_numpy
    u = _three_bars()
    labels = _cc(u, 1.0)[0]
    out, info = filter_components_numpy(u, 1.0, min_size=4)            # exactly min_size: kept
    assert info["min_size"] == 4 and info["keep_root"] == -1
    _check_filter(u, 1.0, out, [79], labels)
    out, _ = filter_components_numpy(u, 1.0, min_size=5)
    _check_filter(u, 1.0, out, [0, 79], labels)
    # min_fraction: ceil(f * largest_size) in integers: 0.6 * 6 = 3.6 -> 4 keeps the bar of 4, 0.67 * 6 = 4.02 -> 5 drops it
    out, info = filter_components_numpy(u, 1.0, min_fraction=0.6)
    assert info["min_size"] == 4 == math.ceil(0.6 * 6)
    _check_filter(u, 1.0, out, [79], labels)
    out, info = filter_components_numpy(u, 1.0, min_fraction=0.67)
    assert info["min_size"] == 5
    _check_filter(u, 1.0, out, [0, 79], labels)
    out, info = filter_components_numpy(u, 1.0, min_size=6, min_fraction=0.1)       # the larger of the two
    assert info["min_size"] == 6
    out, info = filter_components_numpy(u, 1.0, largest=True, min_size=7)           # rules combine: nothing passes both
    assert _cc(out, 1.0)[2].tolist() == [0, -1, 0, 0]
    with pytest.raises(ValueError):
        filter_components_numpy(u, 1.0)


def test_marching_cubes_of_the_filtered_field_is_the_mesh_without_the_blobs():
    from laenerf_amd.components import filter_components_numpy
    from laenerf_amd.mesh import marching_cubes_numpy
    both, sphere = sphere_and_blobs(24)
    out, info = filter_components_numpy(both, 0.0, largest=True)
    assert info["n_components"] == 4
    v, t = marching_cubes_numpy(out, 0.0)
    v0, t0 = marching_cubes_numpy(sphere, 0.0)
    v1, t1 = marching_cubes_numpy(both, 0.0)
    assert len(t0) > 500 and len(t1) > len(t0)
    assert np.array_equal(t, t0) and np.array_equal(v.view(np.uint32), v0.view(np.uint32))
    out, _ = filter_components_numpy(both, 0.0, min_fraction=0.5)
    v, t = marching_cubes_numpy(out, 0.0)
    assert np.array_equal(t, t0) and np.array_equal(v.view(np.uint32), v0.view(np.uint32))


# ---- the C ABI
def test_symbols_and_tag(hip_lib):
    from laenerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    for name in NAMES:
        assert re.search(r"LAE_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES
    assert re.search(r'#define\s+LAE_ABI_TAG\s+"(\w+)"', hdr).group(1) == "abi28"
    assert _lib.ABI_TAG == b"abi28" and hip_lib.lae_version().split()[-1] == b"abi28"
    assert "components.hip" in __import__("laenerf_amd.build", fromlist=["SOURCES"]).SOURCES


def test_arguments_are_rejected_before_any_launch(hip_lib):
    one = ctypes.c_void_p(16)
    # sides outside [2, 512]: LAE_EINVAL; NULL: LAE_ENULL
    assert hip_lib.lae_components_label(one, 1, 4, 4, 0.5, one, None) == -1
    assert hip_lib.lae_components_label(one, 4, 4, 513, 0.5, one, None) == -1
    assert hip_lib.lae_components_label(None, 4, 4, 4, 0.5, one, None) == -3
    assert hip_lib.lae_components_label(one, 4, 4, 4, 0.5, None, None) == -3
    # N == 0: OK without touching pointers
    assert hip_lib.lae_components_sizes(None, 0, None, None, None) == 0
    assert hip_lib.lae_components_filter(None, None, None, 0, 0.5, 0, -1, None, None) == 0
    assert hip_lib.lae_components_sizes(None, 8, one, one, None) == -3
    assert hip_lib.lae_components_sizes(one, 8, None, one, None) == -3
    assert hip_lib.lae_components_sizes(one, 8, one, None, None) == -3
    assert hip_lib.lae_components_sizes(one, 512 ** 3 + 1, one, one, None) == -1
    assert hip_lib.lae_components_sizes(one, 8, one, ctypes.c_void_p(20), None) == -1      # stats must be 8-byte aligned
    for k in range(4):
        args = [one, one, one, 8, 0.5, 0, -1, one, None]
        args[(0, 1, 2, 7)[k]] = None
        assert hip_lib.lae_components_filter(*args) == -3
    assert hip_lib.lae_components_filter(one, one, one, 512 ** 3 + 1, 0.5, 0, -1, one, None) == -1


def test_python_argument_checks_need_no_gpu():
    import torch
    from laenerf_amd import components
    with pytest.raises(RuntimeError):
        components.label_components(torch.zeros(4, 4, 4), 0.5)         # a CPU tensor: no fallback
    with pytest.raises(TypeError):
        components.label_components([[[0.0]]], 0.5)
    with pytest.raises(ValueError):
        components.keep_rule([1, 0, 8, 8])
    assert components.keep_rule([3, 20, 6, 17], largest=True) == (0, 20)
    assert components.keep_rule([0, -1, 0, 0], largest=True) == (0, -1)
    assert components.keep_rule([3, 20, 6, 17], min_size=2, min_fraction=0.5) == (3, -1)


def test_trainer_save_mesh_forwards_the_rule():
    from laenerf_amd.trainer import Trainer
    calls = []

    class Renderer:
        def save_mesh(self, path, **kw):
            calls.append(kw)
            return path

    class Holder:
        r = Renderer()

    rule = dict(keep_largest=False, min_component=None, min_component_fraction=None)
    assert Trainer.save_mesh(Holder(), "m.ply") == "m.ply" and calls[-1] == dict(resolution=256, threshold=10)      # today's call
    Trainer.save_mesh(Holder(), "m.ply", keep_largest=True)
    assert calls[-1] == dict(resolution=256, threshold=10, **dict(rule, keep_largest=True))
    Trainer.save_mesh(Holder(), "m.ply", normals=True, min_component=5, color_chunk=7)
    assert calls[-1] == dict(resolution=256, threshold=10, normals=True, colors=False, color_chunk=7, **dict(rule, min_component=5))
    Trainer.save_mesh(Holder(), "m.ply", colors=True)
    assert calls[-1] == dict(resolution=256, threshold=10, normals=False, colors=True)
