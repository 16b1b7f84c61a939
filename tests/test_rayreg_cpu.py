"""Ray registration without a GPU: ray_registration_numpy against the reference's recorded results (tests/golden/rayreg_case.npz,
written by tests/golden/make_golden_rayreg.py from the reference's get_ref_supervision), its degenerate rules, and the host size
helpers and argument validation of the lae_rayreg_* entry points."""
import ctypes

import numpy as np

from conftest import golden
from rayreg_util import GAP_MARGIN, GOLDEN_SHAPE, THRESHOLD_MARGIN, brute_force, check_against_golden, separation, surface_case, unit


def golden_case():
    g = golden("rayreg_case")
    assert tuple(g["shape"].tolist()) == GOLDEN_SHAPE
    return g, surface_case(*GOLDEN_SHAPE, int(g["seed"]))


def test_numpy_restatement_reproduces_the_reference_fixture():
    from laenerf_amd.editing import ray_registration_numpy
    g, (ref_x, ref_rgb, ref_dirs, x, dirs) = golden_case()
    best, second, _ = brute_force(ref_x, x)
    thr, gap = separation(best, second)
    assert thr > THRESHOLD_MARGIN and gap > GAP_MARGIN and min(thr, gap) >= float(g["margin"]) > GAP_MARGIN    # what the generator chose the seed for
    res = ray_registration_numpy(ref_x, ref_rgb, ref_dirs, x, dirs, reg_dist=float(g["reg_dist"]), radius=float(g["radius"]),
                                 min_tv_factor=float(g["min_tv_factor"]))
    assert res["count"] == g["mask_dist"].size and np.array_equal(res["indices_ray_reg"], g["mask_dist"])
    check_against_golden(g, res, res["min_dist"], res["mask"], res["targets"], res["target_weights"], res["style_guide"])
    w = res["target_weights"]
    assert (w >= 0).all() and (w <= 1).all() and w.max() > 0.5                            # the caller's clamp_min(., 0) is a no-op


def test_numpy_restatement_degenerate_rules():
    from laenerf_amd.editing import ray_registration_numpy
    rng = np.random.default_rng(1)
    # dmax == dmin (one registered row; equal distances): the normalised term is 0, weight = the direction factor, no NaN
    ref_x = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    rgb = rng.random((2, 3)).astype(np.float32)
    rd = unit(np.array([[0, 0, 1.0], [0, 1.0, 0]])).astype(np.float32)
    x = np.array([[0.01, 0, 0], [1, 0.01, 0], [0.5, 0, 0]], np.float32)
    dirs = unit(np.array([[0, 0, 1.0], [0, -1.0, 0.0], [1, 0, 0]])).astype(np.float32)
    r = ray_registration_numpy(ref_x, rgb, rd, x, dirs)
    assert r["indices_ray_reg"].tolist() == [0, 1] and r["nn"].tolist() == [0, 1, -1]
    assert np.allclose(r["target_weights"], [1.0, 0.0]) and np.array_equal(r["targets"], rgb.astype(np.float64))
    tenth = float(np.float32(0.1))                                                        # the scalars are the fp32 values
    assert r["min_dist"][2] == tenth and r["min_dist_unclamped"][2] == 0.5
    assert r["style_guide"].tolist() == [tenth, tenth, 1.0]
    one = ray_registration_numpy(ref_x, rgb, rd, x[:1], dirs[:1])
    assert one["target_weights"].tolist() == [1.0]
    # R == 0: nothing registered, empty outputs, the guide still defined
    far = ray_registration_numpy(ref_x, rgb, rd, x + 5, dirs)
    assert far["count"] == 0 and far["targets"].shape == (0, 3) and far["target_weights"].shape == (0,) and (far["nn"] == -1).all()
    assert (far["style_guide"] == 1.0).all() and (far["min_dist"] == tenth).all()
    # M == 0 and non-finite rows: d = radius, nn = -1
    e = ray_registration_numpy(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), x, dirs)
    assert e["count"] == 0 and (e["nn"] == -1).all() and (e["min_dist"] == tenth).all()
    xb = x.copy()
    xb[0, 1] = np.nan
    xb[1, 0] = np.inf
    b = ray_registration_numpy(ref_x, rgb, rd, xb, dirs)
    assert b["nn"].tolist() == [-1, -1, -1] and b["count"] == 0
    # ties go to the lowest index; n == 0 is a no-op
    t = ray_registration_numpy(np.concatenate([ref_x, ref_x]), np.concatenate([rgb, rgb]), np.concatenate([rd, rd]), x, dirs)
    assert t["nn"].tolist() == [0, 1, -1]
    z = ray_registration_numpy(ref_x, rgb, rd, np.zeros((0, 3)), np.zeros((0, 3)))
    assert z["count"] == 0 and z["min_dist"].shape == (0,) and z["style_guide"].shape == (0,)


def test_workspace_sizes(hip_lib):
    L = hip_lib
    assert L.lae_rayreg_build_bytes(0) >= 256 + 16
    small, big = L.lae_rayreg_build_bytes(3001), L.lae_rayreg_build_bytes(1500000)
    assert 16 * 3001 <= small <= 16 * 3001 + (1 << 17)                                   # the sorted copy + a cell table of 4 M entries
    assert 16 * 1500000 <= big <= 16 * 1500000 + (9 << 20)                               # the cell table stops growing at 2^21 cells
    sizes = [L.lae_rayreg_build_bytes(m) for m in (0, 1, 15, 16, 17, 3001, 1 << 19, 1 << 21, 1 << 24)]
    assert sizes == sorted(sizes)
    q = [L.lae_rayreg_query_bytes(n, 3001) for n in (0, 1, 63, 64, 65, 255, 256, 257, 4099, 500000)]
    assert q == sorted(q) and q[-1] >= 8 * 500000 and q[-1] <= 8 * 500000 + (1 << 18)
    assert L.lae_rayreg_query_bytes(4099, 1500000) <= 8 * 4099 + (18 << 20)


def test_arguments_are_validated_before_any_launch(hip_lib):
    one = ctypes.c_void_p(256)
    L = hip_lib
    # n == 0: OK without touching pointers
    assert L.lae_rayreg_query(None, 5, None, 0, 0.1, 0, None, None, None, None) == 0
    assert L.lae_rayreg_supervise(None, None, 0, None, None, 5, None, 0.02, 0.1, 0.02, 0.1, None, None, None, None, None, None) == 0
    # NULL -> LAE_ENULL (build: the cloud may be NULL only when M == 0)
    assert L.lae_rayreg_build(None, 5, 0.1, one, None) == -3
    assert L.lae_rayreg_build(one, 5, 0.1, None, None) == -3
    assert L.lae_rayreg_build(None, 0, 0.1, None, None) == -3
    for hole in (0, 2, 6, 7, 8):
        a = [one, 5, one, 4, 0.1, 0, one, one, one, None]
        a[hole] = None
        assert L.lae_rayreg_query(*a) == -3, hole
    for hole in (0, 1, 3, 4, 6, 11, 12, 13, 14, 15):
        a = [one, one, 4, one, one, 5, one, 0.02, 0.1, 0.02, 0.1, one, one, one, one, one, None]
        a[hole] = None
        assert L.lae_rayreg_supervise(*a) == -3, hole
    a = [one, one, 4, None, None, 0, one, 0.02, 0.1, 0.02, 0.1, one, one, one, one, one, None]      # M == 0: no cloud arrays needed ...
    a[0] = None
    assert L.lae_rayreg_supervise(*a) == -3                                                         # ... everything else still is
    # bad scalars -> LAE_EINVAL
    for radius in (0.0, -0.1, float("nan"), float("inf")):
        assert L.lae_rayreg_build(one, 5, radius, one, None) == -1
        assert L.lae_rayreg_query(one, 5, one, 4, radius, 0, one, one, one, None) == -1
    assert L.lae_rayreg_query(one, 5, one, 4, 0.1, 2, one, one, one, None) == -1                    # unknown mode
    assert L.lae_rayreg_query(one, 5, one, 4, 0.1, -1, one, one, one, None) == -1
    assert L.lae_rayreg_build(one, 5, 0.1, ctypes.c_void_p(8), None) == -1                          # grid: 16-byte aligned
    assert L.lae_rayreg_query(ctypes.c_void_p(8), 5, one, 4, 0.1, 0, one, one, one, None) == -1
    assert L.lae_rayreg_query(one, 5, one, 4, 0.1, 0, one, one, ctypes.c_void_p(8), None) == -1
    assert L.lae_rayreg_build(one, (1 << 30) + 1, 0.1, one, None) == -1
    sup = lambda reg, radius, gmin, tv: L.lae_rayreg_supervise(one, one, 4, one, one, 5, one, reg, radius, gmin, tv, one, one, one, one, one, None)
    assert sup(0.0, 0.1, 0.02, 0.1) == -1 and sup(-1.0, 0.1, 0.02, 0.1) == -1                       # 0 < reg_dist
    assert sup(0.2, 0.1, 0.02, 0.1) == -1                                                           # reg_dist <= radius
    assert sup(0.02, 0.1, 0.1, 0.1) == -1 and sup(0.02, 0.1, 0.5, 0.1) == -1                        # guide_min < radius
    assert sup(0.02, 0.0, 0.01, 0.1) == -1 and sup(float("nan"), 0.1, 0.02, 0.1) == -1
    assert sup(0.02, 0.1, float("nan"), 0.1) == -1 and sup(0.02, 0.1, 0.02, float("nan")) == -1
    # n == 0 beats a bad pointer but not a bad scalar
    assert L.lae_rayreg_query(None, 5, None, 0, -1.0, 0, None, None, None, None) == -1
