"""-m gpu: ray registration in the cell grid (csrc/rayreg.hip, laenerf_amd.editing.ray_registration) against the float64
restatement: the query row by row (the chosen point is a nearest one, the index where the inputs are clear of ties), the
supervision arrays, the reference's fixture through the kernels, every shape at which the code takes another path, points and
queries placed on the grid's own cell faces, ties, a derandomised fuzz, and the two reference stages end to end on a small scene."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

from conftest import golden
from gpu_util import DEV, N, T
from rayreg_util import (GAP_MARGIN, GOLDEN_SHAPE, MIN_TV, RADIUS, REG_DIST, THRESHOLD_MARGIN, brute_force, check_against_golden,
                         chosen_distance, guide_bound, separation, surface_case, unit, weight_bound)

pytestmark = pytest.mark.gpu
FUZZ = dict(deadline=None, derandomize=True, database=None,
            suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large, HealthCheck.filter_too_much])


def shifted_case(M, n, seed):
    """rayreg_util.surface_case with the first 64 queries moved by +1: outside the cloud's box"""
    ref_x, ref_rgb, ref_dirs, x, dirs = surface_case(M, n, seed)
    x = x.copy()
    x[:64] += np.float32(1.0)
    return ref_x, ref_rgb, ref_dirs, x, dirs


def cube_case(M, n, seed):
    """a cloud inside a 0.05-wide cube (one cell, longer than an LDS tile); queries in and around it"""
    rng = np.random.default_rng([seed, M, n])
    ref_x = (0.3 + 0.05 * rng.random((M, 3))).astype(np.float32)
    x = (0.3 + 0.025 + (rng.random((n, 3)) - 0.5) * np.where(rng.random((n, 1)) < 0.5, 0.05, 0.4)).astype(np.float32)
    return ref_x, rng.random((M, 3)).astype(np.float32), unit(rng.standard_normal((M, 3))).astype(np.float32), x, \
        unit(rng.standard_normal((n, 3))).astype(np.float32)


def point_case(M, n, seed):
    """a cloud of one point, queries scattered around it up to 0.2 away"""
    rng = np.random.default_rng([seed, M, n])
    ref_x = rng.standard_normal((M, 3)).astype(np.float32)
    x = (ref_x[:1] + unit(rng.standard_normal((n, 3))) * (0.2 * rng.random((n, 1)))).astype(np.float32)
    if n == 1:
        x = (ref_x[:1] + np.float32(0.01)).astype(np.float32)
    return ref_x, rng.random((M, 3)).astype(np.float32), unit(rng.standard_normal((M, 3))).astype(np.float32), x, \
        unit(rng.standard_normal((n, 3))).astype(np.float32)


SHAPES = {"1x1": (point_case, 1, 1), "1x300": (point_case, 1, 300), "cube5000x2000": (cube_case, 5000, 2000),
          "3001x4099": (shifted_case, 3001, 4099), "20011x4099": (shifted_case, 20011, 4099)}


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """inputs, the float64 brute force and the float64 restatement of one shape, computed once and shared (read only)"""
    from laenerf_amd.editing import ray_registration_numpy
    make, M, n = SHAPES[name]
    arrays = make(M, n, seed)
    best, second, arg = brute_force(arrays[0], arrays[3])
    res = ray_registration_numpy(*arrays, reg_dist=REG_DIST, radius=RADIUS, min_tv_factor=MIN_TV)
    return arrays, (best, second, arg), res


def cloud_of(arrays, radius=RADIUS):
    from laenerf_amd.editing import RefCloud
    return RefCloud(T(arrays[0]), T(arrays[1]), T(arrays[2]), radius=radius)


def check_query(ref_x, x, d, nn, best, radius=RADIUS, exact_threshold=True):
    """the query's contract against float64, row by row: the chosen point is a nearest one to 1e-6, d is its distance to 1e-6,
    nn == -1 exactly where the float64 minimum is at least the radius (exact_threshold=False: up to 1e-6 either side)"""
    radius = float(np.float32(radius))
    d, nn = np.asarray(d, np.float64), np.asarray(nn, np.int64)
    hit = nn >= 0
    assert (nn[hit] < ref_x.shape[0]).all()
    chosen = chosen_distance(ref_x, x, nn)
    assert (chosen[hit] <= best[hit] * (1 + 1e-6)).all()
    want = np.minimum(best, radius)
    assert (np.abs(d - want) <= 1e-6 * want).all()
    assert (d[~hit] == radius).all() and (d[hit] < radius).all()
    if exact_threshold:
        assert np.array_equal(~hit, best >= radius)
    else:
        assert (best[~hit] >= radius * (1 - 1e-6)).all() and (best[hit] <= radius * (1 + 1e-6)).all()


def check_supervision(arrays, got, res):
    """register_rays' arrays against the float64 restatement `res` (the inputs are clear of the thresholds and of ties)"""
    ref_x, ref_rgb = arrays[0], arrays[1]
    nn = N(got["nn"]).astype(np.int64)
    idx = N(got["indices_ray_reg"])
    assert got["indices_ray_reg"].dtype == torch.int64 and got["count"] == idx.size == res["count"]
    assert np.array_equal(idx, res["indices_ray_reg"])
    assert np.array_equal(N(got["targets"]).view(np.uint32), ref_rgb[nn[idx]].view(np.uint32))        # an exact copy
    wb, gb = weight_bound(res["min_dist"], res["mask"]), guide_bound()
    if idx.size:
        dw = np.abs(N(got["target_weights"]).astype(np.float64) - res["target_weights"]).max()
        print("weights: max deviation", dw, "bound", wb)
        assert dw <= wb
    dg = np.abs(N(got["style_guide"]).astype(np.float64) - res["style_guide"]).max() if res["style_guide"].size else 0.0
    print("guide: max deviation", dg, "bound", gb)
    assert dg <= gb


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_query_and_supervision_against_float64(seed):
    from laenerf_amd.editing import register_rays
    arrays, (best, second, arg), res = case("3001x4099", seed)
    thr, gap = separation(best, second)
    near = best < float(np.float32(RADIUS))
    print("within radius", near.mean(), "registered", res["mask"].mean(), "threshold margin", thr, "gap", gap)
    assert thr > THRESHOLD_MARGIN and gap > GAP_MARGIN                       # nothing has to be left out of a comparison
    assert near.mean() > 0.9 and 0.5 < res["mask"].mean() < 0.8 and not near[:64].any()
    cloud = cloud_of(arrays)
    assert cloud.M == 3001 and (cloud.cells >= 10).all() and cloud.s >= RADIUS * (1 + 2.0 ** -11)
    got = register_rays(cloud, T(arrays[3]), T(arrays[4]), reg_dist=REG_DIST, min_tv_factor=MIN_TV)
    check_query(arrays[0], arrays[3], N(got["min_dist"]), N(got["nn"]), best)
    assert np.array_equal(N(got["nn"]).astype(np.int64), np.where(near, arg, -1))          # with the asserted gaps: the same indices
    check_supervision(arrays, got, res)


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    from laenerf_amd.editing import register_rays
    arrays, (best, second, arg), res = case(name)
    thr, _ = separation(best, second)
    assert thr > THRESHOLD_MARGIN
    cloud = cloud_of(arrays)
    for mode in ("binned", "gather"):
        d, nn = cloud.query(T(arrays[3]), mode=mode)
        check_query(arrays[0], arrays[3], N(d), N(nn), best)
    got = register_rays(cloud, T(arrays[3]), T(arrays[4]), reg_dist=REG_DIST, min_tv_factor=MIN_TV)
    assert np.array_equal(N(got["min_dist"]), N(d)) and np.array_equal(N(got["nn"]), N(nn))         # the two modes agree bit for bit
    _, gap = separation(best, second)
    assert gap > GAP_MARGIN                                                              # the seeds are chosen for it
    assert np.array_equal(N(nn).astype(np.int64), res["nn"])
    check_supervision(arrays, got, res)
    if name == "cube5000x2000":
        assert (cloud.cells == 1).all() and (best < 0.1).sum() > 1000
    if name == "1x1":
        assert got["count"] == 1                                                         # dmax == dmin: the weight is the direction factor


def test_degenerate_inputs():
    """an empty cloud, no queries, non-finite rows, a single registered row (dmax == dmin: the weight is the direction factor)"""
    from laenerf_amd.editing import RefCloud, register_rays
    arrays, _, _ = case("1x300")
    x, dirs = T(arrays[3]), T(arrays[4])
    empty = RefCloud(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV))
    got = register_rays(empty, x, dirs)
    tenth = float(np.float32(0.1))
    assert got["count"] == 0 and (N(got["nn"]) == -1).all() and (N(got["min_dist"]) == tenth).all() and (N(got["style_guide"]) == 1.0).all()
    assert got["targets"].shape == (0, 3) and got["target_weights"].shape == (0,)
    cloud = cloud_of(arrays)
    none = register_rays(cloud, x[:0], dirs[:0])
    assert none["count"] == 0 and none["min_dist"].shape == (0,) and none["style_guide"].shape == (0,)
    ref = arrays[0][0]
    xb = np.stack([ref + np.float32(0.01), ref + np.float32(0.01), ref + np.float32(0.01), ref + np.float32(0.005)]).astype(np.float32)
    xb[0, 1], xb[1, 0], xb[2, 2] = np.nan, np.inf, -np.inf
    db = np.tile(arrays[2][:1], (4, 1))                                                  # the cloud point's own direction: cos = 1, f = 1
    got = register_rays(cloud, T(xb), T(db))
    assert N(got["nn"]).tolist() == [-1, -1, -1, 0] and N(got["min_dist"])[:3].tolist() == [tenth] * 3
    assert N(got["indices_ray_reg"]).tolist() == [3] and N(got["target_weights"]).tolist() == [1.0]
    assert np.array_equal(N(got["targets"]), arrays[1][:1])
    # a cloud with non-finite points: they are never chosen
    bad = arrays[0].repeat(3, 0).copy()
    bad[0, 0], bad[2, 1] = np.nan, np.inf
    c3 = RefCloud(T(bad), T(arrays[1].repeat(3, 0)), T(arrays[2].repeat(3, 0)))
    d3, nn3 = c3.query(x)
    d1, nn1 = cloud.query(x)
    assert np.array_equal(N(d3), N(d1)) and np.array_equal(N(nn3), np.where(N(nn1) >= 0, 1, -1))


def test_golden_fixture_through_the_kernels():
    from laenerf_amd.editing import ray_registration_numpy, register_rays
    g = golden("rayreg_case")
    arrays = surface_case(*GOLDEN_SHAPE, int(g["seed"]))
    res = ray_registration_numpy(*arrays, reg_dist=float(g["reg_dist"]), radius=float(g["radius"]), min_tv_factor=float(g["min_tv_factor"]))
    got = register_rays(cloud_of(arrays, float(g["radius"])), T(arrays[3]), T(arrays[4]), reg_dist=float(g["reg_dist"]),
                        min_tv_factor=float(g["min_tv_factor"]))
    mask = np.zeros(GOLDEN_SHAPE[1], bool)
    mask[N(got["indices_ray_reg"])] = True
    check_against_golden(g, res, N(got["min_dist"]).astype(np.float64), mask, N(got["targets"]), N(got["target_weights"]), N(got["style_guide"]))


def face_case(axis):
    """points on the faces of the grid's own cells and one ulp either side, each with a query just under the radius away across
    that face, on either side; every pair at a place of its own (more than the radius from every other pair).  The grid is fixed
    by two corner points and the point count, so it is built once with the points parked in a corner to read lo and s."""
    from laenerf_amd.editing import RefCloud
    G, fill = 40, 16400
    s0 = float(np.float32(np.float32(RADIUS) * np.float32(1 + 2.0 ** -10)))
    corner = np.float32(39.5 * s0)
    ks, variants, sides = range(1, G), (-1, 0, 1), (-1, 1)
    sites = [(k, v, sd) for k in ks for v in variants for sd in sides]
    M = 2 + fill + len(sites)
    parked = np.zeros((M, 3), np.float32)
    parked[1] = corner
    probe = RefCloud(T(parked), T(parked), T(parked), radius=RADIUS)
    lo, s = probe.lo, probe.s
    assert (probe.cells == G).all() and (lo == 0).all() and s >= RADIUS * (1 + 2.0 ** -11)
    ref_x, x = parked.copy(), np.zeros((len(sites), 3), np.float32)
    others = [a for a in range(3) if a != axis]
    limit = float(np.float32(RADIUS)) * (1 - 2.5e-6)
    for j, (k, v, sd) in enumerate(sites):
        p = np.zeros(3, np.float32)
        p[others[0]] = np.float32(lo[others[0]] + (2.5 + 2 * (j % 18)) * s)
        p[others[1]] = np.float32(lo[others[1]] + (2.5 + 2 * (j // 18)) * s)
        face = np.float32(lo[axis] + k * s)
        for _ in range(abs(v)):
            face = np.nextafter(face, np.float32(np.inf * v))
        p[axis] = face
        q = p.copy()
        q[axis] = np.float32(float(face) + sd * float(np.float32(RADIUS)))
        while abs(float(q[axis]) - float(face)) > limit:                                  # the nearest fp32 position just under the radius
            q[axis] = np.nextafter(q[axis], face)
        ref_x[2 + fill + j], x[j] = p, q
    assert 2 * (len(sites) // 18) + 2.5 < G - 3
    return ref_x, x, (lo, s, G)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cell_faces(axis):
    """fails if the cell side has no rounding margin over the radius: a point just under a face and a query just under the radius
    beyond it can then land two cells apart"""
    from laenerf_amd.editing import RefCloud
    ref_x, x, (lo, s, G) = face_case(axis)
    best, second, arg = brute_force(ref_x, x)
    radius = float(np.float32(RADIUS))
    thr = np.abs(best / radius - 1).min()
    assert (best < radius).all() and thr > THRESHOLD_MARGIN and (best > radius * (1 - 1e-5)).all()      # every pair just under the radius
    assert (second > radius).all()                                                      # and alone
    cells_p = np.floor((ref_x[arg, axis].astype(np.float64) - lo[axis]) / s)
    cells_q = np.floor((x[:, axis].astype(np.float64) - lo[axis]) / s)
    assert set(np.abs(cells_p - cells_q).astype(int).tolist()) == {0, 1}
    cloud = RefCloud(T(ref_x), T(ref_x), T(ref_x), radius=RADIUS)
    assert (cloud.lo == lo).all() and cloud.s == s and (cloud.cells == G).all()
    for mode in ("binned", "gather"):
        d, nn = cloud.query(T(x), mode=mode)
        check_query(ref_x, x, N(d), N(nn), best)
        assert np.array_equal(N(nn).astype(np.int64), arg)


def test_ties_and_order_independence():
    arrays, (best, second, arg), _ = case("3001x4099")
    ref_x, ref_rgb, ref_dirs, x, dirs = arrays
    M = ref_x.shape[0]
    near = best < float(np.float32(RADIUS))
    twice = tuple(np.concatenate([a, a]) for a in (ref_x, ref_rgb, ref_dirs))
    cloud2 = cloud_of(twice)
    d_a, nn_a = cloud2.query(T(x))
    d_b, nn_b = cloud2.query(T(x))
    assert torch.equal(d_a, d_b) and torch.equal(nn_a, nn_b)                             # two runs: the same bits
    assert np.array_equal(N(nn_a).astype(np.int64), np.where(near, arg, -1))             # of the two copies the lower index
    d_g, nn_g = cloud2.query(T(x), mode="gather")
    assert torch.equal(d_a, d_g) and torch.equal(nn_a, nn_g)
    rebuilt = cloud_of(twice)                                                            # another scatter order
    d_c, nn_c = rebuilt.query(T(x))
    assert torch.equal(d_a, d_c) and torch.equal(nn_a, nn_c)
    d_1, nn_1 = cloud_of(arrays).query(T(x))
    assert torch.equal(d_1, d_a)
    perm = np.random.default_rng(7).permutation(M)
    d_p, nn_p = cloud_of((ref_x[perm], ref_rgb[perm], ref_dirs[perm])).query(T(x))
    assert torch.equal(d_p, d_1)
    back = np.where(N(nn_p) >= 0, perm[np.maximum(N(nn_p), 0)], -1)
    assert np.array_equal(back, N(nn_1))


def test_query_equals_min_dist_to_points():
    from laenerf_amd.editing.edit_dataset import min_dist_to_points
    arrays, _, _ = case("3001x4099")
    d, _ = cloud_of(arrays).query(T(arrays[3]))
    want, _ = min_dist_to_points(T(arrays[3]), T(arrays[0]), RADIUS)
    assert torch.allclose(d, want, rtol=1e-6, atol=0) and (d < 0.1).float().mean() > 0.9


@settings(max_examples=50, **FUZZ)
@given(st.integers(1, 3000), st.integers(1, 3000), st.floats(0.02, 0.3), st.tuples(*[st.floats(-10, 10)] * 3), st.floats(0.05, 2.0),
       st.integers(0, 2 ** 31), st.booleans())
def test_fuzz_chosen_is_a_nearest(M, n, radius, offset, spread, seed, surface):
    """random sizes, radii, offsets and extents (clouds of one cell up to the cell cap): the chosen point is a nearest one"""
    from laenerf_amd.editing import RefCloud
    rng = np.random.default_rng(seed)
    draw = (lambda k: unit(rng.standard_normal((k, 3))) * (1 + 0.02 * rng.standard_normal((k, 1)))) if surface else \
        (lambda k: rng.random((k, 3)) * 2 - 1)
    off = np.asarray(offset)
    ref_x, x = (draw(M) * spread + off).astype(np.float32), (draw(n) * spread * 1.1 + off).astype(np.float32)
    best, _, _ = brute_force(ref_x, x)
    cloud = RefCloud(T(ref_x), T(ref_x), T(ref_x), radius=radius)
    d, nn = cloud.query(T(x), mode="binned" if seed % 4 else "gather")
    check_query(ref_x, x, N(d), N(nn), best, radius=radius, exact_threshold=False)


# ------------------------------------------------------------------------------------------------ end to end on a small scene
def poses_looking_at_origin(n, radius, seed):
    """tests/test_gpu_edit_dataset.py's helper"""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        p = rng.standard_normal(3); p = p / np.linalg.norm(p) * radius
        f = -p / np.linalg.norm(p)
        up = np.array([0, 0, 1.0]) if abs(f[2]) < 0.9 else np.array([0, 1.0, 0])
        r = np.cross(up, f); r /= np.linalg.norm(r)
        u = np.cross(f, r)
        P[i, :3, 0], P[i, :3, 1], P[i, :3, 2], P[i, :3, 3], P[i, 3, 3] = r, u, f, p, 1
    return P


def test_reference_view_stylization_end_to_end():
    """extract_ref_cloud -> register_views on the synthetic sphere scene: every view's registration equals the float64 restatement
    on the view's own rows; the template's own view registers onto itself; the views train through EditSet / StyleTrainer"""
    from test_gpu_frame import make
    from laenerf_amd.editing import EditSet, LAENeRF, StyleTrainer, extract_ref_cloud, ray_registration_numpy, register_views
    net, r = make(bound=1, seed=2)
    H = W = 96
    intr = np.array([133.3, 133.3, 48.0, 48.0], np.float32)
    P = poses_looking_at_origin(3, 3.2, seed=1)
    P[1, :3, 3] = P[0, :3, 3] + 0.3 * P[0, :3, 0]                    # view 1: the template's camera moved sideways, still looking along f
    P[1, :3, :3] = P[0, :3, :3]
    poses = T(P)
    r.density_scale = 30.0                                           # opaque surfaces
    g = torch.Generator().manual_seed(3)
    images = torch.rand(3, H, W, 4, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = (((yy - 48) ** 2 + (xx - 48) ** 2) < 30 ** 2).to(DEV)
    images[..., 3] = torch.where(inside, images[..., 3] * 0.5 + 0.5, torch.zeros_like(images[..., 3]))
    painted = torch.rand(H, W, 4, generator=g).to(DEV)
    torch.manual_seed(11)
    cloud = extract_ref_cloud(r, poses[0], intr, H, W, painted, images[0, ..., 3], n_jitter=2)
    K = int(inside.sum())
    assert cloud.M == 3 * K
    assert torch.equal(cloud.rgb[:K], (painted[..., :3] * painted[..., 3:]).reshape(-1, 3)[inside.reshape(-1)])
    assert torch.equal(cloud.rgb[:K], cloud.rgb[K:2 * K]) and not torch.equal(cloud.dirs[:K], cloud.dirs[K:2 * K])     # jittered directions
    views, skipped = register_views(r, poses, intr, H, W, images, cloud, REG_DIST, MIN_TV, batch_views=2)
    assert skipped == [] and [v["pose_idx"] for v in views] == [0, 1, 2]
    radius = float(np.float32(RADIUS))
    registered = 0
    for v in views:
        x, dirs = N(v["x_term"]), N(v["dirs"])
        assert x.shape == (K, 3) and torch.equal(v["indices"], inside.reshape(-1).nonzero(as_tuple=True)[0])
        tg = images[v["pose_idx"]].reshape(-1, 4)[v["indices"]]
        assert torch.equal(v["targets"], tg[:, :3] * tg[:, 3:])
        res = ray_registration_numpy(N(cloud.points), N(cloud.rgb), N(cloud.dirs), x, dirs, reg_dist=REG_DIST, radius=RADIUS, min_tv_factor=MIN_TV)
        want = np.minimum(res["min_dist_unclamped"], radius)
        assert (np.abs(N(v["min_dist"]) - want) <= 1e-6 * want).all()
        clear = np.abs(res["min_dist_unclamped"] / float(np.float32(REG_DIST)) - 1) > THRESHOLD_MARGIN
        got_mask = np.zeros(K, bool)
        got_mask[N(v["indices_ray_reg"])] = True
        assert np.array_equal(got_mask[clear], res["mask"][clear]) and (~clear).sum() <= 2
        same = got_mask & res["mask"]
        rows = np.nonzero(same)[0]
        pos_g, pos_r = np.searchsorted(N(v["indices_ray_reg"]), rows), np.searchsorted(res["indices_ray_reg"], rows)
        wb = weight_bound(res["min_dist"], res["mask"])
        if v["pose_idx"] != 0 and rows.size:
            agree = np.array_equal(N(v["ref_targets"])[pos_g], res["targets"][pos_r].astype(np.float32))
            assert agree                                                                 # the same neighbours (no ties off the template)
            assert np.abs(N(v["target_weights"])[pos_g] - res["target_weights"][pos_r]).max() <= wb
        # the style guide, scattered into the crop
        x0, x1, y0, y1 = (int(t) for t in v["cut_min_max_xy"])
        full = np.zeros(H * W)
        full[N(v["indices"])] = res["style_guide"]
        assert np.abs(N(v["style_guide"]) - full.reshape(H, W)[x0:x1, y0:y1]).max() <= guide_bound()
        assert v["style_guide"].shape == v["cut_gt"].shape[:2]
        registered += v["indices_ray_reg"].numel()
    assert views[1]["indices_ray_reg"].numel() > 50                   # the neighbouring view sees the painted surface
    # the template's own view, rendered with the same flags and the same seed as the cloud's first render: registered onto itself
    torch.manual_seed(11)
    (own,), none = register_views(r, poses[:1], intr, H, W, images[:1], cloud, REG_DIST, MIN_TV)
    assert none == [] and torch.equal(own["x_term"], cloud.points[:K])
    assert (own["min_dist"] == 0).all() and own["indices_ray_reg"].numel() == K and (own["target_weights"] == 1).all()
    hit = (own["weights_densitygrid"][own["indices"]] > 0.5)
    assert hit.sum() > 100 and torch.equal(own["ref_targets"][hit], cloud.rgb[:K][hit])
    # the first stage: the palette network on the unedited views through the existing trainer
    es = EditSet.from_views(views, image_hw=(H, W), device=DEV)
    params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(0)
    m = LAENeRF(params, dir_encoding="sphere_harmonics").to(DEV)
    tr = StyleTrainer(m, es, params, iters=16, distill_palette_steps=-1, seed=1)
    tr.train(16)
    assert tr.global_step == 16 and es.V == 3
    # an empty mask: the view is skipped
    blank = images.clone()
    blank[1, ..., 3] = 0
    v2, sk = register_views(r, poses[:2], intr, H, W, blank[:2], cloud, REG_DIST, MIN_TV)
    assert sk == [1] and len(v2) == 1
