"""Inputs and float64 helpers shared by test_rayreg_cpu.py, test_gpu_rayreg.py and tests/golden/make_golden_rayreg.py."""
import numpy as np

GOLDEN_SHAPE = (500, 300)                  # (M, n) of tests/golden/rayreg_case.npz
GOLDEN_SEEDS = range(64)                   # the generator records the first one that is clear of every threshold and tie
REG_DIST, RADIUS, MIN_TV = 2e-2, 0.1, 0.1
THRESHOLD_MARGIN, GAP_MARGIN = 2e-6, 4e-6  # relative: no row this close to reg_dist / radius, no best / second-best gap this small


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def surface_case(M, n, seed, sphere=0.5, noise=4e-3):
    """cloud and queries on a noisy sphere surface (what termination points of an object look like), painted colours and unit view
    directions, all fp32: ref_x, ref_rgb, ref_dirs [M,3], x, dirs [n,3]"""
    rng = np.random.default_rng([int(seed), int(M), int(n)])
    on = lambda k: unit(rng.standard_normal((k, 3))) * (sphere + noise * rng.standard_normal((k, 1)))
    ref_x, x = on(M), on(n)
    ref_rgb = rng.random((M, 3))
    ref_dirs, dirs = unit(rng.standard_normal((M, 3))), unit(rng.standard_normal((n, 3)))
    return tuple(a.astype(np.float32) for a in (ref_x, ref_rgb, ref_dirs, x, dirs))


def brute_force(ref_x, x, chunk=512):
    """float64: per query the smallest and second smallest distance to the cloud and the index of the smallest (inf / -1 without
    points; the second is inf for M < 2)"""
    ref_x, x = np.asarray(ref_x, np.float64), np.asarray(x, np.float64)
    n, M = x.shape[0], ref_x.shape[0]
    best, second, arg = np.full(n, np.inf), np.full(n, np.inf), np.full(n, -1, np.int64)
    if M == 0:
        return best, second, arg
    for i0 in range(0, n, chunk):
        diff = x[i0:i0 + chunk, None, :] - ref_x[None]
        d = np.sqrt((diff * diff).sum(-1))
        j = d.argmin(1)
        rows = np.arange(d.shape[0])
        best[i0:i0 + chunk], arg[i0:i0 + chunk] = d[rows, j], j
        if M > 1:
            d[rows, j] = np.inf
            second[i0:i0 + chunk] = d.min(1)
    return best, second, arg


def separation(best, second, reg_dist=REG_DIST, radius=RADIUS):
    """(smallest relative distance of a row's minimum from reg_dist and radius, smallest relative best / second-best gap among the
    rows whose minimum lies within radius) in float64 -- what a comparison of indices and masks with fp32 arithmetic hinges on"""
    reg_dist, radius = float(np.float32(reg_dist)), float(np.float32(radius))
    thr = min(np.abs(best / reg_dist - 1).min(), np.abs(best / radius - 1).min()) if best.size else np.inf
    near = best < radius
    gap = ((second[near] - best[near]) / np.maximum(best[near], 1e-300)).min() if near.any() else np.inf
    return float(thr), float(gap)


def chosen_distance(ref_x, x, nn):
    """float64 distance of every row to the cloud point nn chose (inf where nn < 0)"""
    ref_x, x, nn = np.asarray(ref_x, np.float64), np.asarray(x, np.float64), np.asarray(nn, np.int64)
    out = np.full(x.shape[0], np.inf)
    ok = nn >= 0
    out[ok] = np.linalg.norm(x[ok] - ref_x[nn[ok]], axis=1)
    return out


def weight_bound(min_dist, mask):
    """8 * 2^-24 * (dmax / (dmax - dmin) + 1) over the registered rows (float64 values): d carries about 3.5 * 2^-24 relative error
    from the fp32 squared distance and its root, the normalised term amplifies the two ends' errors by dmax / (dmax - dmin), and the
    direction factor adds its own rounding"""
    d = np.asarray(min_dist, np.float64)[mask]
    if d.size == 0 or d.max() == d.min():
        return 8 * 2.0 ** -24
    return 8 * 2.0 ** -24 * (d.max() / (d.max() - d.min()) + 1)


def guide_bound(radius=RADIUS, guide_min=REG_DIST):
    return 8 * 2.0 ** -24 * radius / (radius - guide_min)


def check_against_golden(g, res, min_dist, mask, targets, weights, guide):
    """what every implementation owes the fixture: mask, indices and targets exactly, the clamped distance to relative 1e-6,
    weights and guide within rayreg_util's bounds (computed from the float64 restatement `res`)"""
    radius, reg, tv = float(g["radius"]), float(g["reg_dist"]), float(g["min_tv_factor"])
    assert np.array_equal(np.nonzero(mask)[0], g["mask_dist"]) and g["mask_dist"].size > 20
    assert np.array_equal(np.asarray(targets, np.float32), g["target"])
    want_d = np.minimum(g["min_dist"].astype(np.float64), np.float32(radius))
    assert np.abs(min_dist - want_d).max() <= 1e-6 * radius and (np.abs(min_dist - want_d) <= 1e-6 * want_d + 1e-12).all()
    wb = weight_bound(res["min_dist"], res["mask"])
    assert np.abs(np.asarray(weights, np.float64) - g["target_weights"]).max() <= wb
    # the caller's lines :230-232 on the reference's own distances
    ref_guide = np.maximum(tv, (np.clip(g["min_dist"].astype(np.float64), reg, radius) - reg) / (radius - reg))
    assert np.abs(np.asarray(guide, np.float64) - ref_guide).max() <= guide_bound(radius, reg)
