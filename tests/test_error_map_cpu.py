"""The error-map sampler's rules restated in numpy (laenerf_amd.data: neg_log_u, draw_cells, cell_pixels, ema_update) against
float64, exact probabilities, torch.multinomial, the reference's own get_rays (tests/golden/error_map_rays.npz) and its
EMA expressions; ResidentImages' argument checks.  No GPU needed."""
import itertools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "error_map_rays.npz")


def test_log_meets_2_pow_minus_20_on_every_input():
    from laenerf_amd.data import neg_log_u
    worst = 0.0
    for lo in range(0, 1 << 24, 1 << 22):
        k = np.arange(lo, lo + (1 << 22), dtype=np.int64)
        E = neg_log_u(2 * k + 1).astype(np.float64)
        ref = -np.log((k + 0.5) * 2.0 ** -24)
        assert (E > 0).all()
        worst = max(worst, float(np.max(np.abs(E - ref) / ref)))
    print("neg_log_u: worst relative error", worst, "=", np.log2(worst), "bits")
    assert worst <= 2.0 ** -20


def _set_probabilities(w, n):
    """exact probabilities of every n-set under successive sampling without replacement (sum over draw orders)"""
    w = np.asarray(w, np.float64)
    probs = {}
    for order in itertools.permutations(range(len(w)), n):
        p, left = 1.0, w.sum()
        for c in order:
            p *= w[c] / left
            left -= w[c]
        key = tuple(sorted(order))
        probs[key] = probs.get(key, 0.0) + p
    return probs


def _chi2(counts, probs, total):
    x = 0.0
    for key, p in probs.items():
        if p > 0:
            e = p * total
            x += (counts.get(key, 0) - e) ** 2 / e
    return x


@pytest.mark.parametrize("w,n", [([1, 2, 3, 4], 2), ([0.5, 1, 1, 4, 8], 2), ([3, 1, 0.25, 2, 5, 1], 3), ([1, 1, 1, 1, 1], 3)])
def test_restated_draw_follows_the_without_replacement_law(w, n):
    from laenerf_amd.data import draw_cells
    S = 40000
    cells = draw_cells(1234, np.arange(S)[:, None], np.array(w, np.float32), n)
    assert (np.diff(cells, axis=-1) > 0).all()                        # distinct, increasing
    counts = {}
    for row in map(tuple, cells.tolist()):
        counts[row] = counts.get(row, 0) + 1
    probs = _set_probabilities(w, n)
    x, dof = _chi2(counts, probs, S), len(probs) - 1
    print("law", w, n, "chi2", x, "dof", dof)
    assert x < dof + 8 * np.sqrt(2 * dof)                              # deterministic draws: a fixed threshold, no flakiness


@pytest.mark.parametrize("w,n", [([1, 2, 3, 4, 10], 2), ([0.5, 1, 1, 4, 8, 2], 3)])
def test_restated_draw_matches_torch_multinomial(w, n):
    from laenerf_amd.data import draw_cells
    S = 40000
    ours = draw_cells(99, np.arange(S)[:, None], np.array(w, np.float32), n)
    g = torch.Generator().manual_seed(5)
    theirs = np.sort(torch.multinomial(torch.tensor(w, dtype=torch.float32).expand(S, len(w)), n, replacement=False,
                                       generator=g).numpy(), axis=-1)
    keys = sorted(set(map(tuple, ours.tolist())) | set(map(tuple, theirs.tolist())))
    a = np.array([np.sum((ours == k).all(-1)) for k in keys], np.float64)
    b = np.array([np.sum((theirs == k).all(-1)) for k in keys], np.float64)
    x = float((((a - b) ** 2) / (a + b)).sum())                         # two-sample chi-square, equal sample sizes
    dof = len(keys) - 1
    assert x < dof + 8 * np.sqrt(2 * dof), (x, dof)


def test_ties_and_zero_weights():
    from laenerf_amd.data import cell_keys, draw_cells
    w = np.zeros(16384, np.float32)
    assert np.array_equal(draw_cells(3, 7, w, 5), np.arange(5))                    # all zero: the lowest cells
    w[[100, 9000]] = 1.0
    assert np.array_equal(draw_cells(3, 7, w, 4), [0, 1, 100, 9000])                # positive first, then zeros from 0
    w[[5, 6]] = [-1.0, np.nan]
    w[7] = np.inf
    assert (cell_keys(3, 7, w)[[5, 6, 7]] == 0).all()                               # negative, NaN, inf count as 0
    assert np.array_equal(draw_cells(3, 7, w, 4), [0, 1, 100, 9000])
    big = np.full(16384, 3e38, np.float32)                     # every key with E < 1 overflows to +inf: thousands tie
    inf = np.flatnonzero(cell_keys(3, 7, big) == 0x7F800000)
    assert len(inf) > 1000
    assert np.array_equal(draw_cells(3, 7, big, 6), inf[:6])
    assert np.array_equal(draw_cells(3, 7, np.ones(16384, np.float32), 16384), np.arange(16384))


def test_reference_pixels_lie_in_the_cell_span():
    from laenerf_amd.data import cell_pixels, cell_span
    g = np.load(GOLDEN)
    for tag in ("small", "wide", "square", "odd"):
        H, W, N = (int(v) for v in g[f"{tag}_cfg"])
        inds, coarse, emap = g[f"{tag}_inds"], g[f"{tag}_inds_coarse"], g[f"{tag}_map"]
        for b in range(inds.shape[0]):
            assert (emap[b][coarse[b]] > 0).all()
            r0, r1, c0, c1 = cell_span(coarse[b], H, W)
            row, col = inds[b] // W, inds[b] % W
            assert ((r0 <= row) & (row <= r1) & (c0 <= col) & (col <= c1)).all(), tag
            mine = cell_pixels(17, 3, coarse[b], H, W)
            mr, mc = mine // W, mine % W
            assert ((r0 <= mr) & (mr <= r1) & (c0 <= mc) & (mc <= c1)).all() and (mine < H * W).all()


def test_ema_update_within_one_ulp_of_the_reference_expressions():
    from laenerf_amd.data import ema_update
    rng = np.random.default_rng(4)
    n_img, H, W, N = 3, 40, 30, 2000
    emap = rng.random((n_img, 16384), dtype=np.float32) * 2
    img = 1
    cells = rng.choice(16384, N, replace=False)
    inds = img * H * W + rng.integers(0, H * W, N)
    pred = rng.random((N, 3), dtype=np.float32)
    gt = rng.random((N, 3), dtype=np.float32)
    got = ema_update(emap, inds, cells, pred, gt, H, W)
    # nerf/utils.py:597 (criterion MSELoss(reduction='none')).mean(-1) and :609-631, in torch on the CPU
    t = torch.from_numpy(emap.copy())
    error = torch.nn.MSELoss(reduction="none")(torch.from_numpy(pred), torch.from_numpy(gt)).mean(-1)[None]
    em = t[[img]]
    ci = torch.from_numpy(cells)[None]
    em.scatter_(1, ci, 0.1 * em.gather(1, ci) + 0.9 * error)
    t[[img]] = em
    want = t.numpy()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1
    untouched = np.ones_like(got, bool)
    untouched[img, cells] = False
    assert np.array_equal(got[untouched], emap[untouched])


def test_resident_images_validates_error_map_arguments():
    from laenerf_amd.data import ResidentImages
    img = np.zeros((2, 8, 9, 3), np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    with pytest.raises(ValueError):
        ResidentImages(img, poses, (5, 5, 4, 4), mode="all", error_map=True, device="cpu")
    d = ResidentImages(img, poses, (5, 5, 4, 4), error_map=True, device="cpu")
    assert d.error_map.shape == (2, 16384) and d.error_map.dtype == torch.float32 and (d.error_map == 1).all()
    with pytest.raises(ValueError):
        d.sample(16385)
    with pytest.raises(ValueError):
        d.sample(0)
    d.error_map = torch.ones(2, 128, 128)
    with pytest.raises(ValueError):
        d.sample(16)
    d.error_map = torch.ones(3, 16384)
    with pytest.raises(ValueError):
        d.sample(16)
    assert (d.enable_error_map(0.5) == 0.5).all()
    u = ResidentImages(img, poses, (5, 5, 4, 4), mode="all", device="cpu")
    assert u.error_map is None
    with pytest.raises(ValueError):
        u.enable_error_map()
    with pytest.raises(ValueError):
        u.update_error_map(torch.zeros(4, 3), {})
