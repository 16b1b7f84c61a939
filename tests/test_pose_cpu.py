"""Pose refinement, the CPU half: the float64 restatements of laenerf_amd/poses.py against finite differences and against the oracle's
dy_dx path, Rodrigues' formula, and the three symbols of the C ABI."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from laenerf_amd import poses as P

BASE, LEVELS = 16, 16


def _f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


@pytest.fixture(scope="module")
def grid(O):
    """the shipped level sizes (16 levels, 16 -> 2048, 2^19 entries per hashed level): offsets, log2(per_level_scale), an fp16 table"""
    offsets, pls = O.grid_offsets(desired_resolution=2048)
    rng = np.random.default_rng(7)
    table = _f16(rng.uniform(-1, 1, (int(offsets[-1]), 2)))
    return offsets, pls, np.float32(np.log2(pls)), table


def _interior_points(S, n, seed):
    """float32 points in the unit cube whose fractional coordinate lies in [0.05, 0.95] at every level and on every axis (drawn by
    rejection; 0.9^48 of the draws pass)"""
    rng = np.random.default_rng(seed)
    keep = np.zeros((0, 3), np.float32)
    while keep.shape[0] < n:
        x = rng.uniform(0.02, 0.98, (200000, 3)).astype(np.float32)
        _, _, fr, _ = P.grid_cells_f32(x, LEVELS, S, BASE)
        ok = np.all((fr >= 0.05) & (fr <= 0.95), axis=(0, 2))
        keep = np.concatenate([keep, x[ok]])
    return keep[:n]


def test_grid_input_grad_matches_central_differences(grid):
    """d/dx of sum(features * g) by central differences (step 1e-6 of the unit cube) of the all-float64 forward against the restatement,
    which takes cell and fractional position from the float32 computation.  The trilinear forward is a polynomial of degree one in each
    coordinate, so the central difference along an axis has no truncation error inside a cell.  What separates the two: the float32
    position p = fmaf(x, scale, 0.5) is off by at most ulp(p) / 2 <= (scale + 0.5) 2^-24 =: d_l, so each of the two weights of a term,
    both in [0.05, 0.95] here, is off by at most d_l / 0.05 of itself: |difference| <= sum_l A_l ((1 + d_l / 0.05)^2 - 1), A_l the sum of
    the absolute values of the level's terms; plus the differences' own rounding, 2^-52 (sum |feature g|) * 4 / (2 h)."""
    offsets, pls, S, table = grid
    n, h = 48, 1e-6
    x = _interior_points(S, n, 3)
    assert x.shape == (n, 3)
    _, _, fr, scales = P.grid_cells_f32(x, LEVELS, S, BASE)
    assert np.all((fr >= 0.05) & (fr <= 0.95))                       # no point is left out
    g = _f16(np.random.default_rng(5).uniform(-1, 1, (LEVELS, n, 2)))
    got, A, Al = P.grid_input_grad_numpy(x, table, offsets, g, S, BASE, full=True)
    gd64 = g.astype(np.float64)
    x64 = x.astype(np.float64)
    fd = np.zeros((n, 3))
    fmag = np.abs(P.grid_forward_numpy(x64, table, offsets, S, BASE) * gd64).sum(axis=(0, 2))
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        up = (P.grid_forward_numpy(x64 + e, table, offsets, S, BASE) * gd64).sum(axis=(0, 2))
        dn = (P.grid_forward_numpy(x64 - e, table, offsets, S, BASE) * gd64).sum(axis=(0, 2))
        fd[:, d] = (up - dn) / (2 * h)
    dl = (scales.astype(np.float64) + 0.5) * 2.0 ** -24
    bound = (Al * ((1 + dl / 0.05) ** 2 - 1)[:, None, None]).sum(0) + (2.0 ** -52 * 4 / (2 * h)) * fmag[:, None]
    err = np.abs(got - fd)
    print("max |restatement - FD| =", err.max(), " max bound =", bound.max(), " worst ratio =", (err / bound).max())
    assert np.all(A > 0) and np.all(err <= bound)


@pytest.mark.parametrize("gridtype,align", [(0, False), (1, False), (0, True)])
def test_grid_input_grad_matches_the_oracle_dy_dx_path(O, grid, gridtype, align):
    """the reference's own route -- K13 writes dy_dx, K15 multiplies and sums -- in the oracle's float32 mode, on a table and on
    gradients that hold fp16 values.  Bound: 2^-16 A per output (the kernel's own bound; both sides round each of the 128 terms a handful of
    times and add them in float32 or better)."""
    offsets, pls, S, table = grid
    if align:
        offsets, pls = O.grid_offsets(desired_resolution=2048, align_corners=True)
        table = table[:int(offsets[-1])]
    rng = np.random.default_rng(11)
    n = 200
    x = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    x[:6] = [[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75], [1 / 15, 2 / 15, 1], [0, 1, 0.5], [1, 0, 1 / 3]]
    g = _f16(rng.uniform(-1, 1, (LEVELS, n, 2)))
    _, dy = O.grid_encode_forward(x, table.astype(np.float32), offsets, pls, BASE, calc_dy_dx=True, gridtype=gridtype, align_corners=align)
    _, ref = O.grid_encode_backward(g.astype(np.float32), x, table.shape, offsets, pls, BASE, dy_dx=dy, gridtype=gridtype,
                                    align_corners=align)
    got, A, _ = P.grid_input_grad_numpy(x, table, offsets, g, S, BASE, gridtype=gridtype, align_corners=align, full=True)
    err = np.abs(got - ref.astype(np.float64))
    print("max err / (2^-16 A) =", (err / np.maximum(2.0 ** -16 * A, 1e-300)).max())
    assert np.all(err <= 2.0 ** -16 * A)


def test_grid_input_grad_outside_rows_and_input_map(grid):
    offsets, pls, S, table = grid
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    x[0], x[1], x[2] = [1.0001, 0, 0], [0, -1.5, 0], [0.3, 0.2, -1.001]
    g = _f16(rng.uniform(-1, 1, (LEVELS, 40, 2)))
    in_map = (1.0, 0.5)
    got = P.grid_input_grad_numpy(x, table, offsets, g, S, BASE, in_map=in_map)
    assert np.all(got[:3] == 0) and np.all(np.abs(got[3:]).sum(1) > 0)
    # the map's factor: the same points already mapped, gradient times in_scale
    plain = P.grid_input_grad_numpy((x + np.float32(1)) * np.float32(0.5), table, offsets, g, S, BASE)
    assert np.array_equal(got, plain * 0.5)


def _smooth_loss(x):
    """a smooth scalar field summed over the points, and its gradient per point"""
    k = np.array([1.3, -0.7, 2.1])
    ph = x @ k
    val = np.sin(ph) + 0.5 * (x ** 2).sum(1)
    grad = np.cos(ph)[:, None] * k + x
    return val.sum(), grad


def test_pose_ray_grad_matches_differences_of_the_rigid_motion():
    """L(T + t + Exp(w)(x - T)) differentiated at w = t = 0 by central differences (h = 1e-6: truncation h^2 / 6 |L'''| ~ 1e-12 per
    sample, rounding 2^-52 |L| / h ~ 2e-10 |L|) against out = (sum g, sum (x - T) x g); bound 1e-8 (1 + |L|), two decades above both"""
    rng = np.random.default_rng(4)
    counts = [0, 1, 2, 63, 64, 65, 200]
    N, M = len(counts), sum(counts) + 5
    order = rng.permutation(N)
    rays = np.zeros((N, 3), np.int32)
    off = 0
    for row, c in enumerate(counts):
        rays[row] = (order[row], off, c)
        off += c
    x = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    o = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    got = P.pose_ray_grad_numpy(rays, x, np.zeros((M, 3), np.float32), o)
    assert np.all(got == 0)
    for idx, off, cnt in rays:
        xs, T = x[off:off + cnt].astype(np.float64), o[idx].astype(np.float64)
        L0, g = _smooth_loss(xs) if cnt else (0.0, np.zeros((0, 3)))
        gfull = np.zeros((M, 3), np.float32)
        g32 = g.astype(np.float32)
        gfull[off:off + cnt] = g32
        out = P.pose_ray_grad_numpy(rays, x, gfull, o)
        assert np.all(np.delete(out, idx, axis=0) == 0)
        fd = np.zeros(6)
        h = 1e-6
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            up = _smooth_loss(T + d[:3] + (xs - T) @ P.exp_so3(d[3:]).T)[0] if cnt else 0.0
            dn = _smooth_loss(T - d[:3] + (xs - T) @ P.exp_so3(-d[3:]).T)[0] if cnt else 0.0
            fd[c] = (up - dn) / (2 * h)
        # the restatement sees the float32 gradient; the difference quotient the float64 one
        slack = 2.0 ** -23 * np.concatenate([np.abs(g).sum(0), (np.abs(xs - T).sum(1)[:, None] * np.abs(g)).sum(0) * np.ones(3)]) if cnt else 0
        assert np.all(np.abs(out[idx] - fd) <= 1e-8 * (1 + abs(L0)) + slack), (cnt, out[idx], fd)
    # a ray whose samples do not fit gives zeros
    rays[-1, 2] = M
    gfull = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    assert np.all(P.pose_ray_grad_numpy(rays, x, gfull, o)[rays[-1, 0]] == 0)


def test_exp_so3():
    assert np.array_equal(P.exp_so3([0, 0, 0]), np.eye(3))
    assert np.array_equal(P.exp_so3([-0.0, 0.0, -0.0]), np.eye(3))
    rng = np.random.default_rng(0)
    for s in (1e-9, 1e-7, 1e-3, 0.3, 3.0):
        w = rng.standard_normal(3)
        w *= s / np.linalg.norm(w)
        R = P.exp_so3(w)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15
        assert np.abs(np.linalg.det(R) - 1) < 1e-15
        assert np.allclose(R @ w, w, rtol=0, atol=1e-15 * s)                  # the axis is fixed
    # the two branches at the switch, t^2 = 1e-12: the series' first neglected terms are t^4 / 120 and t^4 / 720 (1e-26); the closed
    # form's 1 - cos t is off by up to an ulp of 1, 2^-53, which B K^2 = (1 - cos t) / t^2 * K^2 passes on undiminished (|K^2| <= t^2)
    ax = np.array([0.6, -0.48, 0.64])
    below, above = P.exp_so3(ax * np.nextafter(1e-6, 0)), P.exp_so3(ax * np.nextafter(1e-6, 1))
    assert (ax * np.nextafter(1e-6, 0)) @ (ax * np.nextafter(1e-6, 0)) < 1e-12 <= (ax * np.nextafter(1e-6, 1)) @ (ax * np.nextafter(1e-6, 1))
    assert np.abs(below - above).max() <= 2.0 ** -52
    ang, dist = P.pose_error(np.stack([np.c_[P.exp_so3(ax * 0.01), [1, 2, 3]]]), np.stack([np.c_[np.eye(3), [1, 2, 2]]]))
    assert abs(ang[0] - 0.01) < 1e-15 and dist[0] == 1.0


def test_pose_step_numpy_rules():
    rng = np.random.default_rng(1)
    n_img, hw, N = 5, 100, 64
    master = np.concatenate([np.stack([P.exp_so3(rng.standard_normal(3)) for _ in range(n_img)]), rng.standard_normal((n_img, 3, 1))], 2)
    master[0, 0, 3] = -0.0
    master = master.reshape(n_img, 12)
    m, v, counts = np.zeros((n_img, 6)), np.zeros((n_img, 6)), np.zeros(n_img, np.int32)
    img = rng.integers(0, n_img, N)
    img[img == 3] = 2                                                          # image 3 receives no ray
    inds = img * hw + rng.integers(0, hw, N)
    rg = rng.standard_normal((N, 6))
    rg[np.flatnonzero(img == 1)[0], 2] = np.nan                                # image 1's gradient is not finite
    a = P.pose_step_numpy(rg, inds, hw, master, m, v, counts, inv_scale=0.5, lr=1e-2)
    for i in (1, 3):
        assert a[0][i].tobytes() == master[i].tobytes() and not a[1][i].any() and not a[2][i].any() and a[3][i] == 0
    for i in (0, 2, 4):
        assert a[3][i] == 1
        g = rg[img == i].sum(0) * 0.5
        assert np.allclose(a[1][i], 0.1 * g, rtol=1e-15) and np.allclose(a[2][i], 0.01 * g * g, rtol=1e-14)
        # the first Adam step moves every component by lr against the gradient's sign (eps = 1e-15)
        assert np.allclose(a[0][i].reshape(3, 4)[:, 3] - master[i].reshape(3, 4)[:, 3], -np.float32(1e-2) * np.sign(g[:3]), rtol=1e-9)
        R0, R1 = master[i].reshape(3, 4)[:, :3], a[0][i].reshape(3, 4)[:, :3]
        assert np.allclose(R1 @ R0.T, P.exp_so3(-np.float64(np.float32(1e-2)) * np.sign(g[3:])), atol=1e-12)
    assert np.array_equal(a[4], a[0].astype(np.float32))
    # a skipped optimizer step touches nothing; lr = 0 moves no pose and keeps every bit, signed zeros included
    b = P.pose_step_numpy(rg, inds, hw, master, m, v, counts, skip=True)
    assert b[0].tobytes() == master.tobytes() and not b[1].any() and not b[3].any()
    c = P.pose_step_numpy(rg, inds, hw, master, m, v, counts, lr=0.0)
    assert c[0].tobytes() == master.tobytes() and c[3].tolist() == [1, 0, 1, 0, 1]


def test_abi_has_the_three_symbols():
    from laenerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    for name in ("lae_grid_input_grad", "lae_pose_ray_grad", "lae_pose_step"):
        assert re.search(r"LAE_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    # header and table agree on the argument counts
    for name in ("lae_grid_input_grad", "lae_pose_ray_grad", "lae_pose_step"):
        proto = re.search(name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name


def test_unsupported_configurations_are_refused_before_a_launch(hip_lib):
    one = 16
    ok = dict(M=4, D=3, C=2, L=16, gridtype=0, interp=0, dtype=1)

    def call(**kw):
        a = {**ok, **kw}
        return hip_lib.lae_grid_input_grad(one, one, one, one, one, a["M"], a["D"], a["C"], a["L"], 0.5, 16, a["gridtype"], 0, a["interp"],
                                           a["dtype"], 0.0, 1.0, None)
    assert call(D=2) == -1 and call(C=4) == -1 and call(L=0) == -1 and call(L=33) == -1
    assert call(gridtype=2) == -1 and call(interp=1) == -1 and call(dtype=0) == -1
    assert call(M=0) == 0
    assert hip_lib.lae_grid_input_grad(None, one, one, one, one, 4, 3, 2, 16, 0.5, 16, 0, 0, 0, 1, 0.0, 1.0, None) == -3
    assert hip_lib.lae_pose_ray_grad(None, None, None, None, 0, 0, None, None) == 0
    assert hip_lib.lae_pose_ray_grad(None, one, one, one, 4, 4, one, None) == -3
    assert hip_lib.lae_pose_step(one, one, 4, 0, 2, one, one, one, one, one, one, one, 0.9, 0.99, 1e-15, None) == -1     # hw = 0
    assert hip_lib.lae_pose_step(one, one, 4, 16, 2, None, one, one, one, one, one, one, 0.9, 0.99, 1e-15, None) == -3
