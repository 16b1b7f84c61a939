"""Exposure / white-balance refinement, the CPU half: the float64 restatements of laenerf_amd/exposure.py against central differences of
the float64 loss, the publish step's centring, the skip / no-ray / non-finite rules, the perturbation helper and the four symbols of the
C ABI."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from laenerf_amd import exposure as E

LN2 = float(np.log(2.0))
DELTA = 0.1


def _batch(seed, n_img=4, hw=50, N=64, with_alpha=True):
    """a batch whose residuals keep clear of the criteria's kinks: |pred - gt| in [0.02, 0.08] or [0.12, 0.5], so a gain step of 1e-4
    (it moves gt by less than 1e-4) crosses neither 0 nor Huber's delta = 0.1"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, n_img, N)
    inds = img * hw + rng.integers(0, hw, N)
    colour = rng.uniform(0.1, 0.9, (N, 3))
    a = rng.uniform(0.2, 1.0, (N, 1)) if with_alpha else np.ones((N, 1))
    fg = colour * a
    rest = rng.uniform(0, 1, (N, 3)) * (1 - a)
    gt = fg + rest
    mag = np.where(rng.random((N, 3)) < 0.5, rng.uniform(0.02, 0.08, (N, 3)), rng.uniform(0.12, 0.5, (N, 3)))
    pred = gt + mag * np.where(rng.random((N, 3)) < 0.5, -1.0, 1.0)
    plane = rng.uniform(0.25, 2.0, n_img * hw)
    return dict(img=img, inds=inds, fg=fg, rest=rest, gt=gt, pred=pred, plane=plane, n_img=n_img, hw=hw, N=N)


def _elem(kind, a, den):
    """the criteria's element loss in float64 for the residual a; den: MAPE's detached denominator |gt| + 0.01"""
    r = np.abs(a)
    if kind == "mse":
        return a * a
    if kind == "l1":
        return r
    if kind == "huber":
        return np.where(r > DELTA, r - 0.5 * DELTA, (0.5 / DELTA) * r * r)
    return r / den


def _loss(b, kind, w2, shift):
    """mean over the 3 N elements of w^2 * crit(pred - gt(e)), gt(e) = fg * 2^shift + rest; shift [N,3], the log2 gain of each
    element on top of the batch's"""
    gt = b["fg"] * np.exp2(shift) + b["rest"]
    den = np.abs(b["gt"]) + np.float64(np.float32(1e-2))                      # detached: the unshifted target's
    terms = w2[:, None] * _elem(kind, b["pred"] - gt, den)
    return terms.sum() / (3 * b["N"]), np.abs(terms).sum() / (3 * b["N"])


def _third_derivative_bound(b, kind, w2):
    """a bound on |d^3 L / d e^3| along any of the directions used below.  With u = fg * 2^e (u' = ln 2 u) and a = pred - rest the
    element loss is, between its kinks, c (a - u)^2 (MSE: c = 1; Huber's inner branch: c = 1 / (2 delta)) or k |a - u| (L1, Huber's
    outer branch: k = 1; MAPE: k = 1 / den): |((a - u)^2)'''| = ln2^3 |-2 a u + 8 u^2| and ||a - u|'''| = ln2^3 u.  Summed over a ray's
    three channels where the direction moves them together ('gray'), which only adds non-negative terms."""
    u, a = b["fg"], b["pred"] - b["rest"]
    quad = LN2 ** 3 * (2 * np.abs(a) * u + 8 * u * u)
    lin = LN2 ** 3 * u
    den = np.abs(b["gt"]) + 1e-2
    per = {"mse": quad, "l1": lin, "huber": np.maximum(quad * (0.5 / DELTA), lin), "mape": lin / den}[kind]
    return (w2[:, None] * per).sum() / (3 * b["N"])


@pytest.mark.parametrize("mode", ["rgb", "gray"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["mse", "l1", "huber", "mape"])
def test_gradient_matches_central_differences(kind, weighted, mode):
    """G of exposure_step_numpy (elem_dtype float64: residual and derivative in the loss's own precision) against (L(e + h) - L(e - h))
    / (2 h), h = 1e-4, per image and channel ('rgb') or per image with the three channels moved together ('gray').  Expected agreement:
    the central difference's truncation h^2 / 6 * max |L'''| (the bound above, times 1.001 for the change of u over [e - h, e + h]) plus
    its rounding, (3 N + 10) 2^-53 * sum |terms| per evaluation, two evaluations, over 2 h."""
    b = _batch(11 + 7 * weighted + (mode == "gray"))
    h = 1e-4
    w2 = b["plane"][b["inds"]] ** 2 if weighted else np.ones(b["N"])
    z = np.zeros((b["n_img"], 3))
    G = E.exposure_step_numpy(b["pred"], b["gt"], b["fg"], b["inds"], b["hw"], z, z, z, np.zeros(b["n_img"], np.int32),
                              weights=b["plane"] if weighted else None, loss=kind, huber_delta=DELTA, mode=mode, elem_dtype=np.float64,
                              full=True)[4]
    _, labs = _loss(b, kind, w2, np.zeros((b["N"], 3)))
    bound = h * h / 6 * 1.001 * _third_derivative_bound(b, kind, w2) + (3 * b["N"] + 10) * 2.0 ** -53 * labs * 1.001 / h
    worst = 0.0
    for i in range(b["n_img"]):
        sel = (b["img"] == i)[:, None]
        assert sel.any()
        for c in range(3):
            d = np.zeros((b["N"], 3))
            if mode == "gray":
                d[:] = sel
            else:
                d[:, c] = sel[:, 0]
            fd = (_loss(b, kind, w2, h * d)[0] - _loss(b, kind, w2, -h * d)[0]) / (2 * h)
            err = abs(G[i, c] - fd)
            worst = max(worst, err / bound)
            assert err <= bound, (i, c, G[i, c], fd, err, bound)
            assert abs(fd) > 100 * bound                                      # the comparison resolves the gradient
    if mode == "gray":
        assert np.array_equal(G[:, 0], G[:, 1]) and np.array_equal(G[:, 0], G[:, 2])
    print(f"{kind} weighted={weighted} {mode}: worst |G - FD| / bound = {worst:.3f}, bound {bound:.2e}, |G| ~ {np.abs(G).mean():.2e}")


def test_float32_elements_agree_with_float64_ones():
    """the kernel's precision (float32 residual and derivative) moves G by no more than the float32 rounding of the residual allows:
    |dv32 - dv64| <= 2^-23 (1 + 1 / delta) for data of magnitude <= 2 away from the kinks, times w^2 fg ln 2 / (3 N) summed"""
    b = _batch(5)
    z = np.zeros((b["n_img"], 3))
    args = (b["pred"].astype(np.float32), b["gt"].astype(np.float32), b["fg"].astype(np.float32), b["inds"], b["hw"], z, z, z,
            np.zeros(b["n_img"], np.int32))
    for kind in ("mse", "l1", "huber"):
        g32 = E.exposure_step_numpy(*args, loss=kind, huber_delta=DELTA, full=True)[4]
        g64 = E.exposure_step_numpy(*args, loss=kind, huber_delta=DELTA, elem_dtype=np.float64, full=True)[4]
        tol = 2.0 ** -23 * (1 + 1 / DELTA) * 2 * LN2 * np.abs(b["fg"]).sum() / (3 * b["N"])
        assert np.all(np.abs(g32 - g64) <= tol) and np.abs(g64).min() > 0


def test_publish_centres_and_zeros_publish_exact_ones():
    rng = np.random.default_rng(2)
    master = rng.standard_normal((7, 3)) + np.array([3.0, -2.0, 0.5])          # a large common mode per channel
    gains, ex = E.exposure_publish_numpy(master, full=True)
    assert gains.dtype == np.float32 and gains.shape == (7, 3)
    assert np.all(np.abs(ex.mean(0)) <= 1e-15) and np.all(np.abs(ex - (master - master.mean(0))) <= 1e-15)
    assert np.array_equal(gains, np.exp2(ex).astype(np.float32))
    assert np.all(np.abs(np.log2(gains.astype(np.float64)).mean(0)) < 1e-7)    # the gains' geometric mean per channel is 1
    # a common shift of the master changes no gain beyond the rounding of the shift itself
    assert np.all(np.abs(E.exposure_publish_numpy(master + 0.25, full=True)[1] - ex) <= 1e-15)
    raw, ex_raw = E.exposure_publish_numpy(master, center=False, full=True)
    assert np.array_equal(ex_raw, master) and np.array_equal(raw, np.exp2(master).astype(np.float32))
    for n in (1, 5, 300):
        assert E.exposure_publish_numpy(np.zeros((n, 3))).tobytes() == np.ones((n, 3), np.float32).tobytes()
    assert E.exposure_publish_numpy(np.array([[0.7, -1.3, 2.0]])).tobytes() == np.ones((1, 3), np.float32).tobytes()   # n_img = 1


def test_step_rules():
    b = _batch(3, n_img=5)
    img = b["img"].copy()
    img[img == 3] = 2                                                          # image 3 receives no ray
    inds = img * b["hw"] + b["inds"] % b["hw"]
    pred = b["pred"].astype(np.float32)
    pred[np.flatnonzero(img == 1)[0], 1] = np.nan                              # image 1's gradient is not finite
    rng = np.random.default_rng(4)
    master = rng.standard_normal((5, 3)) * 0.1
    master[0, 0] = -0.0
    z, counts = np.zeros((5, 3)), np.zeros(5, np.int32)
    for kind in ("mse", "l1", "huber", "mape"):                                # a NaN residual reaches G under every criterion
        a = E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], master, z, z, counts, loss=kind, lr=1e-2, full=True)
        assert np.isnan(a[4][1, 1]) and np.isfinite(a[4][[0, 2, 4]]).all() and not a[4][3].any()
        for i in (1, 3):
            assert a[0][i].tobytes() == master[i].tobytes() and not a[1][i].any() and not a[2][i].any() and a[3][i] == 0
        for i in (0, 2, 4):
            G = a[4][i]
            assert a[3][i] == 1 and np.allclose(a[1][i], 0.1 * G, rtol=1e-15) and np.allclose(a[2][i], 0.01 * G * G, rtol=1e-14)
            # the first Adam step moves every component by lr against the gradient's sign (eps = 1e-15)
            assert np.allclose(a[0][i] - master[i], -np.float64(np.float32(1e-2)) * np.sign(G), rtol=1e-9)
    g = E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], master, z, z, counts, mode="gray", lr=1e-2, full=True)
    assert np.array_equal(g[4][:, 0], g[4][:, 1], equal_nan=True) and np.all(g[1][:, 0] == g[1][:, 2]) and np.isnan(g[4][1]).all()
    assert np.allclose(g[4][0, 0], a_sum(pred, b, inds, 0), rtol=1e-12)
    # a skipped optimizer step touches nothing; lr = 0 moves no gain and keeps every bit, the signed zero included
    s = E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], master, z, z, counts, skip=True)
    assert s[0].tobytes() == master.tobytes() and not s[1].any() and not s[3].any()
    c = E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], master, z, z, counts, lr=0.0)
    assert c[0].tobytes() == master.tobytes() and c[3].tolist() == [1, 0, 1, 0, 1] and c[1][0].any()
    with pytest.raises(ValueError, match="mode"):
        E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], master, z, z, counts, mode="hsv")


def a_sum(pred, b, inds, i):
    """'gray' G of image i: the sum of the three 'rgb' components"""
    z = np.zeros((5, 3))
    G = E.exposure_step_numpy(pred, b["gt"], b["fg"], inds, b["hw"], z, z, z, np.zeros(5, np.int32), full=True)[4]
    return G[i].sum()


def test_gained_targets_restate_the_blend():
    rng = np.random.default_rng(6)
    f32 = np.float32
    v, a, bg = rng.random((97, 3)).astype(f32), rng.random(97).astype(f32), rng.random((97, 3)).astype(f32)
    gains = rng.uniform(0.5, 2.0, (97, 3)).astype(f32)
    gt1, fg1 = E.gained_targets_numpy(v, np.ones((97, 3), f32), a, bg)
    assert np.array_equal(gt1, v * a[:, None] + bg * (f32(1) - a[:, None])) and np.array_equal(fg1, v * a[:, None])    # today's blend
    gt, fg = E.gained_targets_numpy(v, gains, a, bg)
    assert gt.dtype == f32 and np.array_equal(fg, (v * gains) * a[:, None]) and np.array_equal(gt, fg + bg * (f32(1) - a[:, None]))
    gt3, fg3 = E.gained_targets_numpy(v, gains)
    assert np.array_equal(gt3, v * gains) and np.array_equal(fg3, gt3)
    gtw, _ = E.gained_targets_numpy(v, gains, a, 1.0)
    assert np.array_equal(gtw, fg + (f32(1) - a[:, None]))


def test_perturb_exposures():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (6, 4, 5, 4), dtype=np.uint8)
    out, u = E.perturb_exposures(img, 0.5, seed=3)
    assert out.dtype == np.float32 and u.shape == (6, 3) and np.all(np.abs(u.mean(0)) < 1e-15)
    assert np.array_equal(u[:, 0], u[:, 1]) and 0.1 < np.abs(u).max() <= 1.0
    base = img.astype(np.float32) / np.float32(255)
    assert np.array_equal(out[..., 3], base[..., 3])
    assert np.array_equal(out[..., :3], base[..., :3] * np.exp2(u).astype(np.float32)[:, None, None, :])
    assert out[..., :3].max() > 1.0                                            # nothing clips
    out2, u2 = E.perturb_exposures(base, 0.5, seed=3, wb_stops=0.2)
    assert not np.array_equal(u2[:, 0], u2[:, 1]) and np.all(np.abs(u2.mean(0)) < 1e-15)
    assert np.array_equal(E.perturb_exposures(base, 0.5, seed=3)[0], out)


NAMES = ("lae_sample_train_batch_gain", "lae_sample_train_batch_weighted_gain", "lae_exposure_step", "lae_exposure_publish")


def test_abi_has_the_four_symbols():
    from laenerf_amd import _lib
    from laenerf_amd import build as B
    hdr = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    for name in NAMES:
        assert re.search(r"LAE_API\s+int\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
        proto = re.search(name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    # the gained samplers take two more arguments than their siblings, whose prototypes stand as they were
    for name, base in ((NAMES[0], "lae_sample_train_batch"), (NAMES[1], "lae_sample_train_batch_weighted")):
        assert len(_lib.SIGNATURES[name]) == len(_lib.SIGNATURES[base]) + 2
    assert "exposure.hip" in B.SOURCES and os.path.exists(os.path.join(B.CSRC, "exposure.hip"))
    tag = re.search(r'#define LAE_ABI_TAG "(abi\d+)"', hdr).group(1)
    assert tag.encode() == _lib.ABI_TAG and int(tag[3:]) >= 25


def test_bad_arguments_are_refused_before_a_launch(hip_lib):
    one = 16
    step = lambda **kw: hip_lib.lae_exposure_step(
        kw.get("pred", one), one, one, one, kw.get("N", 4), kw.get("hw", 16), kw.get("n_img", 2), kw.get("w", None), kw.get("wd", 0),
        kw.get("kind", 0), kw.get("param", 0.0), 0, kw.get("master", one), one, one, one, one, one, kw.get("b1", 0.9), 0.99, 1e-15, None)
    assert step(n_img=0) == 0
    assert step(hw=0) == -1 and step(b1=1.0) == -1 and step(kind=4) == -1 and step(kind=2, param=0.0) == -1
    assert step(w=one, wd=0) == -1                                             # a uint8 weight plane
    assert step(pred=None) == -3 and step(master=None) == -3
    assert hip_lib.lae_exposure_publish(one, 0, 1, one, None) == 0
    assert hip_lib.lae_exposure_publish(None, 3, 1, one, None) == -3 and hip_lib.lae_exposure_publish(one, 3, 1, None, None) == -3
    # the gained samplers refuse a missing gains / fg before anything else
    args = [one, 0, 2, 4, 4, 3, one, 1.0, 1.0, 2.0, 2.0, 8, one, 0.2, 0, one, 0, 0, 0]
    tail = [one] * 5
    assert hip_lib.lae_sample_train_batch_gain(*args, None, *tail, one, one, one, None) == -3
    assert hip_lib.lae_sample_train_batch_gain(*args, one, *tail, None, one, one, None) == -3
