"""metrics.consistency_numpy, the float64 restatement of lae_consistency_pair, on its own: closed-form cases, the two-view fixture
of tests/consistency_util.py, undefined inputs.  tests/test_gpu_consistency.py holds the kernel against this restatement.

Figures of the restatement on the fixture (float64 unless noted):

                                              24 x 40         37 x 53
    valid pixels                              710 of 960      1600 of 1961
    invalid, by the first reason that applies
      no geometry at the pixel (rows 0-1)     80              106
      lands outside the frame                 103             175
      a tap without geometry                  0               3
      motion-boundary rule                    55              55
      occlusion rule                          12              22
    warp_mse over the valid pixels            6.35e-5         2.03e-4
    ... with both rules ignored               9.29e-4         7.33e-4
    smallest margin                           1.09e-2         2.8e-3
    float32 run: decisions                    as float64      as float64
    float32 flow - float64 flow, max          6.7e-6 px       8.6e-6 px
    float32 warped - float64 warped, max      2.83e-7         2.93e-7      (MEASURED_W below; the GPU tolerance is 8 x that)
"""
import warnings

import numpy as np
import pytest

import consistency_util as U

MEASURED_W = 3.0e-7          # max |float32 restatement - float64 restatement| of the warped colour on the fixture, rounded up
MARGIN = 1e-3                # exclusion band of the validity comparison: over a hundred times the float32 flow error above
MARGIN_CAP = 0.02            # at most this share of the pixels may lie inside the band


def _cn(*a, **k):
    from laenerf_amd.metrics import consistency_numpy
    return consistency_numpy(*a, **k)


def _plane(H, W, Z, Pa, Pb, texture):
    """a fronto-parallel plane z = Z seen by two cameras that look along +z, in float64"""
    out = []
    for P in (Pa, Pb):
        gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        d = np.stack([(gx + 0.5 - W / 2) / U.FOCAL, (gy + 0.5 - H / 2) / U.FOCAL, np.ones_like(gx)], -1)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = (Z - P[2, 3]) / d[..., 2]
        X = P[:3, 3] + t[..., None] * d
        out.append((texture(X[..., 0], X[..., 1]), t, np.ones((H, W))))
    (Fa, Da, Aa), (Fb, Db, Ab) = out
    return Fa, Fb, Da, Aa, Db, Ab, Pa, Pb, (U.FOCAL, U.FOCAL, W / 2, H / 2), H, W


def test_plane_sideways_translation_constant_flow_and_shifted_texture():
    H, W, Z, bx = 12, 20, 4.0, 0.25
    Pa, Pb = np.eye(4), np.eye(4)
    Pa[0, 3] = bx                                              # fw = proj_a(X_b(p)) - p = (-fx bx / Z, 0) = (-2.5, 0)
    tex = lambda x, y: np.stack([0.5 + 0.3 * np.sin(1.7 * x + 0.3 * y), 0.5 + 0.2 * np.cos(2.1 * y), 0.4 + 0.1 * x * y], -1)
    a = _plane(H, W, Z, Pa, Pb, tex)
    r = _cn(*a)
    flow = -U.FOCAL * bx / Z
    interior = np.zeros((H, W), bool)
    interior[:, 3:] = True                                     # x - 2.5 >= 0
    assert np.abs(r["fw"][..., 0] - flow).max() <= 1e-12 and np.abs(r["fw"][..., 1]).max() <= 1e-12
    assert np.array_equal(r["valid"], interior)
    assert np.all(r["reason"][~interior] == 2)
    Fa = a[0]
    want = 0.5 * (Fa[:, 0:W - 3] + Fa[:, 1:W - 2])             # the landing point x - 2.5: the mean of the pixels x - 3 and x - 2
    assert np.abs(r["warped"][:, 3:] - want).max() <= 1e-12
    assert r["count"] == interior.sum()
    # the plane's texture is a function of the world point: the warped frame differs from b only by the bilinear filter
    assert r["warp_mse"] < 1e-4 and r["sse"] == pytest.approx(r["err"][interior].sum(), rel=1e-15)
    assert np.all(r["lpips_in"][0][:, ~interior] == r["lpips_in"][1][:, ~interior])


@pytest.mark.parametrize("shape", U.SHAPES)
def test_fixture_figures(shape):
    H, W = shape
    f, r = U.fixture(H, W), U.restated(H, W)
    assert r["count"] == r["valid"].sum() == {(24, 40): 710, (37, 53): 1600}[shape]
    assert np.bincount(r["reason"].ravel(), minlength=7).tolist() == {(24, 40): [710, 80, 103, 0, 0, 55, 12],
                                                                     (37, 53): [1600, 106, 175, 0, 3, 55, 22]}[shape]
    assert np.all(r["reason"][:2] == 1)                          # the transparent rows
    # a kernel that drops the two rules shows up: the error with them ignored is several times larger
    no_rules = r["err"][np.isin(r["reason"], [0, 5, 6])].mean()
    assert r["warp_mse"] == pytest.approx({(24, 40): 6.350e-5, (37, 53): 2.030e-4}[shape], rel=1e-3)
    assert no_rules > 3.5 * r["warp_mse"]
    # premise of the identity-pair bound of the GPU test: neighbouring pixels differ by less than 0.2
    for fr in (f["frame_a"], f["frame_b"]):
        assert max(np.abs(np.diff(fr, axis=0)).max(), np.abs(np.diff(fr, axis=1)).max()) < 0.2


@pytest.mark.parametrize("shape", U.SHAPES)
def test_fixture_hidden_pixels_are_invalid(shape):
    """Every far-plane pixel of b whose four taps in a are all occluder pixels is invalid: fw is the far plane's flow, bw~ the
    occluder's, and their sum is the parallax between the depths 4 and 2.  From the translation (0.15, 0.02, 0.01) alone (a
    rotation's flow does not depend on depth and cancels): fx * (1/2 - 1/4) * (0.15, 0.02) = (1.5, 0.2) px, less at most
    16 px * 0.01 / 4 = 0.04 px from the motion along z, so |fw + bw~|^2 >= 1.45^2 = 2.1.  The threshold: |fw| <= 1.5 + 1.3 px
    (the yaw adds fx * 0.03 = 1.2 px and the edge of the field a little), |bw~| <= 3 + 1.4 px, so
    0.01 (|fw|^2 + |bw~|^2) + 0.5 <= 0.77.  Measured: min 2.235 / 2.243, max threshold 0.751 / 0.751.  Both inequalities are
    asserted on the fixture, so a changed fixture cannot void the test silently."""
    H, W = shape
    f, r = U.fixture(H, W), U.restated(H, W)
    x0, y0 = r["taps"][..., 0], r["taps"][..., 1]
    all_near = np.ones((H, W), bool)
    for k in range(4):
        all_near &= f["near_a"][y0 + (k >> 1), x0 + (k & 1)]
    hidden = ~f["near_b"] & ~np.isin(r["reason"], [1, 2, 3, 4]) & all_near
    assert hidden.sum() >= 10
    assert r["occ_lhs"][hidden].min() >= 2.1 and r["occ_rhs"][hidden].max() <= 0.77
    assert not r["valid"][hidden].any()


@pytest.mark.parametrize("shape", U.SHAPES)
def test_fixture_float32_decides_as_float64_outside_the_margin(shape):
    H, W = shape
    r64, r32 = U.restated(H, W), U.restated(H, W, "float32")
    band = r64["margin"] < MARGIN
    assert band.mean() <= MARGIN_CAP
    assert band.sum() == 0                                      # the fixture stays clear of the band altogether
    assert np.array_equal(r64["valid"][~band], r32["valid"][~band])
    assert np.all(np.isinf(r64["margin"][np.isin(r64["reason"], [1, 3, 4])]))
    assert np.nanmax(np.abs(r32["fw"].astype(np.float64) - r64["fw"])) <= 1e-5
    both = r64["valid"] & r32["valid"]
    assert np.abs(r32["warped"].astype(np.float64) - r64["warped"])[both].max() <= MEASURED_W


def _empty(r, H, W):
    assert not r["valid"].any() and r["count"] == 0 and r["sse"] == 0.0 and np.isnan(r["warp_mse"])
    assert np.all(np.isinf(r["margin"]))
    assert np.array_equal(r["lpips_in"][0], r["lpips_in"][1]) and np.isfinite(r["lpips_in"]).all()
    assert np.all(r["warped"][~np.isfinite(r["landing"]).all(-1)] == 0)


def test_undefined_inputs_give_an_empty_pair_without_warnings():
    H, W = 24, 40
    f = U.fixture(H, W)
    behind = np.eye(4, dtype=np.float32)
    behind[2, 3] = 10.0                                         # camera a beyond both surfaces, looking along +z: q.z < 0
    away = np.eye(4, dtype=np.float32)
    away[0, 0] = away[2, 2] = -1.0                              # camera b turned by pi about y: the two look away from each other
    zero = np.zeros((H, W), np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for dtype in (np.float64, np.float32):
            _empty(_cn(*U.args(f, opacity_b=zero, depth_b=zero), dtype=dtype), H, W)                      # transparent target
            _empty(_cn(*U.args(f, opacity_a=zero, depth_a=zero, opacity_b=zero, depth_b=zero), dtype=dtype), H, W)
            r = _cn(*U.args(f, pose_a=behind), dtype=dtype)
            _empty(r, H, W)
            assert np.all(r["reason"] == 1)
            _empty(_cn(*U.args(f, pose_b=away), dtype=dtype), H, W)
        # transparent source only: the target's flow is defined, every tap is not
        r = _cn(*U.args(f, opacity_a=zero, depth_a=zero))
        assert not r["valid"].any() and r["count"] == 0 and np.isnan(r["warp_mse"])
        assert set(np.unique(r["reason"])) <= {1, 2, 4}


def test_uint8_frames_are_read_as_the_kernel_reads_them():
    H, W = 24, 40
    f = U.fixture(H, W)
    a8, b8 = ((f[k] * 255 + 0.5).astype(np.uint8) for k in ("frame_a", "frame_b"))
    r8 = _cn(*U.args(f, frame_a=a8, frame_b=b8))
    rf = _cn(*U.args(f, frame_a=a8.astype(np.float32) * (np.float32(1) / np.float32(255)),
                     frame_b=b8.astype(np.float32) * (np.float32(1) / np.float32(255))))
    assert r8["sse"] == rf["sse"] and np.array_equal(r8["warped"], rf["warped"]) and np.array_equal(r8["valid"], rf["valid"])
