"""Undistortion on the CPU: the camera models, laenerf_amd.undistort's float64 / float32 restatements, target_intrinsics and the
loader.  These tests assert the figures tests/test_gpu_undistort.py relies on, for the very cameras it uses (tests/undistort_util.py).

Measured (float32 against float64 restatement, in ulps of max(H, W) = 56: the spacing of fp32 there, 3.8e-6 px):
  forward map   three_37x53 2.2 (OpenCV 1.6 and 2.2, fisheye 1.3), one_16x16 1.08, three_16x16 2.21
  inverse map   three_37x53 4.8, one_16x16 0.74, three_16x16 1.43; the converged flags of the two restatements are equal
  The GPU bound is three times the figure of undistort_util.MEASURED_MAP_ULPS / MEASURED_INVERSE_ULPS (the compiler may order the
  kernel's sums differently; atanf / tanf are another library's), i.e. at most 6.9 ulps = 2.6e-5 px forward, 14.7 ulps inverse.
Newton steps (float64, largest residual in source pixels): 3840 x 2160 fx = 3000 k1 = 0.16 k2 = -0.23: 6.7e-13 after 3; the
  strong barrel k1 = -0.3 k2 = 0.09 at fx = W / 2: 3e-9 after 5, 8e-13 after 6 at 3840 x 2160; 1e-9 after 5, 9e-15 after 6 at
  40 x 56; fisheye 1e-14 after 3.  NEWTON_ITERS = 8.
Largest displacement of the test lenses 5.2 to 11.7 px; share of map values outside the source up to 57 %."""
import warnings

import numpy as np
import pytest

import undistort_util as U
from laenerf_amd.undistort import (NEWTON_ITERS, CameraModel, distort_map_numpy, remap_numpy, target_intrinsics, undistort_map_numpy,
                                   undistort_numpy)


def test_hand_case():
    cam = CameraModel(1.0, 1.0, 0.0, 0.0, k1=0.1, k2=-0.05, k3=0.0, p1=0.01, p2=-0.02)
    xd, yd = cam.distort(0.5, -0.25)
    assert abs(xd - 0.49443359375) <= 1e-15 and abs(yd - (-0.247216796875)) <= 1e-15


@pytest.mark.parametrize("model", (0, 1))
def test_zero_coefficients_give_the_identity_map_exactly(model):
    cam = CameraModel(31.0, 29.0, 20.25, 14.5, model=0)
    H, W = 29, 41
    for dt in (np.float64, np.float32):
        m = undistort_map_numpy(cam, (31.0, 29.0, 20.25, 14.5), H, W, dt)
        i, j = np.meshgrid(np.arange(W), np.arange(H))
        if dt is np.float64:
            assert np.abs(m[0, ..., 0] - i).max() <= 4e-15 * W and np.abs(m[0, ..., 1] - j).max() <= 4e-15 * W
        # quarter-pixel intrinsics and power-of-two focal lengths: every step is exact, in either precision
        m = undistort_map_numpy(CameraModel(32.0, 16.0, 20.25, 14.5, model=0), (32.0, 16.0, 20.25, 14.5), H, W, dt)
        assert (m[0, ..., 0] == i).all() and (m[0, ..., 1] == j).all()
    if model == 1:          # the fisheye's identity is theta_d = theta, not zero coefficients of the pinhole: atan is not the identity
        x = np.array([0.0, 0.3]); y = np.array([0.0, -0.4])
        xd, yd = CameraModel(1, 1, 0, 0, model=1).distort(x, y)
        assert xd[0] == 0.0 and yd[0] == 0.0 and abs(np.hypot(xd[1], yd[1]) - np.arctan(0.5)) <= 1e-15


@pytest.mark.parametrize("cam,size", [(U.CAM_4K, (2160, 3840)), (U.CAM_4K_BARREL, (2160, 3840))] + [(c, U.SRC_A) for c in U.CAMS_A],
                         ids=["4k", "4k_barrel", "barrel", "pincushion", "fisheye"])
def test_round_trip_forward_of_inverse(cam, size):
    """forward(inverse(p)) = p within 1e-9 px in float64, every pixel converged (a lattice of about 200 x 200 pixels and the last
    row and column of the frame)"""
    Hs, Ws = size
    i = np.append(np.arange(0, Ws, max(1, Ws // 200), dtype=np.float64), Ws - 1.0)
    j = np.append(np.arange(0, Hs, max(1, Hs // 200), dtype=np.float64), Hs - 1.0)
    xd, yd = np.meshgrid((i + 0.5 - cam.cx) / cam.fx, (j + 0.5 - cam.cy) / cam.fy)
    x, y, ok = cam.undistort_points(xd, yd)
    assert ok.all()
    xe, ye = cam.distort(x, y)
    res = max(np.abs(xe - xd).max() * cam.fx, np.abs(ye - yd).max() * cam.fy)
    r5 = cam.undistort_points(xd, yd, iters=5)
    x5, y5 = cam.distort(r5[0], r5[1])
    print("residual px after", NEWTON_ITERS, "steps", res, "after 5", max(np.abs(x5 - xd).max() * cam.fx, np.abs(y5 - yd).max() * cam.fy))
    assert res <= 1e-9


def _smooth(x, y):
    """a smooth function of the ray direction (x, y, 1)"""
    return 0.5 + 0.25 * np.sin(3.0 * x + 0.4) * np.cos(2.0 * y - 0.3) + 0.1 * x * y


@pytest.mark.parametrize("k", (0, 1, 2))
def test_undistorting_a_rendered_function_gives_the_function_on_the_pinhole_grid(k):
    """The distorted image is rendered through the float64 Newton INVERSE (source pixel -> ray -> f), undistort_numpy uses the
    FORWARD model only, and the result is compared with f on the pinhole grid: the two directions share no formula.

    The bound.  undistort_numpy interpolates g(u, v) = f(ray of source position (u, v)) bilinearly on the unit lattice of the
    source pixels.  Linear interpolation of a C2 function on an interval of length h errs by at most h^2 / 8 max|g''|; bilinear
    interpolation is that along u followed by that along v of the u-interpolated values (a convex combination, so the second
    derivative along v is no larger), and it is exact in the u v term: |error| <= (max|g_uu| + max|g_vv|) / 8 with h = 1 pixel.
    The two maxima are taken from g itself -- second differences with step 1/4 pixel over the source frame, through the same
    Newton inverse, increased by 5 % for the lattice's spacing -- not from the code under test.  2^-24 is added for the float32
    image the function is stored in."""
    cam, (Hs, Ws) = U.CAMS_A[k], U.SRC_A

    def g(u, v):
        x, y, ok = cam.undistort_points((u + 0.5 - cam.cx) / cam.fx, (v + 0.5 - cam.cy) / cam.fy)
        assert ok.all()
        return _smooth(x, y)
    i, j = np.meshgrid(np.arange(Ws, dtype=np.float64), np.arange(Hs, dtype=np.float64))
    img = g(i, j).astype(np.float32)[None, ..., None]
    H, W = 37, 53
    target = target_intrinsics(cam, Hs, Ws, 0.0)                      # the frame every pixel of which the capture covers
    target = (target[0], target[1], 26.0 + (target[2] - cam.cx), 18.0 + (target[3] - cam.cy))   # a 37 x 53 window of that frame
    out, valid = undistort_numpy(img, cam, target, H, W, return_valid=True)
    assert valid.all()
    ti, tj = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    want = _smooth((ti + 0.5 - target[2]) / target[0], (tj + 0.5 - target[3]) / target[1])
    q = 0.25
    fi, fj = np.meshgrid(np.arange(0, Ws - 1 + q, q), np.arange(0, Hs - 1 + q, q))
    c = g(fi, fj)
    guu = np.abs(c[:, 2:] - 2 * c[:, 1:-1] + c[:, :-2]).max() / q ** 2
    gvv = np.abs(c[2:] - 2 * c[1:-1] + c[:-2]).max() / q ** 2
    bound = 1.05 * (guu + gvv) / 8 + 2.0 ** -24
    err = np.abs(out[0, ..., 0].astype(np.float64) - want).max()
    print("largest error", err, "bound", bound)
    assert err <= bound
    assert err > 1e-7                                                  # a test that interpolates nothing would prove nothing


@pytest.mark.parametrize("cams,size", [(U.CAMS_A[:1], U.SRC_A), (U.CAMS_A, U.SRC_A), (U.CAMS_B, U.SRC_B), ((U.CAM_4K,), (2160, 3840))],
                         ids=["barrel", "three", "small", "4k"])
def test_target_intrinsics(cams, size):
    H, W = size
    cams = list(cams)
    t0 = target_intrinsics(cams, H, W, 0.0)
    step = max(1, W // 400)                                             # the 4k frame: every ninth pixel and the border are enough

    def valid(t, dt):
        m = undistort_map_numpy(cams, t, H, W, dt)
        ok = (m[..., 0] >= 0) & (m[..., 0] <= W - 1) & (m[..., 1] >= 0) & (m[..., 1] <= H - 1)
        return ok if step == 1 else np.concatenate([ok[:, ::step, ::step].reshape(len(cams), -1), ok[:, (0, -1), :].reshape(len(cams), -1),
                                                    ok[:, :, (0, -1)].reshape(len(cams), -1)], 1)
    assert valid(t0, np.float64).all() and valid(t0, np.float32).all()
    assert not valid((0.99 * t0[0], 0.99 * t0[1], t0[2], t0[3]), np.float64).all()
    assert t0[2] == np.mean([c.cx for c in cams]) and t0[3] == np.mean([c.cy for c in cams])
    t1 = target_intrinsics(cams, H, W, 1.0)
    if step == 1:
        m, ok = distort_map_numpy(cams, H, W, t1, iters=2 * NEWTON_ITERS)
        assert ok.all()
        assert (m[..., 0] >= -0.5 - 1e-9).all() and (m[..., 0] <= W - 0.5 + 1e-9).all()
        assert (m[..., 1] >= -0.5 - 1e-9).all() and (m[..., 1] <= H - 0.5 + 1e-9).all()
        # and no zoom larger by 1 % keeps them all inside
        m, _ = distort_map_numpy(cams, H, W, (1.01 * t1[0], 1.01 * t1[1], t1[2], t1[3]), iters=2 * NEWTON_ITERS)
        assert not ((m[..., 0] >= -0.5) & (m[..., 0] <= W - 0.5) & (m[..., 1] >= -0.5) & (m[..., 1] <= H - 0.5)).all()
    th = target_intrinsics(cams, H, W, 0.5)
    assert abs(th[0] - 0.5 * (t0[0] + t1[0])) <= 1e-12 * t0[0] and abs(th[1] - 0.5 * (t0[1] + t1[1])) <= 1e-12 * t0[1]
    with pytest.raises(ValueError):
        target_intrinsics(cams, H, W, 1.5)


@pytest.mark.parametrize("name", [c[0] for c in U.MAP_CASES])
def test_float32_restatement_against_float64_on_the_gpu_tests_cameras(name):
    _, cams, (Hs, Ws), (H, W, t) = next(c for c in U.MAP_CASES if c[0] == name)
    m64, m32 = U.maps(name), U.maps(name, "float32")
    ulp = U.ulp_of(max(H, W, Hs, Ws))
    d = np.abs(m32.astype(np.float64) - m64).max() / ulp
    (i64, ok64), (i32, ok32) = U.inverse_maps(name), U.inverse_maps(name, "float32")
    both = (ok64 & ok32).astype(bool)
    di = np.abs(i32.astype(np.float64) - i64)[both].max() / ulp
    print(name, "largest map difference", d, "ulps of max(H, W); inverse map", di)
    assert d <= U.MEASURED_MAP_ULPS[name] and di <= U.MEASURED_INVERSE_ULPS[name]
    assert (ok64 == ok32).all() and ok64.all()
    # the lenses are not gentle: an identity map would fail the GPU test
    ident = undistort_map_numpy([CameraModel(c.fx, c.fy, c.cx, c.cy) for c in cams], t, H, W)
    disp = np.abs(m64 - ident).max(axis=(1, 2, 3))
    outside = (m64[..., 0] < 0) | (m64[..., 0] > Ws - 1) | (m64[..., 1] < 0) | (m64[..., 1] > Hs - 1)
    print("largest displacement per camera", disp, "share outside the source", outside.mean())
    assert (disp >= 5.0).all() and outside.any() and not outside.all()


@pytest.mark.parametrize("C", (1, 3, 4))
@pytest.mark.parametrize("name", ("three_37x53", "one_16x16"))
def test_uint8_inputs_stay_under_the_half_integer_cap(name, C):
    """the GPU test excludes uint8 outputs whose float64 value before rounding lies within the accumulation bound of a
    half-integer; for its inputs that share stays under undistort_util.HALF_CAP"""
    _, cams, (Hs, Ws), _ = next(c for c in U.MAP_CASES if c[0] == name)
    n = len(U.CAM_INDEX) if len(cams) == 3 else 2
    idx = U.CAM_INDEX if len(cams) == 3 else None
    src = U.images(n, Hs, Ws, C, np.uint8)
    pre = remap_numpy(src, U.maps(name, "float32"), idx, pre=True)
    frac = np.abs(pre - np.floor(pre) - 0.5)
    share = (frac <= U.REMAP_RELATIVE * 255.0).mean()
    print("share within the bound of a half-integer", share)
    assert share <= U.HALF_CAP


def test_remap_numpy_rules_by_hand():
    src = np.zeros((1, 2, 3, 4), np.uint8)
    src[0, 0, 0] = (200, 100, 50, 255)
    src[0, 0, 1] = (9, 99, 199, 0)                                      # transparent, arbitrary colour
    src[0, 1, 0] = (100, 100, 100, 255)
    m = np.array([[[[0.5, 0.0], [0.0, 0.5], [2.0, 1.0], [2.0 + 2.0 ** -10, 1.0], [-0.0, 0.0], [np.nan, 0.0], [1e30, 0.0], [-np.inf, 0.0]]]],
                 np.float32)
    out, valid = remap_numpy(src, m, return_valid=True)
    assert valid[0, 0].tolist() == [1, 1, 1, 0, 1, 0, 0, 0]
    assert out[0, 0, 0].tolist() == [200, 100, 50, 128]                 # no fringe: the transparent neighbour's colour has no weight
    assert out[0, 0, 1].tolist() == [150, 100, 75, 255]
    assert out[0, 0, 4].tolist() == [200, 100, 50, 255] and not out[0, 0, 3].any() and not out[0, 0, 5:].any()
    near, nv = remap_numpy(src, np.array([[[[0.49, 0.0], [0.5, 0.0], [2.49, 1.49], [2.5, 0.0], [-0.5, 0.0], [-0.51, 0.0]]]], np.float32), mode="nearest",
                           return_valid=True)
    assert nv[0, 0].tolist() == [1, 1, 1, 0, 1, 0] and near[0, 0, 0].tolist() == [200, 100, 50, 255] and near[0, 0, 1].tolist() == [9, 99, 199, 0]
    # a camera index outside the maps: the image is invalid
    out, valid = remap_numpy(src, m, cam_index=[3], return_valid=True)
    assert not out.any() and not valid.any()


def test_camera_model_from_transforms():
    t = {"w": 56, "h": 40, "fl_x": 28.0, "cx": 27.0, "k1": -0.1, "p2": 0.01, "frames": []}
    c = CameraModel.from_transforms(t, downscale=2)
    assert (c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p2, c.model) == (14.0, 14.0, 13.5, 10.0, -0.1, 0.0, 0.01, 0) and c.distorted
    c = CameraModel.from_transforms(t, {"fl_y": 30.0, "k1": 0.0, "p2": 0.0, "is_fisheye": True, "k4": 0.5})
    assert (c.fx, c.fy, c.k1, c.k4, c.model) == (28.0, 30.0, 0.0, 0.5, 1)
    assert CameraModel.from_transforms(dict(t, camera_model="OPENCV_FISHEYE")).model == 1
    assert not CameraModel.from_transforms({"camera_angle_x": 1.0}, H=40, W=56).distorted
    with pytest.raises(ValueError):
        CameraModel(0.0, 1.0, 0, 0)
    with pytest.raises(ValueError):
        CameraModel(1.0, 1.0, 0, 0, k1=float("nan"))


def test_loader_without_undistort_is_todays_and_warns_once(tmp_path):
    import torch
    from laenerf_amd.data import ResidentImages, nerf_matrix_to_ngp
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    plain, ims, poses, _ = U.write_scene(str(tmp_path / "a"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d = ResidentImages.from_transforms(plain, device="cpu")
    want = ResidentImages.from_arrays(ims, np.stack([nerf_matrix_to_ngp(p.astype(np.float32), scale=0.33, offset=(0, 0, 0)) for p in poses]),
                                      (30.0, 31.0, 28.0, 20.0), device="cpu")
    assert torch.equal(d.images, want.images) and torch.equal(d.poses, want.poses) and d.intrinsics == want.intrinsics
    assert d.undistorter is None and d.pixel_weights is None and d.depths is None and sorted(vars(d)) == sorted(vars(want))
    keyed, _, _, _ = U.write_scene(str(tmp_path / "b"), cam=U.CAMS_A[0], per_frame=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        k = ResidentImages.from_transforms(keyed, device="cpu")
    assert len(w) == 1 and "ignored" in str(w[0].message)
    assert torch.equal(k.images, want.images) and k.intrinsics == (28.0, 27.0, 27.3, 19.6) and k.undistorter is None


def test_package_exports_and_binding():
    import laenerf_amd
    from laenerf_amd import _lib, build
    for name in ("CameraModel", "Undistorter", "undistort_map", "distort_map", "remap", "target_intrinsics", "undistort_numpy"):
        assert getattr(laenerf_amd, name) is getattr(laenerf_amd.undistort, name) and name in laenerf_amd.__all__
    assert laenerf_amd.tsdf_numpy is laenerf_amd.tsdf.tsdf_numpy
    assert all(n in _lib.SIGNATURES for n in ("lae_undistort_map", "lae_distort_map", "lae_remap")) and "undistort.hip" in build.SOURCES
    assert _lib.ABI_TAG == b"abi28"
    with pytest.raises(AttributeError):
        laenerf_amd.no_such_thing


def test_entry_points_reject_bad_arguments_before_any_launch(hip_lib):
    import ctypes
    from laenerf_amd import _lib
    for name in ("lae_undistort_map", "lae_distort_map", "lae_remap"):
        getattr(hip_lib, name).argtypes = _lib.SIGNATURES[name]
    one = ctypes.c_void_p(64)
    rec = np.ascontiguousarray(np.stack([c.record() for c in U.CAMS_A]).astype(np.float32))

    def cams(**kw):
        r = rec.copy()
        for k, v in kw.items():
            r[1, k if isinstance(k, int) else int(k[1:])] = v
        return r

    def umap(c=rec, n=3, fx=25.0, fy=24.0, cx=26.0, h=37, w=53, m=one):
        return hip_lib.lae_undistort_map(None if c is None else c.ctypes.data, n, fx, fy, cx, 18.0, h, w, m, None)

    def dmap(c=rec, n=3, fx=25.0, h=40, w=56, it=0, m=one, ok=None):
        return hip_lib.lae_distort_map(None if c is None else c.ctypes.data, n, h, w, fx, 24.0, 26.0, 18.0, it, m, ok, None)
    assert umap(c=None) == -3 and umap(m=None) == -3 and dmap(c=None) == -3 and dmap(m=None) == -3
    assert umap(c=None, n=0, m=None) == 0 and dmap(c=None, n=0, m=None) == 0
    for kw in (dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")), dict(cx=float("inf")), dict(h=0), dict(w=0), dict(w=32769),
               dict(m=ctypes.c_void_p(68)), dict(c=cams(_0=2.0)), dict(c=cams(_0=0.5)), dict(c=cams(_1=0.0)), dict(c=cams(_2=float("inf"))),
               dict(c=cams(_5=float("nan"))), dict(c=cams(_10=float("-inf")))):
        assert umap(**kw) == -1, kw
    for kw in (dict(fx=0.0), dict(h=0), dict(w=40000), dict(it=65), dict(m=ctypes.c_void_p(68)), dict(c=cams(_0=-1.0)), dict(c=cams(_9=float("nan")))):
        assert dmap(**kw) == -1, kw

    def remap(src=one, dt=0, n=2, hs=40, ws=56, c=4, m=one, idx=None, nc=1, ht=37, wt=53, mode=0, dst=one, valid=None):
        return hip_lib.lae_remap(src, dt, n, hs, ws, c, m, idx, nc, ht, wt, mode, dst, valid, None)
    assert remap(src=None) == -3 and remap(m=None) == -3 and remap(dst=None) == -3
    assert remap(n=0) == 0 and remap(n=0, src=None, m=None, dst=None) == 0
    for kw in (dict(dt=3), dict(dt=-1), dict(c=2), dict(c=0), dict(c=5), dict(hs=0), dict(ws=0), dict(ht=0), dict(wt=32769), dict(nc=0),
               dict(mode=2), dict(mode=-1), dict(src=ctypes.c_void_p(66)), dict(dst=ctypes.c_void_p(66)), dict(dt=1, src=ctypes.c_void_p(68)),
               dict(dt=2, dst=ctypes.c_void_p(72)), dict(dt=2, c=3, src=ctypes.c_void_p(66)), dict(m=ctypes.c_void_p(68)),
               dict(idx=ctypes.c_void_p(66))):
        assert remap(**kw) == -1, kw
    assert remap(n=0, dt=7) == -1                                       # a bad argument is refused even where nothing would run
