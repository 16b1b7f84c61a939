"""csrc/undistort.hip on the device against laenerf_amd.undistort's restatements, on the cameras of tests/undistort_util.py (wide
lenses, fx about W / 2: tests/test_undistort_cpu.py asserts displacements of 5 to 12 px and map values outside the source).

Bounds.
  maps        three times the float32-against-float64 figure the CPU file measures, in ulps of max(H, W) (undistort_util.map_tol).
  lae_remap   is fed the kernel's own fp32 map, and the restatement takes that same map in float64 arithmetic, so what is compared
              is interpolation alone: at most 16 x 2^-24 relative to the largest source value (the derivation is beside
              undistort_util.REMAP_RELATIVE: fp32 accumulation of four products, and one division for RGBA), plus half an fp16 ulp
              for fp16 outputs.  uint8 outputs are equal except where the float64 value before rounding lies within that bound
              of a half-integer; those may differ by one level and are at most 0.5 % (asserted on the CPU for these inputs).
              The valid plane is a comparison of the same fp32 numbers on both sides: it is equal everywhere, and nearest mode
              is equal byte for byte.
  round trip  redistort(images(g)) against g: derived in that test's docstring."""
import numpy as np
import pytest
import torch

import undistort_util as U
from laenerf_amd.undistort import (TOL_PX, CameraModel, Undistorter, distort_map, remap, remap_numpy, target_intrinsics, undistort_map,
                                   undistort_map_numpy)

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = {"uint8": torch.uint8, "float16": torch.float16, "float32": torch.float32}
_MAPS = {}


def case(name):
    return next(c for c in U.MAP_CASES if c[0] == name)


def device_map(name):
    """the kernel's own map of a case, computed once"""
    if name not in _MAPS:
        _, cams, _, (H, W, t) = case(name)
        _MAPS[name] = undistort_map(list(cams), t, H, W, DEV)
    return _MAPS[name]


@pytest.mark.parametrize("name", [c[0] for c in U.MAP_CASES])
def test_maps_against_the_restatement(name):
    _, cams, (Hs, Ws), (H, W, t) = case(name)
    m = device_map(name).cpu().numpy()
    assert m.shape == (len(cams), H, W, 2) and m.dtype == np.float32
    d = np.abs(m.astype(np.float64) - U.maps(name)).max()
    print("forward: largest difference", d, "bound", U.map_tol(name))
    assert d <= U.map_tol(name)
    inv, conv = distort_map(list(cams), Hs, Ws, t, device=DEV)
    want, flags = U.inverse_maps(name)
    assert torch.equal(conv.cpu(), torch.from_numpy(flags.copy())) and flags.all()
    d = np.abs(inv.cpu().numpy().astype(np.float64) - want).max()
    print("inverse: largest difference", d, "bound", U.map_tol(name, U.MEASURED_INVERSE_ULPS))
    assert d <= U.map_tol(name, U.MEASURED_INVERSE_ULPS)
    assert torch.equal(inv, distort_map(list(cams), Hs, Ws, t, iters=8, device=DEV)[0])          # 0 means the default count


def test_inverse_map_flags_what_did_not_converge():
    """a lens whose model folds over inside the frame (k2 < 0 at fx = W / 2): pixels beyond the fold have no ideal position.
    NaN exactly where the flag is 0; where it is 1 the float64 forward model takes the result back to the pixel within the
    flag's residual bound (doubled for the fp32 arithmetic the kernel judged it in)."""
    cam = CameraModel(28.0, 28.0, 27.5, 19.5, k1=0.16, k2=-0.23)
    Hs, Ws = U.SRC_A
    t = (30.0, 30.0, 27.5, 19.5)
    inv, conv = distort_map(cam, Hs, Ws, t, device=DEV)
    inv, conv = inv.cpu().numpy()[0].astype(np.float64), conv.cpu().numpy()[0]
    assert set(np.unique(conv)) == {0, 1}
    assert (np.isnan(inv).all(-1) == (conv == 0)).all() and (np.isnan(inv).any(-1) == (conv == 0)).all()
    x, y = (inv[..., 0] + 0.5 - t[2]) / t[0], (inv[..., 1] + 0.5 - t[3]) / t[1]
    xd, yd = cam.distort(x, y)
    j, i = np.meshgrid(np.arange(Hs), np.arange(Ws), indexing="ij")
    ok = conv == 1
    assert np.abs(xd * cam.fx + cam.cx - 0.5 - i)[ok].max() <= 2 * TOL_PX and np.abs(yd * cam.fy + cam.cy - 0.5 - j)[ok].max() <= 2 * TOL_PX
    # an invalid position stays invalid through lae_remap
    img = torch.ones(1, 37, 53, 1, device=DEV)
    out, valid = remap(img, torch.from_numpy(inv.astype(np.float32)[None]).to(DEV), return_valid=True)
    assert not valid.cpu().numpy()[0][~ok].any() and not out.cpu().numpy()[0, ..., 0][~ok].any()


def check_remap(src, m_dev, idx, mode, M=1.0):
    """lae_remap on the device against remap_numpy(float64) on the same fp32 map, under this file's rules"""
    dev_idx = None if idx is None else torch.from_numpy(np.asarray(idx, np.int32)).to(DEV)
    out, valid = remap(torch.from_numpy(src).to(DEV), m_dev, dev_idx, mode, return_valid=True)
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    m = m_dev.cpu().numpy()
    want, wvalid = remap_numpy(src, m, idx, mode, return_valid=True)
    assert out.dtype == src.dtype and out.shape == want.shape
    assert (valid == wvalid).all()
    assert not out[valid == 0].any()
    if mode == "nearest":
        assert out.tobytes() == want.tobytes()
        return out, valid
    pre = remap_numpy(src, m, idx, mode, pre=True)
    if src.dtype == np.uint8:
        tol = U.REMAP_RELATIVE * 255.0
        close = np.abs(pre - np.floor(pre) - 0.5) <= tol
        diff = np.abs(out.astype(np.int32) - want.astype(np.int32))
        print("share excluded", close.mean(), "of them different", (diff[close] > 0).mean() if close.any() else 0.0)
        assert (diff[~close] == 0).all() and diff.max() <= 1 and close.mean() <= U.HALF_CAP
    else:
        tol = U.float_tol(M, src.dtype)
        d = np.abs(out.astype(np.float64) - pre).max()
        print("largest difference", d, "bound", tol)
        assert d <= tol
    return out, valid


@pytest.mark.parametrize("mode", ("bilinear", "nearest"))
@pytest.mark.parametrize("C", (1, 3, 4))
@pytest.mark.parametrize("dtype", ("uint8", "float16", "float32"))
@pytest.mark.parametrize("name", ("three_37x53", "one_16x16"))
def test_remap_against_the_restatement(name, dtype, C, mode):
    _, cams, (Hs, Ws), _ = case(name)
    idx = U.CAM_INDEX if len(cams) == 3 else None                    # three cameras: a shuffled per-image index; one: a shared map
    n = len(U.CAM_INDEX) if len(cams) == 3 else 2
    out, valid = check_remap(U.images(n, Hs, Ws, C, np.dtype(dtype)), device_map(name), idx, mode)
    assert valid.any() and not valid.all()


def test_one_by_one_images():
    src = U.images(3, 1, 1, 4, np.uint8)
    m = torch.tensor([[[[0.0, 0.0], [-0.0, 0.0], [2.0 ** -10, 0.0], [0.0, -(2.0 ** -10)], [0.4, 0.0], [-0.5, 0.4]]]], device=DEV)
    out, valid = check_remap(src, m, None, "bilinear")
    assert valid[0, 0].tolist() == [1, 1, 0, 0, 0, 0] and (out[:, 0, 0] == src[:, 0, 0]).all()
    out, valid = check_remap(src, m, None, "nearest")
    assert valid[0, 0].tolist() == [1, 1, 1, 1, 1, 1]
    # a 1 x 1 target
    _, cams, (Hs, Ws), _ = case("one_16x16")
    t = target_intrinsics(list(cams), Hs, Ws)
    one = undistort_map(list(cams), (t[0], t[1], 0.5, 0.5), 1, 1, DEV)      # the principal ray: it lands at the source's (cx, cy) - 0.5
    assert one.shape == (1, 1, 1, 2) and abs(float(one[0, 0, 0, 0]) - (cams[0].cx - 0.5)) < 1e-4
    check_remap(U.images(2, Hs, Ws, 3, np.float32), one, None, "bilinear")


@pytest.mark.parametrize("dtype,C", [("uint8", 4), ("float16", 3), ("float32", 4), ("uint8", 1)])
def test_special_map_values_are_invalid_never_undefined(dtype, C):
    Hs, Ws = U.SRC_A
    src = U.images(2, Hs, Ws, C, np.dtype(dtype))
    xs = [0.0, Ws - 1.0, -0.0, Ws - 1.0 + 2.0 ** -10, np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, 2.0 ** 32 + 7, -(2.0 ** -20)]
    ys = [0.0, Hs - 1.0, -0.0, Hs - 1.0 + 2.0 ** -10, np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2.0 ** 31, 2.0 ** 32 + 7, -(2.0 ** -20)]
    m = np.full((1, 3, len(xs), 2), 5.3, np.float32)
    m[0, 0, :, 0], m[0, 1, :, 1], m[0, 2, :, 0], m[0, 2, :, 1] = xs, ys, xs, ys
    want_valid = [1, 1, 1, 0] + [0] * 9 + [0]
    md = torch.from_numpy(m).to(DEV)
    for mode in ("bilinear", "nearest"):
        out = torch.full((2, 3, len(xs), C), 171 if dtype == "uint8" else float("nan"), dtype=T[dtype], device=DEV)      # poisoned
        valid = torch.full((2, 3, len(xs)), 171, dtype=torch.uint8, device=DEV)
        remap(torch.from_numpy(src).to(DEV), md, None, mode, out=out, valid=valid)
        torch.cuda.synchronize()
        v = valid.cpu().numpy()
        # nearest: -2^-20 rounds to pixel 0 and W - 1 + 2^-10 to pixel W - 1
        expect = want_valid if mode == "bilinear" else [1, 1, 1, 1] + [0] * 9 + [1]
        assert all(v[k, r].tolist() == expect for k in range(2) for r in range(3)), v
        o = out.cpu().numpy()
        assert not np.isnan(o.astype(np.float64)).any() and not o[v == 0].any()
        check_remap(src, md, None, mode)


def test_rgba_premultiplication_leaves_no_colour_fringe():
    """transparent pixels (alpha 0) of arbitrary colour beside opaque pixels of one colour: wherever the output has any alpha its
    colour is the opaque colour, to the accumulation bound; where it has none the colour is zero"""
    Hs, Ws = U.SRC_A
    g = np.random.default_rng(5)
    colour = np.array([0.2, 0.55, 0.7], np.float32)
    for dtype in (np.float32, np.uint8):
        src = g.random((2, Hs, Ws, 4)).astype(np.float32)
        opaque = np.zeros((Hs, Ws), bool)
        opaque[5:30, 10:44] = True
        opaque[12:20, 20:30] = False                                   # a transparent hole
        src[:, opaque, :3], src[:, opaque, 3], src[:, ~opaque, 3] = colour, 1.0, 0.0
        if dtype is np.uint8:
            src = np.floor(src * 255 + 0.5).astype(np.uint8)
        out, valid = check_remap(src, device_map("three_37x53"), U.CAM_INDEX[:2], "bilinear")
        scale = 255.0 if dtype is np.uint8 else 1.0
        want = src[0, 6, 11, :3].astype(np.float64)
        a = remap_numpy(src, device_map("three_37x53").cpu().numpy(), U.CAM_INDEX[:2], pre=True)[..., 3]     # the alpha before rounding
        some = a > 0
        assert some.any() and (~some & (valid == 1)).any() and ((a > 0) & (a < scale)).any()
        err = np.abs(out[..., :3].astype(np.float64) - want)[some].max()
        assert err <= (0.5 if dtype is np.uint8 else 0.0) + U.REMAP_RELATIVE * scale and not out[..., :3][~some].any()


def test_two_calls_and_a_graph_replay_give_the_same_bytes():
    _, cams, (Hs, Ws), (H, W, _) = case("three_37x53")
    m = device_map("three_37x53")
    idx = torch.from_numpy(U.CAM_INDEX).to(DEV)
    n = len(U.CAM_INDEX)
    for dtype, C, mode in (("uint8", 4, "bilinear"), ("float16", 3, "bilinear"), ("float32", 1, "nearest")):
        src = torch.from_numpy(U.images(n, Hs, Ws, C, np.dtype(dtype))).to(DEV)
        a, va = remap(src, m, idx, mode, return_valid=True)
        b, vb = remap(src, m, idx, mode, return_valid=True)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and torch.equal(va, vb)
        out, valid = torch.empty_like(a), torch.empty_like(va)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            remap(src, m, idx, mode, out=out, valid=valid)             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            remap(src, m, idx, mode, out=out, valid=valid)
        out.fill_(0); valid.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == a.cpu().numpy().tobytes() and torch.equal(valid, va)


def _g(u, v):
    """a smooth image in source-pixel coordinates"""
    return 0.5 + 0.3 * np.sin(0.11 * u + 0.2) * np.cos(0.09 * v - 0.1) + 0.002 * u


def test_from_transforms_undistorts_on_the_device(tmp_path):
    """The loader on a scene written with PIL: two cameras (per-frame overrides), balance 0 and 0.6.

    redistort(images(g)) against g, on pixels valid both ways.  Pass one interpolates g on the source lattice: error at most
    B1 = (max|g_uu| + max|g_vv|) / 8 (h = 1 pixel; the derivation is in test_undistort_cpu).  Pass two interpolates the result
    T = g(S(.)) + e1 on the target lattice: the e1 part is a convex combination, at most B1 again, and the g(S(.)) part errs by
    at most B2 = (max|h_uu| + max|h_vv|) / 8 with h = g(S(.)), whose second derivatives are taken from second differences of the
    float64 function with step 1/4 pixel, increased by 5 %.  What is left is g's gradient times the coordinate errors: the
    forward and inverse maps' fp32 error (2e-4 px allowed: their bounds in this file are at most 15 ulps of 64 = 1.1e-4) and
    the Newton residual (below 1e-6 px after 8 steps on such a lens), and 32 x 2^-24 for two fp32 accumulations."""
    from laenerf_amd.data import ResidentImages
    Hs, Ws = U.SRC_A
    n = 5
    path, ims, poses, cams = U.write_scene(str(tmp_path), n=n, H=Hs, W=Ws, cam=U.CAMS_A[0], per_frame=True)
    uniq, index = [cams[0], cams[1]], [k % 2 for k in range(n)]
    g = np.random.default_rng(11)
    depths = (1.0 + g.random((n, Hs, Ws))).astype(np.float32)
    weights = g.random((n, Hs, Ws)).astype(np.float16)
    for balance in (0.0, 0.6):
        data = ResidentImages.from_transforms(path, undistort=True, balance=balance, depths=depths, pixel_weights=weights, device=DEV)
        und = data.undistorter
        target = target_intrinsics(uniq, Hs, Ws, balance)
        assert data.intrinsics == target and (data.H, data.W, data.n_img) == (Hs, Ws, n)
        assert [c.record().tolist() for c in und.cams] == [c.record().tolist() for c in uniq] and und.cam_index.tolist() == index
        m = und.maps.cpu().numpy()
        want_map = undistort_map_numpy(uniq, target, Hs, Ws)
        assert np.abs(m - want_map).max() <= 3 * 2.3 * U.ulp_of(Ws)      # the largest of the measured forward figures
        out, valid = check_remap(ims, und.maps, index, "bilinear")
        assert data.images.cpu().numpy().tobytes() == out.tobytes()
        assert (und.valid.cpu().numpy() == valid).all()
        assert (valid == 1).all() == (balance == 0.0)
        d_want = remap_numpy(depths[..., None], m, index, "nearest")[..., 0]
        w_want = remap_numpy(weights[..., None], m, index, "nearest")[..., 0]
        assert data.depths.dtype == torch.float32 and data.depths.cpu().numpy().tobytes() == d_want.tobytes()
        assert data.pixel_weights.dtype == torch.float16
        assert data.pixel_weights.cpu().numpy().tobytes() == (w_want * valid.astype(np.float16)).tobytes()
        batch = data.sample(64)
        torch.cuda.synchronize()
        assert batch["rays_o"].shape == (64, 3) and bool(torch.isfinite(batch["rays_d"]).all()) and bool(torch.isfinite(batch["gt"]).all())
    # without weights of the caller's, balance > 0 sets the valid plane; balance 0 sets none
    data = ResidentImages.from_transforms(path, undistort=True, balance=0.6, device=DEV)
    assert torch.equal(data.pixel_weights, data.undistorter.valid.float())
    assert ResidentImages.from_transforms(path, undistort=True, device=DEV).pixel_weights is None
    # masks go the same way (nearest)
    from PIL import Image
    from laenerf_amd.metrics import load_masks
    mask = (g.random((Hs, Ws)) < 0.5).astype(np.uint8) * 255
    Image.fromarray(mask).save(str(tmp_path / "r_1_mask.png"))
    masks = load_masks(path, undistorter=data.undistorter)
    assert [k for k, v in enumerate(masks) if v is not None] == [1]
    want = remap_numpy(mask[None, ..., None], data.undistorter.maps.cpu().numpy(), [1], "nearest")[0, ..., 0]
    assert masks[1].cpu().numpy().tobytes() == want.tobytes()
    # frames of different sizes are refused
    Image.fromarray(ims[0][:-2]).save(str(tmp_path / "r_0.png"))
    with pytest.raises(ValueError):
        ResidentImages.from_transforms(path, undistort=True, device=DEV)

    # the round trip, on the last undistorter (balance 0.6: both passes have invalid pixels)
    und = data.undistorter
    target = und.target
    j, i = np.meshgrid(np.arange(Hs, dtype=np.float64), np.arange(Ws, dtype=np.float64), indexing="ij")
    img = np.repeat(_g(i, j).astype(np.float32)[None, ..., None], n, 0)
    fwd, v1 = und.images(torch.from_numpy(img), return_valid=True)
    back, v2 = und.redistort(fwd, return_valid=True)
    assert back.shape == (n, Hs, Ws, 1) and torch.equal(und.distort_images(fwd), back)
    inv = und.inverse[0].cpu().numpy().astype(np.float64)
    q = 0.25
    fi, fj = np.meshgrid(np.arange(0, Ws - 1 + q, q), np.arange(0, Hs - 1 + q, q))
    c = _g(fi, fj)
    B1 = 1.05 * (np.abs(c[:, 2:] - 2 * c[:, 1:-1] + c[:, :-2]).max() + np.abs(c[2:] - 2 * c[1:-1] + c[:-2]).max()) / q ** 2 / 8
    grad = 1.05 * max(np.abs(np.diff(c, axis=1)).max(), np.abs(np.diff(c, axis=0)).max()) / q * np.sqrt(2)
    for k in range(n):
        cam = uniq[index[k]]
        xd, yd = cam.distort((fi + 0.5 - target[2]) / target[0], (fj + 0.5 - target[3]) / target[1])
        h = _g(xd * cam.fx + cam.cx - 0.5, yd * cam.fy + cam.cy - 0.5)
        B2 = 1.05 * (np.abs(h[:, 2:] - 2 * h[:, 1:-1] + h[:, :-2]).max() + np.abs(h[2:] - 2 * h[1:-1] + h[:-2]).max()) / q ** 2 / 8
        bound = B1 + B2 + grad * (2 * 2e-4 + 1e-6) + 32 * 2.0 ** -24
        # valid both ways: the second pass's pixel is valid and its four neighbours in the first pass's output were
        p = inv[index[k]]
        ok = v2[k].cpu().numpy() == 1
        x0, y0 = np.floor(np.where(ok, p[..., 0], 0)).astype(int), np.floor(np.where(ok, p[..., 1], 0)).astype(int)
        x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
        vk = v1[k].cpu().numpy() == 1
        ok &= vk[y0, x0] & vk[y0, x1] & vk[y1, x0] & vk[y1, x1]
        err = np.abs(back[k, ..., 0].cpu().numpy().astype(np.float64) - img[k, ..., 0])[ok].max()
        print("view", k, "round trip error", err, "bound", bound, "pixels", ok.sum())
        assert ok.sum() > Hs * Ws // 2 and err <= bound
