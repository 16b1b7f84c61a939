"""Undistortion at the door: lens-distorted captures resampled once into the single pinhole camera every later stage assumes
(csrc/undistort.hip, where the camera models are written down; include/laenerf.h).

    CameraModel(fx, fy, cx, cy, k1.., model)              a source camera; CameraModel.from_transforms(transforms dict, frame)
    undistort_map(cams, target, H, W)                     per target pixel the source position, fp32 [n_cam, H, W, 2] (lae_undistort_map)
    distort_map(cams, Hs, Ws, target)                     per source pixel the target position + converged flags (lae_distort_map)
    remap(src, map, cam_index, mode)                      images or planes through a map (lae_remap)
    target_intrinsics(cams, H, W, balance)                the pinhole camera to resample into (host, float64)
    Undistorter(cams, cam_index, target, H, W)            the maps of a scene: .images / .plane / .valid / .redistort / .distort_images
    undistort_map_numpy / distort_map_numpy / remap_numpy the three kernels restated in a chosen dtype; undistort_numpy chains
                                                          the first and the last

Positions are in pixel-index units: pixel (i, j)'s centre is (i, j), its normalised coordinates x = (i + 0.5 - cx) / fx.
`ResidentImages.from_transforms(undistort=True)` and `metrics.load_masks(undistorter=)` use all of it."""
import numpy as np

OPENCV, FISHEYE = 0, 1              # LAE_CAM_OPENCV / LAE_CAM_FISHEYE
CAM_FLOATS = 12                     # LAE_CAM_FLOATS: model, fx, fy, cx, cy, k1, k2, k3, k4, p1, p2, 0
NEWTON_ITERS = 8                    # LAE_UNDISTORT_NEWTON_ITERS (why 8: include/laenerf.h)
TOL_PX = 0.015625                   # LAE_UNDISTORT_TOL_PX: the converged flag's residual bound, in source pixels
MODES = {"bilinear": 0, "nearest": 1}          # LAE_REMAP_*
MAX_SIDE = 32768
_COEFFS = ("k1", "k2", "k3", "k4", "p1", "p2")
_FISHEYE_NAMES = ("OPENCV_FISHEYE", "FISHEYE", "fisheye", "opencv_fisheye")


class CameraModel:
    """one source camera: fx, fy, cx, cy in pixels, the coefficients of its model (OPENCV: k1, k2, k3, p1, p2; FISHEYE: k1..k4)"""
    __slots__ = ("model", "fx", "fy", "cx", "cy") + _COEFFS

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0, p1=0.0, p2=0.0, model=OPENCV):
        if model not in (OPENCV, FISHEYE):
            raise ValueError("CameraModel: model must be OPENCV (0) or FISHEYE (1)")
        self.model = int(model)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.k3, self.k4, self.p1, self.p2 = (float(v) for v in (k1, k2, k3, k4, p1, p2))
        if not (self.fx > 0 and self.fy > 0) or not np.isfinite(self.record()).all():
            raise ValueError("CameraModel: focal lengths must be positive and every value finite")

    @classmethod
    def from_transforms(cls, transform, frame=None, H=None, W=None, downscale=1):
        """the camera of a transforms dict (the keys scripts/colmap2nerf.py writes): fl_x / fl_y or camera_angle_x / _y, cx / cy
        (default W/2, H/2), k1..k4, p1, p2, is_fisheye or camera_model; a key of `frame` (one entry of transform["frames"])
        overrides the global one.  downscale divides fx, fy, cx, cy and the size; the coefficients are scale-free.
        H, W: the image's size before downscaling where the file has no h / w."""
        import math
        d = dict(transform)
        d.update(frame or {})
        H = int(d["h"]) if "h" in d else H
        W = int(d["w"]) if "w" in d else W
        if "fl_x" in d or "fl_y" in d:
            fx = d["fl_x"] if "fl_x" in d else d["fl_y"]
            fy = d["fl_y"] if "fl_y" in d else d["fl_x"]
        elif "camera_angle_x" in d or "camera_angle_y" in d:
            fx = W / (2 * math.tan(d["camera_angle_x"] / 2)) if "camera_angle_x" in d else None
            fy = H / (2 * math.tan(d["camera_angle_y"] / 2)) if "camera_angle_y" in d else None
            fx = fy if fx is None else fx
            fy = fx if fy is None else fy
        else:
            raise RuntimeError("CameraModel.from_transforms: no focal length in the transforms file")
        cx = d["cx"] if "cx" in d else W / 2
        cy = d["cy"] if "cy" in d else H / 2
        fish = bool(d.get("is_fisheye", False)) or d.get("camera_model") in _FISHEYE_NAMES
        s = float(downscale)
        return cls(fx / s, fy / s, cx / s, cy / s, model=FISHEYE if fish else OPENCV, **{k: d.get(k, 0.0) for k in _COEFFS})

    def record(self):
        """the LAE_CAM_FLOATS values of the C ABI, as float64"""
        return np.array([self.model, self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.k3, self.k4, self.p1, self.p2, 0.0])

    @property
    def distorted(self):
        return any(getattr(self, k) != 0.0 for k in _COEFFS) or self.model == FISHEYE

    def distort(self, x, y, dtype=np.float64):
        """the forward model: ideal normalised (x, y) -> distorted (xd, yd)"""
        return _distort(self.record().astype(dtype), np.asarray(x, dtype), np.asarray(y, dtype), dtype)

    def undistort_points(self, xd, yd, iters=NEWTON_ITERS, dtype=np.float64):
        """the inverse: distorted normalised (xd, yd) -> ideal (x, y) and the converged flags (NaN where not converged)"""
        return _undistort(self.record().astype(dtype), np.asarray(xd, dtype), np.asarray(yd, dtype), int(iters), dtype)

    def __repr__(self):
        return "CameraModel(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


# ------------------------------------------------------------------------------------------------------------- restatements
# Statement for statement the kernels of csrc/undistort.hip; `dt` is the arithmetic (np.float32: the kernel's own roundings).
def _distort(c, x, y, dt):
    k1, k2, k3, k4, p1, p2 = c[5:11]
    two = dt(2)
    r2 = x * x + y * y
    if c[0] == OPENCV:
        rad = dt(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (x * rad + (two * p1) * (x * y)) + p2 * (r2 + two * (x * x))
        yd = (y * rad + p1 * (r2 + two * (y * y))) + (two * p2) * (x * y)
        return xd, yd
    r = np.sqrt(r2)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (dt(1) + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 0, thd / np.where(r > 0, r, dt(1)), dt(1)).astype(dt)
    return x * s, y * s


def _undistort(c, xd, yd, iters, dt):
    fx, fy = c[1], c[2]
    k1, k2, k3, k4, p1, p2 = c[5:11]
    one, two, tol = dt(1), dt(2), dt(TOL_PX)
    with np.errstate(all="ignore"):
        if c[0] == OPENCV:
            x, y = xd.copy(), yd.copy()
            for _ in range(iters):
                r2 = x * x + y * y
                rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
                drad = k1 + r2 * (two * k2 + (dt(3) * k3) * r2)
                fxv = ((x * rad + (two * p1) * (x * y)) + p2 * (r2 + two * (x * x))) - xd
                fyv = ((y * rad + p1 * (r2 + two * (y * y))) + (two * p2) * (x * y)) - yd
                cross = (two * (x * y)) * drad + (two * p1) * x + (two * p2) * y
                jxx = (rad + (two * (x * x)) * drad) + (two * p1) * y + (dt(6) * p2) * x
                jyy = (rad + (two * (y * y)) * drad) + (dt(6) * p1) * y + (two * p2) * x
                det = jxx * jyy - cross * cross
                x, y = x - (jyy * fxv - cross * fyv) / det, y - (jxx * fyv - cross * fxv) / det
            xe, ye = _distort(c, x, y, dt)
            ok = (np.abs(xe - xd) * fx <= tol) & (np.abs(ye - yd) * fy <= tol)
        else:
            rd = np.sqrt(xd * xd + yd * yd)
            th = rd.copy()

            def poly(t2):
                return one + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
            for _ in range(iters):
                t2 = th * th
                f = th * poly(t2) - rd
                df = one + t2 * (dt(3) * k1 + t2 * (dt(5) * k2 + t2 * (dt(7) * k3 + t2 * (dt(9) * k4))))
                th = th - f / df
            res = th * poly(th * th) - rd
            ok = (np.abs(res) * max(fx, fy) <= tol) & (th >= 0) & (th < dt(np.float32(np.pi / 2)))
            s = np.where(rd > 0, np.tan(th) / np.where(rd > 0, rd, one), one).astype(dt)
            x, y = xd * s, yd * s
    nan = dt(np.nan)
    return np.where(ok, x, nan).astype(dt), np.where(ok, y, nan).astype(dt), ok


def _records(cams, dt=np.float64):
    cams = [cams] if isinstance(cams, CameraModel) else list(cams)
    if not cams or any(not isinstance(c, CameraModel) for c in cams):
        raise ValueError("undistort: cams must be a CameraModel or a non-empty list of them")
    return np.stack([c.record() for c in cams]).astype(dt)


def _target(target, H, W):
    if len(target) != 4:
        raise ValueError("undistort: target = (fx, fy, cx, cy)")
    t = tuple(float(v) for v in target)
    if not (t[0] > 0 and t[1] > 0) or not np.isfinite(t).all() or not (1 <= int(H) <= MAX_SIDE and 1 <= int(W) <= MAX_SIDE):
        raise ValueError(f"undistort: focal lengths must be positive, every value finite and 1 <= H, W <= {MAX_SIDE}")
    return t


def _grid(H, W, cx, cy, fx, fy, dt):
    i = (np.arange(W, dtype=dt) + dt(0.5)) - dt(cx)
    j = (np.arange(H, dtype=dt) + dt(0.5)) - dt(cy)
    x, y = np.meshgrid(i / dt(fx), j / dt(fy))
    return x.astype(dt), y.astype(dt)


def undistort_map_numpy(cams, target, H, W, dtype=np.float64):
    """lae_undistort_map restated: -> [n_cam, H, W, 2] of `dtype`, the source position of every target pixel"""
    fx, fy, cx, cy = _target(target, H, W)
    dt = np.dtype(dtype).type
    x, y = _grid(H, W, cx, cy, fx, fy, dt)
    out = []
    for c in _records(cams, dt):
        xd, yd = _distort(c, x, y, dt)
        out.append(np.stack([(xd * c[1] + c[3]) - dt(0.5), (yd * c[2] + c[4]) - dt(0.5)], -1))
    return np.stack(out).astype(dt)


def distort_map_numpy(cams, Hs, Ws, target, iters=NEWTON_ITERS, dtype=np.float64):
    """lae_distort_map restated: -> ([n_cam, Hs, Ws, 2] of `dtype`: the target position of every source pixel, NaN where the
    Newton iteration did not converge; converged uint8 [n_cam, Hs, Ws])"""
    fx, fy, cx, cy = _target(target, Hs, Ws)
    dt = np.dtype(dtype).type
    maps, conv = [], []
    for c in _records(cams, dt):
        xd, yd = _grid(Hs, Ws, c[3], c[4], c[1], c[2], dt)
        x, y, ok = _undistort(c, xd, yd, int(iters) or NEWTON_ITERS, dt)
        maps.append(np.stack([(x * dt(fx) + dt(cx)) - dt(0.5), (y * dt(fy) + dt(cy)) - dt(0.5)], -1))
        conv.append(ok.astype(np.uint8))
    return np.stack(maps).astype(dt), np.stack(conv)


def remap_numpy(src, map, cam_index=None, mode="bilinear", return_valid=False, dtype=np.float64, pre=False):
    """lae_remap restated: src [n, Hs, Ws, C] (uint8, float16 or float32; C = 1, 3 or 4) through map [n_cam, Ht, Wt, 2], taken
    as given (the kernel's own fp32 map separates coordinate error from interpolation error), arithmetic in `dtype`.
    -> dst [n, Ht, Wt, C] of src's dtype, or (dst, valid uint8 [n, Ht, Wt]); pre=True: the values before the last rounding, as `dtype`"""
    src, m = np.asarray(src), np.asarray(map)
    if src.ndim != 4 or src.shape[-1] not in (1, 3, 4) or src.dtype not in (np.uint8, np.float16, np.float32):
        raise ValueError("remap_numpy: src must be [n, Hs, Ws, 1 | 3 | 4] of uint8, float16 or float32")
    if m.ndim != 4 or m.shape[-1] != 2 or mode not in MODES:
        raise ValueError("remap_numpy: map must be [n_cam, Ht, Wt, 2], mode 'bilinear' or 'nearest'")
    dt = np.dtype(dtype).type
    n, Hs, Ws, C = src.shape
    idx = np.zeros(n, np.int64) if cam_index is None else np.asarray(cam_index, np.int64)
    cam_ok = (idx >= 0) & (idx < m.shape[0])
    s = m[np.where(cam_ok, idx, 0)]                                   # [n, Ht, Wt, 2]
    sx, sy = s[..., 0], s[..., 1]
    img = np.arange(n)[:, None, None]
    if mode == "nearest":
        half = sx.dtype.type(0.5)                                     # the sums in the map's own precision, as the kernel's
        xr, yr = np.floor(sx + half), np.floor(sy + half)
        ok = (xr >= 0) & (xr <= Ws - 1) & (yr >= 0) & (yr <= Hs - 1) & cam_ok[:, None, None]
        xi, yi = np.where(ok, xr, 0).astype(np.int64), np.where(ok, yr, 0).astype(np.int64)
        val = src[img, yi, xi].astype(dt)
    else:
        ok = (sx >= 0) & (sx <= Ws - 1) & (sy >= 0) & (sy <= Hs - 1) & cam_ok[:, None, None]
        sx, sy = np.where(ok, sx, 0).astype(dt), np.where(ok, sy, 0).astype(dt)
        x0f, y0f = np.floor(sx), np.floor(sy)
        ax, ay = (sx - x0f)[..., None], (sy - y0f)[..., None]
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
        bx, by = dt(1) - ax, dt(1) - ay
        w = (bx * by, ax * by, bx * ay, ax * ay)
        p = tuple(src[img, yy, xx].astype(dt) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))

        def acc(t):
            return ((w[0] * t[0] + w[1] * t[1]) + w[2] * t[2]) + w[3] * t[3]
        if C == 4:
            A = acc(tuple(q[..., 3:4] for q in p))
            P = acc(tuple(q[..., :3] * q[..., 3:4] for q in p))
            with np.errstate(invalid="ignore", divide="ignore"):
                col = np.where(A != 0, P / np.where(A != 0, A, dt(1)), dt(0))
            val = np.concatenate([col, A], -1).astype(dt)
        else:
            val = acc(p).astype(dt)
    val = np.where(ok[..., None], val, dt(0)).astype(dt)
    if pre:
        out = val
    elif src.dtype == np.uint8:
        out = np.clip(np.floor(val + dt(0.5)), 0, 255).astype(np.uint8)
    else:
        out = val.astype(src.dtype)
    return (out, ok.astype(np.uint8)) if return_valid else out


def undistort_numpy(images, cams, target, H, W, cam_index=None, mode="bilinear", dtype=np.float64, return_valid=False):
    """images [n, Hs, Ws, C] captured by `cams` resampled into the pinhole `target` of H x W: undistort_map_numpy, then remap_numpy,
    both in `dtype`"""
    return remap_numpy(images, undistort_map_numpy(cams, target, H, W, dtype), cam_index, mode, return_valid, dtype)


# ---------------------------------------------------------------------------------------------------------- the target camera
def _border(H, W, inner=0):
    """pixel indices (i, j) of the frame's border, plus a coarse interior lattice"""
    i, j = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    bi = np.concatenate([i, i, np.zeros(H), np.full(H, W - 1.0)])
    bj = np.concatenate([np.zeros(W), np.full(W, H - 1.0), j, j])
    if inner:
        gi, gj = np.meshgrid(np.linspace(0, W - 1, inner), np.linspace(0, H - 1, inner))
        bi, bj = np.concatenate([bi, gi.ravel()]), np.concatenate([bj, gj.ravel()])
    return bi, bj


def target_intrinsics(cams, H, W, balance=0.0):
    """the pinhole camera (fx, fy, cx, cy) to resample H x W captures of `cams` into, in float64 on the host: the cameras' mean
    focal lengths times one scale s, their mean principal point, the same size.
      balance = 0   the smallest zoom at which every target pixel is valid for every camera (found to within a thirtieth of a
                    source pixel: the source positions of the target frame's border, and of a coarse interior lattice, stay
                    1/64 pixel inside the source frame -- the fp32 map's error is below 1e-3 pixel at 3840 x 2160 -- so the
                    kernel's valid plane is all ones too)
      balance = 1   every source pixel centre lands inside the target frame [-0.5, W - 0.5] x [-0.5, H - 0.5]
    and linear in s in between."""
    rec = _records(cams)
    H, W = int(H), int(W)
    if not 0.0 <= float(balance) <= 1.0:
        raise ValueError("target_intrinsics: balance must be in [0, 1]")
    fx0, fy0, cx, cy = (float(rec[:, k].mean()) for k in (1, 2, 3, 4))
    bi, bj = _border(H, W, inner=33)

    def all_valid(s):
        x, y = (bi + 0.5 - cx) / (s * fx0), (bj + 0.5 - cy) / (s * fy0)
        for c in rec:
            xd, yd = _distort(c, x, y, np.float64)
            sx, sy = xd * c[1] + c[3] - 0.5, yd * c[2] + c[4] - 0.5
            m = min(1.0 / 64, (W - 1) / 2.0, (H - 1) / 2.0)
            if not ((sx >= m) & (sx <= W - 1 - m) & (sy >= m) & (sy <= H - 1 - m)).all():
                return False
        return True
    lo = hi = 1.0
    if all_valid(1.0):
        while all_valid(lo) and lo > 1e-3:
            hi, lo = lo, lo / 1.05
    else:
        while not all_valid(hi) and hi < 1e3:
            lo, hi = hi, hi * 1.05
    if not all_valid(hi) or all_valid(lo):
        raise RuntimeError("target_intrinsics: no zoom in [1e-3, 1e3] brackets the valid frame (are the coefficients those of this lens?)")
    while (hi - lo) * max(H, W) > lo / 64:                            # a border position moves by about (hi - lo) / lo * max(H, W) / 2 pixels
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if all_valid(mid) else (mid, hi)
    s0 = hi
    s = s0
    if balance > 0.0:
        si, sj = _border(H, W)
        bounds = []
        for c in rec:
            x, y, ok = _undistort(c, (si + 0.5 - c[3]) / c[1], (sj + 0.5 - c[4]) / c[2], 2 * NEWTON_ITERS, np.float64)
            x, y = x[ok], y[ok]
            # -0.5 <= x s fx0 + cx - 0.5 <= W - 0.5
            with np.errstate(divide="ignore"):
                bounds += [np.min((W - cx) / (fx0 * x[x > 0]), initial=np.inf), np.min(cx / (fx0 * -x[x < 0]), initial=np.inf),
                           np.min((H - cy) / (fy0 * y[y > 0]), initial=np.inf), np.min(cy / (fy0 * -y[y < 0]), initial=np.inf)]
        s1 = min(bounds)
        if np.isfinite(s1):
            s = s0 + float(balance) * (s1 - s0)
    return (s * fx0, s * fy0, cx, cy)


# -------------------------------------------------------------------------------------------------------------- the operators
def _torch():
    import torch
    from .backend import undistort_backend
    return torch, undistort_backend


def _host_cams(cams):
    return np.ascontiguousarray(_records(cams, np.float32))


def undistort_map(cams, target, H, W, device=None):
    """lae_undistort_map: -> fp32 [n_cam, H, W, 2] on the device, the source position of every pixel of the pinhole `target`"""
    torch, backend = _torch()
    target = _target(target, H, W)
    rec = _host_cams(cams)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(len(rec), int(H), int(W), 2, dtype=torch.float32, device=device)
    backend.undistort_map(rec, target, H, W, out)
    return out


def distort_map(cams, Hs, Ws, target, iters=0, device=None):
    """lae_distort_map: -> (fp32 [n_cam, Hs, Ws, 2] on the device: the position in the pinhole `target` of every source pixel,
    NaN where the Newton iteration did not converge; converged uint8 [n_cam, Hs, Ws]).  iters = 0: NEWTON_ITERS."""
    torch, backend = _torch()
    target = _target(target, Hs, Ws)
    if not 0 <= int(iters) <= 64:
        raise ValueError("distort_map: iters must be in [0, 64]")
    rec = _host_cams(cams)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(len(rec), int(Hs), int(Ws), 2, dtype=torch.float32, device=device)
    conv = torch.empty(len(rec), int(Hs), int(Ws), dtype=torch.uint8, device=device)
    backend.distort_map(rec, Hs, Ws, target, iters, out, conv)
    return out, conv


def remap(src, map, cam_index=None, mode="bilinear", return_valid=False, out=None, valid=None):
    """lae_remap: src [n, Hs, Ws, C] on the device (uint8, fp16 or fp32; C = 1, 3 or 4) through map fp32 [n_cam, Ht, Wt, 2];
    cam_index int32 [n] on the device picks each image's map, None shares map[0].  mode 'bilinear' (RGBA interpolated
    premultiplied by alpha) or 'nearest' (masks, depth and weight planes).  -> dst [n, Ht, Wt, C] of src's dtype, or
    (dst, valid uint8 [n, Ht, Wt]); an invalid output is all zeros.  out / valid: buffers to write into (a captured call)."""
    torch, backend = _torch()
    codes = backend.DTYPES
    if not torch.is_tensor(src) or src.dim() != 4 or src.shape[-1] not in (1, 3, 4) or src.dtype not in codes or not src.is_contiguous():
        raise ValueError("remap: src must be a contiguous [n, Hs, Ws, 1 | 3 | 4] tensor of uint8, float16 or float32")
    if not torch.is_tensor(map) or map.dim() != 4 or map.shape[-1] != 2 or map.dtype != torch.float32 or not map.is_contiguous() or \
            map.shape[0] < 1:
        raise ValueError("remap: map must be a contiguous fp32 tensor [n_cam, Ht, Wt, 2]")
    if mode not in MODES:
        raise ValueError("remap: mode must be 'bilinear' or 'nearest'")
    n, Hs, Ws, C = (int(v) for v in src.shape)
    Ht, Wt = (int(v) for v in map.shape[1:3])
    if cam_index is not None and (not torch.is_tensor(cam_index) or cam_index.dtype != torch.int32 or tuple(cam_index.shape) != (n,) or
                                  not cam_index.is_contiguous()):
        raise ValueError(f"remap: cam_index must be a contiguous int32 tensor [{n}]")
    if out is None:
        out = torch.empty(n, Ht, Wt, C, dtype=src.dtype, device=src.device)
    elif tuple(out.shape) != (n, Ht, Wt, C) or out.dtype != src.dtype or not out.is_contiguous():
        raise ValueError(f"remap: out must be a contiguous {src.dtype} tensor [{n}, {Ht}, {Wt}, {C}]")
    if valid is None and return_valid:
        valid = torch.empty(n, Ht, Wt, dtype=torch.uint8, device=src.device)
    elif valid is not None and (tuple(valid.shape) != (n, Ht, Wt) or valid.dtype != torch.uint8 or not valid.is_contiguous()):
        raise ValueError(f"remap: valid must be a contiguous uint8 tensor [{n}, {Ht}, {Wt}]")
    backend.remap(src, map, cam_index, MODES[mode], out, valid)
    return (out, valid) if return_valid or valid is not None else out


class Undistorter:
    """the maps of one scene.  cams: the source cameras (CameraModel or a list), cam_index: per image the index of its camera
    (None: every image is cams[0]'s), target (fx, fy, cx, cy): the pinhole camera of H x W to resample into, src_hw: the
    captures' size (default H x W).  maps / inverse: maps computed before (undistort_map / distort_map's results), else they are
    computed on first use on `device`.
      .images(x)            captures [n, Hs, Ws, C] -> the pinhole camera's [n, H, W, C], bilinear
      .plane(x, mode)       a plane [n, Hs, Ws] (mask, depth, weights) -> [n, H, W], nearest by default
      .valid                uint8 [n_img, H, W]: 1 where .images' pixel lies inside its capture
      .redistort(frames)    frames [n, H, W, C] rendered in the pinhole camera -> the capture's geometry [n, Hs, Ws, C], for
                            comparison with the original photographs; return_valid=True adds the uint8 plane [n, Hs, Ws]
      .distort_images(x)    the same resampling under the name the tools use: synthetic distorted captures of pinhole images"""

    def __init__(self, cams, cam_index, target, H, W, src_hw=None, device=None, maps=None, inverse=None):
        torch, _ = _torch()
        self.cams = [cams] if isinstance(cams, CameraModel) else list(cams)
        _records(self.cams)
        self.H, self.W = int(H), int(W)
        self.target = _target(target, H, W)
        self.Hs, self.Ws = (self.H, self.W) if src_hw is None else (int(src_hw[0]), int(src_hw[1]))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        idx = None
        if cam_index is not None:
            idx = np.asarray(cam_index.cpu() if torch.is_tensor(cam_index) else cam_index, dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= len(self.cams)):
                raise ValueError(f"Undistorter: cam_index must lie in [0, {len(self.cams)})")
        self._idx_host = idx
        self.cam_index = None if idx is None else torch.from_numpy(idx.astype(np.int32)).to(self.device)
        self._maps, self._inverse, self._valid = maps, inverse, None

    @property
    def maps(self):
        if self._maps is None:
            self._maps = undistort_map(self.cams, self.target, self.H, self.W, self.device)
        return self._maps

    @property
    def inverse(self):
        """(map fp32 [n_cam, Hs, Ws, 2], converged uint8 [n_cam, Hs, Ws])"""
        if self._inverse is None:
            self._inverse = distort_map(self.cams, self.Hs, self.Ws, self.target, device=self.device)
        return self._inverse

    def _index(self, n):
        if self.cam_index is None:
            return None
        if self.cam_index.numel() != n:
            raise ValueError(f"Undistorter: {n} images for {self.cam_index.numel()} camera indices")
        return self.cam_index

    def _apply(self, x, m, hw, mode, return_valid, who):
        torch, _ = _torch()
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x))
        plane = x.dim() == 3
        if plane:
            x = x.unsqueeze(-1)
        if x.dim() != 4 or tuple(x.shape[1:3]) != hw:
            raise ValueError(f"Undistorter.{who}: expected [n, {hw[0]}, {hw[1]}{'' if plane else ', C'}], got {list(x.shape)}")
        r = remap(x.to(self.device).contiguous(), m, self._index(x.shape[0]), mode, return_valid)
        if not plane:
            return r
        return (r[0].squeeze(-1), r[1]) if return_valid else r.squeeze(-1)

    def images(self, x, return_valid=False):
        return self._apply(x, self.maps, (self.Hs, self.Ws), "bilinear", return_valid, "images")

    def plane(self, x, mode="nearest", return_valid=False):
        return self._apply(x, self.maps, (self.Hs, self.Ws), mode, return_valid, "plane")

    @property
    def valid(self):
        if self._valid is None:
            torch, _ = _torch()
            ones = torch.ones(len(self.cams), self.Hs, self.Ws, 1, dtype=torch.uint8, device=self.device)
            per_cam = remap(ones, self.maps, torch.arange(len(self.cams), dtype=torch.int32, device=self.device), "bilinear", True)[1]
            self._valid = per_cam if self.cam_index is None else per_cam[self.cam_index.long()].contiguous()
        return self._valid

    def redistort(self, frames, mode="bilinear", return_valid=False):
        return self._apply(frames, self.inverse[0], (self.H, self.W), mode, return_valid, "redistort")

    def distort_images(self, x, mode="bilinear", return_valid=False):
        return self.redistort(x, mode, return_valid)
