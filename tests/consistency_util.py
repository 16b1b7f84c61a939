"""The two-view scene of the consistency tests, built in float64 and handed over as fp32.

A far plane z = 4 and a near occluder |x| < 0.4, |y| < 0.3 at z = 2, seen by camera a (the identity pose) and camera b (a 0.03 rad
yaw, translated by (0.15, 0.02, 0.01)); fx = fy = 40, cx = W / 2, cy = H / 2.  The colours are smooth functions of the hit point
and the occluder's differ from the plane's; no two neighbouring pixels differ by 0.2 or more in any channel (the identity-pair
bound of tests/test_gpu_consistency.py rests on that; tests/test_consistency_cpu.py asserts it).  Opacity is 1 except in rows 0-1,
where it is 0.2: transparent, the geometry is undefined there.  D = t * A.  The disparity of the far plane is fx * 0.15 / 4 = 1.5 px,
of the occluder 3 px."""
import functools

import numpy as np

SHAPES = [(24, 40), (37, 53)]       # neither pixel count is a multiple of 256; the second is odd both ways
YAW = 0.03
SHIFT = (0.15, 0.02, 0.01)
FOCAL = 40.0


def poses():
    c, s = np.cos(YAW), np.sin(YAW)
    Pb = np.eye(4)
    Pb[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    Pb[:3, 3] = SHIFT
    return np.eye(4), Pb


def render(P, H, W, opaque_everywhere=False):
    """one view of the scene in float64 -> frame [H,W,3], depth D = t * A [H,W], opacity A [H,W], occluder mask [H,W]"""
    cx, cy = W / 2, H / 2
    gx, gy = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(gx + 0.5 - cx) / FOCAL, (gy + 0.5 - cy) / FOCAL, np.ones_like(gx)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d @ P[:3, :3].T
    o = P[:3, 3]
    t2 = (2.0 - o[2]) / d[..., 2]
    hit2 = o + t2[..., None] * d
    near = (np.abs(hit2[..., 0]) < 0.4) & (np.abs(hit2[..., 1]) < 0.3)
    t = np.where(near, t2, (4.0 - o[2]) / d[..., 2])
    X = o + t[..., None] * d
    x, y = X[..., 0], X[..., 1]
    plane = np.stack([0.45 + 0.05 * np.sin(1.3 * x + 0.4 * y), 0.50 + 0.05 * np.cos(0.9 * y - 0.5 * x), 0.40 + 0.05 * np.sin(0.7 * (x + y))], -1)
    occl = np.stack([0.57 + 0.03 * np.sin(3 * x), 0.38 + 0.03 * np.cos(4 * y), 0.52 + 0.03 * np.sin(2 * x - 3 * y)], -1)
    frame = np.where(near[..., None], occl, plane)
    A = np.ones((H, W))
    if not opaque_everywhere:
        A[:2] = 0.2
    return frame, t * A, A, near


@functools.lru_cache(maxsize=None)
def fixture(H, W):
    """-> dict of fp32 arrays frame_a, frame_b [H,W,3], depth_a, opacity_a, depth_b, opacity_b [H,W], pose_a, pose_b [4,4], the
    intrinsics tuple, and the bool occluder masks near_a, near_b.  Cached: do not write into the arrays."""
    Pa, Pb = poses()
    out = {"pose_a": Pa.astype(np.float32), "pose_b": Pb.astype(np.float32), "intrinsics": (FOCAL, FOCAL, W / 2, H / 2), "H": H, "W": W}
    for v, P in (("a", Pa), ("b", Pb)):
        frame, D, A, near = render(P, H, W)
        out["frame_" + v], out["depth_" + v], out["opacity_" + v] = frame.astype(np.float32), D.astype(np.float32), A.astype(np.float32)
        out["near_" + v] = near
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def args(fx, **over):
    """the positional arguments of consistency_numpy / the array arguments of consistency_pair, in order"""
    f = dict(fx, **over)
    return (f["frame_a"], f["frame_b"], f["depth_a"], f["opacity_a"], f["depth_b"], f["opacity_b"], f["pose_a"], f["pose_b"],
            f["intrinsics"], f["H"], f["W"])


@functools.lru_cache(maxsize=None)
def restated(H, W, dtype="float64", identity=False):
    """consistency_numpy on the fixture (identity: the pair (a, a)), computed once per shape and dtype"""
    from laenerf_amd.metrics import consistency_numpy
    f = fixture(H, W)
    if identity:
        return consistency_numpy(*args(f, frame_b=f["frame_a"], depth_b=f["depth_a"], opacity_b=f["opacity_a"], pose_b=f["pose_a"]),
                                 dtype=np.dtype(dtype))
    return consistency_numpy(*args(f), dtype=np.dtype(dtype))
