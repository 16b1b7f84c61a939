"""The cameras, shapes, inputs and bounds that tests/test_undistort_cpu.py and tests/test_gpu_undistort.py share.  The CPU file
asserts, for these very inputs, what the GPU file relies on."""
import functools
import json
import os

import numpy as np

from laenerf_amd.undistort import FISHEYE, CameraModel, distort_map_numpy, undistort_map_numpy

# source frames 40 x 56 and 33 x 47 (H x W), wide lenses: fx about W / 2, so the corners sit at r2 of about 1.5
SRC_A, SRC_B = (40, 56), (33, 47)
CAMS_A = (CameraModel(28.0, 27.0, 27.3, 19.6, k1=-0.3, k2=0.09, p1=0.004, p2=-0.003),           # a strong barrel, decentred
          CameraModel(30.0, 30.5, 28.2, 20.4, k1=0.12, k2=-0.02, k3=0.003, p1=-0.002, p2=0.001),  # a pincushion
          CameraModel(28.5, 28.0, 27.5, 20.2, k1=-0.04, k2=0.01, k3=-0.002, k4=0.0005, model=FISHEYE))
CAMS_B = (CameraModel(23.0, 23.5, 23.1, 16.2, k1=-0.25, k2=0.06, p1=-0.003, p2=0.002),)
# targets 37 x 53 and 16 x 16: other sizes than the sources', fields of view that reach past the sources' frames
TGT_A, TGT_B = (37, 53, (25.0, 24.5, 26.1, 18.7)), (16, 16, (7.5, 7.0, 8.2, 7.6))
# (name, cameras, source size, (Ht, Wt, target intrinsics))
MAP_CASES = (("three_37x53", CAMS_A, SRC_A, TGT_A), ("one_16x16", CAMS_B, SRC_B, TGT_B), ("three_16x16", CAMS_A, SRC_A, TGT_B))
# the shuffled per-image camera index of the n_cam = 3 cases
CAM_INDEX = np.array([2, 0, 1, 1, 0, 2, 0], np.int32)

# the 3840 x 2160 camera of scripts/colmap2nerf.py's example and a strong barrel on it
CAM_4K = CameraModel(3000.0, 3000.0, 1920.0, 1080.0, k1=0.16, k2=-0.23)
CAM_4K_BARREL = CameraModel(1900.0, 1900.0, 1925.0, 1071.0, k1=-0.3, k2=0.09, p1=0.001, p2=-0.002)

# Map bounds, in ulps of max(H, W) (the spacing of fp32 at that value): three times the largest difference between the float32
# and the float64 restatement, which tests/test_undistort_cpu.py prints and asserts to be at most these MEASURED figures.  The
# factor three: the compiler may contract or order the kernel's sums differently, and atanf / tanf are another library's.
MEASURED_MAP_ULPS = {"three_37x53": 2.3, "one_16x16": 1.1, "three_16x16": 2.3}
MEASURED_INVERSE_ULPS = {"three_37x53": 4.9, "one_16x16": 0.8, "three_16x16": 1.5}
EPS32 = 2.0 ** -24


def ulp_of(v):
    return float(np.spacing(np.float32(v)))


def map_tol(name, measured=MEASURED_MAP_ULPS):
    _, _, src, tgt = next(c for c in MAP_CASES if c[0] == name)
    return 3.0 * measured[name] * ulp_of(max(tgt[0], tgt[1], *src))


@functools.lru_cache(None)
def maps(name, dtype="float64"):
    _, cams, _, (H, W, t) = next(c for c in MAP_CASES if c[0] == name)
    m = undistort_map_numpy(cams, t, H, W, np.dtype(dtype))
    m.setflags(write=False)
    return m


@functools.lru_cache(None)
def inverse_maps(name, dtype="float64"):
    _, cams, (Hs, Ws), (H, W, t) = next(c for c in MAP_CASES if c[0] == name)
    m, ok = distort_map_numpy(cams, Hs, Ws, t, dtype=np.dtype(dtype))
    m.setflags(write=False); ok.setflags(write=False)
    return m, ok


# lae_remap's bounds.  With the kernel's own fp32 map the weights' inputs are exact, so what is left is fp32 rounding of:
# 1 - a (1), the weight's product (1), colour x alpha (1, C = 4), weight x value (1), three sums (3) -- at most 7 roundings on a
# sum of non-negative terms, each relative 2^-24: |v32 - v| <= 7 eps |v| for A and for P, and the quotient P / A adds both and its
# own rounding: 15 eps.  REMAP_RELATIVE = 16 eps covers both; it scales with the largest value M of the source.
REMAP_RELATIVE = 16 * EPS32
HALF_CAP = 0.005                    # share of uint8 outputs that may sit within the bound of a half-integer before rounding


def float_tol(M, dtype):
    """|kernel - float64 restatement| for a float output: the accumulation bound, plus half an fp16 ulp (2^-11 relative, 2^-25 in
    the subnormals) where the output is rounded to fp16"""
    t = REMAP_RELATIVE * M
    return t + (2.0 ** -11 * M + 2.0 ** -25 if np.dtype(dtype) == np.float16 else 0.0)


def images(n, H, W, C, dtype, seed=0):
    """smooth-plus-noise images with transparent (alpha 0, arbitrary colour) blocks next to opaque ones"""
    g = np.random.default_rng([seed, H, W, C])
    v = g.random((n, H, W, C))
    if C == 4:
        a = np.ones((n, H, W))
        a[:, : H // 2, W // 3:] = 0.0                                   # a hard edge: alpha 0 with arbitrary colour beside alpha 1
        a[:, H // 2:, : W // 4] = g.random((n, H - H // 2, W // 4))
        v[..., 3] = a
    if np.dtype(dtype) == np.uint8:
        return np.floor(v * 255.0 + 0.5).astype(np.uint8)
    return v.astype(dtype)


def write_scene(root, n=5, H=40, W=56, cam=None, per_frame=False, rgba=True, seed=3):
    """a blender-style scene under `root` written with PIL: n frames of H x W, the keys of `cam` (and, with per_frame, a second
    camera's keys on the odd frames).  -> (path of transforms.json, images uint8 [n, H, W, C], poses [n, 4, 4], cameras per frame)"""
    from PIL import Image
    g = np.random.default_rng(seed)
    C = 4 if rgba else 3
    ims = images(n, H, W, C, np.uint8, seed)
    t = {"w": W, "h": H, "frames": []}
    cams = []
    if cam is not None:
        t.update(fl_x=cam.fx, fl_y=cam.fy, cx=cam.cx, cy=cam.cy, k1=cam.k1, k2=cam.k2, p1=cam.p1, p2=cam.p2)
        if cam.model == FISHEYE:
            t.update(is_fisheye=True, k3=cam.k3, k4=cam.k4)
    else:
        t.update(fl_x=30.0, fl_y=31.0)
    poses = []
    for k in range(n):
        Image.fromarray(ims[k]).save(os.path.join(root, f"r_{k}.png"))
        a = 2 * np.pi * k / n
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, R @ np.array([0, 0, 2.5]) + 0.05 * g.standard_normal(3)
        fr = {"file_path": f"r_{k}", "transform_matrix": m.tolist()}
        c = cam
        if per_frame and k % 2:
            c = CameraModel(cam.fx * 1.05, cam.fy * 1.05, cam.cx - 0.4, cam.cy + 0.3, k1=cam.k1 * 0.8, k2=cam.k2, p1=cam.p1, p2=cam.p2)
            fr.update(fl_x=c.fx, fl_y=c.fy, cx=c.cx, cy=c.cy, k1=c.k1)
        cams.append(c)
        t["frames"].append(fr)
        poses.append(m)
    path = os.path.join(root, "transforms.json")
    with open(path, "w") as f:
        json.dump(t, f)
    return path, ims, np.stack(poses), cams
