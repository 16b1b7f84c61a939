"""Times of undistortion on the device (csrc/undistort.hip) against the same rule written with torch operators.

    python tools/undistort_bench.py [--views 100] [--res 800] [--reps 200]

Prints one JSON line:
  kernels   per resolution (800 x 800 and 3840 x 2160, uint8 RGBA, a barrel lens): lae_undistort_map and lae_distort_map in us with
            the floor of their 8 (+ 1) bytes per pixel written; lae_remap (bilinear, one image, no valid plane) in us with its HBM
            floor -- bytes in plus bytes out: 4 of the image and 8 of the map read, 4 written per pixel -- and the torch chain
            (to float, premultiply by alpha, F.grid_sample over the same map, divide, round, to uint8) with the share of bytes on
            which the two differ (grid_sample pads with zeros where the kernel declares the pixel invalid, and rounds half to even)
  loader    ResidentImages.from_transforms on --views PNG frames of --res x --res written to a temporary directory: seconds end to
            end with undistort=False and undistort=True (two passes each, alternating; PNG decoding on the host dominates both),
            and the device part alone (upload of the captures + maps + remap) between two synchronisations"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29                 # measured float4-copy bandwidth of one MI355X (tools/eval_bench.py)


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps             # us


def torch_chain(src, m):
    """the rule of lae_remap (bilinear, RGBA uint8) with torch operators: src uint8 [n, H, W, 4], m fp32 [Ht, Wt, 2] -> uint8 [n, Ht, Wt, 4]"""
    n, Hs, Ws, _ = src.shape
    x = src.permute(0, 3, 1, 2).float()
    x = torch.cat([x[:, :3] * x[:, 3:], x[:, 3:]], 1)
    grid = torch.stack([(2 * m[..., 0] + 1) / Ws - 1, (2 * m[..., 1] + 1) / Hs - 1], -1)[None].expand(n, -1, -1, -1)
    y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    a = y[:, 3:]
    rgb = torch.where(a != 0, y[:, :3] / a, torch.zeros_like(y[:, :3]))
    return torch.cat([rgb, a], 1).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def kernel_row(dev, H, W, reps):
    from laenerf_amd.undistort import CameraModel, distort_map, remap, target_intrinsics, undistort_map
    cam = CameraModel(0.6 * W, 0.6 * W, W / 2 + 3.5, H / 2 - 2.25, k1=-0.3, k2=0.09, p1=0.001, p2=-0.002)
    target = target_intrinsics(cam, H, W, 0.0)
    g = torch.Generator(device=dev).manual_seed(H)
    src = torch.randint(0, 256, (1, H, W, 4), dtype=torch.uint8, device=dev, generator=g)
    m = undistort_map(cam, target, H, W, dev)
    out = torch.empty_like(src)
    px = H * W
    row = {"res": [H, W], "target_zoom": round(target[0] / cam.fx, 4)}
    row["undistort_map_us"] = round(_time(lambda: undistort_map(cam, target, H, W, dev), reps), 2)
    row["undistort_map_floor_us"] = round(8 * px / HBM_TBS / 1e6, 2)
    row["distort_map_us"] = round(_time(lambda: distort_map(cam, H, W, target, device=dev), reps), 2)
    row["distort_map_floor_us"] = round(9 * px / HBM_TBS / 1e6, 2)
    row["remap_us"] = round(_time(lambda: remap(src, m, None, "bilinear", out=out), reps), 2)
    row["remap_bytes"] = 16 * px
    row["remap_hbm_floor_us"] = round(16 * px / HBM_TBS / 1e6, 2)
    row["torch_chain_us"] = round(_time(lambda: torch_chain(src, m[0]), max(10, reps // 10)), 2)
    ours, valid = remap(src, m, None, "bilinear", return_valid=True)
    row["valid_frac"] = round(float(valid.float().mean().item()), 6)
    row["torch_chain_bytes_different_frac"] = round(float((torch_chain(src, m[0]) != ours).float().mean().item()), 6)
    return row


def loader_row(dev, views, res):
    from PIL import Image
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.undistort import CameraModel, Undistorter, target_intrinsics
    j, i = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    with tempfile.TemporaryDirectory() as root:
        t = {"w": res, "h": res, "fl_x": 0.6 * res, "fl_y": 0.6 * res, "cx": res / 2 + 3.5, "cy": res / 2 - 2.25, "k1": -0.3, "k2": 0.09,
             "p1": 0.001, "p2": -0.002, "frames": []}
        for k in range(views):                         # smooth frames: the PNG codec's time is part of every loader, not of this feature
            im = np.stack([(i + 2 * k) % 256, (j + 3 * k) % 256, (i + j) % 256, np.where((i - res / 2) ** 2 + (j - res / 2) ** 2 < (0.45 * res) ** 2, 255, 0)], -1)
            Image.fromarray(im.astype(np.uint8)).save(os.path.join(root, f"r_{k}.png"), compress_level=1)
            t["frames"].append({"file_path": f"r_{k}", "transform_matrix": np.eye(4).tolist()})
        path = os.path.join(root, "transforms.json")
        with open(path, "w") as f:
            json.dump(t, f)
        import warnings
        secs = {False: [], True: []}
        for _ in range(2):
            for flag in (False, True):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    data = ResidentImages.from_transforms(path, undistort=flag, device=dev)
                torch.cuda.synchronize()
                secs[flag].append(round(time.perf_counter() - t0, 3))
        host = data.images.cpu()
        cam = CameraModel.from_transforms(t)
        dev_ms = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            und = Undistorter(cam, None, target_intrinsics(cam, res, res), res, res, device=dev)
            und.images(host)
            torch.cuda.synchronize()
            dev_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    return {"views": views, "res": [res, res], "seconds_plain": secs[False], "seconds_undistort": secs[True],
            "upload_maps_remap_ms": dev_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench: needs a GPU (times on a CPU say nothing)")
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    line = {"kernels": [kernel_row(dev, 800, 800, args.reps), kernel_row(dev, 2160, 3840, args.reps)],
            "loader": loader_row(dev, args.views, args.res), "reps": args.reps, "hbm_tbs": HBM_TBS}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
