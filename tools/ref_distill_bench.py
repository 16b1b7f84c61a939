"""Cost of the Ref-NPR distillation stage (laenerf_amd/editing/ref_distill.py): building its data set, and one training step.

    python tools/ref_distill_bench.py [--views 100] [--res 800] [--steps 512] [--rays 4096]

prints one JSON line:
  build: `build_ref_distill_data` over --views synthetic registered views of --res x --res (a disc of extracted pixels per view, a
    quarter of them registered; uint8 RGBA training images) in ms, all-in (moving the host-side views to the device and packing their
    rows, the palette network over the extracted rows, the two launches), the packing alone, and the reference-shaped loop on the same inputs: dataloader_nerf
    (editing/single_view_edit_dataset.py:455-513) restated here view by view with torch indexing -- host tensors moved to the device,
    one network call and five device-to-host copies per view, as the reference; its PNG files are left out.
  step: ms/step of the Trainer as `distill_ref_npr` builds it (pixel_weights=True, second_weight=0.5, depth_weight=1e-3) against the
    default Trainer on the scene of tools/train_loop.py (24 training views of 128 x 128, the planes filled with random weights in
    [0, 2], a random RGBA second target and the teacher's depth): all-in, after the first 64 steps, and five 16-step replay windows
    each."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def synthetic_views(n, res, seed=0):
    """-> uint8 images [n, res, res, 4] and n view dicts on the host, with what build_ref_distill_data reads"""
    rng = np.random.default_rng(seed)
    H = W = res
    yy, xx = np.mgrid[0:H, 0:W]
    disc = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.3 * res) ** 2).reshape(-1)
    idx = torch.from_numpy(np.nonzero(disc)[0].astype(np.int64))
    K = idx.numel()
    images = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    images[..., 3] = np.where(disc.reshape(H, W), 255, 0)
    views = []
    g = torch.Generator().manual_seed(seed)
    for i in range(n):
        reg = torch.sort(torch.randperm(K, generator=g)[:K // 4]).values
        views.append({"pose_idx": i, "indices": idx, "indices_ray_reg": reg, "ref_targets": torch.rand(reg.numel(), 3, generator=g),
                      "target_weights": torch.rand(reg.numel(), generator=g), "x_term": torch.rand(K, 3, generator=g) * 1.6 - 0.8,
                      "dirs": torch.nn.functional.normalize(torch.randn(K, 3, generator=g), dim=-1), "depths": torch.rand(K, generator=g) * 3 + 1,
                      })
    return images, views


@torch.no_grad()
def reference_loop(images, views, style_enc, dev):
    """the shape of dataloader_nerf's loop: per view the host tensors go to the device, five dense planes (weights, target image, style
    image, depth, depth weights) are filled by torch indexing around one call of the network, and each plane is copied to the host"""
    n, H, W, _ = images.shape
    planes = {k: [] for k in ("weights", "target", "style", "depth", "depth_weights")}
    style_enc.eval()
    for v in views:
        img = torch.from_numpy(images[v["pose_idx"]]).to(dev).float().div_(255).view(H * W, 4)
        alpha = img[:, 3]
        pix = v["indices"].to(dev)
        reg_pix = v["indices"][v["indices_ray_reg"]].to(dev)
        weight = torch.zeros(H * W, device=dev)
        weight[reg_pix] = v["target_weights"].to(dev)
        planes["weights"].append((weight + (1 - alpha)).view(H, W).cpu())
        target = torch.zeros_like(img)
        target[:, 3] = alpha
        target[reg_pix, :3] = v["ref_targets"].to(dev)
        planes["target"].append(target.view(H, W, 4).cpu())
        with torch.autocast("cuda", dtype=torch.float16):
            colours = style_enc(v["x_term"].to(dev), d=v["dirs"].to(dev))
        style = torch.zeros_like(img)
        style[pix, 3] = alpha[pix]
        style[pix, :3] = colours.float()
        planes["style"].append(style.view(H, W, 4).cpu())
        depth, on = torch.zeros(H * W, device=dev), torch.zeros(H * W, device=dev)
        depth[pix] = v["depths"].to(dev)
        on[pix] = 1.0
        planes["depth"].append(depth.view(H, W).cpu())
        planes["depth_weights"].append(on.view(H, W).cpu())
    style_enc.train()
    return planes


def _ms(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def bench_build(dev, n, res):
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.editing import LAENeRF, build_ref_distill_data, pack_ref_rows
    images, views = synthetic_views(n, res)
    params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(0)
    enc = LAENeRF(params, dir_encoding="sphere_harmonics").to(dev)
    focal = 0.5 * res / np.tan(0.5 * 0.69)
    data = ResidentImages.from_arrays(images, S.lookat_poses(n, seed=0), (focal, focal, res / 2, res / 2), device=dev)
    build_ref_distill_data(data, views[:2], enc)                                     # warm-up: library load, network workspaces
    reference_loop(images, views[:2], enc, dev)
    pack_ms, _ = _ms(lambda: pack_ref_rows(views, n, res * res, device=dev), dev)
    build_ms, out = _ms(lambda: build_ref_distill_data(data, views, enc), dev)
    ref_ms, ref = _ms(lambda: reference_loop(images, views, enc, dev), dev)
    # the two agree (up to the fp16 store) on a view
    i = n // 2
    same_w = float((out.pixel_weights[i].float().cpu() - ref["weights"][i]).abs().max())
    same_s = float((out.second_target[i].float().cpu() - ref["style"][i]).abs().max())
    K = int(views[0]["indices"].numel())
    return {"views": n, "res": res, "extracted_rows": n * K, "registered_rows": n * (K // 4), "build_ms": round(build_ms, 2),
            "of_which_packing_ms": round(pack_ms, 2), "reference_loop_ms": round(ref_ms, 2),
            "speedup": round(ref_ms / build_ms, 2), "max_abs_diff_weights": same_w, "max_abs_diff_second_target": same_s}


def bench_step(dev, steps, rays):
    import train_loop as TL
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    images, poses, intr = TL.teacher_views(dev, 28, 128, 128)
    held = 4
    images, poses = images[held:], poses[held:]
    depths = TL.teacher_depths(dev, poses, intr, 128, 128)
    rng = np.random.default_rng(5)
    w = rng.uniform(0, 2, images.shape[:3]).astype(np.float16)
    second = rng.uniform(0, 1, images.shape).astype(np.float16)
    out = {}
    for name, kw in (("default", {}), ("distill", dict(pixel_weights=True, second_weight=0.5, depth_weight=1e-3))):
        torch.manual_seed(0)
        net = NeRFNetwork(bound=1).to(dev)
        r = NeRFRenderer(net, bound=1, density_thresh=10).to(dev)
        opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
        data = ResidentImages.from_arrays(images, poses, intr, bg="random", device=dev, depths=depths, pixel_weights=w, second_target=second)
        tr = Trainer(r, opt, data, steps, 1e-2, num_rays=rays, seed=0, **kw)
        all_in, steady = TL._timed_run(tr, steps)
        _, windows = TL._replay_windows(tr)
        out[name] = {"ms_per_step_all_in": round(all_in, 4), "ms_per_step_after_64": round(steady, 4),
                     "replay_ms_per_step_windows": [round(v, 4) for v in windows], "mean_count": tr.r.mean_count, "captures": tr.captures,
                     "final_loss": float(tr.losses()[-16:].mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--rays", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    print(json.dumps({"build": bench_build(dev, args.views, args.res), "step": bench_step(dev, args.steps, args.rays)}), flush=True)


if __name__ == "__main__":
    main()
