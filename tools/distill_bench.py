"""LAENeRF's distillation stage (laenerf_amd.editing.distill): the dataset rewrite and the distillation training, at the reference's
scale (100 training views at 800x800).  The training images are tools/train_loop.py's teacher scene (RGBA, 8-bit); each view gets an
extracted edit set of about 53 k rows (tools/style_train_bench.py's mean K) inside the object's silhouette, with random edit weights,
render colours, points and directions.  A student NeRF is fitted briefly, then trained on the distilled images with error maps.
Reported:
  distill_images_ms            distill_images (copy to fp16, palette network over all rows, one compose launch), error maps off
  distill_images_seed_ms       the same with the error-map seed
  reference_chain_ms           the reference's per-view loop restated (gui.py:400-480: per view the rows to the device, forward_train,
                               the edit / blend / mask / clamp torch ops, the error map through interpolate (torchvision 0.15's
                               Resize), the image to the device and back to the host; no PNG writes)
  trainer_ms_per_step          the distillation Trainer (error_map 'ema', graph replay) after warm-up
  projected_stage_s_3000       distill_images_seed_ms + distill_steps(3000) steps
Times: median of several windows after a warm-up, HIP events around a synchronised region.  One JSON line.

    python tools/distill_bench.py [--views 100] [--res 800] [--rows 53000]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def event_ms(fn, windows, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def make_views(images, rows, seed=0):
    """per view: `rows` pixels drawn inside the silhouette (alpha > 0.5), the reference's per-view entries as extract_views returns
    them (full-image weights_editgrid / pred_imgs on the host, as the reference's EditDataset keeps them)"""
    g = torch.Generator().manual_seed(seed)
    n, H, W, _ = images.shape
    views = []
    for i in range(n):
        inside = torch.nonzero(torch.from_numpy(images[i, ..., 3]).reshape(-1) > 127, as_tuple=True)[0]
        k = min(rows, int(inside.numel()))
        idx = inside[torch.randperm(inside.numel(), generator=g)[:k]].sort().values
        w = torch.rand(k, generator=g) * 0.99 + 0.01
        full_w = torch.zeros(H * W)
        full_w[idx] = w
        views.append(dict(pose_idx=i, indices=idx, w8s=w, weights_editgrid=full_w, pred_imgs=torch.rand(H * W, 3, generator=g) * 0.8,
                          x_term=(torch.rand(k, 3, generator=g) - 0.5) * 0.6,
                          dirs=torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=-1)))
    return views


def reference_chain(enc, views, host_images, palette, p_weights, p_bias, H, W, error_map, blend_thresh=0.5):
    """distill_dataset's per-view loop (gui.py:400-480) on the host images, without its PNG writes"""
    F = torch.nn.functional
    for v in views:
        idx = v["pose_idx"]
        indices = v["indices"].cuda()
        w8s_edit = v["weights_editgrid"].cuda()[..., None]
        pred_img = v["pred_imgs"].cuda()
        x_term, dirs = v["x_term"].cuda(), v["dirs"].cuda()
        weight_img = torch.zeros((H, W), device="cuda")
        weight_img.flatten(0, 1)[...] = w8s_edit[..., 0]
        resized = F.interpolate(weight_img[None, None], (128, 128), mode="bilinear", align_corners=False)[0]
        error_map[idx] = torch.clamp(resized + 15e-2, 0, 1).flatten()
        train_image_gpu = host_images[idx, ..., :3].cuda()
        style_image_gpu = torch.zeros_like(train_image_gpu)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            _, weights_og, offsets = enc.forward_train(x_term, d=dirs)
            weights = torch.clamp_min(p_bias[None] + p_weights[None] * weights_og, 0)
            weights /= weights.sum(-1)[..., None].half()
            pred_colors = torch.clamp(offsets.half() + weights.half() @ palette.half(), 0, 1)
        style_image_gpu.flatten(0, 1)[indices] = pred_colors.float()
        style_image_gpu = (1 - w8s_edit).reshape(H, W, 1) * pred_img.reshape(H, W, -1) + w8s_edit.reshape(H, W, 1) * style_image_gpu
        mask = (w8s_edit <= blend_thresh).reshape(H, W, -1)
        train_image_gpu = torch.clamp(~mask * style_image_gpu + mask * train_image_gpu, min=0, max=1)
        host_images[idx, ..., :3] = train_image_gpu.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--rows", type=int, default=53000)
    ap.add_argument("--fit-steps", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from laenerf_amd import build
    build.build()
    from laenerf_amd.editing import DistillSet, LAENeRF, distill_images, distill_steps
    from laenerf_amd.trainer import Trainer
    from tools.train_loop import make_trainer, teacher_views

    images, poses, intr = teacher_views(dev, a.views, a.res, a.res)
    H = W = a.res
    views = make_views(images, a.rows)
    torch.manual_seed(7)
    enc = LAENeRF(SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0), dir_encoding="sphere_harmonics").to(dev)
    enc.encoder.embeddings.data.uniform_(-1.0, 1.0)
    g = torch.Generator(device=dev).manual_seed(0)
    palette = torch.rand(8, 3, device=dev, generator=g)
    p_weights = torch.rand(8, device=dev, generator=g) * 2
    p_bias = torch.randn(8, device=dev, generator=g) * 0.1

    tr = make_trainer(dev, images, poses, intr, iters=a.fit_steps)
    tr.train(a.fit_steps)
    data = tr.data
    dset = DistillSet.from_views(views, [], data.n_img, device=dev)
    K = dset.counts_host
    out = {"views": dset.V, "H": H, "W": W, "rows": dset.R, "K_mean": int(K.mean()), "K_min": int(K.min()), "K_max": int(K.max())}
    kw = dict(palette=palette, p_weights=p_weights, p_bias=p_bias)
    out["distill_images_ms"] = round(event_ms(lambda: distill_images(data, enc, dset, **kw), a.windows), 3)
    holder = {}

    def seeded():
        holder["d"] = distill_images(data, enc, dset, error_maps=True, **kw)
    out["distill_images_seed_ms"] = round(event_ms(seeded, a.windows), 3)

    host_images = images.astype(np.float32) / 255
    host_t = torch.from_numpy(host_images)
    em = torch.ones(data.n_img, 128 * 128, device=dev)
    out["reference_chain_ms"] = round(event_ms(lambda: reference_chain(enc, views, host_t, palette, p_weights, p_bias, H, W, em),
                                               max(1, a.windows // 2)), 3)
    out["rewrite_speedup"] = round(out["reference_chain_ms"] / out["distill_images_seed_ms"], 1)

    distilled = holder["d"]
    tr2 = Trainer(tr.r, tr.opt, distilled, iters=3000, lr=1e-2, error_map="ema")
    tr2.train(64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr2.train(a.steps)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    out["trainer_ms_per_step"] = round(step_ms, 4)
    out["trainer_captures"] = tr2.captures
    n = distill_steps(3000)
    out["distill_steps_3000"] = n
    out["projected_stage_s_3000"] = round((out["distill_images_seed_ms"] + n * step_ms) / 1e3, 3)
    out["rewrite_fraction_of_stage"] = round(out["distill_images_seed_ms"] / (out["distill_images_seed_ms"] + n * step_ms), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
