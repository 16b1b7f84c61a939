"""Time of evaluating a trained NeRF per view: Trainer.evaluate_one_epoch (render + lae_eval_view + AlexNet + lae_lpips_head)
against the reference-shaped path (render_eval, host copy, numpy PSNR, LPIPS as torch ops), and the two new kernels against
their torch equivalents.

    python tools/eval_bench.py [--views 100] [--res 800]

The scene is tools/train_loop.py's teacher network; the student is trained 64 steps with ema_decay=0.95 (the numbers are
times, not quality); LPIPS weights are LPIPS.random(0).  Prints one JSON line.  Byte counts are what each kernel must move:
lae_eval_view reads pred (12 B), depth (4 B) and the uint8 RGBA ground truth (4 B) per pixel and writes the LPIPS input
(24 B); the head reads both feature maps of every layer once."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29                 # measured float4-copy bandwidth of one MI355X (MI355X_MICROARCH)


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps             # us


def lpips_torch(lp, feats):
    """the lpips package's head as torch ops (normalize_tensor, 1x1 conv, spatial mean, sum): what LPIPSMeter runs"""
    val = 0
    for f, w in zip(feats, lp.lins):
        f0, f1 = f[0::2], f[1::2]
        n0 = torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True))
        n1 = torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True))
        d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
        val = val + torch.nn.functional.conv2d(d, w.view(1, -1, 1, 1)).mean([2, 3])
    return val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--res", type=int, default=800)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.metrics import LPIPS, eval_view, LPIPS_SHIFT, LPIPS_SCALE
    from tools.train_loop import teacher_views, make_trainer
    H = W = args.res
    train_imgs, train_poses, intr = teacher_views(dev, 8, 128, 128)
    tr = make_trainer(dev, train_imgs, train_poses, intr, iters=64, ema_decay=0.95)
    tr.train(64)
    imgs, poses, intr = teacher_views(dev, args.views, H, W, seed=1)
    test = ResidentImages.from_arrays(imgs, poses, intr, device=dev)
    lp = LPIPS.random(0, device=dev)

    tr.evaluate_one_epoch(ResidentImages.from_arrays(imgs[:2], poses[:2], intr, device=dev), lpips=lp)   # warm-up
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = tr.evaluate_one_epoch(test, lpips=lp)
    torch.cuda.synchronize(); ours_ms = (time.perf_counter() - t0) * 1e3 / args.views

    # the reference-shaped path: EMA weights in, render, host copies, numpy PSNR, LPIPS as torch ops
    shift = torch.tensor(LPIPS_SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, device=dev).view(1, 3, 1, 1)
    ref_psnr, ref_lp = [], []
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with tr._eval_weights(), torch.no_grad():
        for i in range(args.views):
            pred, _ = tr._render_view(test, i, scale_depth=False)
            img = test.images[i].reshape(-1, 4).float() / 255
            gt = img[:, :3] * img[:, 3:] + (1 - img[:, 3:])
            p, g = pred.cpu().numpy(), gt.cpu().numpy()
            ref_psnr.append(-10 * np.log10(np.mean((p - g) ** 2)))
            x = torch.stack([gt, pred]).reshape(2, H, W, 3).permute(0, 3, 1, 2)
            x = ((2 * x - 1) - shift) / scale
            ref_lp.append(float(lpips_torch(lp, lp.features(x))))
    torch.cuda.synchronize(); ref_ms = (time.perf_counter() - t0) * 1e3 / args.views

    # kernels alone, on the last view
    pred = torch.rand(H * W, 3, device=dev); depth = torch.rand(H * W, device=dev)
    gt = test.images[0]
    sse = torch.zeros(1, dtype=torch.float64, device=dev)
    lp_in = torch.empty(2, 3, H, W, device=dev)
    scratch = torch.empty(2048, dtype=torch.float64, device=dev)
    ev_us = _time(lambda: eval_view(pred, gt, depth=depth, sse=sse, lpips_in=lp_in, scratch=scratch), 200)

    def torch_view():
        img = gt.reshape(-1, 4).float() / 255
        g = img[:, :3] * img[:, 3:] + (1 - img[:, 3:])
        s = ((pred - g) ** 2).sum()
        x = torch.stack([g, pred]).reshape(2, H, W, 3).permute(0, 3, 1, 2)
        return s, ((2 * x - 1) - shift) / scale
    ev_torch_us = _time(torch_view, 200)
    feats = lp.features(lp_in)
    head_us = _time(lambda: lp.head(feats), 200)
    head_torch_us = _time(lambda: lpips_torch(lp, feats), 50)
    ev_bytes = H * W * (12 + 4 + 4 + 24)
    head_bytes = sum(f.numel() * 4 for f in feats)
    print(json.dumps({
        "views": args.views, "res": [H, W],
        "ms_per_view": {"evaluate_one_epoch": round(ours_ms, 3), "reference_shaped": round(ref_ms, 3)},
        "mean_psnr": round(res["mean_psnr"], 4), "reference_shaped_mean_psnr": round(float(np.mean(ref_psnr)), 4),
        "mean_lpips": res["mean_lpips"], "reference_shaped_mean_lpips": float(np.mean(ref_lp)),
        "eval_view_us": round(ev_us, 2), "eval_view_torch_us": round(ev_torch_us, 2), "eval_view_bytes": ev_bytes,
        "eval_view_hbm_bound_us": round(ev_bytes / HBM_TBS / 1e6, 2),
        "lpips_head_us": round(head_us, 2), "lpips_head_torch_us": round(head_torch_us, 2), "lpips_head_bytes": head_bytes,
        "lpips_head_hbm_bound_us": round(head_bytes / HBM_TBS / 1e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
