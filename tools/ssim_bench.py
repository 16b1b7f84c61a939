"""Times of SSIM on the device (csrc/ssim.hip) against the reference-shaped torch chain on the same inputs.

    python tools/ssim_bench.py [--views 20] [--res 800] [--reps 200]

Prints one JSON line:
  metric        lae_ssim in us at 800 x 800 and 1920 x 1080 under both data-range rules, its HBM floor (24 bytes per pixel read: both
                fp32 images once) and the torch chain torchmetrics runs (reflect pad by 5, F.conv2d(groups=3) of the five stacked fp32
                planes with the 11 x 11 window, crop, the elementwise tail, mean), with the difference of the two values
  patch         lae_ssim_patch_forward + lae_ssim_patch_backward through losses.ssim_patch_loss and autograd, in us, at 4 patches of
                32 x 32 and 1 patch of 64 x 64, against the same chain under torch autograd
  evaluate      Trainer.evaluate_one_epoch in ms per view (--res, --views) with and without ssim=True, two timed passes each,
                alternating
The scene of `evaluate` is tools/eval_bench.py's: train_loop's teacher, a student trained 64 steps (times, not quality)."""
import argparse
import json
import os
import sys
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


def _kernel(dev, dtype=torch.float32):
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) / 1.5) ** 2 / 2)
    g = (g / g.sum())[None]
    return torch.matmul(g.t(), g).expand(3, 1, 11, 11).contiguous().to(dev, dtype)


def torch_chain(p, t, kernel, data_range=None):
    """torchmetrics' _ssim_update on [N, 3, H, W] images -> the mean over each image's cropped map, [N]"""
    if data_range is None:
        data_range = torch.maximum(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    n = p.shape[0]
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    o = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=3)
    mu_p, mu_t = o[0:n], o[n:2 * n]
    s_p, s_t, s_pt = o[2 * n:3 * n] - mu_p * mu_p, o[3 * n:4 * n] - mu_t * mu_t, o[4 * n:] - mu_p * mu_t
    full = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_p + s_t + c2))
    return full[..., 5:-5, 5:-5].reshape(n, -1).mean(-1)


def metric_row(dev, H, W, reps):
    from laenerf_amd.metrics import ssim, ssim_scratch_doubles
    g = torch.Generator(device=dev).manual_seed(H)
    gt = torch.rand(H * W, 3, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(H * W, 3, device=dev, generator=g)).contiguous()
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = torch.empty(ssim_scratch_doubles(H, W), dtype=torch.float64, device=dev)
    kernel = _kernel(dev)
    p4, t4 = (v.reshape(1, H, W, 3).permute(0, 3, 1, 2).contiguous() for v in (pred, gt))
    row = {"res": [H, W], "bytes": 24 * H * W, "hbm_floor_us": round(24 * H * W / HBM_TBS / 1e6, 2)}
    row["ssim_us_data_rule"] = round(_time(lambda: ssim(pred, gt, H, W, out=out, scratch=scratch), reps), 2)
    ours = float(out.item())
    row["ssim_us_fixed_range"] = round(_time(lambda: ssim(pred, gt, H, W, data_range=1.0, out=out, scratch=scratch), reps), 2)
    row["torch_chain_us_data_rule"] = round(_time(lambda: torch_chain(p4, t4, kernel), max(10, reps // 10)), 2)
    row["torch_chain_us_fixed_range"] = round(_time(lambda: torch_chain(p4, t4, kernel, 1.0), max(10, reps // 10)), 2)
    row["value"] = ours
    row["torch_chain_fp32_minus_ours"] = float(torch_chain(p4, t4, kernel).item()) - ours
    return row


def patch_row(dev, n_patch, P, reps):
    from laenerf_amd.losses import ssim_patch_loss
    g = torch.Generator(device=dev).manual_seed(P)
    gt = torch.rand(n_patch * P * P, 3, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(n_patch * P * P, 3, device=dev, generator=g)).contiguous().requires_grad_(True)
    kernel = _kernel(dev)

    def ours():
        pred.grad = None
        ssim_patch_loss(pred, gt, P).backward()

    def chain():
        pred.grad = None
        p4 = pred.reshape(n_patch, P, P, 3).permute(0, 3, 1, 2)
        t4 = gt.reshape(n_patch, P, P, 3).permute(0, 3, 1, 2)
        (1.0 - torch_chain(p4, t4, kernel, 1.0).mean()).backward()

    row = {"n_patch": n_patch, "P": P, "forward_backward_us": round(_time(ours, reps), 2)}
    g_ours = pred.grad.clone()
    row["torch_chain_forward_backward_us"] = round(_time(chain, max(10, reps // 4)), 2)
    row["max_grad_difference_fp32_chain"] = float((pred.grad - g_ours).abs().max().item())
    return row


def evaluate_rows(dev, views, res):
    from laenerf_amd.data import ResidentImages
    from tools.train_loop import make_trainer, teacher_views
    train_imgs, train_poses, intr = teacher_views(dev, 8, 128, 128)
    tr = make_trainer(dev, train_imgs, train_poses, intr, iters=64, ema_decay=0.95)
    tr.train(64)
    imgs, poses, intr = teacher_views(dev, views, res, res, seed=1)
    test = ResidentImages.from_arrays(imgs, poses, intr, device=dev)
    warm = ResidentImages.from_arrays(imgs[:2], poses[:2], intr, device=dev)
    tr.evaluate_one_epoch(warm)
    tr.evaluate_one_epoch(warm, ssim=True)
    ms = {False: [], True: []}
    out = None
    for _ in range(2):
        for flag in (False, True):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = tr.evaluate_one_epoch(test, ssim=flag)
            torch.cuda.synchronize()
            ms[flag].append(round((time.perf_counter() - t0) * 1e3 / views, 3))
            if flag:
                out = r
    return {"views": views, "res": [res, res], "ms_per_view_plain": ms[False], "ms_per_view_with_ssim": ms[True],
            "mean_psnr": round(out["mean_psnr"], 4), "mean_ssim": round(out["mean_ssim"], 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench: needs a GPU (times on a CPU say nothing)")
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    line = {"metric": [metric_row(dev, 800, 800, args.reps), metric_row(dev, 1080, 1920, args.reps)],
            "patch": [patch_row(dev, 4, 32, args.reps), patch_row(dev, 1, 64, args.reps)],
            "evaluate": evaluate_rows(dev, args.views, args.res), "reps": args.reps}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
