"""Time of scoring multi-view consistency: lae_consistency_pair per pair of views at 800 x 800 and 1920 x 1080 against its HBM
floor and against the same metric as a reference-shaped torch chain (the two remaps of scripts/eval/consistency_metrics.py as
F.grid_sample, elementwise masks, LPIPS as torch ops), and Trainer.evaluate_consistency per view on a seeded model.

    python tools/consistency_bench.py [--views 12] [--res 800]

The pair is synthetic: a smooth wavy surface around z = 3 seen by two cameras 0.03 rad and (0.15, 0.02, 0.01) apart, opaque
except a 2 % frame, smooth colours; fp32 frames.  The model of the last figure is tools/train_loop.py's teacher scene trained
64 steps (the numbers are times, not quality); LPIPS weights are LPIPS.random(0).  Prints one JSON line.

Bytes the kernel must move per pixel of the target view, with the LPIPS input written as evaluate_consistency does:
    read  frame b 12, depth b + opacity b 8            (the right and lower neighbours come out of the same cache lines)
    read  frame a 12, depth a + opacity a 8            (four taps per pixel, every line of a once when the flow is smooth)
    write lpips_in 2 x 3 x 4 = 24
    = 64 B; the two fp64 partials per block and the two 4 x 4 poses do not count."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29                 # measured float4-copy bandwidth of one MI355X (MI355X_MICROARCH)
BYTES_PER_PIXEL = 12 + 8 + 12 + 8 + 24


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


def _rays(P, intr, H, W, dev):
    fx, fy, cx, cy = intr
    gy, gx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d = torch.stack([(gx + 0.5 - cx) / fx, (gy + 0.5 - cy) / fy, torch.ones_like(gx)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    return P[:3, 3], d @ P[:3, :3].T, gx, gy


def synthetic_pair(H, W, dev):
    """-> frame_a, frame_b [H,W,3], depth_a, opacity_a, depth_b, opacity_b [H,W], pose_a, pose_b [4,4], intrinsics"""
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    intr = (focal, focal, W / 2, H / 2)
    c, s = np.cos(0.03), np.sin(0.03)
    Pa = torch.eye(4, device=dev)
    Pb = torch.tensor([[c, 0, s, 0.15], [0, 1, 0, 0.02], [-s, 0, c, 0.01], [0, 0, 0, 1]], dtype=torch.float32, device=dev)
    out = []
    for P in (Pa, Pb):
        o, d, gx, gy = _rays(P, intr, H, W, dev)
        t = (3.0 - o[2]) / d[..., 2]
        for _ in range(4):                                       # the surface z = 3 + 0.1 sin(3x) cos(2y), by fixed-point steps
            X = o + t[..., None] * d
            t = (3.0 + 0.1 * torch.sin(3 * X[..., 0]) * torch.cos(2 * X[..., 1]) - o[2]) / d[..., 2]
        X = o + t[..., None] * d
        frame = torch.stack([0.5 + 0.3 * torch.sin(5 * X[..., 0] + X[..., 1]), 0.5 + 0.3 * torch.cos(4 * X[..., 1]),
                             0.5 + 0.2 * torch.sin(3 * (X[..., 0] - X[..., 1]))], -1)
        A = torch.ones(H, W, device=dev)
        m = max(1, H // 50)
        A[:m] = A[-m:] = 0.2
        A[:, :m] = A[:, -m:] = 0.2
        out.append((frame.contiguous(), (t * A).contiguous(), A))
    (fa, da, aa), (fb, db, ab) = out
    return fa, fb, da, aa, db, ab, Pa.contiguous(), Pb.contiguous(), intr


def torch_chain(fa, fb, da, aa, db, ab, Pa, Pb, intr, min_opacity=0.5):
    """the metric as the script computes it, in torch ops: both flows as full images, cv2.remap as F.grid_sample (bilinear,
    align_corners=True: pixel-index coordinates), detect_occlusion's masks elementwise -> sse, count, the LPIPS pair [2,3,H,W]"""
    F = torch.nn.functional
    H, W = da.shape
    dev = da.device
    fx, fy, cx, cy = intr

    def flow(P_src, D, A, P_dst):
        o, d, gx, gy = _rays(P_src, intr, H, W, dev)
        ok = A >= min_opacity
        X = o + (D / A.clamp(min=1e-6))[..., None] * d
        q = (X - P_dst[:3, 3]) @ P_dst[:3, :3]
        ok = ok & (q[..., 2] > 0)
        z = torch.where(ok, q[..., 2], torch.ones_like(q[..., 2]))
        return torch.stack([fx * q[..., 0] / z + cx - 0.5 - gx, fy * q[..., 1] / z + cy - 0.5 - gy], -1), ok, gx, gy

    fw, ok_b, gx, gy = flow(Pb, db, ab, Pa)
    bw, ok_a, _, _ = flow(Pa, da, aa, Pb)
    lx, ly = gx + fw[..., 0], gy + fw[..., 1]
    grid = torch.stack([2 * lx / (W - 1) - 1, 2 * ly / (H - 1) - 1], -1)[None]
    src = torch.cat([bw, ok_a[..., None].float(), fa], -1).permute(2, 0, 1)[None]
    smp = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0)
    bw_w, taps_ok, warped = smp[..., :2], smp[..., 2] >= 1.0, smp[..., 3:]
    inside = (lx >= 0) & (lx <= W - 1) & (ly >= 0) & (ly <= H - 1)
    mag = (fw ** 2).sum(-1)
    occ = ((fw + bw_w) ** 2).sum(-1) > 0.01 * (mag + (bw_w ** 2).sum(-1)) + 0.5
    du, dv = torch.zeros_like(fw), torch.zeros_like(fw)
    du[:, :-1] = fw[:, :-1] - fw[:, 1:]
    dv[:-1] = fw[:-1] - fw[1:]
    nb = ok_b.clone()
    nb[:, :-1] &= ok_b[:, 1:]
    nb[:-1] &= ok_b[1:]
    bnd = (du ** 2).sum(-1) + (dv ** 2).sum(-1) > 0.01 * mag + 0.002
    valid = ok_b & nb & inside & taps_ok & ~occ & ~bnd
    err = ((warped - fb) ** 2).sum(-1)
    sse, count = (err.double() * valid).sum(), valid.sum()
    shift = torch.tensor([-0.030, -0.088, -0.188], device=dev).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=dev).view(1, 3, 1, 1)
    x = torch.stack([torch.where(valid[..., None], warped, fb), fb]).permute(0, 3, 1, 2)
    return sse, count, ((2 * x - 1) - shift) / scale


def bench_pair(H, W, dev, lp):
    from laenerf_amd.metrics import CONSISTENCY_SCRATCH_DOUBLES, consistency_pair
    from tools.eval_bench import lpips_torch
    fa, fb, da, aa, db, ab, Pa, Pb, intr = synthetic_pair(H, W, dev)
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    lp_in = torch.empty(2, 3, H, W, device=dev)
    lp_out = torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = torch.empty(CONSISTENCY_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    args = (fa.view(-1, 3), fb.view(-1, 3), da.view(-1), aa.view(-1), db.view(-1), ab.view(-1), Pa, Pb, intr, H, W)
    kernel = lambda: consistency_pair(*args, sse=sums[0:1], count=sums[1:2], lpips_in=lp_in, scratch=scratch)
    k_us = _time(kernel, 200)
    k_sums_us = _time(lambda: consistency_pair(*args, sse=sums[0:1], count=sums[1:2], scratch=scratch), 200)
    ours_us = _time(lambda: (kernel(), lp(lp_in, out=lp_out)), 50)
    t_us = _time(lambda: torch_chain(fa, fb, da, aa, db, ab, Pa, Pb, intr), 50)
    ref_us = _time(lambda: lpips_torch(lp, lp.features(torch_chain(fa, fb, da, aa, db, ab, Pa, Pb, intr)[2])), 20)
    kernel()
    t_sse, t_count, _ = torch_chain(fa, fb, da, aa, db, ab, Pa, Pb, intr)
    s = sums.cpu().numpy()
    nbytes = H * W * BYTES_PER_PIXEL
    return {"res": [H, W], "kernel_us": round(k_us, 2), "kernel_sums_only_us": round(k_sums_us, 2), "kernel_bytes": nbytes,
            "kernel_hbm_bound_us": round(nbytes / HBM_TBS / 1e6, 2), "torch_chain_us": round(t_us, 2),
            "ms_per_pair": {"kernel_and_lpips": round(ours_us / 1e3, 3), "torch_chain_and_torch_lpips": round(ref_us / 1e3, 3)},
            "valid_share": round(float(s[1]) / (H * W), 4), "warp_mse": float(s[0] / max(s[1], 1.0)),
            "torch_chain_valid_share": round(float(t_count) / (H * W), 4), "torch_chain_warp_mse": float(t_sse / max(float(t_count), 1.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--res", type=int, default=800)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.metrics import LPIPS
    from tools.train_loop import teacher_views, make_trainer
    lp = LPIPS.random(0, device=dev)
    pairs = [bench_pair(H, W, dev, lp) for H, W in ((800, 800), (1080, 1920))]

    H = W = args.res
    train_imgs, train_poses, intr = teacher_views(dev, 8, 128, 128)
    tr = make_trainer(dev, train_imgs, train_poses, intr, iters=64, ema_decay=0.95)
    tr.train(64)
    imgs, poses, intr = teacher_views(dev, args.views, H, W, seed=1)
    test = ResidentImages.from_arrays(imgs, poses, intr, device=dev)
    tr.evaluate_consistency(ResidentImages.from_arrays(imgs[:3], poses[:3], intr, device=dev), step=1, lpips=lp)   # warm-up
    out = {}
    for step in (1, 7):
        if step >= args.views:
            continue
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = tr.evaluate_consistency(test, step=step, lpips=lp)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3 / args.views
        out[f"step{step}"] = {"ms_per_view": round(ms, 3), "mean_warp_mse": res["mean_warp_mse"], "mean_lpips": res["mean_lpips"],
                              "mean_valid_share": round(float(np.mean(res["valid_share"])), 4), "empty_pairs": res["empty_pairs"]}
    print(json.dumps({"pairs": pairs, "evaluate_consistency": {"views": args.views, "res": [H, W], **out}}), flush=True)


if __name__ == "__main__":
    main()
