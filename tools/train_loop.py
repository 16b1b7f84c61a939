"""Wall time of the graph-replayed training loop (laenerf_amd.trainer.Trainer) on a lego-shaped synthetic image set.

A teacher network (random but structured parameters on a sphere-and-boxes occupancy grid, as tools/fit_scene.py) renders
RGBA views from cameras on a sphere: colour = image over a black background / weights_sum (straight colour), alpha =
weights_sum; 8-bit like a real dataset.  A fresh student trains on them with the reference's loop (random background,
refresh every 16 steps, lr 1e-2 decaying by 0.1 over `iters`) and is evaluated on held-out views over white.

    python tools/train_loop.py [--steps 1024] [--rays 4096] [--capacity bucket|exact] [--no-graph] [--error-map none|ema|fixed] [--ema]

prints one JSON line: all-in ms/step (refreshes and graph captures included), the same without the first 64 steps, its
ratio to the README's train-step headline, captures / cache misses / eager warm groups, scaler-skipped steps, PSNR."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADLINE_MS = 0.353           # README.md: bench.py's train step (fixed resident batches, no grid refresh)


def teacher_views(dev, n_views, H, W, seed=0, bound=1, opacity=1.5, radius=3.2):
    """-> images [n, H, W, 4] uint8 (straight colour + alpha), poses [n, 4, 4] float32, intrinsics (fx, fy, cx, cy)"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.rays import get_rays
    g = torch.random.fork_rng(devices=[dev])
    with g:
        torch.manual_seed(11)
        net = NeRFNetwork(bound=bound).to(dev).eval()
        net.encoder.embeddings.data.uniform_(-1.0, 1.0)
        net.sigma_net.weights.data.mul_(opacity)
    r = NeRFRenderer(net, bound=bound, density_thresh=10).to(dev).eval()
    r.density_bitfield = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=r.cascade, bound=float(bound)), 10.0)).to(dev)
    poses = S.lookat_poses(n_views, radius=radius, seed=seed)
    focal = 0.5 * W / np.tan(0.5 * 0.69)                                  # camera_angle_x of the blender scenes
    intr = (focal, focal, W / 2, H / 2)
    out = []
    with torch.no_grad():
        for i in range(n_views):
            ray = get_rays(torch.from_numpy(poses[i:i + 1]).to(dev), intr, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=0, max_steps=1024)
            ws = res["weights_sum"].float().clamp(0, 1)
            rgb = torch.where(ws[:, None] > 0, res["image"].float() / ws.clamp(min=1e-6)[:, None], torch.zeros_like(res["image"].float()))
            rgba = torch.cat([rgb.clamp(0, 1), ws[:, None]], 1).reshape(H, W, 4)
            out.append((rgba * 255 + 0.5).to(torch.uint8).cpu().numpy())
    return np.stack(out), poses, intr


def make_trainer(dev, images, poses, intr, iters, lr=1e-2, n_rays=4096, graph=True, capacity="bucket", seed=0, student_seed=0,
                 error_map=None, ema_decay=None):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    torch.manual_seed(student_seed)
    net = NeRFNetwork(bound=1).to(dev)
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(dev)
    opt = FusedAdam(net, param_groups=net.get_params(lr), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    data = ResidentImages.from_arrays(images, poses, intr, bg="random", device=dev)
    return Trainer(r, opt, data, iters, lr, num_rays=n_rays, seed=seed, graph=graph, capacity=capacity, error_map=error_map,
                   ema_decay=ema_decay)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--capacity", default="bucket", choices=["bucket", "exact"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--views", type=int, default=28)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--error-map", default="none", choices=["none", "ema", "fixed"])
    ap.add_argument("--ema", action="store_true", help="Trainer(ema_decay=0.95): the gated EMA update in every step")
    args = ap.parse_args()
    error_map = None if args.error_map == "none" else args.error_map
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    images, poses, intr = teacher_views(dev, args.views, args.res, args.res)
    held = 4
    tr = make_trainer(dev, images[held:], poses[held:], intr, iters=args.steps, n_rays=args.rays, graph=not args.no_graph,
                      capacity=args.capacity, error_map=error_map, ema_decay=0.95 if args.ema else None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train(64)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    tr.train(args.steps - 64)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    from laenerf_amd.data import ResidentImages
    test = ResidentImages.from_arrays(images[:held], poses[:held], intr, device=dev)
    p = tr.evaluate(range(held), data=test, bg_color=1.0)
    # where the time goes (after the measurement; each part synchronised on its own): the refresh with its host read, a
    # 16-step replay at the current capacity, and the padding rows of that capacity
    refresh_ms, group_ms = [], []
    if tr.graph and tr.r.mean_count > 0:
        for _ in range(5):
            torch.cuda.synchronize(); a = time.perf_counter()
            tr._refresh()
            torch.cuda.synchronize(); b = time.perf_counter()
            tr.m_limit.fill_(tr._m())
            tr._run_group(tr._m_cap())
            torch.cuda.synchronize(); c = time.perf_counter()
            tr.global_step += 16
            refresh_ms.append((b - a) * 1e3); group_ms.append((c - b) * 1e3 / 16)
    all_in = (t2 - t0) * 1e3 / args.steps
    steady = (t2 - t1) * 1e3 / (args.steps - 64)
    print(json.dumps({
        "ms_per_step_all_in": round(all_in, 4), "ms_per_step_after_64": round(steady, 4), "steps": args.steps, "rays": args.rays,
        "ratio_to_headline": round(all_in / HEADLINE_MS, 3), "ratio_after_64_to_headline": round(steady / HEADLINE_MS, 3),
        "headline_ms": HEADLINE_MS, "graph": not args.no_graph, "capacity": args.capacity,
        **({"error_map": args.error_map} if error_map is not None else {}), **({"ema_decay": 0.95} if args.ema else {}),
        "captures": tr.captures,
        "cache_misses": tr.cache_misses, "warm_groups": tr.warm_groups, "capacities": sorted(tr.graphs),
        "mean_count": tr.r.mean_count, "steps_skipped": tr.steps_skipped, "heldout_psnr_white": round(p, 3),
        "final_loss": float(tr.losses()[-16:].mean()),
        "breakdown": {"refresh_ms": round(float(np.median(refresh_ms)), 4) if refresh_ms else None,
                      "replay_ms_per_step": round(float(np.median(group_ms)), 4) if group_ms else None,
                      "padding_rows_frac": round(1 - tr._m() / tr._m_cap(), 4) if tr.r.mean_count > 0 else None},
        "scene": f"{args.views - held} training + {held} held-out {args.res}x{args.res} RGBA uint8 views of a teacher network"}), flush=True)


if __name__ == "__main__":
    main()
