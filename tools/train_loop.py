"""Wall time of the graph-replayed training loop (laenerf_amd.trainer.Trainer) on a lego-shaped synthetic image set.

A teacher network (random but structured parameters on a sphere-and-boxes occupancy grid, as tools/fit_scene.py) renders
RGBA views from cameras on a sphere: colour = image over a black background / weights_sum (straight colour), alpha =
weights_sum; 8-bit like a real dataset.  A fresh student trains on them with the reference's loop (random background,
refresh every 16 steps, lr 1e-2 decaying by 0.1 over `iters`) and is evaluated on held-out views over white.

    python tools/train_loop.py [--steps 1024] [--rays 4096] [--capacity bucket|exact] [--no-graph] [--error-map none|ema|fixed] [--ema] [--depth] [--distort W]
                                [--loss mse|l1|huber|mape] [--huber-delta D] [--entropy W] [--outliers P]
                                [--mask-outliers P] [--pose-noise DEG,DIST] [--pose-lr LR]
                                [--exposure-noise STOPS] [--exposure-lr LR]
                                [--patch-size P] [--lpips-weight W] [--lpips-weights ALEXNET.pth,ALEX.pth] [--ssim-weight W]
                                [--lens K1,K2]

prints one JSON line: all-in ms/step (refreshes and graph captures included), the same without the first 64 steps, its
ratio to the README's train-step headline, captures / cache misses / eager warm groups, scaler-skipped steps, PSNR.
--depth: a second, identically seeded student trains with depth supervision (Trainer(depth_weight=...)) on the teacher's own depth
(its rendered ray-origin distance where the view is opaque, zero elsewhere); the line then carries ms/step with and without the
term ("depth": {...}) and the replay time of five windows for each.
--distort W: every student of the run trains with the distortion regularizer (Trainer(distort_weight=W)); the line then carries the
term's first and last 16-step mean ("distort": {...}).  Compare ms/step with a run without the option (and `--depth --distort W`
with `--depth`) for the term's cost: the runs differ in nothing else, though their mean_count drifts apart as the geometry does.
--loss / --huber-delta: every student of the run trains with that colour criterion (Trainer(loss=..., huber_delta=...)); final_loss is
then that criterion's mean.  --entropy W: ... with the opacity-entropy regularizer (Trainer(opacity_weight=W)); the line then carries the
term's first and last 16-step mean ("opacity": {...}).  Compare ms/step with a run without the options for their cost.
--outliers P: the share P of the training pixels (never the held-out views) is overwritten with opaque uniformly random colours before
training, the specular / exposure outliers of a real capture in their crudest form; the held-out PSNR under --loss mse and --loss huber
is what the robust criterion buys.
--mask-outliers P: --outliers P with a weight plane that is 0 on the overwritten pixels and 1 elsewhere (Trainer(pixel_weights=True)): the
outliers cannot matter, and the held-out PSNR is that of the clean pixels alone.  Compare ms/step with a run without the option for
the cost of the weighted step.
--pose-noise DEG,DIST: every training camera (never the held-out ones) is rotated by DEG degrees about a random axis through its origin
and moved by DIST in a random direction before training, the pose error of a real capture.  --pose-lr LR: the student refines its
cameras (Trainer(pose_refine=True, pose_lr=LR)).  With either the line carries "pose": the mean rotation (degrees) and translation
error of the training cameras against the true ones before and after the run; compare heldout_psnr_white with and without --pose-lr
for what the refinement buys, and breakdown.replay_ms_per_step for its cost.
--exposure-noise STOPS: the colour of every training image (never the held-out ones) is multiplied by 2^u, u uniform in [-STOPS, STOPS]
and centred over the images (exposure.perturb_exposures; the images become float32, nothing clips): the auto-exposure of a hand-held
capture.  --exposure-lr LR: the student learns a gain per image and channel (Trainer(exposure_refine=True, exposure_lr=LR)).  With
either the line carries "exposure": the RMS of the training images' log2 exposure error before and after the run (after: learned +
applied, 0 = compensated) and the time of the two launches per step; compare heldout_psnr_white with and without --exposure-lr for
what the refinement buys, and breakdown.replay_ms_per_step for its cost.
--patch-size P --lpips-weight W [--lpips-weights ALEXNET.pth,ALEX.pth]: the student trains on rays // P^2 patches of P x P pixels per
step with the LPIPS term (Trainer(patch_size=P, perceptual_weight=W, lpips=...)); without weight files the term uses LPIPS.random(0),
seeded stand-in weights, and the line says so.  The line then carries "patch": ms_per_step (after the first 64 steps), truncated_steps,
the peak-to-mean ratio of the per-step sample count, the LPIPS term's first and last 16-step mean and the held-out PSNR.
--ssim-weight W (with --patch-size P): the D-SSIM term 1 - SSIM of the patches with weight W (Trainer(ssim_weight=W)); "patch" then also
carries its first and last 16-step mean.  With --lpips-weight 0 and no --lpips-weights the trainer gets lpips=None: D-SSIM alone, and
P >= 11 is enough.
--lens K1,K2 (write `--lens=-0.3,0.09` where K1 is negative): the training views (never the held-out ones) are also captured through an OpenCV radial lens with those coefficients
(undistort.Undistorter.distort_images of the teacher's pinhole views; what that lens sees beyond the teacher's frame is transparent),
and two more identically seeded students train: one on the captures with the distortion ignored (the loader's undistort=False), one on
the captures undistorted on the device (undistort=True's path: target_intrinsics at balance 0, Undistorter.images).  The line then
carries "lens": the held-out PSNR of the three students on the true pinhole held-out views -- a measurement, not an assertion.
--save PATH: the first student's checkpoint is written after the run (Trainer.save_checkpoint; a `.pth` path or a directory);
--resume PATH: the first student loads it before training and then trains --steps further steps (the same --steps as the saved run
keeps the learning-rate horizon, which the load checks).  The line then carries "checkpoint": the file size in bytes and the save /
load wall times in ms -- plain numbers, bounded by nothing."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADLINE_MS = 0.353           # README.md: bench.py's train step (fixed resident batches, no grid refresh)


def _teacher(dev, bound, opacity):
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    g = torch.random.fork_rng(devices=[dev])
    with g:
        torch.manual_seed(11)
        net = NeRFNetwork(bound=bound).to(dev).eval()
        net.encoder.embeddings.data.uniform_(-1.0, 1.0)
        net.sigma_net.weights.data.mul_(opacity)
    r = NeRFRenderer(net, bound=bound, density_thresh=10).to(dev).eval()
    r.density_bitfield = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=r.cascade, bound=float(bound)), 10.0)).to(dev)
    return r


def teacher_depths(dev, poses, intr, H, W, bound=1, opacity=1.5, min_alpha=0.5):
    """-> [n, H, W] float32: the teacher's composited depth (distance from the ray origin) of teacher_views' views where the view is
    opaque enough (weights_sum > min_alpha), zero (= no supervision) elsewhere"""
    from laenerf_amd.rays import get_rays
    r = _teacher(dev, bound, opacity)
    out = []
    with torch.no_grad():
        for i in range(len(poses)):
            ray = get_rays(torch.from_numpy(poses[i:i + 1]).to(dev), intr, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=0, max_steps=1024, perturb=False, scale_depth=False)
            ws = res["weights_sum"].float()
            d = torch.where(ws > min_alpha, res["depth"].float() / ws.clamp(min=1e-6), torch.zeros_like(ws))
            out.append(d.reshape(H, W).cpu().numpy())
    return np.stack(out).astype(np.float32)


def teacher_views(dev, n_views, H, W, seed=0, bound=1, opacity=1.5, radius=3.2):
    """-> images [n, H, W, 4] uint8 (straight colour + alpha), poses [n, 4, 4] float32, intrinsics (fx, fy, cx, cy)"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    r = _teacher(dev, bound, opacity)
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
                 error_map=None, ema_decay=None, depths=None, depth_weight=None, depth_grad=True, distort_weight=None, loss="mse",
                 huber_delta=0.1, opacity_weight=None, pixel_weights=None, pose_lr=None, exposure_lr=None, patch_size=1, lpips=None,
                 perceptual_weight=1e-3, ssim_weight=None):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    torch.manual_seed(student_seed)
    net = NeRFNetwork(bound=1).to(dev)
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(dev)
    opt = FusedAdam(net, param_groups=net.get_params(lr), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    data = ResidentImages.from_arrays(images, poses, intr, bg="random", device=dev, depths=depths, pixel_weights=pixel_weights)
    depth_kw = {} if depth_weight is None else {"depth_weight": depth_weight, "depth_grad": depth_grad}
    if distort_weight is not None:
        depth_kw["distort_weight"] = distort_weight
    if loss != "mse" or opacity_weight is not None:
        depth_kw.update(loss=loss, huber_delta=huber_delta, opacity_weight=opacity_weight)
    if pixel_weights is not None:
        depth_kw["pixel_weights"] = True
    if pose_lr is not None:
        depth_kw.update(pose_refine=True, pose_lr=pose_lr)
    if exposure_lr is not None:
        depth_kw.update(exposure_refine=True, exposure_lr=exposure_lr)
    if patch_size != 1:
        depth_kw.update(patch_size=patch_size, lpips=lpips, perceptual_weight=perceptual_weight)
        if ssim_weight is not None:
            depth_kw["ssim_weight"] = ssim_weight
    return Trainer(r, opt, data, iters, lr, num_rays=n_rays, seed=seed, graph=graph, capacity=capacity, error_map=error_map,
                   ema_decay=ema_decay, **depth_kw)


def _replay_windows(tr, n=5):
    """after a run: n windows of (refresh ms, ms per step of a 16-step replay at the current capacity)"""
    refresh_ms, group_ms = [], []
    if tr.graph and tr.r.mean_count > 0:
        for _ in range(n):
            torch.cuda.synchronize(); a = time.perf_counter()
            tr._refresh()
            torch.cuda.synchronize(); b = time.perf_counter()
            tr.m_limit.fill_(tr._m())
            tr._run_group(tr._m_cap())
            torch.cuda.synchronize(); c = time.perf_counter()
            tr.global_step += 16
            refresh_ms.append((b - a) * 1e3); group_ms.append((c - b) * 1e3 / 16)
    return refresh_ms, group_ms


def _exposure_launch_us(tr, n=200):
    """after a run: the time of lae_exposure_step + lae_exposure_publish on one batch, n calls between two events (the state moves on)"""
    b = tr.data.sample(tr.num_rays)
    pred = torch.zeros_like(b["gt"])
    call = lambda: tr.data.exposure_step(pred, b, tr.opt.dev_state, tr.exposure_lr_dev, loss=tr.loss, huber_delta=tr.huber_delta)
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _timed_run(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train(64)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    tr.train(steps - 64)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3 / steps, (t2 - t1) * 1e3 / (steps - 64)


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
    ap.add_argument("--depth", action="store_true", help="also train a second student with depth supervision on the teacher's depth")
    ap.add_argument("--depth-weight", type=float, default=1e-3)
    ap.add_argument("--depth-value-only", action="store_true", help="depth_grad=False: the reference's value-only depth term")
    ap.add_argument("--distort", type=float, default=None, metavar="W", help="Trainer(distort_weight=W) for every student of the run")
    ap.add_argument("--loss", default="mse", choices=["mse", "l1", "huber", "mape"], help="Trainer(loss=...) for every student of the run")
    ap.add_argument("--huber-delta", type=float, default=0.1, metavar="D")
    ap.add_argument("--entropy", type=float, default=None, metavar="W", help="Trainer(opacity_weight=W) for every student of the run")
    ap.add_argument("--outliers", type=float, default=0.0, metavar="P", help="share of training pixels overwritten with random colours")
    ap.add_argument("--mask-outliers", type=float, default=0.0, metavar="P", help="--outliers P with weight 0 on the overwritten pixels")
    ap.add_argument("--pose-noise", default=None, metavar="DEG,DIST", help="perturb every training camera by DEG degrees and DIST")
    ap.add_argument("--pose-lr", type=float, default=None, metavar="LR", help="Trainer(pose_refine=True, pose_lr=LR)")
    ap.add_argument("--exposure-noise", type=float, default=None, metavar="STOPS", help="multiply every training image by 2^u, |u| <= STOPS")
    ap.add_argument("--exposure-lr", type=float, default=None, metavar="LR", help="Trainer(exposure_refine=True, exposure_lr=LR)")
    ap.add_argument("--patch-size", type=int, default=1, metavar="P", help="Trainer(patch_size=P): rays // P^2 patches per step, LPIPS term")
    ap.add_argument("--lpips-weight", type=float, default=1e-3, metavar="W", help="Trainer(perceptual_weight=W)")
    ap.add_argument("--lpips-weights", default=None, metavar="ALEXNET.pth,ALEX.pth", help="torchvision alexnet + lpips v0.1 alex weights")
    ap.add_argument("--ssim-weight", type=float, default=None, metavar="W",
                    help="Trainer(ssim_weight=W), with --patch-size: the D-SSIM term; with --lpips-weight 0 and no --lpips-weights, lpips=None")
    ap.add_argument("--lens", default=None, metavar="K1,K2", help="also train on the views captured through this radial lens: ignored / undistorted")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the first student's checkpoint after the run")
    ap.add_argument("--resume", default=None, metavar="PATH", help="load a checkpoint into the first student before training")
    args = ap.parse_args()
    error_map = None if args.error_map == "none" else args.error_map
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    images, poses, intr = teacher_views(dev, args.views, args.res, args.res)
    held = 4
    if args.mask_outliers > 0 and args.outliers > 0:
        ap.error("--mask-outliers P implies --outliers P: give one of the two")
    share = max(args.outliers, args.mask_outliers)
    mask = None
    if share > 0:
        rng = np.random.default_rng(17)
        hit = rng.random(images[held:].shape[:3]) < share
        noise = rng.integers(0, 256, size=images[held:].shape, dtype=np.uint8)
        noise[..., 3] = 255
        images[held:][hit] = noise[hit]
        if args.mask_outliers > 0:
            mask = np.where(hit, 0.0, 1.0).astype(np.float16)
    crit_kw = dict(loss=args.loss, huber_delta=args.huber_delta, opacity_weight=args.entropy, pixel_weights=mask, pose_lr=args.pose_lr,
                   exposure_lr=args.exposure_lr)
    patch = None
    if args.ssim_weight is not None and args.patch_size == 1:
        ap.error("--ssim-weight needs --patch-size P")
    if args.patch_size != 1:
        from laenerf_amd.metrics import LPIPS, load_lpips_alex
        if args.lpips_weights:
            lp = load_lpips_alex(*args.lpips_weights.split(","), device=dev)
        elif args.ssim_weight is not None and args.lpips_weight == 0:
            lp = None                                                  # D-SSIM alone: no LPIPS chain, no weights
        else:
            lp = LPIPS.random(0, device=dev)
        patch = {"patch_size": args.patch_size, "lpips_weight": args.lpips_weight,
                 "lpips_weights": args.lpips_weights or ("none: lpips=None" if lp is None else
                                                          "LPIPS.random(0): seeded stand-in weights, not a perceptual metric")}
        crit_kw.update(patch_size=args.patch_size, lpips=lp, perceptual_weight=args.lpips_weight)
        if args.ssim_weight is not None:
            patch["ssim_weight"] = args.ssim_weight
            crit_kw["ssim_weight"] = args.ssim_weight
    true_poses = poses.copy()
    if args.pose_noise:
        from laenerf_amd.poses import perturb_poses
        deg, dist = (float(v) for v in args.pose_noise.split(","))
        poses = poses.copy()
        poses[held:] = perturb_poses(poses[held:], deg, dist, seed=23)
    train_images, stops = images[held:], None
    if args.exposure_noise:
        from laenerf_amd.exposure import perturb_exposures
        train_images, stops = perturb_exposures(images[held:], args.exposure_noise, seed=29)
    tr = make_trainer(dev, train_images, poses[held:], intr, iters=args.steps, n_rays=args.rays, graph=not args.no_graph,
                      capacity=args.capacity, error_map=error_map, ema_decay=0.95 if args.ema else None, distort_weight=args.distort,
                      **crit_kw)
    ckpt = {}
    if args.resume:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tr.load_checkpoint(args.resume)
        torch.cuda.synchronize()
        ckpt.update(load_ms=round((time.perf_counter() - t0) * 1e3, 2), resumed_at_step=tr.global_step)
    all_in, steady = _timed_run(tr, args.steps)
    if args.save:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        path = tr.save_checkpoint(args.save)
        ckpt.update(save_ms=round((time.perf_counter() - t0) * 1e3, 2), file_bytes=os.path.getsize(path), path=path,
                    saved_at_step=tr.global_step)
    from laenerf_amd.data import ResidentImages
    test = ResidentImages.from_arrays(images[:held], poses[:held], intr, device=dev)
    p = tr.evaluate(range(held), data=test, bg_color=1.0)
    pose = None
    if args.pose_noise or args.pose_lr is not None:
        from laenerf_amd.poses import pose_error
        a0, d0 = pose_error(poses[held:], true_poses[held:])
        a1, d1 = pose_error(tr.refined_poses().cpu().numpy(), true_poses[held:])
        pose = {"noise": args.pose_noise, "pose_lr": args.pose_lr, "start_rotation_deg": round(float(np.rad2deg(a0.mean())), 5),
                "end_rotation_deg": round(float(np.rad2deg(a1.mean())), 5), "start_translation": round(float(d0.mean()), 6),
                "end_translation": round(float(d1.mean()), 6)}
    exposure = None
    if args.exposure_noise or args.exposure_lr is not None:
        u = np.zeros((args.views - held, 3)) if stops is None else stops
        rms = lambda a: round(float(np.sqrt(np.mean(a * a))), 5)
        exposure = {"noise_stops": args.exposure_noise, "exposure_lr": args.exposure_lr, "start_rms_stops": rms(u),
                    "end_rms_stops": rms(tr.exposures() + u)}
    # where the time goes (after the measurement; each part synchronised on its own): the refresh with its host read, a
    # 16-step replay at the current capacity, and the padding rows of that capacity
    if patch is not None:
        perc = tr.perceptual_losses()
        patch.update(ms_per_step=round(steady, 4), rays_per_step=tr.n_rays, truncated_steps=tr.truncated_steps(),
                     peak_count=int(tr.r.peak_count), peak_to_mean=round(tr.peak_to_mean(), 3), patch_headroom=tr.patch_headroom,
                     first_lpips=float(perc[:16].mean()), final_lpips=float(perc[-16:].mean()), heldout_psnr_white=round(p, 3))
        if args.ssim_weight is not None:
            ds = tr.ssim_losses()
            patch.update(first_dssim=float(ds[:16].mean()), final_dssim=float(ds[-16:].mean()))
    refresh_ms, group_ms = _replay_windows(tr)
    if exposure is not None and args.exposure_lr is not None:
        exposure["step_and_publish_us"] = round(_exposure_launch_us(tr), 2)
    depth = None
    if args.depth:
        planes = teacher_depths(dev, poses[held:], intr, args.res, args.res)
        td = make_trainer(dev, images[held:], poses[held:], intr, iters=args.steps, n_rays=args.rays, graph=not args.no_graph,
                          capacity=args.capacity, error_map=error_map, ema_decay=0.95 if args.ema else None, depths=planes,
                          depth_weight=args.depth_weight, depth_grad=not args.depth_value_only, distort_weight=args.distort, **crit_kw)
        d_all_in, d_steady = _timed_run(td, args.steps)
        d_psnr = td.evaluate(range(held), data=test, bg_color=1.0)
        _, d_group_ms = _replay_windows(td)
        depth = {"ms_per_step_all_in": round(d_all_in, 4), "ms_per_step_after_64": round(d_steady, 4), "depth_weight": args.depth_weight,
                 "depth_grad": not args.depth_value_only, "supervised_pixels_frac": round(float((planes > 0).mean()), 4),
                 "replay_ms_per_step_windows": [round(v, 4) for v in d_group_ms], "mean_count": td.r.mean_count,
                 "first_depth_loss": float(td.depth_losses()[:16].mean()), "final_depth_loss": float(td.depth_losses()[-16:].mean()),
                 "final_loss": float(td.losses()[-16:].mean()), "heldout_psnr_white": round(d_psnr, 3), "steps_skipped": td.steps_skipped,
                 **({"first_distort_loss": float(td.distort_losses()[:16].mean()),
                     "final_distort_loss": float(td.distort_losses()[-16:].mean())} if args.distort is not None else {})}
    lens = None
    if args.lens:
        from laenerf_amd.undistort import CameraModel, Undistorter, target_intrinsics, undistort_map_numpy
        k1, k2 = (float(v) for v in args.lens.split(","))
        H = W = args.res
        cam = CameraModel(*intr, k1=k1, k2=k2)
        captured, cvalid = Undistorter(cam, None, intr, H, W, device=dev).distort_images(torch.from_numpy(images[held:]), return_valid=True)
        target = target_intrinsics(cam, H, W, 0.0)
        und = Undistorter(cam, None, target, H, W, device=dev)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fixed = und.images(captured)
        torch.cuda.synchronize()
        remap_ms = (time.perf_counter() - t0) * 1e3                     # the maps' first use included
        shift = np.abs(undistort_map_numpy(cam, intr, H, W) - undistort_map_numpy(CameraModel(*intr), intr, H, W)).max()
        lens = {"k1": k1, "k2": k2, "largest_displacement_px": round(float(shift), 2), "capture_valid_frac": round(float(cvalid.float().mean()), 4),
                "target_intrinsics": [round(v, 3) for v in target], "undistort_ms": round(remap_ms, 3), "heldout_psnr_white_true_pinhole": round(p, 3)}
        for name, ims, k in (("ignored", captured, intr), ("undistorted", fixed, target)):
            tl = make_trainer(dev, ims, poses[held:], k, iters=args.steps, n_rays=args.rays, graph=not args.no_graph, capacity=args.capacity)
            tl.train(args.steps)
            lens[f"heldout_psnr_white_{name}"] = round(tl.evaluate(range(held), data=test, bg_color=1.0), 3)
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
                      "replay_ms_per_step_windows": [round(v, 4) for v in group_ms],
                      "padding_rows_frac": round(1 - tr._m() / tr._m_cap(), 4) if tr.r.mean_count > 0 else None},
        **({"distort": {"distort_weight": args.distort, "first_distort_loss": float(tr.distort_losses()[:16].mean()),
                        "final_distort_loss": float(tr.distort_losses()[-16:].mean())}} if args.distort is not None else {}),
        **({"loss": args.loss, **({"huber_delta": args.huber_delta} if args.loss == "huber" else {})} if args.loss != "mse" else {}),
        **({"opacity": {"opacity_weight": args.entropy, "first_opacity_loss": float(tr.opacity_losses()[:16].mean()),
                        "final_opacity_loss": float(tr.opacity_losses()[-16:].mean())}} if args.entropy is not None else {}),
        **({"outliers": args.outliers} if args.outliers > 0 else {}),
        **({"mask_outliers": args.mask_outliers, "masked_pixels_frac": round(float((mask == 0).mean()), 4)} if mask is not None else {}),
        **({"pose": pose} if pose is not None else {}), **({"exposure": exposure} if exposure is not None else {}),
        **({"depth": depth} if depth is not None else {}), **({"checkpoint": ckpt} if ckpt else {}),
        **({"patch": patch} if patch is not None else {}), **({"lens": lens} if lens is not None else {}),
        "scene": f"{args.views - held} training + {held} held-out {args.res}x{args.res} RGBA uint8 views of a teacher network"}), flush=True)


if __name__ == "__main__":
    main()
