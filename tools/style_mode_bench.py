"""Time LAENeRF's stylization step on the device and print one JSON line (README "Stylize").

Per style step, on a synthetic edit set (views of ~K points, crops of ~crop_hw pixels) with seeded random VGG-19 weights:
  image_fwd_ms / image_bwd_ms   the new kernels (lae_style_image_forward / _backward)
  vgg_fwd_bwd_ms                VGG-19 layers 0..14 on the [3,S,S] input, forward + data gradient (torch / MIOpen, fp32)
  gram_ms                       Gram matrices + MSE, forward + backward
  step_eager_ms / step_graph_ms a whole StyleTrainer step with every term on, eager and graph-replayed
  point_step_ms                 the step without the image terms (graph-replayed), for comparison
  projected_10k_stage_s         10 000 steps at the graph-replayed rate (1008 point-only warm-up steps + the rest stylized)
  torch_chain_ms                the reference-shaped torch chain of the non-VGG part: scatter, crop, interpolate, normalize and the
                                three image terms as torch ops, forward + backward
Device times are CUDA-event intervals around `--reps` repetitions after `--warmup` ones.

    python tools/style_mode_bench.py [--size 256] [--points 20000] [--reps 50]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def make_views(n_views, H, W, crop, seed=0):
    from laenerf_amd.editing.edit_dataset import _crop_terms
    g = torch.Generator().manual_seed(seed)
    views = []
    for v in range(n_views):
        x0 = int(torch.randint(0, H - crop[0], (1,), generator=g))
        y0 = int(torch.randint(0, W - crop[1], (1,), generator=g))
        keep = torch.rand(crop[0] + 1, crop[1] + 1, generator=g) > 0.1
        keep[0, 0] = keep[-1, -1] = True
        ii, jj = keep.nonzero(as_tuple=True)
        mask = ((ii + x0) * W + (jj + y0)).long()
        K = mask.numel()
        w8s = 0.97 + 0.03 * torch.rand(K, generator=g)
        target = torch.rand(K, 3, generator=g)
        out = _crop_terms(H, W, mask, w8s, target, 1 + torch.rand(K, generator=g), torch.rand(K, generator=g))
        x = (torch.rand(3, generator=g) * 0.4 - 0.2) + (torch.rand(K, 3, generator=g) - 0.5) * 0.3
        d = torch.nn.functional.normalize(torch.randn(K, 3, generator=g), dim=-1)
        views.append(dict(x_term=x, dirs=d, targets=target, depth_factor=torch.tensor(0.6 / 1024), indices=mask, **out))
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="crop_size S (the VGG input is S x S)")
    ap.add_argument("--points", type=int, default=20000, help="edit pixels per view (about)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from laenerf_amd.backend import style_backend
    from laenerf_amd.editing import EditSet, LAENeRF, StyleNetwork, StyleTrainer
    from laenerf_amd.editing.style_image import image_blocks, reference_image_terms
    from laenerf_amd.editing.style_network import vgg19_features
    from laenerf_amd.editing.style_trainer import capacity_for
    dev = torch.device("cuda", 0)
    S = args.size
    side = max(2, int(round(args.points ** 0.5)))
    H, W = side + 40, side + 60
    views = make_views(args.views, H, W, (side, side))
    es = EditSet.from_views(views, image_hw=(H, W), device=dev)
    torch.manual_seed(0)
    vgg = vgg19_features(14).to(dev)
    yy, xx = np.mgrid[0:300, 0:400]
    style_img = torch.from_numpy(np.stack([((xx + yy) // 12) % 2, ((xx - yy) // 20) % 2, np.full_like(xx, 1) * 0.5]).astype(np.float32))
    net = StyleNetwork(style_img, vgg, size=S, generator=torch.Generator().manual_seed(0))
    flags = 63
    K = views[0]["x_term"].shape[0]
    cap = capacity_for(K)
    es.set_schedule([0])
    _, _, _, m = es.sample(cap, step=0)
    pred16 = torch.rand(cap, 3, device=dev).half()
    vgg_in = torch.empty(3, S, S, device=dev)
    terms = torch.empty(3, device=dev)
    nb = image_blocks(es.max_crop_pixels)
    g_pred = torch.empty(cap, 3, device=dev)
    gv, gt = torch.randn(3, S, S, device=dev), torch.randn(3, device=dev)
    out = {"size": S, "points": K, "cap": cap, "crop": [side, side], "views": args.views}
    out["image_fwd_ms"] = timed(lambda: style_backend.style_image_forward(es, pred16, cap, m, S, vgg_in, flags, nb, terms), args.reps, args.warmup)
    out["image_bwd_ms"] = timed(lambda: style_backend.style_image_backward(es, pred16, cap, m, S, gv, gt, flags, g_pred), args.reps, args.warmup)
    x_in = torch.randn(3, S, S, device=dev, requires_grad=True)

    def vgg_fb():
        f = net.features(x_in)
        f.backward(torch.ones_like(f))
    out["vgg_fwd_bwd_ms"] = timed(vgg_fb, args.reps, args.warmup)
    feats = net.features(x_in).detach().requires_grad_(True)

    def gram_fb():
        from laenerf_amd.editing.style_network import gram_matrix
        torch.nn.functional.mse_loss(gram_matrix(feats), net.gram_target).backward()
    out["gram_ms"] = timed(gram_fb, args.reps, args.warmup)
    # the reference-shaped torch chain of the non-VGG part on the same view
    v0 = views[0]
    idx, box = v0["indices"].to(dev), v0["cut_min_max_xy"].tolist()
    gt_, th, tv, sm = (v0[k].to(dev) for k in ("cut_gt", "cut_tv_h", "cut_tv_v", "cut_smooth_trans"))

    def torch_chain():
        p = pred16[:K].float().requires_grad_(True)
        r, a, b, c = reference_image_terms(p, idx, box, H, W, gt_, th, tv, sm, S, flags)
        ((r * gv).sum() + a + b + c).backward()
    out["torch_chain_ms"] = timed(torch_chain, args.reps, args.warmup)

    # whole steps through the trainer
    def trainer(graph, style):
        params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=1e3 if style else 0, weight_loss_uniform=1e-3,
                                 weight_loss_non_uniform=1e-3, offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2,
                                 tv_weight=1e-3 if style else 0, tv_depth_guide=True, depth_disc_weight=1e-3 if style else 0,
                                 smooth_trans_weight=1e-3 if style else 0, warmup_iterations=-1, crop_size=S)
        torch.manual_seed(0)
        enc = LAENeRF(params, dir_encoding="sphere_harmonics").to(dev)
        es2 = EditSet.from_views(views, image_hw=(H, W), device=dev)
        n = args.reps + args.warmup + 32
        return StyleTrainer(enc, es2, params, iters=n, distill_palette_steps=-1, graph=graph, style_net=net if style else None)

    for name, graph, style in (("step_eager_ms", False, True), ("step_graph_ms", True, True), ("point_step_ms", True, False)):
        tr = trainer(graph, style)
        tr.train(args.warmup + 16)
        torch.cuda.synchronize()
        out[name] = timed(lambda: tr.train(1), args.reps, 0)
        if name == "step_graph_ms":
            out["capture_error"] = tr.capture_error
            out["captures"] = tr.captures
    out["projected_10k_stage_s"] = (1008 * out["point_step_ms"] + (10000 - 1008) * out["step_graph_ms"]) / 1e3
    out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
