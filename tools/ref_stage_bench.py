"""Time the Ref-NPR second stage (editing/ref_stage.py) on the device and print one JSON line (README "Stylize from one painted
view").

On 8 synthetic 1080p views (an edit region of about --points pixels each, a third of the rows registered) with seeded
He-initialised VGG-16 weights:
  gt_step_graph_ms / gt_step_eager_ms     a RefStyleTrainer step of the gt phase, graph-replayed and eager
  ref_step_graph_ms / ref_step_eager_ms   a step of the ref phase with every term on (registered MSE, template feature term at
                                          --size, colour patch on the 67 x 120 relu5 grid, depth-guided TV, depth discontinuity)
  torch_gt_ms / torch_ref_ms              the reference-shaped torch chain (reference_ref_step) on the same inputs, forward + backward
  ref_terms_fwd_ms / ref_terms_bwd_ms     the new kernels alone (lae_ref_terms_forward / _backward, ref phase)
  supervision_ms_per_view                 build_ref_supervision, per view
Device times are CUDA-event intervals around `--reps` repetitions after `--warmup` ones.

    python tools/ref_stage_bench.py [--size 256] [--points 60000] [--reps 30]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H, W = 1080, 1920


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


def make_views(n_views, side, seed=0):
    from laenerf_amd.editing.edit_dataset import _crop_terms
    g = torch.Generator().manual_seed(seed)
    views = []
    for _ in range(n_views):
        x0 = int(torch.randint(0, H - side - 1, (1,), generator=g))
        y0 = int(torch.randint(0, W - side - 1, (1,), generator=g))
        keep = torch.rand(side + 1, side + 1, generator=g) > 0.1
        keep[0, 0] = keep[-1, -1] = True
        ii, jj = keep.nonzero(as_tuple=True)
        mask = ((ii + x0) * W + (jj + y0)).long()
        K = mask.numel()
        w8s = 0.97 + 0.0299 * torch.rand(K, generator=g)
        target = torch.rand(K, 3, generator=g)
        crop = _crop_terms(H, W, mask, w8s, target, 1 + torch.rand(K, generator=g))
        rows = torch.randperm(K, generator=g)[:K // 3].sort().values
        x = (torch.rand(3, generator=g) * 0.4 - 0.2) + (torch.rand(K, 3, generator=g) - 0.5) * 0.3
        d = torch.nn.functional.normalize(torch.randn(K, 3, generator=g), dim=-1)
        image = torch.zeros(H * W, 4)
        image[mask, :3], image[mask, 3] = target, 1.0
        views.append(dict(x_term=x, dirs=d, targets=target, depth_factor=torch.tensor(0.6 / 1024), indices=mask, w8s=w8s,
                          ref_targets=target[rows][:, [1, 2, 0]], target_weights=torch.rand(rows.numel(), generator=g), indices_ray_reg=rows,
                          style_guide=0.1 + 0.9 * torch.rand(crop["cut_gt"].shape[:2], generator=g), image=image.view(H, W, 4), **crop))
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="feature_size (the VGG input of the template term is size x size)")
    ap.add_argument("--points", type=int, default=60000, help="edit pixels per view (about)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from laenerf_amd.backend import ref_stage_backend as be
    from laenerf_amd.editing import LAENeRF
    from laenerf_amd.editing.ref_stage import GT, REF, RefEditSet, RefStyleTrainer, reference_ref_step
    from laenerf_amd.editing.semantic_encoder import SemanticEncoder, build_ref_supervision, vgg16_features
    from laenerf_amd.editing.style_trainer import capacity_for
    dev = torch.device("cuda", 0)
    S = args.size
    side = max(32, int(round(args.points ** 0.5)))
    views = make_views(args.views, side)
    torch.manual_seed(0)
    vgg = vgg16_features(29)
    for layer in vgg:
        if isinstance(layer, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.zeros_(layer.bias)
    sem = SemanticEncoder(vgg.to(dev))
    t0 = views[0]
    x0, x1, y0, y1 = (int(b) for b in t0["cut_min_max_xy"])
    template = {"painted": t0["image"][..., [2, 0, 1]] * t0["image"][..., 3:], "original": t0["image"][..., :3], "box": (x0, x1, y0, y1)}
    build_ref_supervision(views[:1], template, sem, feature_size=S)                       # MIOpen's first-call searches
    torch.cuda.synchronize()
    t_sup = time.perf_counter()
    sup = build_ref_supervision(views, template, sem, feature_size=S)
    torch.cuda.synchronize()
    out = {"size": S, "image": [H, W], "views": args.views, "points": int(views[0]["x_term"].shape[0]),
           "supervision_ms_per_view": (time.perf_counter() - t_sup) * 1e3 / len(views)}

    def params(warm):
        return SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                               offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2, tv_weight=1e-3, tv_depth_guide=True,
                               depth_disc_weight=1e-3, smooth_trans_weight=0, warmup_iterations=warm, mse_loss=6.0, cos_loss_factor=2.5,
                               color_patch_loss=30.0, feature_size=S)

    def trainer(graph, warm):
        p = params(warm)
        torch.manual_seed(0)
        enc = LAENeRF(p, dir_encoding="sphere_harmonics").to(dev)
        es = RefEditSet.from_views(views, (H, W), supervision=sup, device=dev)
        return RefStyleTrainer(enc, es, p, iters=args.reps + args.warmup + 48, sem=sem, distill_palette_steps=-1, graph=graph)

    tr = None
    for name, graph, warm in (("gt_step_graph_ms", True, 10 ** 9), ("gt_step_eager_ms", False, 10 ** 9), ("ref_step_graph_ms", True, -1),
                              ("ref_step_eager_ms", False, -1)):
        tr = trainer(graph, warm)
        tr.train(args.warmup + 32)
        torch.cuda.synchronize()
        out[name] = timed(lambda: tr.train(1), args.reps, 0)
        if name == "ref_step_graph_ms":
            out["capture_error"], out["captures"] = tr.capture_error, tr.captures

    # the new kernels alone and the reference-shaped torch chain, on view 0
    es, enc = tr.es, tr.enc
    K = int(views[0]["x_term"].shape[0])
    cap = capacity_for(K)
    es.set_schedule([0])
    x, d, t, m = es.sample(cap, step=0)
    pred16 = torch.rand(cap, 3, device=dev).half()
    p16, p32 = torch.empty(cap, 3, dtype=torch.half, device=dev), torch.empty(cap, 3, device=dev)
    resid, terms = torch.empty(es.n_out, 3, dtype=torch.float64, device=dev), torch.empty(2, device=dev)
    g_pw, g_t, g = torch.randn(cap, 3, device=dev), torch.ones(2, device=dev), torch.empty(cap, 3, device=dev)
    out["ref_terms_fwd_ms"] = timed(lambda: be.forward(es, pred16, cap, m, t, REF, p16, p32, resid, terms), args.reps, args.warmup)
    out["ref_terms_bwd_ms"] = timed(lambda: be.backward(es, pred16, cap, m, t, REF, resid, g_pw, g_t, g), args.reps, args.warmup)
    cp = sup["color_patch"][0].to(dev)
    v0 = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in views[0].items() if k != "image"}
    for name, mode in (("torch_gt_ms", GT), ("torch_ref_ms", REF)):
        def chain():
            tr.opt.zero_grad()
            loss, _ = reference_ref_step(enc, tr.params, x[:K], d[:K], t[:K], v0, (H, W), mode, sem=sem, style_feat=es.style_feat,
                                         tmpl_z=es.tmpl_z[0], color_patch=cp)
            (loss * 128.0).backward()
        out[name] = timed(chain, args.reps, args.warmup)
    out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
