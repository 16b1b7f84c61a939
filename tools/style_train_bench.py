"""Training the LAENeRF palette network on extracted views (laenerf_amd.editing.StyleTrainer): the middle stage of the recolor flow
(extract -> ~10 000 style steps -> recolor).  Scene as bench.py's `edit_extract`: the fixed eval model at bound 2, density scale 30,
flower occupancy, a box edit grid around the centre, 8 orbit poses at 1920x1080; extract_views gives the views.  Reported, all-in wall
time per step after warm-up:
  bucket_graph_ms   StyleTrainer, capacity 'bucket', one graph per capacity (the default)
  exact_graph_ms    capacity 'exact': one graph per view size, no pad rows (the floor the bucketing is measured against)
  bucket_eager_ms   the same steps without graphs
  user_path_ms      what a user writes today: torch jitter + forward_train at K + the torch losses of nerf/utils.py:990-995 +
                    FusedAdam with its GradScaler, eager
plus the palette distillation's time, the captures and the projected seconds for 10 000 steps.  One JSON line.

    python tools/style_train_bench.py [--steps 160]
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
import bench                                                                         # noqa: E402


def scene_views(dev, n_views=8, H=1080, W=1920):
    """bench.py edit_extract's scene and poses -> the extracted views"""
    from laenerf_amd import raymarching, synthetic as S
    from laenerf_amd.editing import extract_views
    net, r = bench.eval_model(dev, bound=2, seed=1234)
    r.density_scale = 30.0
    f = 1111.1 * H / 800
    intr = np.array([f, f, W / 2, H / 2], np.float32)
    poses = np.zeros((n_views, 4, 4), np.float32)
    for i in range(n_views):
        a = 2 * np.pi * i / n_views
        p = np.array([1.6 * np.cos(a), 1.6 * np.sin(a), 0.35 + 0.1 * np.sin(3 * a)])
        fwd = -p / np.linalg.norm(p)
        right = np.cross(np.array([0, 0, 1.0]), fwd); right /= np.linalg.norm(right)
        up = np.cross(fwd, right)
        poses[i, :3, 0], poses[i, :3, 1], poses[i, :3, 2], poses[i, :3, 3], poses[i, 3, 3] = right, up, fwd, p, 1
    poses = torch.from_numpy(poses).to(dev)
    dens = torch.from_numpy(S.flower_density_grid()).to(dev)
    coords = raymarching.morton3D_invert(torch.arange(128 ** 3, dtype=torch.int32, device=dev))
    near_origin = ((coords.float() - 63.5).abs().amax(dim=1) < 20)
    edit = raymarching.packbits(torch.where(near_origin[None], dens, torch.zeros_like(dens)).contiguous(), 10.0)
    images = torch.rand(n_views, H, W, 3, device=dev)
    views, _ = extract_views(r, poses, intr, H, W, edit, images, batch_views=2)
    return views


def make_net(dev):
    from laenerf_amd.editing import LAENeRF
    params = SimpleNamespace(bound=2, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(7)
    return LAENeRF(params, dir_encoding="sphere_harmonics").to(dev), params


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def trainer_ms(es, capacity, graph, warm, steps):
    from laenerf_amd.editing import StyleTrainer
    m, params = make_net(es.device)
    tr = StyleTrainer(m, es, params, iters=10000, seed=0, graph=graph, capacity=capacity)
    tr.train(warm)
    ms = timed(tr.train, steps)
    return tr, ms


def user_path_ms(es, sched, warm, steps):
    """eager forward_train at K + torch losses + FusedAdam, the view's jitter drawn with torch as EditDataset.collate does"""
    from laenerf_amd.optim import FusedAdam
    m, params = make_net(es.device)
    opt = FusedAdam(m, param_groups=m.get_params(1e-3), betas=(0.9, 0.999), eps=1e-8)
    state = {"s": 0}

    def run(n):
        for _ in range(n):
            v = int(sched[state["s"] % sched.size])
            state["s"] += 1
            x_term, dirs, target = es.view_arrays(v)
            x = x_term + ((torch.rand(x_term.shape[0], device=x_term.device) - 0.5) * es.depth_factor[v])[..., None] * dirs
            with torch.autocast("cuda", dtype=torch.float16):
                pred, w, o = m.forward_train(x, dirs)
                loss = torch.nn.functional.mse_loss(pred, target.half())
                loss = loss + m.weights_loss(w, params).half() + m.offset_loss(o, params).half() + m.palet_loss(params).half()
            opt.backward(opt.scale(loss))
            opt.step()
    run(warm)
    return timed(run, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--warm", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from laenerf_amd.editing import EditSet
    from laenerf_amd.editing.style_trainer import capacity_for
    views = scene_views(dev)
    es = EditSet.from_views(views, device=dev)
    K = es.counts_host
    out = {"views": int(es.V), "K_min": int(K.min()), "K_mean": int(K.mean()), "K_max": int(K.max())}
    tr_b, out["bucket_graph_ms"] = trainer_ms(es, "bucket", True, a.warm, a.steps)
    sched = tr_b._sched
    caps = np.array([capacity_for(K[v]) for v in sched[:a.warm + a.steps]])
    ks = K[sched[:a.warm + a.steps]]
    out["pad_fraction"] = round(float((caps - ks).sum() / caps.sum()), 4)
    out["bucket_captures"] = tr_b.captures
    out["bucket_distinct_capacities"] = int(len(set(caps.tolist())))
    tr_e, out["exact_graph_ms"] = trainer_ms(es, "exact", True, a.warm, a.steps)
    out["exact_captures"] = tr_e.captures
    _, out["bucket_eager_ms"] = trainer_ms(es, "bucket", False, 8, min(a.steps, 64))
    out["user_path_ms"] = user_path_ms(es, sched, 8, min(a.steps, 64))
    tr_b._distill()
    out["distill_ms"] = round(tr_b.distill_ms, 2)
    for k in ("bucket_graph_ms", "exact_graph_ms", "bucket_eager_ms", "user_path_ms"):
        out[k] = round(out[k], 4)
    out["bucket_over_exact"] = round(out["bucket_graph_ms"] / out["exact_graph_ms"], 3)
    out["speedup_over_user_path"] = round(out["user_path_ms"] / out["bucket_graph_ms"], 2)
    out["projected_s_10000_steps"] = round(out["bucket_graph_ms"] * 10000 / 1e3 + out["distill_ms"] / 1e3, 1)
    out["steps_skipped"] = tr_b.steps_skipped
    print(json.dumps(out))


if __name__ == "__main__":
    main()
