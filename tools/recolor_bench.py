"""Recolored views (laenerf_amd.editing.recolor) at 800x800 and 1920x1080: prepare once per pose, then one compose launch per palette
edit, against the reference-shaped torch chain that test_gui_styleenc runs for every edit (nerf/utils.py:1230-1311: re-render,
nonzero, get_weights / get_offsets, the edit expressions).  Synthetic scene as bench.py's `edit_extract`: the fixed eval model at
bound 2, density scale 30, flower occupancy, a box edit grid around the centre; a seeded LAENeRF with 8 bases.  One JSON line.

    python tools/recolor_bench.py
"""
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench                                                                         # noqa: E402


def pose_at(angle, radius=1.6):
    p = np.array([radius * np.cos(angle), radius * np.sin(angle), 0.35])
    fwd = -p / np.linalg.norm(p)
    right = np.cross(np.array([0, 0, 1.0]), fwd); right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    P = np.eye(4, dtype=np.float32)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, up, fwd, p
    return P


def reference_chain(r, enc, pose, intr, H, W, edit, bg, palette, p_weights, p_bias):
    from laenerf_amd.rays import get_rays
    rays = get_rays(pose[None], intr, H, W, -1)
    o, d = rays["rays_o"].view(-1, 3), rays["rays_d"].view(-1, 3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        res = r.render_eval(o, d, bg_color=bg, scale_depth=False, dens_grid=edit, image_hw=(H, W))
        preds, depth, pred_t = res["image"], res["depth"], res["weights_sum"]
        dd = torch.zeros_like(depth)
        dd[~depth.isnan()] = depth[~depth.isnan()]
        x_term = o + dd[..., None] * d
        idx = dd.flatten().nonzero(as_tuple=True)
        w = enc.get_weights(x_term[idx])
        off = enc.get_offsets(x_term[idx], d[idx])
        pw = torch.clamp_min(p_bias[None] + p_weights[None] * w, 0)
        pw /= pw.sum(-1)[..., None]
        pred = torch.clamp(off.half() + pw.half() @ palette.half(), 0, 1) + (1 - pred_t[idx][..., None]) * bg
        preds[idx] = pred.float()
    return preds


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(dev, H, W, r, enc, edit):
    from laenerf_amd.editing import RecolorView
    f = 1111.1 * H / 800
    intr = np.array([f, f, W / 2, H / 2], np.float32)
    pose = torch.from_numpy(pose_at(0.7)).to(dev)
    bg = torch.ones(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    palette = torch.rand(8, 3, device=dev, generator=g)
    p_weights = torch.rand(8, device=dev, generator=g) * 2
    p_bias = torch.randn(8, device=dev, generator=g) * 0.1
    view = RecolorView(r, enc)
    view.prepare(pose, intr, H, W, edit, bg)                                         # warm-up (workspaces)
    prepare_ms = median_ms(lambda: view.prepare(pose, intr, H, W, edit, bg), 5)
    out = torch.empty(H, W, 3, device=dev)
    out_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    for _ in range(5):
        view.compose(palette, p_weights, p_bias, out=out, out_u8=out_u8)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for a, b in ev:
        a.record()
        view.compose(palette, p_weights, p_bias, out=out, out_u8=out_u8)
        b.record()
    torch.cuda.synchronize()
    compose_us = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
    chain_ms = median_ms(lambda: reference_chain(r, enc, pose, intr, H, W, edit, bg, palette, p_weights, p_bias), 5)
    return {"H": H, "W": W, "K": view.K, "prepare_ms": round(prepare_ms, 3), "compose_us": round(compose_us, 2),
            "compose_launches": len(ev), "reference_chain_ms_per_edit": round(chain_ms, 3),
            "edit_speedup": round(chain_ms * 1e3 / compose_us, 1)}


def main():
    from laenerf_amd import raymarching
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import LAENeRF
    dev = torch.device("cuda", 0)
    net, r = bench.eval_model(dev, bound=2, seed=1234)
    r.density_scale = 30.0                                                           # a trained scene: opaque surfaces
    dens = torch.from_numpy(S.flower_density_grid()).to(dev)
    coords = raymarching.morton3D_invert(torch.arange(128 ** 3, dtype=torch.int32, device=dev))
    box = (coords.float() - 63.5).abs().amax(dim=1) < 20
    edit = raymarching.packbits(torch.where(box[None], dens, torch.zeros_like(dens)).contiguous(), 10.0)
    torch.manual_seed(7)
    enc = LAENeRF(SimpleNamespace(bound=2, num_palette_bases=8, style_weight=0), dir_encoding="sphere_harmonics").to(dev).eval()
    res = [run(dev, H, W, r, enc, edit) for H, W in ((800, 800), (1080, 1920))]
    print(json.dumps({"recolor": res, "bars": {"compose_us_max_1080p": 100.0, "edit_speedup_min": 50.0},
                      "note": "prepare: get_rays + edit-grid render + compaction + one K read + the two MLPs; compose: one launch per "
                              "palette edit (HIP events, median of 100); reference chain: the per-edit torch path of test_gui_styleenc"}))


if __name__ == "__main__":
    main()
