"""Time and quality of lifting 2D masks into the edit grid (lae_mask_lift_pack / lae_mask_lift, EditGrid.new_from_masks).

    python tools/mask_lift_bench.py [--res 800] [--views 8 100] [--iou-views 8]

The scene is the synthetic one of laenerf_amd/synthetic.py: a randomly initialised default network with `sphere_density_grid`
(a sphere and two boxes, 128^3 cells, one cascade) as its occupancy and density_scale 30, so that surfaces are opaque; cameras
from `lookat_poses`.  The masks are painted from a known 3D region: a pixel is set where its surface point has x > 0.  Prints one
JSON line:
  occupied_share          the share of cells whose density_bitfield bit is set
  render_ms_per_view      render_eval of one depth view, as new_from_masks renders it
  pack_us_per_view        lae_mask_lift_pack of one view
  lift_us / torch_lift_us lae_mask_lift at V views, and the same rule written with torch operators on the same packed planes
                          (occupied cells by nonzero, one pass of elementwise operators and a gather per view, a scatter into the
                          bitfield); cells_differ: the cells on which the two disagree (float32 operators, another rounding order)
  iou                     the mean IoU of selection_masks(lifted grid) against the input masks, the grid lifted from --iou-views
                          views, at depth_margin 2 (the default), 1 and 4"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def make_renderer(dev):
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1).to(dev)
    net.encoder.embeddings.data.uniform_(-0.5, 0.5)
    r = NeRFRenderer(net, bound=1, min_near=0.2).to(dev)
    r.density_bitfield = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=r.cascade, bound=1.0), 10.0)).to(dev)
    r.density_scale = 30.0
    net.eval(); r.eval()
    return r


@torch.no_grad()
def render_view(r, pose, intr, H, W):
    from laenerf_amd.rays import get_rays
    ray = get_rays(pose[None], intr, H, W)
    with torch.autocast("cuda", dtype=torch.float16):
        res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=False, image_hw=(H, W))
    return ray, res["depth"].float().contiguous(), res["weights_sum"].float().contiguous()


@torch.no_grad()
def torch_lift(packed, poses, intr, H, W, bits, C, bound, G, depth_margin=2.0, min_views=1, min_share=0.5):
    """lae_mask_lift's rule with torch operators -> the bitfield"""
    from laenerf_amd.editing.mask_lift import _compact_bits as _compact
    dev = packed.device
    fx, fy, cx, cy = intr
    shifts = torch.arange(8, dtype=torch.uint8, device=dev)
    occ = ((bits[:, None] >> shifts) & 1).reshape(-1).bool()
    cells = occ.nonzero(as_tuple=True)[0]
    cas, m = cells // G ** 3, cells % G ** 3
    mip = torch.minimum(torch.pow(2.0, cas.float()), torch.tensor(float(bound), device=dev))
    coord = torch.stack([_compact(m), _compact(m >> 1), _compact(m >> 2)], -1).float()
    w = (((coord + 0.5) / G) * 2 - 1) * mip[:, None]
    slack = depth_margin * (2 * mip / G)
    n_in = torch.zeros(cells.numel(), dtype=torch.int32, device=dev)
    n_out = torch.zeros_like(n_in)
    for v in range(packed.shape[0]):
        d = w - poses[v, :3, 3]
        q = d @ poses[v, :3, :3]
        front = q[:, 2] > 0
        z = torch.where(front, q[:, 2], torch.ones_like(q[:, 2]))
        pu, pv = fx * q[:, 0] / z + cx, fy * q[:, 1] / z + cy
        inside = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        px = pu.clamp(0, W - 1).long()
        py = pv.clamp(0, H - 1).long()
        p = packed[v].reshape(-1)[py * W + px]
        visible = inside & (d.norm(dim=-1) <= p.abs() + slack)
        m_set = torch.signbit(p)
        n_in += visible & m_set
        n_out += visible & ~m_set
    sel = (n_in >= min_views) & (n_in.float() >= min_share * (n_in + n_out).float())
    chosen = torch.zeros(C * G ** 3, dtype=torch.uint8, device=dev)
    chosen[cells[sel]] = 1
    return (chosen.reshape(-1, 8) << shifts).sum(-1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--views", type=int, nargs="+", default=[8, 100])
    ap.add_argument("--iou-views", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import EditGrid, lift_masks, mask_iou, mask_lift_pack, selection_masks
    r = make_renderer(dev)
    H = W = args.res
    focal = 1111.1 * W / 800
    intr = (focal, focal, W / 2, H / 2)
    n_views = max(args.views + [args.iou_views])
    poses = torch.from_numpy(S.lookat_poses(n_views, radius=3.2, seed=0)).to(dev)
    render_view(r, poses[0], intr, H, W)                             # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    packed = torch.empty(n_views, H, W, device=dev)
    masks = []
    render_ms = 0.0
    for i in range(n_views):
        t0.record()
        ray, depth, opacity = render_view(r, poses[i], intr, H, W)
        t1.record()
        torch.cuda.synchronize()
        render_ms += t0.elapsed_time(t1)
        x = ray["rays_o"][0].reshape(-1, 3)[:, 0] + depth / opacity.clamp_min(1e-6) * ray["rays_d"][0].reshape(-1, 3)[:, 0]
        mask = ((opacity >= 0.5) & (x > 0)).to(torch.uint8)
        mask_lift_pack(depth, opacity, mask, out=packed[i])
        if i < args.iou_views:
            masks.append(mask.reshape(H, W))
        last = (depth, opacity, mask)
    pack_us = _time(lambda: mask_lift_pack(*last, out=packed[n_views - 1]), 200)
    bits, C, G = r.density_bitfield, r.cascade, r.grid_size
    out = {"res": [H, W], "grid": [C, G], "occupied_share": round(float(np.unpackbits(bits.cpu().numpy()).mean()), 5),
           "opaque_pixel_share": round(float((last[1] >= 0.5).float().mean()), 4),
           "render_ms_per_view": round(render_ms / n_views, 3), "pack_us_per_view": round(pack_us, 2), "lift": []}
    for V in args.views:
        a = (packed[:V], poses[:V].contiguous(), intr, H, W, bits, C, r.bound)
        grid = torch.empty_like(bits)
        k_us = _time(lambda: lift_masks(*a, grid_size=G, out=grid), 50)
        t_us = _time(lambda: torch_lift(*a, G), 3)
        differ = torch_lift(*a, G) ^ grid
        out["lift"].append({"views": V, "lift_us": round(k_us, 2), "torch_lift_us": round(t_us, 1),
                            "render_ms_of_these_views": round(render_ms / n_views * V, 2),
                            "selected_cells": int(np.unpackbits(grid.cpu().numpy()).sum()),
                            "cells_differ": int(np.unpackbits(differ.cpu().numpy()).sum())})
    iou = {}
    nv = args.iou_views
    for dm in (2.0, 1.0, 4.0):
        eg = EditGrid()
        eg.grid = lift_masks(packed[:nv], poses[:nv].contiguous(), intr, H, W, bits, C, r.bound, grid_size=G, depth_margin=dm)
        back = selection_masks(r, eg, poses[:nv], intr, H, W)
        iou[f"depth_margin_{dm:g}"] = round(float(np.mean([mask_iou(back[i], masks[i]) for i in range(nv)])), 4)
    out["iou"] = {"views": nv, **iou}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
