"""Time and quality of the region transform (lae_region_warp / lae_region_occupancy, render_transformed, bake_region_transform).

    python tools/region_bench.py [--res 800] [--bake-steps 384] [--fit-steps 512]

Prints one JSON line:
  warp            lae_region_warp in place at 254 k and 5 M rows: us, the bytes it moves (24 in + 28 out per row) and
                  floor_us = bytes / 6.29 TB/s (the HBM rate a float4 copy reaches; 254 k rows fit the caches, so the floor is
                  only a yardstick there)
  occupancy       lae_region_occupancy (move) in us on the scene of laenerf_amd/synthetic.py (`sphere_density_grid`: a sphere and
                  two boxes) with one box selected, at cascade 1 (bound 1) and cascade 2 (bound 2)
  render          render_transformed against render_eval(frame_loop=False) on the same --res x --res frame, ms per frame, and the
                  fused frame loop beside them
  bake            a student fitted to 24 teacher views of 64 x 64 (tools/train_loop.py), one box moved: bake_region_transform ms
                  (renders + seeding + training) and the held-out PSNR of the student's plain render against render_transformed
                  of the unbaked model, before and after baking"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29          # MI355X HBM rate measured with a float4 copy (tools/mesh_bench.py)


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


def box_selection(bits, cascade, bound, dev):
    """the occupied cells of sphere_density_grid's second box, enlarged by a few cells, as a selection bitfield"""
    from laenerf_amd.editing.region_transform import coords_table
    G = 128
    c = np.stack(coords_table(G), -1)
    sel = np.zeros((cascade, G ** 3), bool)
    for k in range(cascade):
        x = (((c + 0.5) / G) * 2 - 1) * min(2.0 ** k, bound)
        sel[k] = (np.abs(x[:, 0] + 0.5) < 0.16) & (np.abs(x[:, 1] - 0.45) < 0.34) & (np.abs(x[:, 2] - 0.4) < 0.34)
    return bits & torch.from_numpy(np.packbits(sel.reshape(-1), bitorder="little")).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--fit-steps", type=int, default=512)
    ap.add_argument("--bake-steps", type=int, default=384)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import build
    build.build()
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import RegionTransform, bake_region_transform, region_occupancy, region_warp, render_transformed
    from laenerf_amd.rays import get_rays
    from tools.mask_lift_bench import make_renderer
    from tools import train_loop as tl
    rot = np.array([[np.cos(0.5), -np.sin(0.5), 0.0], [np.sin(0.5), np.cos(0.5), 0.0], [0.0, 0.0, 1.0]])
    out = {"warp": [], "occupancy": []}

    # ---- the two kernels
    for cascade, bound in ((1, 1.0), (2, 2.0)):
        bits = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=cascade, bound=bound), 10.0)).to(dev)
        sel = box_selection(bits, cascade, bound, dev)
        rt = RegionTransform(sel, rotation=rot, translation=[0.9, 0.0, -0.9], scale=1.2, mode="move")
        comp = torch.empty_like(bits)
        us = _time(lambda: region_occupancy(rt, bits, out=comp), 100)
        unpack = lambda t: int(np.unpackbits(t.cpu().numpy()).sum())
        out["occupancy"].append({"cascade": cascade, "us": round(us, 2), "occupied": unpack(bits), "selected": unpack(sel), "composed": unpack(comp)})
        if cascade == 1:
            g = torch.Generator(device=dev).manual_seed(0)
            for M in (254_000, 5_000_000):
                x = (torch.rand(M, 3, device=dev, generator=g) * 2 - 1).contiguous()
                d = torch.nn.functional.normalize(torch.randn(M, 3, device=dev, generator=g), dim=-1).contiguous()
                us = _time(lambda: region_warp(rt, x, d, inplace=True), 50)
                nbytes = 52 * M
                out["warp"].append({"rows": M, "us": round(us, 2), "bytes": nbytes, "floor_us": round(nbytes / (HBM_TBS * 1e6), 2)})

    # ---- a transformed frame beside the plain operator loop
    r = make_renderer(dev)
    rt = RegionTransform(box_selection(r.density_bitfield, 1, 1.0, dev), rotation=rot, translation=[0.9, 0.0, -0.9], mode="move")
    H = W = args.res
    focal = 1111.1 * W / 800
    ray = get_rays(torch.from_numpy(S.lookat_poses(1, radius=3.2, seed=0)).to(dev), (focal, focal, W / 2, H / 2), H, W)
    o, d = ray["rays_o"][0], ray["rays_d"][0]

    def frame(fn, **kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return fn(o, d, bg_color=1.0, perturb=False, image_hw=(H, W), **kw)
    out["render"] = {"res": [H, W],
                     "render_transformed_ms": round(_time(lambda: frame(lambda *a, **k: render_transformed(r, rt, *a, **k)), 5) / 1e3, 3),
                     "operator_loop_ms": round(_time(lambda: frame(r.render_eval, frame_loop=False), 5) / 1e3, 3),
                     "frame_loop_ms": round(_time(lambda: frame(r.render_eval), 5) / 1e3, 3)}

    # ---- baking
    Hs = Ws = 64
    images, poses, intr = tl.teacher_views(dev, 24, Hs, Ws)
    tr = tl.make_trainer(dev, images, poses, intr, iters=args.fit_steps)
    tr.train(args.fit_steps)
    rs = tr.r
    rt = RegionTransform(box_selection(rs.density_bitfield, 1, 1.0, dev), translation=[0.9, 0.0, -0.9], mode="move")
    held = get_rays(torch.from_numpy(S.lookat_poses(4, radius=3.2, seed=77)).to(dev), intr, Hs, Ws)

    def held_out(fn):
        rs.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            res = [fn(held["rays_o"][i], held["rays_d"][i], bg_color=1.0, perturb=False, image_hw=(Hs, Ws))["image"].float() for i in range(4)]
        rs.train()
        return torch.stack(res)
    target = held_out(lambda *a, **k: render_transformed(rs, rt, *a, **k))
    psnr = lambda a: float(-10 * torch.log10(((a - target) ** 2).mean()))
    before = psnr(held_out(rs.render_eval))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bake_region_transform(rs, tr.opt, tr.data, rt, steps=args.bake_steps, lr=1e-2)
    torch.cuda.synchronize()
    bake_ms = (time.perf_counter() - t0) * 1e3
    out["bake"] = {"views": 24, "res": [Hs, Ws], "fit_steps": args.fit_steps, "bake_steps": args.bake_steps, "bake_ms": round(bake_ms, 1),
                   "held_out_psnr_before": round(before, 2), "held_out_psnr_after": round(psnr(held_out(rs.render_eval)), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
