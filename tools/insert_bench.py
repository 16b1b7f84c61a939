"""Time and quality of the scene insert (lae_insert_route / lae_insert_blend / lae_insert_occupancy, render_inserted, bake_insert).

    python tools/insert_bench.py [--res 800] [--bake-steps 384] [--fit-steps 512]

Prints one JSON line:
  route           lae_insert_route (with deltas) at 254 k and 5 M rows with no row, a tenth of the rows (a slab of the source grid
                  selected) and every row inserted: us, the inserted share, and floor_us = bytes / 6.29 TB/s with the bytes a
                  single pass would have to move: 24 read + 8 of deltas + 4 of slot per row, 24 written per inserted row (the HBM
                  rate a float4 copy reaches; 254 k rows fit the caches, so the floor is only a yardstick there)
  blend           lae_insert_blend (add, fp16 fields, the route's slots) at the same sizes and shares: us and floor_us for
                  4 + 8 read and 16 written per row, 8 read per inserted row
  occupancy       lae_insert_occupancy in us for source and destination grids of 1 and 2 cascades of 128^3 cells: the scene of
                  laenerf_amd/synthetic.py (`sphere_density_grid`) with one box selected, placed as tools/region_bench.py moves it
  render          render_inserted (add) against render_eval(frame_loop=False) of the destination alone on the same --res x --res
                  frame, ms per frame, with the host reads each makes per frame, and the fused frame loop beside them
  bake            two students fitted to 24 teacher views of 64 x 64 (tools/train_loop.py); one box of the first inserted into the
                  second: bake_insert ms (renders + seeding + training) and the held-out PSNR of the destination student's plain
                  render against render_inserted of the unbaked pair, before and after baking"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29          # MI355X HBM rate measured with a float4 copy (tools/mesh_bench.py)
G = 128


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
    from laenerf_amd.editing import SceneInsert, bake_insert, insert_blend, insert_occupancy, insert_route, render_inserted
    from laenerf_amd.editing.region_transform import coords_table
    from laenerf_amd.rays import get_rays
    from tools.mask_lift_bench import make_renderer
    from tools.region_bench import _time, box_selection
    from tools import train_loop as tl
    rot = np.array([[np.cos(0.5), -np.sin(0.5), 0.0], [np.sin(0.5), np.cos(0.5), 0.0], [0.0, 0.0, 1.0]])
    out = {"route": [], "blend": [], "occupancy": []}

    # ---- route and blend: the identity map between two one-cascade grids, a full source occupancy, three selections
    full = torch.full((G ** 3 // 8,), 0xFF, dtype=torch.uint8, device=dev)
    slab = torch.from_numpy(np.packbits(coords_table(G)[0] < 13, bitorder="little")).to(dev)          # 13 / 128 of the box
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (254_000, 5_000_000):
        x = (torch.rand(M, 3, device=dev, generator=g) * 2 - 1).contiguous()
        d = torch.nn.functional.normalize(torch.randn(M, 3, device=dev, generator=g), dim=-1).contiguous()
        deltas = torch.full((M, 2), 0.01, device=dev)
        sd, rd = (torch.rand(M, device=dev, generator=g) * 40).half(), torch.rand(M, 3, device=dev, generator=g).half()
        ss, rs = (torch.rand(M, device=dev, generator=g) * 40).half(), torch.rand(M, 3, device=dev, generator=g).half()
        bufs = (torch.empty(M, dtype=torch.int32, device=dev), torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev),
                torch.empty(1, dtype=torch.int32, device=dev))
        bo = (torch.empty(M, device=dev), torch.empty(M, 3, device=dev))
        for sel in (torch.zeros_like(full), slab, full):
            ins = SceneInsert(sel, (1, G), (1, G), pivot=[0, 0, 0], mode="add")
            us = _time(lambda: insert_route(ins, x, d, full, deltas=deltas, out=bufs), 50)
            k = int(bufs[3].item())
            nbytes = 36 * M + 24 * k
            out["route"].append({"rows": M, "inserted": k, "share": round(k / M, 4), "us": round(us, 2), "bytes": nbytes,
                                 "floor_us": round(nbytes / (HBM_TBS * 1e6), 2)})
            us = _time(lambda: insert_blend(ins, sd, rd, ss[:k], rs[:k], bufs[0], out=bo), 50)
            nbytes = 28 * M + 8 * k
            out["blend"].append({"rows": M, "inserted": k, "us": round(us, 2), "bytes": nbytes, "floor_us": round(nbytes / (HBM_TBS * 1e6), 2)})

    # ---- occupancy
    unpack = lambda t: int(np.unpackbits(t.cpu().numpy()).sum())
    scene = {c: torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=c, bound=float(2 ** (c - 1))), 10.0)).to(dev) for c in (1, 2)}
    for Cs in (1, 2):
        sel = box_selection(scene[Cs], Cs, float(2 ** (Cs - 1)), dev)
        for Cd in (1, 2):
            ins = SceneInsert(sel, (Cs, G), (Cd, G), rotation=rot, scale=1.2, pivot=[-0.5, 0.45, 0.4], position=[0.4, 0.45, -0.5])
            comp = torch.empty_like(scene[Cd])
            us = _time(lambda: insert_occupancy(ins, scene[Cd], scene[Cs], out=comp), 100)
            out["occupancy"].append({"src_cascade": Cs, "dst_cascade": Cd, "us": round(us, 2), "selected": unpack(sel & scene[Cs]),
                                     "destination": unpack(scene[Cd]), "composed": unpack(comp)})

    # ---- an inserted frame beside the destination's plain operator loop
    dst, src = make_renderer(dev), make_renderer(dev)
    ins = SceneInsert(box_selection(src.density_bitfield, 1, 1.0, dev), (1, G), (1, G), rotation=rot, pivot=[-0.5, 0.45, 0.4],
                      position=[0.4, 0.45, -0.5], mode="add")
    H = W = args.res
    focal = 1111.1 * W / 800
    ray = get_rays(torch.from_numpy(S.lookat_poses(1, radius=3.2, seed=0)).to(dev), (focal, focal, W / 2, H / 2), H, W)
    o, d = ray["rays_o"][0], ray["rays_d"][0]

    def frame(fn, **kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return fn(o, d, bg_color=1.0, perturb=False, image_hw=(H, W), **kw)
    inserted = lambda *a, **k: render_inserted(dst, src, ins, *a, **k)
    st_i, st_p = frame(inserted, want_stats=True)["stats"], frame(dst.render_eval, frame_loop=False, want_stats=True)["stats"]
    out["render"] = {"res": [H, W],
                     "render_inserted_ms": round(_time(lambda: frame(inserted), 5) / 1e3, 3),
                     "operator_loop_ms": round(_time(lambda: frame(dst.render_eval, frame_loop=False), 5) / 1e3, 3),
                     "frame_loop_ms": round(_time(lambda: frame(dst.render_eval), 5) / 1e3, 3),
                     "host_reads_inserted": 2 * st_i["iterations"], "host_reads_operator_loop": st_p["iterations"],
                     "rows_inserted_frame": st_i["rows"], "rows_operator_loop": st_p["rows"], "rows_routed_to_source": st_i["inserted_rows"],
                     "source_calls": st_i["source_calls"]}

    # ---- baking
    Hs = Ws = 64
    images, poses, intr = tl.teacher_views(dev, 24, Hs, Ws)
    students = []
    for seed in (1, 0):
        tr = tl.make_trainer(dev, images, poses, intr, iters=args.fit_steps, student_seed=seed)
        tr.train(args.fit_steps)
        students.append(tr)
    rs, rd_ = students[0].r, students[1].r
    ins = SceneInsert(box_selection(rs.density_bitfield, 1, 1.0, dev), (1, G), (1, G), pivot=[-0.5, 0.45, 0.4], position=[0.4, 0.45, -0.5],
                      mode="add")
    held = get_rays(torch.from_numpy(S.lookat_poses(4, radius=3.2, seed=77)).to(dev), intr, Hs, Ws)

    def held_out(fn):
        rd_.eval(); rs.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            res = [fn(held["rays_o"][i], held["rays_d"][i], bg_color=1.0, perturb=False, image_hw=(Hs, Ws))["image"].float() for i in range(4)]
        rd_.train(); rs.train()
        return torch.stack(res)
    target = held_out(lambda *a, **k: render_inserted(rd_, rs, ins, *a, **k))
    psnr = lambda a: float(-10 * torch.log10(((a - target) ** 2).mean()))
    before = psnr(held_out(rd_.render_eval))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bake_insert(rd_, students[1].opt, students[1].data, rs, ins, steps=args.bake_steps, lr=1e-2)
    torch.cuda.synchronize()
    bake_s = time.perf_counter() - t0
    out["bake"] = {"views": 24, "res": [Hs, Ws], "fit_steps": args.fit_steps, "bake_steps": args.bake_steps, "bake_s": round(bake_s, 3),
                   "held_out_psnr_before": round(before, 2), "held_out_psnr_after": round(psnr(held_out(rd_.render_eval)), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
