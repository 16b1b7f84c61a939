"""Mesh simplification (laenerf_amd/simplify.py, csrc/simplify.hip) on the teacher scene of tools/mesh_bench.py.  Prints one JSON
line with, per resolution R and per cell (in lattice spacings):
    V, T, V_out, T_out
    stage_us         HIP-event time of every stage of simplify_mesh, medians of --reps runs: keys, pairs, reduce, compact (the
                     kernels; compact includes the final allocation) and vertex_order, pair_order, dedup_order (torch: the stable
                     sorts with their running sums, searchsorted and the two host reads; dedup_order includes lae_simplify_first)
    total_ms         simplify_mesh on the host clock; order_share = the three *_order stages / the sum of all stages
    reduce_us_lanes  the reduce kernel with 1, 16 and 64 lanes per cluster
    reduce_bytes     what the reduce kernel must move if every gathered vertex came from cache after its first read: vertices
                     and triangles once, the two sorted index lists, the segment starts, the outputs;
                     reduce_floor_us = reduce_bytes / 6.29 TB/s
    torch_ms         the same rule written in torch operators (fp64 index_add_, torch.linalg.solve; torch_rule below) on the host
                     clock, torch_run_to_run = the largest difference of its fp32 positions between two runs and the number of
                     positions that differ (index_add_ adds atomically); ours_run_to_run: the same for simplify_mesh
    torch_vs_ours    the largest difference of the two rules' positions (one rule, two summation orders)
and once:
    sphere           on the analytic field r - |X - c| at --sphere-res: RMS and max distance of triangle samples (7 per
                     triangle) to the sphere, for the full mesh, quadric and mean placement at --sphere-cell, and marching cubes
                     re-run at R / cell, with their triangle counts
    textured         save_mesh_textured end to end at --textured-res without and with simplify=4: ms, T, layout cell, texture side

    python tools/simplify_bench.py [--res 256 512] [--cells 2 4 8] [--reps 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_TBS = 6.29
ORDER = ("vertex_order", "pair_order", "dedup_order")


def torch_rule(verts, tris, cell, origin, dims, reg=1e-2):
    """simplify_mesh's positions with torch operators: unique for the clusters, fp64 index_add_ for the sums, linalg.solve"""
    dev = verts.device
    o = torch.as_tensor(np.asarray(origin, np.float64), device=dev)
    c = float(np.float32(cell))
    p = verts.double()
    ijk = torch.floor((p - o) / c).long()
    keys = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    ukeys, vmap = torch.unique(keys, return_inverse=True)
    Vo = ukeys.numel()
    uijk = torch.stack([ukeys // (dims[1] * dims[2]), (ukeys // dims[2]) % dims[1], ukeys % dims[2]], 1)
    centre = o + (uijk.double() + 0.5) * c
    count = torch.zeros(Vo, dtype=torch.float64, device=dev).index_add_(0, vmap, torch.ones_like(p[:, 0]))
    m = torch.zeros(Vo, 3, dtype=torch.float64, device=dev).index_add_(0, vmap, p - centre[vmap]) / count[:, None]
    t = tris.long()
    mt = vmap[t]
    emit = torch.stack([torch.ones_like(mt[:, 0], dtype=torch.bool), mt[:, 1] != mt[:, 0], (mt[:, 2] != mt[:, 0]) & (mt[:, 2] != mt[:, 1])], 1)
    tt, slot = emit.nonzero(as_tuple=True)
    pc = mt[tt, slot]
    q = p[t[tt]] - centre[pc][:, None, :]
    n = torch.linalg.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    d = -(n * q[:, 0]).sum(1)
    A = torch.zeros(Vo, 3, 3, dtype=torch.float64, device=dev).index_add_(0, pc, n[:, :, None] * n[:, None, :])
    b = torch.zeros(Vo, 3, dtype=torch.float64, device=dev).index_add_(0, pc, d[:, None] * n)
    lam = reg * (A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]) / 3.0 + 1e-18 * c ** 4
    x = torch.linalg.solve(A + lam[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev), lam[:, None] * m - b)
    return (centre + x.clamp(-c / 2, c / 2)).float()


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3), res


def staged(fn, reps):
    """fn(probe) -> {stage: median us} from HIP events recorded at every probe"""
    rows = []
    for i in range(reps + 1):
        marks = []

        def probe(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))
        probe("start")
        fn(probe)
        torch.cuda.synchronize()
        if i:
            rows.append({b[0]: a[1].elapsed_time(b[1]) * 1e3 for a, b in zip(marks, marks[1:])})
    return {k: round(float(np.median([r[k] for r in rows])), 1) for k in rows[0]}


def run_to_run(a, b):
    return {"max_abs": float((a - b).abs().max()) if a.numel() else 0.0, "differing": int((a != b).sum())}


def surface_error(verts, tris, centre, radius):
    """distance to the sphere of 7 samples per triangle (corners' mean, edge midpoints, and three interior points)"""
    w = torch.tensor([[1 / 3, 1 / 3, 1 / 3], [.5, .5, 0], [0, .5, .5], [.5, 0, .5], [.6, .2, .2], [.2, .6, .2], [.2, .2, .6]],
                     dtype=torch.float64, device=verts.device)
    p = verts.double()[tris.long()]                                          # [T, 3, 3]
    s = torch.einsum("sk,tka->tsa", w, p)
    d = (s - centre).norm(dim=2) - radius
    return {"T": int(tris.shape[0]), "rms": round(float(d.pow(2).mean().sqrt()), 5), "max": round(float(d.abs().max()), 5)}


def sphere_rows(R, cell, dev):
    from laenerf_amd import mesh
    from laenerf_amd.simplify import simplify_mesh
    centre = torch.tensor([0.13, -0.21, 0.07], dtype=torch.float64, device=dev) + (R - 1) / 2
    radius = 0.357 * R

    def field(n):
        ax = torch.linspace(0, R - 1, n, dtype=torch.float64, device=dev)
        X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
        return (radius - ((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2).sqrt()).float().contiguous()

    v, t = mesh.marching_cubes(field(R), 0.0)
    out = {"R": R, "cell": cell, "radius": radius, "full": surface_error(v, t, centre, radius)}
    origin, dims = np.zeros(3, np.float32), (R // int(cell) + 2,) * 3
    for placement in ("quadric", "mean"):
        s = simplify_mesh(v, t, float(cell), origin=origin, dims=dims, placement=placement)
        out[placement] = surface_error(s["vertices"], s["triangles"], centre, radius)
    n = int(round(R / cell))
    vc, tc = mesh.marching_cubes(field(n), 0.0)
    out["marching_cubes_coarse"] = dict(surface_error(vc * ((R - 1) / (n - 1)), tc, centre, radius), lattice=n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--cells", type=float, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--sphere-res", type=int, default=256)
    ap.add_argument("--sphere-cell", type=float, default=4)
    ap.add_argument("--textured-res", type=int, default=256)
    ap.add_argument("--no-textured", action="store_true")
    args = ap.parse_args()
    from laenerf_amd import mesh
    from laenerf_amd.simplify import simplify_mesh
    from mesh_bench import teacher
    dev = torch.device("cuda:0")
    r = teacher(dev)
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    @torch.no_grad()
    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return r.model.density_sigma(pts)

    out = {"network": "NeRFNetwork(bound=1), teacher of tools/train_loop.py (seed 11)"}
    thresholds = {}
    for R in args.res:
        u = mesh.extract_fields(bmin, bmax, R, query)
        thr = thresholds[R] = float(u.view(-1)[::97].quantile(args.quantile))
        del u
        m = r.extract_mesh_attributes(resolution=R, threshold=thr, colors=False, normals=False)
        v, t = m["vertices"], m["triangles"]
        V, T = v.shape[0], t.shape[0]
        rows = {"V": V, "T": T, "threshold": round(thr, 3)}
        for k in args.cells:
            cell, origin, dims = r.simplify_grid(R, k)
            kw = dict(origin=origin, dims=dims)
            row = {}
            row["total_ms"], s = host_ms(lambda: simplify_mesh(v, t, cell, **kw), args.reps)
            Vo, To = s["vertices"].shape[0], s["triangles"].shape[0]
            row["V_out"], row["T_out"] = Vo, To
            st = staged(lambda probe: simplify_mesh(v, t, cell, probe=probe, **kw), args.reps)
            row["stage_us"] = st
            row["order_share"] = round(sum(st.get(n, 0.0) for n in ORDER) / sum(st.values()), 3)
            row["reduce_us_lanes"] = {str(L): staged(lambda probe: simplify_mesh(v, t, cell, lanes=L, probe=probe, **kw), max(2, args.reps // 2))["reduce"]
                                      for L in (1, 16, 64)}
            pairs = int((s["vertex_map"][t.long()].sort(1)[0].diff(dim=1) != 0).sum()) + T
            row["pairs"] = pairs
            row["reduce_bytes"] = 12 * V + 12 * T + 8 * V + 8 * pairs + (16 + 8) * (Vo + 1) + 24 * Vo
            row["reduce_floor_us"] = round(row["reduce_bytes"] / (HBM_TBS * 1e12) * 1e6, 1)
            again = simplify_mesh(v, t, cell, **kw)
            row["ours_run_to_run"] = run_to_run(s["vertices"], again["vertices"])
            row["torch_ms"], p1 = host_ms(lambda: torch_rule(v, t, cell, origin, dims), max(2, args.reps // 2))
            p2 = torch_rule(v, t, cell, origin, dims)
            row["torch_run_to_run"] = run_to_run(p1, p2)
            row["torch_vs_ours"] = float((p1 - s["vertices"]).abs().max())
            del s, again, p1, p2
            rows[f"cell_{k:g}"] = row
            torch.cuda.empty_cache()
        out[str(R)] = rows
        del m, v, t
        torch.cuda.empty_cache()
    out["sphere"] = sphere_rows(args.sphere_res, args.sphere_cell, dev)
    if not args.no_textured:
        R = args.textured_res
        thr = thresholds.get(R)
        if thr is None:
            thr = float(mesh.extract_fields(bmin, bmax, R, query).view(-1)[::97].quantile(args.quantile))
        tex = {"R": R}
        with tempfile.TemporaryDirectory() as d:
            for name, extra in (("full", {}), ("simplify_4", {"simplify": 4})):
                f = os.path.join(d, name + ".obj")
                ms, (vv, tt) = host_ms(lambda: r.save_mesh_textured(f, resolution=R, threshold=thr, **extra), 2)
                lay = r.extract_mesh_textured(resolution=R, threshold=thr, **extra)["layout"]
                tex[name] = {"ms": ms, "V": len(vv), "T": len(tt), "layout_cell": lay.cell, "texture_side": lay.S,
                             "obj_bytes": os.path.getsize(f), "png_bytes": os.path.getsize(f[:-4] + ".png")}
        out["textured"] = tex
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
