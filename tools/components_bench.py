"""Connected components on the device (csrc/components.hip; laenerf_amd/components.py).  Prints one JSON line with, per lattice
size R and field:
    label_us / sizes_us / filter_us   lae_components_label (3 launches), lae_components_sizes (4), lae_components_filter (1), each
                                      between two HIP events: [median, min, max] of --reps calls after two warm-ups
    *_floor_us, *_share               the pass's algorithmic bytes over the HBM rate, and floor / median.  Bytes, with N = R^3:
                                        label   8 N   the field read once, the labels written once
                                        sizes   8 N   the labels read once, the sizes written once
                                        filter  12 N  the field and the labels read, the output written
                                      (what the passes move beyond that -- the merge and flatten passes' reads of the labels, the
                                      zero fill of sizes, the two statistics passes, the gather of sizes[root] -- is their cost)
    stats                             n_components, largest_root, largest_size, n_inside
  field A  a solid (a ball of radius 0.35 R) plus --blobs small blobs around it: the shape of a trained scene with floaters
  field B  i.i.d. occupancy 0.3116, the simple-cubic site-percolation threshold: the largest, most tortuous clusters -- the merge
           pass's worst realistic case
and, measured in the same run at R = 256: marching cubes on field A (mc_us: count + emit between events) and the density sweep of
the synthetic trained scene of tools/mesh_bench.py (sweep_ms), the two passes the labelling sits between; extract_mesh with and
without keep_largest on that scene, alternated (extract_mesh_ms, extract_mesh_keep_largest_ms, [median, min, max]); and
NeRFRenderer.prune_floaters at H = 128 (prune_floaters_ms).

    python tools/components_bench.py [--res 256 512] [--reps 20] [--blobs 300]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_bench import HBM_TBS, event_us, teacher, timed, timed_range  # noqa: E402


def field_a(R, blobs, dev, seed=0):
    ax = torch.arange(R, device=dev, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (R - 1) / 2.0
    u = 0.35 * R - torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    del x, y, z
    rng = np.random.default_rng(seed)
    for _ in range(blobs):
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        rb = int(rng.integers(1, 4))
        centre = np.clip(np.rint(c + d * rng.uniform(0.35 * R + 6, 0.49 * R)), rb, R - 1 - rb).astype(int)
        u[tuple(slice(int(p) - rb, int(p) + rb + 1) for p in centre)] = 1.0
    return u.contiguous()


def field_b(R, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(R, R, R, device=dev, generator=g) < 0.3116).float()


def passes(u, thr, reps):
    from laenerf_amd import _lib
    lib = _lib.load()
    N = u.numel()
    R = u.shape[0]
    labels = torch.empty(u.shape, dtype=torch.int32, device=u.device)
    sizes = torch.empty(N, dtype=torch.int32, device=u.device)
    stats = torch.empty(4, dtype=torch.int32, device=u.device)
    out = torch.empty_like(u)
    row = {}
    row["label_us"] = event_us(lambda: _lib.check(lib.lae_components_label(u.data_ptr(), R, R, R, thr, labels.data_ptr(), _lib.stream()),
                                                  "label"), reps)
    row["sizes_us"] = event_us(lambda: _lib.check(lib.lae_components_sizes(labels.data_ptr(), N, sizes.data_ptr(), stats.data_ptr(),
                                                                           _lib.stream()), "sizes"), reps)
    st = stats.tolist()
    row["filter_us"] = event_us(lambda: _lib.check(lib.lae_components_filter(u.data_ptr(), labels.data_ptr(), sizes.data_ptr(), N, thr, 0,
                                                                             st[1], out.data_ptr(), _lib.stream()), "filter"), reps)
    for name, per_point in (("label", 8), ("sizes", 8), ("filter", 12)):
        floor = per_point * N / (HBM_TBS * 1e12) * 1e6
        row[name + "_floor_us"] = round(floor, 1)
        row[name + "_share"] = round(floor / row[name + "_us"][0], 3)
    row["total_us"] = round(row["label_us"][0] + row["sizes_us"][0] + row["filter_us"][0], 1)
    row["stats"] = dict(zip(("n_components", "largest_root", "largest_size", "n_inside"), st))
    return row


def mc_us(u, thr, reps):
    from laenerf_amd import _lib
    lib = _lib.load()
    R = u.shape[0]
    scratch = torch.empty(int(lib.lae_marching_cubes_scratch_bytes(R, R, R)), dtype=torch.uint8, device=u.device)
    counts = torch.empty(2, dtype=torch.int32, device=u.device)
    _lib.check(lib.lae_marching_cubes_count(u.data_ptr(), R, R, R, thr, scratch.data_ptr(), counts.data_ptr(), _lib.stream()), "count")
    V, T = counts.tolist()
    verts = torch.empty(max(V, 1), 3, device=u.device)
    tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=u.device)

    def both():
        _lib.check(lib.lae_marching_cubes_count(u.data_ptr(), R, R, R, thr, scratch.data_ptr(), counts.data_ptr(), _lib.stream()), "count")
        _lib.check(lib.lae_marching_cubes_emit(u.data_ptr(), R, R, R, thr, scratch.data_ptr(), verts.data_ptr(), tris.data_ptr(),
                                               _lib.stream()), "emit")

    return event_us(both, reps), V, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blobs", type=int, default=300)
    args = ap.parse_args()
    from laenerf_amd import mesh
    dev = torch.device("cuda:0")
    out = {"hbm_tbs": HBM_TBS, "reps": args.reps}
    for R in args.res:
        row = {}
        u = field_a(R, args.blobs, dev)
        row["A"] = passes(u, 0.0, args.reps)
        if R == 256:
            row["A"]["mc_us"], row["A"]["V"], row["A"]["T"] = mc_us(u, 0.0, args.reps)
        del u
        u = field_b(R, dev)
        row["B"] = passes(u, 0.5, args.reps)
        del u
        torch.cuda.empty_cache()
        out[str(R)] = row
    r = teacher(dev)
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    @torch.no_grad()
    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return r.model.density_sigma(pts)

    scene = {}
    scene["sweep_ms"], u = timed(lambda: mesh.extract_fields(bmin, bmax, 256, query), 5)
    thr = float(u.view(-1)[::97].quantile(0.99))
    del u
    res = timed_range([lambda: r.extract_mesh(resolution=256, threshold=thr),
                       lambda: r.extract_mesh(resolution=256, threshold=thr, keep_largest=True)], 5)
    scene["threshold"] = round(thr, 3)
    scene["extract_mesh_ms"], scene["extract_mesh_keep_largest_ms"] = ([round(x, 3) for x in m] for m in res)
    scene["sweep_ms"] = round(scene["sweep_ms"], 3)
    out["scene_256"] = scene
    r.update_extra_state()
    grid = r.density_grid.clone()
    times = []
    for i in range(6):
        r.density_grid.copy_(grid)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        info = r.prune_floaters(persist=False)
        b.record()
        b.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    out["prune_floaters_ms"] = [round(float(np.median(times)), 3), round(min(times), 3), round(max(times), 3)]
    out["prune_floaters_info"] = info
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
