"""Ray registration (laenerf_amd.editing.ray_registration, csrc/rayreg.hip) at the shape of one 1080p view of an object: M cloud points
and n query points on a noisy sphere surface (radius 0.5, noise 4e-3), radius 0.1, reg_dist 2e-2.  Prints one JSON line:
    build_ms         RefCloud: bounding box, cell counts, scan, scatter (once per cloud)
    query_ms         the binned query (queries binned by cell, neighbour cells through LDS): [median, min, max]
    gather_ms        the lane-per-query query (the A/B predecessor), same form
    supervise_ms     lae_rayreg_supervise on the query's result, same form
    evals_per_row    distance evaluations of the binned query per row (a device counter); evals_share = that over M
    brute_ms         lae_min_dist_to_points on the same inputs: the brute-force kernel (distances only), same form
    torch_chain_ms   the reference's chain (th.linalg.norm(x[z:z+1000, None] - ref, axis=-1).min(-1)) on --torch-rows rows,
                     scaled to n rows
    cells, cell_side the grid the build chose; equal: the binned and the gather query agree bit for bit, and with the brute-force
                     kernel's distances to 1e-6
All times from HIP events around the call on the current stream, --reps launches after two warm-ups, the queries alternated.

    python tools/rayreg_bench.py [--M 1500000] [--n 500000] [--reps 7] [--torch-rows 4000]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def surface(k, gen, dev, sphere=0.5, noise=4e-3):
    v = torch.nn.functional.normalize(torch.randn(k, 3, generator=gen, device=dev), dim=-1)
    return (v * (sphere + noise * torch.randn(k, 1, generator=gen, device=dev))).contiguous()


def event_ms(fns, reps):
    """several calls, alternated: two warm-ups each, then reps rounds between HIP events -> [[median, min, max] ms]"""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for o, fn in zip(out, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            o.append(a.elapsed_time(b))
    return [[round(float(np.median(o)), 3), round(min(o), 3), round(max(o), 3)] for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=1500000)
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-rows", type=int, default=4000)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--reg-dist", type=float, default=2e-2)
    args = ap.parse_args()
    from laenerf_amd.backend import rayreg_backend as be
    from laenerf_amd.editing import RefCloud
    from laenerf_amd.editing.edit_dataset import min_dist_to_points
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    M, n = args.M, args.n
    ref_x, x = surface(M, gen, dev), surface(n, gen, dev)
    ref_rgb = torch.rand(M, 3, generator=gen, device=dev)
    ref_dirs, dirs = surface(M, gen, dev, 1.0, 0.0), surface(n, gen, dev, 1.0, 0.0)
    cloud = RefCloud(ref_x, ref_rgb, ref_dirs, radius=args.radius)
    out = {"M": M, "n": n, "radius": args.radius, "reg_dist": args.reg_dist, "cells": [int(c) for c in cloud.cells], "cell_side": cloud.s}
    out["build_ms"], = event_ms([lambda: be.build(cloud.points, M, cloud.radius, cloud.grid)], args.reps)
    out["query_ms"], out["gather_ms"], out["brute_ms"] = event_ms(
        [lambda: cloud.query(x), lambda: cloud.query(x, mode="gather"), lambda: min_dist_to_points(x, ref_x, args.radius)], args.reps)
    d, nn = cloud.query(x)
    out["evals_per_row"] = round(cloud.last_evals() / n, 1)
    out["evals_share"] = round(cloud.last_evals() / n / M, 5)
    dg, nng = cloud.query(x, mode="gather")
    db, _ = min_dist_to_points(x, ref_x, args.radius)
    out["equal"] = bool(torch.equal(d, dg) and torch.equal(nn, nng) and torch.allclose(d, db, rtol=1e-6, atol=0))
    out["within_radius"] = round(float((nn >= 0).float().mean()), 4)
    nn_reg = torch.empty(n, dtype=torch.int32, device=dev)
    target, weight, guide = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out["supervise_ms"], = event_ms([lambda: be.supervise(d, nn, n, ref_rgb, ref_dirs, M, dirs, args.reg_dist, args.radius, args.reg_dist, 0.1,
                                                         nn_reg, target, weight, guide, stats)], args.reps)
    out["registered"] = int(stats[0])
    rows = min(n, args.torch_rows)

    def chain():
        for z in range(0, rows, 1000):
            torch.linalg.norm(x[z:z + 1000, None, :] - ref_x, axis=-1).min(-1)

    (med, lo, hi), = event_ms([chain], max(2, args.reps // 2))
    out["torch_chain_ms"] = [round(v * n / rows, 1) for v in (med, lo, hi)]
    out["torch_chain_rows"] = rows
    out["speedup_vs_brute"] = round(out["brute_ms"][0] / out["query_ms"][0], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
