"""Mesh extraction (Trainer.save_mesh, nerf/utils.py:722-741) on a structured random NeRFNetwork, set up like tools/train_loop.py's
teacher.  Prints one JSON line with, per resolution R:
    field_ms         extract_fields: the R^3 density sweep into a device field (128^3 chunks)
    mc_count_ms      marching cubes, count + scan + the one host read of V, T
    mc_emit_ms       marching cubes, vertex + triangle passes
    extract_mesh_ms  NeRFRenderer.extract_mesh (sweep, marching cubes, download, scaling)
    save_mesh_ms     NeRFRenderer.save_mesh (the same + the binary PLY)
    V, T
    mc_bytes         bytes the marching-cubes passes must move: the field read by three passes, the per-point words written and
                     read, block counts, vertices and triangles written; mc_floor_us = mc_bytes / 6.29 TB/s
    ref_loop_ms      for contrast: the reference-shaped field loop (host lattice per chunk, a .cpu() copy per 128^3 chunk)
    attrs_us         lae_mesh_vertex_attrs (pos, normals, dirs) from HIP events: [median, min, max] of --reps launches;
                     attrs_bytes = 12 in + 36 out per vertex + the field once (every line touched, each counted once),
                     attrs_floor_us = attrs_bytes / 6.29 TB/s
    pack_us          lae_mesh_pack_ply (27-byte vertex records and the 13-byte face records), same form;
                     pack_bytes = (36 + 27) V + (12 + 13) T, pack_floor_us
    color_ms         the colour query model(pos, dirs) over all vertices in 1 << 20-row chunks
    save_mesh_color_ms   save_mesh(normals=True, colors=True): attributes and PLY bodies on the device
    host_color_ms    the same file the host-shaped way: field and mesh downloaded, vertex_attributes_numpy, the colour query on
                     the device from uploaded positions, numpy structured arrays, one write per array
    Each *_ms value of the three save paths comes with *_ms_range = [min, max]; the three are timed alternately, in one run.
Host clocks around work that ends in a device synchronise; medians of --reps runs after one warm-up.  Kernel times per pass: run
this under `rocprofv3 --kernel-trace --stats` (k_mc_count, k_mc_scan, k_mc_vertices, k_mc_triangles).

The network's density is noise at the lattice scale; the threshold (default: the field's 99th percentile, from every 97th value)
keeps the mesh at a size a PLY on disk can take.

    python tools/mesh_bench.py [--res 256 512] [--reps 5] [--quantile 0.99 | --threshold 10] [--no-ply]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.29          # MI355X HBM rate measured with a float4 copy (79 % of the 8 TB/s spec)


def teacher(dev):
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(11)
    net = NeRFNetwork(bound=1).to(dev).eval()
    net.encoder.embeddings.data.uniform_(-1.0, 1.0)
    net.sigma_net.weights.data.mul_(1.5)
    return NeRFRenderer(net, bound=1, density_thresh=10).to(dev).eval()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), res


def timed_range(fns, reps):
    """several host-timed paths, alternated: one warm-up each, then reps rounds -> [(median, min, max)]"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for o, fn in zip(out, fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            o.append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(o)), float(min(o)), float(max(o))) for o in out]


def event_us(fn, reps):
    """one launch between two HIP events, reps times after two warm-ups -> [median, min, max] us"""
    fn(); fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return [round(float(np.median(out)), 1), round(min(out), 1), round(max(out), 1)]


def host_colored_save(r, path, R, thr, query, bmin, bmax):
    """save_mesh(normals=True, colors=True) the host-shaped way"""
    from laenerf_amd import mesh
    u = mesh.extract_fields(bmin, bmax, R, query)
    v, t = mesh.marching_cubes(u, thr)
    un, vn, tn = u.cpu().numpy(), v.cpu().numpy(), t.cpu().numpy()
    a = mesh.vertex_attributes_numpy(un, vn, bmin, bmax)
    pos, dirs = torch.from_numpy(a["pos"]).cuda(), torch.from_numpy(a["dirs"]).cuda()
    rgb = torch.empty_like(pos)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for i in range(0, len(vn), 1 << 20):
            rgb[i:i + (1 << 20)] = r.model(pos[i:i + (1 << 20)], dirs[i:i + (1 << 20)])[1].float()
    verts = np.empty(len(vn), mesh.vertex_dtype(True, True))
    verts["pos"], verts["normals"], verts["colors"] = a["pos"], a["normals"], mesh.color_bytes_numpy(rgb.cpu().numpy())
    faces = np.empty(len(tn), mesh.FACE_DTYPE)
    faces["n"], faces["i"] = 3, tn
    with open(path, "wb") as f:
        f.write(mesh.ply_header(len(vn), len(tn), True, True))
        f.write(verts.tobytes())
        f.write(faces.tobytes())


def reference_loop(bmin, bmax, R, query, S=128):
    X = torch.linspace(bmin[0], bmax[0], R).split(S)
    Y = torch.linspace(bmin[1], bmax[1], R).split(S)
    Z = torch.linspace(bmin[2], bmax[2], R).split(S)
    u = np.zeros([R, R, R], dtype=np.float32)
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(Y):
            for zi, zs in enumerate(Z):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = \
                    query(pts.to("cuda")).reshape(len(xs), len(ys), len(zs)).cpu().numpy()
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--no-ply", action="store_true", help="skip save_mesh (a large PLY goes through the host's disk)")
    args = ap.parse_args()
    from laenerf_amd import _lib, mesh
    dev = torch.device("cuda:0")
    r = teacher(dev)
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    @torch.no_grad()
    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return r.model.density_sigma(pts)

    lib = _lib.load()
    out = {"network": "NeRFNetwork(bound=1), teacher of tools/train_loop.py (seed 11)"}
    for R in args.res:
        row = {}
        row["field_ms"], u = timed(lambda: mesh.extract_fields(bmin, bmax, R, query), args.reps)
        thr = args.threshold if args.threshold is not None else float(u.view(-1)[::97].quantile(args.quantile))
        row["threshold"] = thr
        nx = ny = nz = R
        scratch = torch.empty(int(lib.lae_marching_cubes_scratch_bytes(nx, ny, nz)), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)

        def count():
            _lib.check(lib.lae_marching_cubes_count(u.data_ptr(), nx, ny, nz, thr, scratch.data_ptr(), counts.data_ptr(),
                                                    _lib.stream()), "marching_cubes_count")
            return [int(x) for x in counts.cpu()]

        row["mc_count_ms"], (V, T) = timed(count, args.reps)
        verts = torch.empty(max(V, 1), 3, device=dev)
        tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=dev)
        row["mc_emit_ms"], _ = timed(lambda: _lib.check(lib.lae_marching_cubes_emit(
            u.data_ptr(), nx, ny, nz, thr, scratch.data_ptr(), verts.data_ptr(), tris.data_ptr(), _lib.stream()), "emit"), args.reps)
        row["V"], row["T"] = V, T
        P, nb = R ** 3, (R ** 3 + 1023) // 1024
        row["mc_bytes"] = 3 * 4 * P + 4 * P + 4 * P + 4 * 4 * nb + 12 * V + 12 * T
        row["mc_floor_us"] = round(row["mc_bytes"] / (HBM_TBS * 1e12) * 1e6, 1)
        if V:
            verts, tris = verts[:V], tris[:T]
            at = {k: torch.empty(V, 3, device=dev) for k in ("pos", "normals", "dirs")}
            box = [float(x) for x in bmin] + [float(x) for x in bmax]
            row["attrs_us"] = event_us(lambda: _lib.check(lib.lae_mesh_vertex_attrs(
                u.data_ptr(), nx, ny, nz, verts.data_ptr(), V, *box, at["pos"].data_ptr(), at["normals"].data_ptr(),
                at["dirs"].data_ptr(), _lib.stream()), "attrs"), args.reps)
            row["attrs_bytes"] = (12 + 36) * V + 4 * P
            row["attrs_floor_us"] = round(row["attrs_bytes"] / (HBM_TBS * 1e12) * 1e6, 1)
            rgb = torch.rand(V, 3, device=dev)
            vb = torch.empty(V * 27, dtype=torch.uint8, device=dev)
            fb = torch.empty(T * 13, dtype=torch.uint8, device=dev)
            row["pack_us"] = event_us(lambda: _lib.check(lib.lae_mesh_pack_ply(
                at["pos"].data_ptr(), at["normals"].data_ptr(), rgb.data_ptr(), V, tris.data_ptr(), T, vb.data_ptr(), fb.data_ptr(),
                _lib.stream()), "pack"), args.reps)
            row["pack_bytes"] = (36 + 27) * V + (12 + 13) * T
            row["pack_floor_us"] = round(row["pack_bytes"] / (HBM_TBS * 1e12) * 1e6, 1)

            @torch.no_grad()
            def colors():
                out = torch.empty(V, 3, device=dev)
                with torch.autocast("cuda", dtype=torch.float16):
                    for i in range(0, V, 1 << 20):
                        out[i:i + (1 << 20)] = r.model(at["pos"][i:i + (1 << 20)], at["dirs"][i:i + (1 << 20)])[1].float()
                return out

            row["color_ms"], _ = timed(colors, args.reps)
            del at, rgb, vb, fb
        del u, scratch, verts, tris
        row["extract_mesh_ms"], _ = timed(lambda: r.extract_mesh(resolution=R, threshold=thr), args.reps)
        if not args.no_ply:
            with tempfile.TemporaryDirectory() as d:
                f = os.path.join(d, "m.ply")
                res = timed_range([lambda: r.save_mesh(f, resolution=R, threshold=thr),
                                   lambda: r.save_mesh(f, resolution=R, threshold=thr, normals=True, colors=True),
                                   lambda: host_colored_save(r, f, R, thr, query, bmin, bmax)], max(1, args.reps // 2))
                for name, (med, lo, hi) in zip(("save_mesh_ms", "save_mesh_color_ms", "host_color_ms"), res):
                    row[name], row[name + "_range"] = med, [round(lo, 3), round(hi, 3)]
                row["ply_color_bytes"] = os.path.getsize(f)
        row["ref_loop_ms"], _ = timed(lambda: reference_loop(bmin, bmax, R, query), max(1, args.reps // 2))
        out[str(R)] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
