"""Time of the TSDF mesh export (lae_tsdf_fuse / lae_tsdf_vertex_colors, NeRFRenderer.save_mesh_tsdf).

    python tools/tsdf_bench.py [--res 256 512] [--views 100] [--hw 800] [--runs 5] [--e2e-views 100]

The fused views are synthetic: an analytic sphere of radius 0.6 in the box [-1, 1]^3 seen from `lookat_poses` cameras at radius 3.2
(focal 1111 at 800 pixels), its surface distance per pixel written as lae_mask_lift_pack writes it, random bytes as frames.
Prints one JSON line:
  fuse[]   per lattice resolution R: fuse_ms with the per-brick cull on and off (LAE_TSDF_CULL), without and with frames (the
           median of --runs timed calls each), torch_ms: the same rule written view by view in torch operators on the device
           (one run after a warm-up, without frames), differ: the voxels whose counts differ between the two, floor_ms: the
           output bytes (u; u + counts + rgb with frames) at 6.3 TB/s
  close    the first --res again with the cameras at radius 1.5, where most of the lattice is outside each frame: the cull on and off
  vertex_colors_us   lae_tsdf_vertex_colors on the R = first --res mesh, and its vertex count
  e2e      at R = 256 on the synthetic renderer of tools/mask_lift_bench.py: save_mesh_tsdf (rendering --e2e-views views of
           --hw pixels, fusing, meshing, writing the PLY; render_ms: the renders alone) beside save_mesh(normals=True, colors=True)
           at the density field's 99th percentile as its threshold (a random network has no level 10), wall-clock ms each"""
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

HBM = 6.3e12
RADIUS = 0.6


def _times(fn, runs):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


@torch.no_grad()
def sphere_views(poses, intr, H, W):
    """the packed planes [V, H, W] of the analytic sphere: the distance along each pixel's ray, +inf where it misses"""
    from laenerf_amd.rays import get_rays
    out = torch.empty(poses.shape[0], H, W, device=poses.device)
    for v in range(poses.shape[0]):
        ray = get_rays(poses[v:v + 1], intr, H, W)
        o, d = ray["rays_o"][0].reshape(-1, 3), ray["rays_d"][0].reshape(-1, 3)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - RADIUS * RADIUS)
        t = -b - disc.clamp_min(0).sqrt()
        out[v] = torch.where((disc > 0) & (t > 0), t, torch.full_like(t, float("inf"))).reshape(H, W)
    return out


@torch.no_grad()
def torch_fuse(packed, poses, intr, H, W, axes, trunc, min_views=1):
    """lae_tsdf_fuse's rule (without frames) with torch operators, view by view -> (u, counts int32 [n, 3])"""
    dev = packed.device
    fx, fy, cx, cy = intr
    xs, ys, zs = (a.to(dev) for a in axes)
    gx, gy, gz = torch.meshgrid(xs, ys, zs, indexing="ij")
    w = torch.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], -1)
    n = w.shape[0]
    cnt = torch.zeros(n, 3, dtype=torch.int32, device=dev)
    S = torch.zeros(n, device=dev)
    for v in range(packed.shape[0]):
        d = w - poses[v, :3, 3]
        q = d @ poses[v, :3, :3]
        front = q[:, 2] > 0
        z = torch.where(front, q[:, 2], torch.ones_like(q[:, 2]))
        pu, pv = fx * q[:, 0] / z + cx, fy * q[:, 1] / z + cy
        inside = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        px, py = pu.clamp(0, W - 1).long(), pv.clamp(0, H - 1).long()
        ts = packed[v].reshape(-1)[py * W + px].abs()
        s = ts - d.norm(dim=-1)
        seen = inside & ~ts.isnan()
        occ = seen & (s < -trunc)
        free = seen & (s > trunc)
        near = seen & ~occ & ~free
        cnt[:, 0] += near
        cnt[:, 1] += free
        cnt[:, 2] += occ
        S += torch.where(near, s / trunc, torch.zeros_like(s))
    n_obs = cnt[:, 0] + cnt[:, 1]
    tsdf = torch.where(n_obs >= min_views, (S + cnt[:, 1].float()) / n_obs.clamp_min(1).float(),
                       torch.where(cnt[:, 2] > 0, -torch.ones_like(S), torch.ones_like(S)))
    return (-tsdf).reshape(xs.numel(), ys.numel(), zs.numel()), cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--e2e-views", type=int, default=100)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import mesh
    from laenerf_amd import synthetic as S
    from laenerf_amd.tsdf import tsdf_fuse, tsdf_vertex_colors
    H = W = args.hw
    focal = 1111.1 * W / 800
    intr = (focal, focal, W / 2, H / 2)
    V = args.views
    poses = torch.from_numpy(S.lookat_poses(max(V, args.e2e_views), radius=3.2, seed=0)).to(dev)
    packed = sphere_views(poses[:V], intr, H, W)
    frames = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device=dev)
    out = {"views": V, "hw": [H, W], "runs": args.runs, "fuse": []}
    first = None
    for R in args.res:
        axes = mesh.lattice([-1.0] * 3, [1.0] * 3, R)
        trunc = 3.0 * float(axes[0][1] - axes[0][0])
        a = (packed, poses[:V].contiguous(), intr, H, W, axes, trunc)
        row = {"res": R, "pairs": R ** 3 * V}
        for cull in (1, 0):
            os.environ["LAE_TSDF_CULL"] = str(cull)
            row[f"fuse_ms_cull{cull}"] = round(_times(lambda: tsdf_fuse(*a), args.runs), 3)
            row[f"fuse_frames_ms_cull{cull}"] = round(_times(lambda: tsdf_fuse(*a, frames=frames), args.runs), 3)
        os.environ.pop("LAE_TSDF_CULL")
        row["floor_ms"] = round(R ** 3 * 4 / HBM * 1e3, 4)
        row["floor_frames_ms"] = round(R ** 3 * (4 + 8 + 12) / HBM * 1e3, 4)
        g = tsdf_fuse(*a, frames=frames)
        if not args.no_torch:
            torch_fuse(*a)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tu, tc = torch_fuse(*a)
            torch.cuda.synchronize()
            row["torch_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["differ"] = int((tc != g["counts"].reshape(-1, 4)[:, :3].to(torch.int32)).any(1).sum())
            del tu, tc
        out["fuse"].append(row)
        if first is None:
            first = (R, g)
    R, g = first
    near = torch.from_numpy(S.lookat_poses(V, radius=1.5, seed=0)).to(dev)
    axes = mesh.lattice([-1.0] * 3, [1.0] * 3, R)
    a = (sphere_views(near, intr, H, W), near, intr, H, W, axes, 3.0 * float(axes[0][1] - axes[0][0]))
    out["close"] = {"res": R, "radius": 1.5}
    for cull in (1, 0):
        os.environ["LAE_TSDF_CULL"] = str(cull)
        out["close"][f"fuse_ms_cull{cull}"] = round(_times(lambda: tsdf_fuse(*a), args.runs), 3)
    os.environ.pop("LAE_TSDF_CULL")
    del a
    verts, tris = mesh.marching_cubes(g["u"], 0.0)
    out["vertex_colors"] = {"res": R, "vertices": int(verts.shape[0]), "triangles": int(tris.shape[0]),
                            "us": round(_times(lambda: tsdf_vertex_colors(g["rgb"], g["counts"], verts), args.runs) * 1e3, 1)}
    del g, first, packed, frames
    # end to end on a renderer
    from mask_lift_bench import make_renderer
    from laenerf_amd.tsdf import render_packed_views
    r = make_renderer(dev)
    ev = args.e2e_views
    sigma = getattr(r.model, "density_sigma", None) or (lambda x: r.model.density(x)["sigma"])

    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return sigma(pts)
    aabb = r.aabb_infer.cpu()
    with torch.no_grad():
        thr = float(mesh.extract_fields(aabb[:3], aabb[3:], 256, query, device=dev).view(-1)[::97].quantile(0.99))
    with tempfile.TemporaryDirectory() as tmp:
        def wall(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return round((time.perf_counter() - t0) * 1e3, 1)
        e2e = {"res": 256, "views": ev, "threshold": thr,
               "render_ms": wall(lambda: render_packed_views(r, poses[:ev], intr, H, W, return_frames=True)),
               "save_mesh_tsdf_ms": wall(lambda: r.save_mesh_tsdf(os.path.join(tmp, "t.ply"), poses[:ev], intr, H, W, resolution=256)),
               "save_mesh_ms": wall(lambda: r.save_mesh(os.path.join(tmp, "d.ply"), resolution=256, threshold=thr, normals=True, colors=True))}
        e2e["tsdf_ply_bytes"], e2e["density_ply_bytes"] = os.path.getsize(os.path.join(tmp, "t.ply")), os.path.getsize(os.path.join(tmp, "d.ply"))
    out["e2e"] = e2e
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
