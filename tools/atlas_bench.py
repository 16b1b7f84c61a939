"""Time and fidelity of the textured mesh export (lae_atlas_texels / lae_atlas_fuse_views / lae_atlas_pack,
NeRFRenderer.save_mesh_textured).

    python tools/atlas_bench.py [--res 256] [--views 100] [--hw 800] [--cell 8] [--runs 5] [--calls 200] [--e2e-views 100]

The geometry is the marching-cubes mesh of tools/tsdf_bench.py's fused analytic sphere (radius 0.6 in [-1, 1]^3, `lookat_poses`
cameras at radius 3.2, focal 1111 at 800 pixels).  The frames show a pattern over the sphere, 0.5 + 0.4 sin(2 pi X / period) per
axis, whose period (1.6 lattice cells) lies above four image pixels and below two lattice cells.  Prints one JSON line:
  mesh        vertices, triangles, the layout (cell, S, texels)
  texels_us / pack_us / fuse_ms_cull1 / fuse_ms_cull0     per call of the Python operator (atlas_texels
              includes its index range check's host read): the median of --runs runs of --calls calls between two events
  fuse_torch_ms   the same fuse rule written view by view in torch operators on the device, one run after a warm-up, in this
              process; fuse_differ: the texels whose counts differ between the two
  fuse_floor_ms   the fuse's output bytes (rgb) at 6.3 TB/s
  error       per min_cos in (0, 0.25, 0.5): RMS error of the baked texture against the pattern at 100 000 random surface points,
              the share of grey texels and the mean number of views per texel; vertex_rms: the same error for lae_tsdf_fuse's
              vertex colours interpolated over the triangles
  e2e         on the synthetic renderer of tools/mask_lift_bench.py at R = --res: save_mesh_textured(source="views",
              geometry="tsdf") wall-clock ms, and its parts measured on their own -- render_ms (the views), bake_ms (texels + fuse +
              pack), obj_text_ms, png_ms -- beside save_mesh_tsdf on the same inputs"""
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
MIN_COS = (0.0, 0.25, 0.5)


def _per_call(fn, runs, calls):
    """ms per call: the median over `runs` of (`calls` calls between two events) / calls"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return float(np.median(out))


def pattern(X, period):
    X = X * (RADIUS / X.norm(dim=-1, keepdim=True))
    return 0.5 + 0.4 * torch.sin(2.0 * np.pi * X / period)


@torch.no_grad()
def pattern_views(poses, intr, H, W, period):
    """-> (packed [V, H, W]: the analytic sphere's distance per pixel, +inf where the ray misses; frames uint8 [V, H, W, 3])"""
    from laenerf_amd.rays import get_rays
    V = poses.shape[0]
    packed = torch.empty(V, H, W, device=poses.device)
    frames = torch.empty(V, H, W, 3, dtype=torch.uint8, device=poses.device)
    for v in range(V):
        ray = get_rays(poses[v:v + 1], intr, H, W)
        o, d = ray["rays_o"][0].reshape(-1, 3), ray["rays_d"][0].reshape(-1, 3)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - RADIUS * RADIUS)
        t = -b - disc.clamp_min(0).sqrt()
        hit = (disc > 0) & (t > 0)
        packed[v] = torch.where(hit, t, torch.full_like(t, float("inf"))).reshape(H, W)
        X = o + t[:, None] * d
        rgb = torch.where(hit[:, None], pattern(torch.where(hit[:, None], X, torch.ones_like(X)), period), torch.ones_like(X))
        frames[v] = (rgb.clamp(0, 1) * 255).to(torch.uint8).reshape(H, W, 3)
    return packed, frames


@torch.no_grad()
def torch_fuse(packed, poses, intr, H, W, frames, pos, nrm, owner, trunc, min_cos):
    """lae_atlas_fuse_views' rule with torch operators, view by view -> (rgb, counts int32)"""
    fx, fy, cx, cy = intr
    n = pos.shape[0]
    cnt = torch.zeros(n, dtype=torch.int32, device=pos.device)
    sums = torch.zeros(n, 3, dtype=torch.int32, device=pos.device)
    live = owner >= 0
    for v in range(packed.shape[0]):
        d = pos - poses[v, :3, 3]
        q = d @ poses[v, :3, :3]
        front = q[:, 2] > 0
        z = torch.where(front, q[:, 2], torch.ones_like(q[:, 2]))
        pu, pv = fx * q[:, 0] / z + cx, fy * q[:, 1] / z + cy
        inside = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
        pix = pv.clamp(0, H - 1).long() * W + pu.clamp(0, W - 1).long()
        ts = packed[v].reshape(-1)[pix].abs()
        t = d.norm(dim=-1)
        take = live & inside & ((ts - t).abs() <= trunc) & (-(nrm * d).sum(-1) / t > min_cos)
        cnt += take
        sums += torch.where(take[:, None], frames[v].reshape(-1, 3)[pix].to(torch.int32), torch.zeros_like(sums))
    rgb = torch.where((cnt > 0)[:, None], sums.float() / cnt.clamp_min(1).float()[:, None] / 255.0, torch.full_like(pos, 0.5))
    return torch.where(live[:, None], rgb, torch.zeros_like(rgb)), cnt


def sample_texture(texture, uv):
    """sample_texture_numpy in torch: texture uint8 [S, S, 3] on the device, uv float64 [n, 2] -> [n, 3] float64"""
    S = texture.shape[0]
    tex = texture.double() / 255.0
    x, y = uv[:, 0] * S - 0.5, (1.0 - uv[:, 1]) * S - 0.5
    x0, y0 = x.floor(), y.floor()
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    X0, X1, Y0, Y1 = (c.clamp(0, S - 1).long() for c in (x0, x0 + 1, y0, y0 + 1))
    return (tex[Y0, X0] * (1 - fx) + tex[Y0, X1] * fx) * (1 - fy) + (tex[Y1, X0] * (1 - fx) + tex[Y1, X1] * fx) * fy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--cell", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--e2e-views", type=int, default=100)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from laenerf_amd import atlas as A
    from laenerf_amd import mesh
    from laenerf_amd import synthetic as S
    from laenerf_amd.tsdf import tsdf_fuse, tsdf_vertex_colors
    H = W = args.hw
    focal = 1111.1 * W / 800
    intr = (focal, focal, W / 2, H / 2)
    V, R = args.views, args.res
    poses = torch.from_numpy(S.lookat_poses(max(V, args.e2e_views), radius=3.2, seed=0)).to(dev)
    pv = poses[:V].contiguous()
    axes = mesh.lattice([-1.0] * 3, [1.0] * 3, R)
    step = float(axes[0][1] - axes[0][0])
    trunc, period = 3.0 * step, 1.6 * step
    packed, frames = pattern_views(pv, intr, H, W, period)
    g = tsdf_fuse(packed, pv, intr, H, W, axes, trunc, frames=frames)
    iv, tris = mesh.marching_cubes(g["u"], 0.0)
    attrs = mesh.vertex_attributes(g["u"], iv, [-1.0] * 3, [1.0] * 3, want=("pos", "normals"))
    verts, normals = attrs["pos"], attrs["normals"]
    vcol, _ = tsdf_vertex_colors(g["rgb"], g["counts"], iv)
    del g
    tx = A.atlas_texels(verts, tris, normals, cell=args.cell)
    lay = tx["layout"]
    out = {"views": V, "hw": [H, W], "res": R, "runs": args.runs, "calls": args.calls, "pixel_world": round(2.6 / focal, 5), "period": round(period, 5),
           "mesh": {"vertices": int(verts.shape[0]), "triangles": int(tris.shape[0]), "cell": lay.cell, "S": lay.S, "texels": lay.n_texels}}
    fa = (packed, pv, intr, H, W, frames, tx["pos"], tx["nrm"], tx["owner"], trunc)
    out["texels_us"] = round(_per_call(lambda: A.atlas_texels(verts, tris, normals, cell=args.cell), args.runs, args.calls) * 1e3, 1)
    for cull in (1, 0):
        os.environ["LAE_ATLAS_CULL"] = str(cull)
        out[f"fuse_ms_cull{cull}"] = round(_per_call(lambda: A.atlas_fuse_views(*fa, 0.25), args.runs, args.calls), 3)
    os.environ.pop("LAE_ATLAS_CULL")
    f = A.atlas_fuse_views(*fa, 0.25, counts=True)
    out["pack_us"] = round(_per_call(lambda: A.atlas_pack(f["rgb"], tx["owner"], lay), args.runs, args.calls) * 1e3, 1)
    out["fuse_floor_ms"] = round(lay.n_texels * 12 / HBM * 1e3, 4)
    ta = (packed, pv, intr, H, W, frames, tx["pos"], tx["nrm"], tx["owner"], trunc, 0.25)
    torch_fuse(*ta)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trgb, tcnt = torch_fuse(*ta)
    torch.cuda.synchronize()
    out["fuse_torch_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["fuse_differ"] = int((tcnt != f["counts"].to(torch.int32)).sum())
    del trgb, tcnt
    # fidelity: random surface points, triangles drawn by area
    p = verts.double()[tris.long()]
    area = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=-1)
    gen = torch.Generator(device=dev).manual_seed(0)
    cdf = torch.cumsum(area, 0)
    t = torch.searchsorted(cdf, torch.rand(args.points, dtype=torch.float64, device=dev, generator=gen) * cdf[-1]).clamp_max(len(area) - 1)
    r = torch.rand(args.points, 2, dtype=torch.float64, device=dev, generator=gen)
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    bary = torch.stack([1 - r.sum(1), r[:, 0], r[:, 1]], -1)
    X = (p[t] * bary[..., None]).sum(1)
    want = pattern(X, period)
    uv = (torch.from_numpy(A.atlas_uv(lay)).to(dev)[t] * bary[..., None]).sum(1)
    owned = tx["owner"] >= 0

    def rms(a):
        return round(float(((a - want) ** 2).mean().sqrt()), 5)
    out["error"] = {"points": args.points, "pattern_rms_about_mean": round(float(((want - want.mean(0)) ** 2).mean().sqrt()), 5),
                    "vertex_rms": rms((vcol.double()[tris.long()[t]] * bary[..., None]).sum(1)), "texture": []}
    for mc in MIN_COS:
        f = A.atlas_fuse_views(*fa, mc, counts=True)
        tex = A.atlas_pack(f["rgb"], tx["owner"], lay)
        out["error"]["texture"].append({"min_cos": mc, "rms": rms(sample_texture(tex, uv)), "grey_share": round(int(f["n_grey"]) / int(owned.sum()), 6),
                                        "views_per_texel": round(float(f["counts"].to(torch.int32)[owned].float().mean()), 2)})
    del f, tex, fa, ta, packed, frames, tx
    if not args.no_e2e:
        from mask_lift_bench import make_renderer
        from laenerf_amd.tsdf import render_packed_views
        rr = make_renderer(dev)
        ev = args.e2e_views
        pe = poses[:ev].contiguous()
        with tempfile.TemporaryDirectory() as tmp:
            def wall(fn):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                return round((time.perf_counter() - t0) * 1e3, 1), res
            kw = dict(resolution=R, cell=args.cell, source="views", geometry="tsdf", poses=pe, intrinsics=intr, H=H, W=W)
            e2e = {"res": R, "views": ev}
            e2e["render_ms"], (pk, fr) = wall(lambda: render_packed_views(rr, pe, intr, H, W, return_frames=True))
            e2e["save_mesh_textured_ms"], _ = wall(lambda: rr.save_mesh_textured(os.path.join(tmp, "t.obj"), **kw))
            e2e["save_mesh_tsdf_ms"], _ = wall(lambda: rr.save_mesh_tsdf(os.path.join(tmp, "t.ply"), pe, intr, H, W, resolution=R))
            m = rr.extract_mesh_textured(**kw)
            e2e["triangles"], e2e["S"] = int(m["triangles"].shape[0]), int(m["texture"].shape[0])
            if e2e["triangles"]:
                step_r = float((rr.aabb_infer[3] - rr.aabb_infer[0]) / (R - 1))

                def bake():
                    x = A.atlas_texels(m["vertices"], m["triangles"], m["normals"], cell=args.cell)
                    y = A.atlas_fuse_views(pk, pe, intr, H, W, fr, x["pos"], x["nrm"], x["owner"], 3.0 * step_r)
                    return A.atlas_pack(y["rgb"], x["owner"], x["layout"])
                e2e["bake_ms"] = round(_per_call(bake, args.runs, 20), 3)
                hv, ht, hn = (m[k].cpu().numpy() for k in ("vertices", "triangles", "normals"))
                huv, htex = m["uv"].cpu().numpy(), m["texture"].cpu().numpy()
                t0 = time.perf_counter()
                text = A.obj_text(hv, ht, huv, "t.mtl", hn)
                e2e["obj_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                t0 = time.perf_counter()
                png = A.png_bytes(htex)
                e2e["png_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                e2e["obj_bytes"], e2e["png_bytes"] = len(text), len(png)
                e2e["ply_bytes"] = os.path.getsize(os.path.join(tmp, "t.ply"))
        out["e2e"] = e2e
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
