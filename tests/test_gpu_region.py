"""-m gpu: the region transform on the device (csrc/region.hip, laenerf_amd/editing/region_transform.py).  The kernels equal
their numpy restatements bit for bit; deleting is exact end to end; a transformed render equals the render of the analytically
transformed scene within the spread of two legitimate discretisations of that scene; baking moves the object in the NeRF."""
import functools
import importlib

import numpy as np
import pytest
import torch

import region_util as U
from gpu_util import DEV, N, T
from laenerf_amd.editing import region_transform as RT
from laenerf_amd.editing.region_transform import RegionTransform, region_occupancy, region_occupancy_numpy, region_warp, region_warp_numpy

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits32(a):
    return np.ascontiguousarray(N(a) if torch.is_tensor(a) else a, dtype=F32).view(np.uint32)


def rows(rng, rt, n):
    """sample rows that meet every branch: uniform in the box, images of selected cells, rows of zeros, rows with dirs zero"""
    x = np.concatenate([rng.uniform(-rt.bound, rt.bound, (n, 3)).astype(F32), U.image_points(rng, rt, n)])
    x = x[rng.permutation(len(x))][:n]
    d = rng.standard_normal(x.shape).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x[3::17] = 0.0
    d[3::17] = 0.0
    d[5::19] = 0.0
    return x, d


def check_warp(rt, x, d):
    want = region_warp_numpy(rt, x, d, dtype=F32)
    for M in (1, 63, 64, 65, 4097):
        xs, ds = T(x[:M]), T(d[:M])
        xo, do, sc = region_warp(rt, xs, ds)
        again = region_warp(rt, xs, ds)
        assert xo.data_ptr() != xs.data_ptr() and torch.equal(xs, T(x[:M])) and torch.equal(ds, T(d[:M]))     # out of place: inputs untouched
        xi, di = xs.clone(), ds.clone()
        xi2, di2, sci = region_warp(rt, xi, di, inplace=True)
        assert xi2.data_ptr() == xi.data_ptr() and di2.data_ptr() == di.data_ptr()
        # rows that start 12 bytes into an allocation: the path without 16-byte loads
        pad_x, pad_d = T(np.concatenate([x[:1], x[:M]])), T(np.concatenate([d[:1], d[:M]]))
        xu, du, scu = region_warp(rt, pad_x[1:], pad_d[1:])
        for got in ((xo, do, sc), again, (xi, di, sci), (xu, du, scu)):
            assert np.array_equal(bits32(got[0]), bits32(want["xyzs"][:M])), M
            assert np.array_equal(bits32(got[1]), bits32(want["dirs"][:M])), M
            assert np.array_equal(bits32(got[2]), bits32(want["sigma_scale"][:M])), M
        assert np.isfinite(N(xo)).all() and np.isfinite(N(sc)).all()
    return want


CASES = [(1, "move", 1.0, "general"), (1, "copy", 0.5, "rot90"), (1, "delete", 2.0, "general"), (2, "move", 2.0, "rot90"),
         (2, "copy", 1.0, "general"), (2, "delete", 0.5, "rot90"), (2, "move", 0.5, "general"), (1, "move", 2.0, "general")]


@pytest.mark.parametrize("C,mode,scale,rot", CASES)
def test_kernels_equal_the_restatements_bit_for_bit(C, mode, scale, rot):
    H = 128
    rng = np.random.default_rng(100 + CASES.index((C, mode, scale, rot)))
    occ, sel = U.random_scene(rng, C, H, fill=0.002)
    rt = U.random_transform(rng, sel, H, mode, scale=scale, rotation=U.ROT90 if rot == "rot90" else None, shift=0.3)
    x, d = rows(rng, rt, 4097)
    want = check_warp(rt, x, d)
    seen = set(want["branch"].tolist())
    assert seen == {"move": {0, 1, 2}, "copy": {0, 2}, "delete": {1, 2}}[mode]
    comp = region_occupancy(rt, T(occ))
    comp2 = region_occupancy(rt, T(occ), out=torch.full_like(comp, 0xA5))
    ref = region_occupancy_numpy(rt, occ, dtype=F32)
    assert np.array_equal(N(comp), ref) and torch.equal(comp, comp2)
    assert not np.array_equal(ref, occ)


@pytest.mark.parametrize("mode", ["move", "copy"])
def test_the_device_bitfield_covers_the_rows_the_warp_moves(mode):
    """an independent check of the KERNEL's bitfield on the production grid (the float32 restatement shares its algorithm): every
    row region_warp_numpy moves finds its bit at every cascade the marcher may probe it at, and no kept row loses one"""
    C, H = 2, 128
    rng = np.random.default_rng(31 + len(mode))
    occ, sel = U.random_scene(rng, C, H, fill=0.002)
    rt = U.random_transform(rng, sel, H, mode, shift=0.3)
    x = np.concatenate([rng.uniform(-rt.bound, rt.bound, (40000, 3)).astype(F32), U.image_points(rng, rt, 40000)])
    w = region_warp_numpy(rt, x, np.ones_like(x), dtype=F32)
    comp, occ_b = RT.unpack_bits(N(region_occupancy(rt, T(occ)))), RT.unpack_bits(occ)
    own = RT.cell_index_numpy(x, C, H, F32)[1]
    moved, kept = w["branch"] == RT.MOVED, w["branch"] == RT.KEPT
    assert moved.sum() > 10000 and kept.sum() > 10000
    for level in range(C):
        idx = U.cell_at_level(x, level, H)
        at = level >= own
        assert comp[idx[moved & at]].all(), level
        assert comp[idx[kept & at & occ_b[idx]]].all(), level
    assert comp.mean() < 0.2                                             # and it is no bitfield of ones


def test_the_warp_writes_into_buffers_of_the_callers():
    H = 32
    rng = np.random.default_rng(12)
    occ, sel = U.random_scene(rng, 1, H)
    rt = U.random_transform(rng, sel, H, "move")
    x, d = rows(rng, rt, 1000)
    xs, ds = T(x), T(d)
    want = region_warp(rt, xs, ds)
    bufs = (torch.empty_like(xs), torch.empty_like(ds), torch.empty(1000, device=DEV))
    got = region_warp(rt, xs, ds, out=bufs)
    assert all(g.data_ptr() == b.data_ptr() for g, b in zip(got, bufs))
    sc = torch.empty(1000, device=DEV)
    inp = region_warp(rt, xs.clone(), ds.clone(), inplace=True, out=sc)
    assert inp[2].data_ptr() == sc.data_ptr()
    for a, b, c in zip(want, got, inp):
        assert np.array_equal(bits32(a), bits32(b)) and np.array_equal(bits32(a), bits32(c))
    with pytest.raises(ValueError, match="region_warp"):
        region_warp(rt, xs, ds, out=(bufs[0], bufs[1], sc[:10]))


@pytest.mark.parametrize("mode", ["move", "copy", "delete"])
def test_empty_and_full_selections(mode):
    H = 32
    rng = np.random.default_rng(4)
    for C in (1, 2):
        occ, _ = U.random_scene(rng, C, H)
        for sel in (np.zeros_like(occ), np.full_like(occ, 0xFF)):
            rt = RegionTransform(sel, rotation=U.rot_z(20.0), translation=[0.1, -0.05, 0.2], scale=1.25, pivot=[0.0, 0.0, 0.0], mode=mode,
                                 grid_size=H)
            x, d = rows(rng, rt, 4097)
            check_warp(rt, x, d)
            for o in (occ, np.full_like(occ, 0xFF)):
                assert np.array_equal(N(region_occupancy(rt, T(o))), region_occupancy_numpy(rt, o, dtype=F32))
            if not sel.any():
                assert np.array_equal(N(region_occupancy(rt, T(occ))), occ)


def test_the_warp_replays_from_a_graph():
    H = 128
    rng = np.random.default_rng(8)
    occ, sel = U.random_scene(rng, 2, H, fill=0.002)
    rt = U.random_transform(rng, sel, H, "move", shift=0.3)
    x, d = rows(rng, rt, 4097)
    xs, ds = T(x), T(d)
    eager = region_warp(rt, xs, ds)
    rt.sel_on(xs.device)
    bx, bd = xs.clone(), ds.clone()
    region_warp(rt, bx, bd, inplace=True)                                 # warm-up
    bx.copy_(xs); bd.copy_(ds)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, _, sc = region_warp(rt, bx, bd, inplace=True)
    bx.copy_(xs); bd.copy_(ds); sc.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (bx, bd, sc)):
        assert np.array_equal(bits32(a), bits32(b))


def test_the_wrappers_refuse_bad_arguments():
    H = 32
    rng = np.random.default_rng(2)
    occ, sel = U.random_scene(rng, 1, H)
    rt = U.random_transform(rng, sel, H, "move")
    x = torch.zeros(8, 3, device=DEV)
    for bad in ((x.double(), x), (x, x[:4]), (x[:, :2], x), (x.t().contiguous().t(), x)):
        with pytest.raises(ValueError, match="region_warp"):
            region_warp(rt, *bad)
    o = T(occ)
    for bad in (dict(occ=o[:-1]), dict(occ=o.float()), dict(occ=o, out=o), dict(occ=o, out=o[:-1].clone())):
        with pytest.raises(ValueError, match="region_occupancy"):
            region_occupancy(rt, **bad)
    with pytest.raises(RuntimeError):
        region_warp(rt, x.cpu(), x.cpu())


# ---------------------------------------------------------------- an analytic scene: smooth blobs
G = 128
CELL = 2.0 / G
WIDTH = 1.5 * CELL                 # the sigmoid's width: a few cells from full density to none
MARGIN = 12 * CELL                 # occupancy and selection reach this far beyond a blob's radius: 8 widths, sigmoid(-8) = 3e-4
SIGMA0 = 60.0
FREQ = 9.0                         # colour frequency in object-local coordinates
A_C, A_R = np.array([-0.45, 0.05, -0.1]), 0.1         # the selected blob
B_C, B_R = np.array([0.6, -0.55, 0.5]), 0.12


class Blobs(torch.nn.Module):
    """model(xyzs, dirs) -> (sigmas [M], rgbs [M, 3]).  A blob: centre c, radius r, object-to-world rotation R and scale s; in its
    local frame p = R^T (x - c) / s the density is SIGMA0 sigmoid((r - |p|) / WIDTH) / s (the rule's density of a scaled object) and
    the colour 0.5 + 0.25 sin(FREQ p + phase) + 0.2 R^T d: a function of the object-local position plus a view-dependent term that
    turns with the object (rot_dir=False feeds it the world direction instead)."""

    def __init__(self, blobs):
        super().__init__()
        self.blobs = [dict(c=T(np.asarray(b["c"], F32)), r=float(b["r"]), Rt=T(np.asarray(b.get("R", np.eye(3)), F32).T.copy()),
                           s=float(b.get("s", 1.0)), phase=float(b["phase"]), rot_dir=b.get("rot_dir", True)) for b in blobs]

    def forward(self, x, d):
        x, d = x.float(), d.float()
        sig, col = [], []
        for b in self.blobs:
            p = ((x - b["c"]) @ b["Rt"].T) / b["s"]
            sig.append(SIGMA0 * torch.sigmoid((b["r"] - p.norm(dim=-1)) / WIDTH) / b["s"])
            dl = d @ b["Rt"].T if b["rot_dir"] else d
            col.append((0.5 + 0.25 * torch.sin(FREQ * p + b["phase"]) + 0.2 * dl).clamp(0, 1))
        sig = torch.stack(sig)
        total = sig.sum(0)
        w = sig / total.clamp(min=1e-30)
        return total, (w[..., None] * torch.stack(col)).sum(0)


@functools.lru_cache(None)
def cell_centres():
    return U.centres(1, G)[0]


def ball_bits(c, r):
    """the analytic occupancy of a blob: cells whose centre lies within r of c -> bool [G^3]"""
    return ((cell_centres() - np.asarray(c)) ** 2).sum(-1) < r * r


def dilate(bits):
    """one cell in each direction (the 3 x 3 x 3 neighbourhood) of a bool [G^3] set in the bitfield's order"""
    co = U.coords(G)
    g = np.zeros((G, G, G), bool)
    g[co[:, 0], co[:, 1], co[:, 2]] = bits
    pad = np.pad(g, 1)
    out = np.zeros_like(g)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out |= pad[a:a + G, b:b + G, c:c + G]
    return out[co[:, 0], co[:, 1], co[:, 2]]


def renderer_of(model, bits):
    from laenerf_amd.renderer import NeRFRenderer
    r = NeRFRenderer(model, bound=1, min_near=0.2).to(DEV)
    r.density_bitfield = T(U.pack(bits))
    r.eval()
    return r


@functools.lru_cache(None)
def camera_rays():
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    ray = get_rays(T(S.lookat_poses(2, radius=3.2, seed=6)), (89.0, 89.0, 32.0, 32.0), 64, 64)
    return ray["rays_o"].reshape(-1, 3).contiguous(), ray["rays_d"].reshape(-1, 3).contiguous()


def render(r, dens_grid=None):
    o, d = camera_rays()
    res = r.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False, dens_grid=dens_grid)
    return torch.cat([res["image"], res["weights_sum"][:, None]], 1).double()


def scene_S():
    A, B = dict(c=A_C, r=A_R, phase=0.3), dict(c=B_C, r=B_R, phase=1.7)
    occ = ball_bits(A_C, A_R + MARGIN) | ball_bits(B_C, B_R + MARGIN)
    sel = ball_bits(A_C, A_R + MARGIN)
    return A, B, occ, sel


def test_delete_is_exact_end_to_end():
    from laenerf_amd.editing import render_transformed
    A, B, occ, sel = scene_S()
    r = renderer_of(Blobs([A, B]), occ)
    rt = RegionTransform(U.pack(sel), rotation=U.rot_z(30.0), translation=[0.1, 0.2, 0.0], mode="delete")
    o, d = camera_rays()
    got = render_transformed(r, rt, o, d, bg_color=1, perturb=False)
    want = r.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False, dens_grid=T(U.pack(occ & ~sel)))
    plain = r.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(bits32(got[k]), bits32(want[k])), k
        assert not np.array_equal(bits32(got[k]), bits32(plain[k])), k
    tiled = render_transformed(r, rt, o[:4096], d[:4096], bg_color=1, perturb=False, image_hw=(64, 64))
    ref = r.render_eval(o[:4096], d[:4096], bg_color=1, perturb=False, frame_loop=False, dens_grid=T(U.pack(occ & ~sel)), image_hw=(64, 64))
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(bits32(tiled[k]), bits32(ref[k])), k


# (rotation in degrees about z through the blob's centre, translation, scale)
TRANSFORMS = {"rotate": (30.0, (0.1, 0.35, -0.2), 1.0), "shrink": (0.0, (0.1, 0.4, -0.25), 0.5), "grow": (0.0, (0.15, 0.3, -0.2), 2.0)}


def placed(A, rot_deg, t, s, **kw):
    return dict(A, c=A_C + np.asarray(t), R=U.rot_z(rot_deg), s=s, **kw)


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_a_transformed_render_equals_the_render_of_the_transformed_scene(name):
    """The yardstick is built here, from paths older than the feature: D0 = max |render_eval(S_T, its tight analytic occupancy) -
    render_eval(S_T, that occupancy dilated by one cell)| over image and opacity, the spread between two legitimate
    discretisations of one scene.  The feature's composed bitfield is such a dilation; its image boxes may spill one cell beyond a
    one-cell dilation, hence 2 D0."""
    from laenerf_amd.editing import render_transformed
    rot, t, s = TRANSFORMS[name]
    A, B, occ, sel = scene_S()
    A_T = placed(A, rot, t, s)
    tight = ball_bits(A_T["c"], s * (A_R + MARGIN)) | ball_bits(B_C, B_R + MARGIN)
    r_T = renderer_of(Blobs([A_T, B]), tight)
    base = render(r_T)
    D0 = float((base - render(r_T, T(U.pack(dilate(tight))))).abs().max())
    r_S = renderer_of(Blobs([A, B]), occ)
    rt = RegionTransform(U.pack(sel), rotation=U.rot_z(rot), translation=t, scale=s, pivot=A_C, mode="move")
    o, d = camera_rays()
    res = render_transformed(r_S, rt, o, d, bg_color=1, perturb=False)
    got = torch.cat([res["image"], res["weights_sum"][:, None]], 1).double()
    err = float((got - base).abs().max())
    plain = float((render(r_S) - base).abs().max())
    unrot = float((render(renderer_of(Blobs([placed(A, rot, t, s, rot_dir=False), B]), tight)) - base).abs().max())
    print(f"region equivalence [{name}]: D0 {D0:.3e}  |transformed - S_T| {err:.3e}  |plain S - S_T| {plain:.3e}  |unrotated dirs - S_T| {unrot:.3e}")
    assert D0 > 0
    assert err <= 2 * D0
    assert plain > 10 * D0                       # power: the untransformed scene is far outside the bound
    if rot:
        assert unrot > 2 * D0                    # power: a view-dependent term fed the unrotated direction is outside it too


# copy keeps the source, and the moved object is pasted over whatever its selection covers: the translation takes the image's
# selection clear of the source's (|t| = 0.66 > 2 (A_R + MARGIN) = 0.575), or the paste would eat the source's soft edge
COPY_TRANSFORM = (30.0, (0.2, 0.55, -0.3), 1.0)


def test_copy_mode_shows_the_object_twice():
    from laenerf_amd.editing import render_transformed
    rot, t, s = COPY_TRANSFORM
    A, B, occ, sel = scene_S()
    A_T = placed(A, rot, t, s)
    img_bits = ball_bits(A_T["c"], s * (A_R + MARGIN))
    tight = img_bits | ball_bits(B_C, B_R + MARGIN)
    r_T = renderer_of(Blobs([A_T, B]), tight)
    moved = render(r_T)
    D0 = float((moved - render(r_T, T(U.pack(dilate(tight))))).abs().max())
    r_S = renderer_of(Blobs([A, B]), occ)
    plain = render(r_S)
    rt = RegionTransform(U.pack(sel), rotation=U.rot_z(rot), translation=t, scale=s, pivot=A_C, mode="copy")
    o, d = camera_rays()
    res = render_transformed(r_S, rt, o, d, bg_color=1, perturb=False)
    got = torch.cat([res["image"], res["weights_sum"][:, None]], 1).double()
    # where each copy of the blob shows: the opacity of the blob alone, from its own occupancy
    src_px = render(renderer_of(Blobs([A]), sel))[:, 3] > 1e-3
    img_px = render(renderer_of(Blobs([A_T]), img_bits))[:, 3] > 1e-3
    assert int((img_px & ~src_px).sum()) >= 50 and int((src_px & ~img_px).sum()) >= 50
    e_img = float((got - moved)[~src_px].abs().max())            # off the source: the scene with the blob at its new place
    e_src = float((got - plain)[~img_px].abs().max())            # off the image: the scene as it was
    print(f"region copy: D0 {D0:.3e}  image region {e_img:.3e}  source region {e_src:.3e}")
    assert e_img <= 2 * D0 and e_src <= 2 * D0
    assert float((got - moved)[src_px & ~img_px].abs().max()) > 10 * D0 and float((got - plain)[img_px & ~src_px].abs().max()) > 10 * D0


def test_transform_views_gives_what_the_exports_take():
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import transform_views
    A, B, occ, sel = scene_S()
    r = renderer_of(Blobs([A, B]), occ)
    rt = RegionTransform(U.pack(sel), translation=[0.1, 0.35, -0.2], pivot=A_C)
    poses = T(S.lookat_poses(2, radius=3.2, seed=6))
    frames, depths, opac = transform_views(r, rt, poses, (89.0, 89.0, 32.0, 32.0), 64, 64)
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == torch.uint8 and depths.shape == opac.shape == (2, 64 * 64)
    assert depths.dtype == opac.dtype == torch.float32 and float(opac.max()) > 0.9 and bool(torch.isfinite(depths).all())
    m = r.extract_mesh_tsdf(poses, (89.0, 89.0, 32.0, 32.0), 64, 64, resolution=32, frames=frames, depths=depths, opacities=opac)
    assert m["vertices"].shape[0] > 0


# ---------------------------------------------------------------- baking
# The teacher is analytic too (the random-field teacher of tools/train_loop.py is translucent everywhere: its largest opacity at
# 64 x 64 is 0.75, and the conditions below ask for 0.9): two opaque blobs large enough to cover 50 pixels of a 64 x 64 view.  The
# translation (|t| = 0.68) takes the moved blob clear of its old place (2 (radius + a soft edge) = 0.6).
BAKE_A = dict(c=np.array([-0.4, 0.1, -0.1]), r=0.22, phase=0.3)
BAKE_B = dict(c=np.array([0.45, -0.3, 0.3]), r=0.25, phase=1.7)
BAKE_T = (0.2, 0.35, 0.55)


def analytic_training_views(n, Hh, Ww):
    """n views of the two blobs as teacher_views makes them: uint8 RGBA (straight colour, alpha = opacity), poses, intrinsics"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    occ = ball_bits(BAKE_A["c"], BAKE_A["r"] + MARGIN) | ball_bits(BAKE_B["c"], BAKE_B["r"] + MARGIN)
    r = renderer_of(Blobs([BAKE_A, BAKE_B]), occ)
    poses = S.lookat_poses(n, radius=3.2, seed=0)
    focal = 0.5 * Ww / np.tan(0.5 * 0.69)
    intr = (focal, focal, Ww / 2, Hh / 2)
    ray = get_rays(T(poses), intr, Hh, Ww)
    res = r.render_eval(ray["rays_o"].reshape(-1, 3), ray["rays_d"].reshape(-1, 3), bg_color=0, perturb=False, frame_loop=False)
    ws = res["weights_sum"].clamp(0, 1)
    rgb = torch.where(ws[:, None] > 0, res["image"] / ws.clamp(min=1e-6)[:, None], torch.zeros_like(res["image"])).clamp(0, 1)
    rgba = torch.cat([rgb, ws[:, None]], 1).reshape(n, Hh, Ww, 4)
    return (rgba * 255 + 0.5).to(torch.uint8).cpu().numpy(), poses, intr


@pytest.mark.parametrize("seed_occupancy", [True])
def test_baking_moves_the_object_in_the_nerf(seed_occupancy):
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import bake_region_transform, render_transformed
    from laenerf_amd.rays import get_rays
    tl = importlib.import_module("tools.train_loop")
    dev = torch.device(DEV)
    Hh = Ww = 64
    images, poses, intr = analytic_training_views(24, Hh, Ww)
    tr = tl.make_trainer(dev, images, poses, intr, iters=512)
    tr.train(512)
    r, data = tr.r, tr.data
    # the selection: what the student holds occupied around blob A
    edit = r.density_bitfield & T(U.pack(ball_bits(BAKE_A["c"], BAKE_A["r"] + 6 * CELL)))
    rt = RegionTransform(edit, translation=BAKE_T, mode="move")
    assert int(RT.unpack_bits(N(edit)).sum()) > 500

    def views(pose):
        ray = get_rays(T(pose[None]), intr, Hh, Ww)
        o, d = ray["rays_o"][0], ray["rays_d"][0]
        r.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            plain = r.render_eval(o, d, bg_color=1.0, perturb=False, image_hw=(Hh, Ww))
            target = render_transformed(r, rt, o, d, bg_color=1.0, perturb=False, image_hw=(Hh, Ww))
        r.train()
        return {k: (plain[k].float(), target[k].float()) for k in ("image", "weights_sum")}

    # held-out poses (another seed than the training poses'); the one whose two regions are largest
    best = None
    for pose in S.lookat_poses(6, radius=3.2, seed=77):
        v = views(pose)
        (po, to) = v["weights_sum"]
        new_px, old_px = (to > 0.9) & (po < 0.1), (po > 0.9) & (to < 0.1)
        score = min(int(new_px.sum()), int(old_px.sum()))
        if best is None or score > best[0]:
            best = (score, pose, v, new_px, old_px)
    score, pose, before, new_px, old_px = best
    psnr = lambda a, b: float(-10 * torch.log10(((a - b) ** 2).mean()))
    psnr_before = psnr(*before["image"])
    assert int(new_px.sum()) >= 50 and int(old_px.sum()) >= 50, (int(new_px.sum()), int(old_px.sum()))
    data_new, tr2 = bake_region_transform(r, tr.opt, data, rt, steps=384, lr=1e-2, seed=seed_occupancy)
    assert data_new is not data and data_new.images.shape == (24, Hh, Ww, 4) and np.isfinite(tr2.losses()).all()
    after = views(pose)
    student_img, student_op = after["image"][0], after["weights_sum"][0]
    psnr_after = psnr(student_img, before["image"][1])
    op_new, op_old = float(student_op[new_px].mean()), float(student_op[old_px].mean())
    print(f"region bake (seeding {seed_occupancy}): held-out PSNR vs the transformed render {psnr_before:.2f} -> {psnr_after:.2f} dB; student "
          f"opacity at the new place {op_new:.3f} ({int(new_px.sum())} px), at the old place {op_old:.3f} ({int(old_px.sum())} px)")
    assert psnr_after > psnr_before
    assert op_new > 0.5                          # the condition the occupancy seeding is there for
    assert op_old < 0.5
