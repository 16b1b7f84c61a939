"""Pose refinement on the GPU: lae_grid_input_grad, lae_pose_ray_grad and lae_pose_step against the float64 restatements of
laenerf_amd/poses.py, the Trainer's pose_refine path (bit-equalities), and a registration run on a smooth teacher."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, T
from laenerf_amd import poses as P

pytestmark = pytest.mark.gpu

BASE = 16


def _f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- kernel 1
@pytest.fixture(scope="module")
def grids():
    """level layouts -> (offsets int32, S float32, fp16 table): the shipped 16 levels (dense 0-4, hashed 5-15), the same with
    align_corners sizes, and two levels"""
    from oracle import oracle as O
    rng = np.random.default_rng(7)
    out = {}
    for name, kw in (("L16", {}), ("L16a", {"align_corners": True}), ("L2", {"num_levels": 2, "per_level_scale": 2.0})):
        if "num_levels" in kw:
            offsets, pls = O.grid_offsets(**kw)
        else:
            offsets, pls = O.grid_offsets(desired_resolution=2048, **kw)
        out[name] = (offsets, np.float32(np.log2(pls)), _f16(rng.uniform(-1, 1, (int(offsets[-1]), 2))))
    return out


def _edge_rows(in_map):
    """rows in the kernel's input space for x' = 0 and 1 exactly, x' = 1/2 (position 8 at level 0: an integer cell position), mixed
    faces, and three rows outside [0, 1]"""
    x01 = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0, 1, 0.5], [1, 0.5, 0], [0.5, 0.25, 0.75],
                    [1.001, 0.5, 0.5], [0.5, -0.25, 0.5], [0.2, 0.3, 1.5]], np.float32)
    x = x01 / np.float32(in_map[1]) - np.float32(in_map[0])
    back = (x + np.float32(in_map[0])) * np.float32(in_map[1])
    assert np.array_equal(back[:6], x01[:6])                                  # the map reproduces the exact values
    return x, 6


def _input_grad(x, table, offsets, g, S, L, gridtype, align, in_map):
    from laenerf_amd.backend import gridencoder_backend as G
    M = x.shape[0]
    out = torch.full((M, 3), float("nan"), dtype=torch.float32, device=DEV)
    G.grid_input_grad(T(x), T(table), T(offsets), T(g), out, M, 3, 2, L, float(S), BASE, gridtype, align, 0, in_map=in_map)
    return out


@pytest.mark.parametrize("layout,M,gridtype,in_map", [
    ("L16", 16, 0, (1.0, 0.5)), ("L16", 80, 0, (1.0, 0.5)), ("L16", 272, 0, (0.0, 1.0)), ("L16", 80, 1, (1.0, 0.5)),
    ("L16a", 80, 0, (0.0, 1.0)), ("L2", 80, 0, (1.0, 0.5)), ("L2", 16, 1, (0.0, 1.0))])
def test_grid_input_grad(grids, layout, M, gridtype, in_map):
    """against the float64 restatement on the same fp16 bits.  Per output: 8 L terms (128 at L = 16), each scale * (wa * wb) * ((vr -
    vl) * g) folded in with one fmaf -- the two 1 - frac, wa * wb, scale *, vr - vl, * g and the fmaf: at most 8 roundings of 2^-24
    each --, then the additions of the partial sums (the fmaf chain, the 7 wave sums) and the in_scale product: below 128 further
    roundings of at most 2^-24 A each.  |out - ref| <= (8 + 128) 2^-24 A < 2^-16 A, A the float64 sum of the terms' absolute values
    (the count holds whatever the order of the additions)."""
    offsets, S, table = grids[layout]
    L, align = offsets.shape[0] - 1, layout == "L16a"
    rng = np.random.default_rng(M + 7 * gridtype)
    lo, hi = (-1.0, 1.0) if in_map[0] else (0.0, 1.0)
    x = rng.uniform(lo, hi, (M, 3)).astype(np.float32)
    edge, n_in = _edge_rows(in_map)
    x[:edge.shape[0]] = edge
    g = _f16(rng.uniform(-1, 1, (L, M, 2)))
    got_t = _input_grad(x, table, offsets, g, S, L, gridtype, align, in_map)
    again = _input_grad(x, table, offsets, g, S, L, gridtype, align, in_map)
    assert torch.equal(got_t.view(torch.int32), again.view(torch.int32))      # bit-identical between two runs
    got = got_t.cpu().numpy().astype(np.float64)
    ref, A, _ = P.grid_input_grad_numpy(x, table, offsets, g, S, BASE, gridtype=gridtype, align_corners=align, in_map=in_map, full=True)
    err = np.abs(got - ref)
    print(f"{layout} M={M} gridtype={gridtype}: max err / (2^-16 A) = {(err / np.maximum(2.0 ** -16 * A, 1e-300)).max():.4f}")
    assert np.all(got[n_in:edge.shape[0]] == 0) and np.all(A[n_in:edge.shape[0]] == 0)      # outside [0, 1]: zeros
    assert np.all(A[:n_in] > 0)
    assert np.all(err <= 2.0 ** -16 * A)


def test_grid_input_grad_refusals(grids):
    from laenerf_amd import _lib
    lib = _lib.load()
    offsets, S, table = grids["L2"]
    x, tab, off = T(np.zeros((16, 3), np.float32)), T(table), T(offsets)
    g, out = T(np.zeros((2, 16, 2), np.float16)), torch.zeros(16, 3, device=DEV)
    ok = dict(M=16, D=3, C=2, L=2, gridtype=0, interp=0, dtype=1)

    def call(**kw):
        a = {**ok, **kw}
        return lib.lae_grid_input_grad(x.data_ptr(), tab.data_ptr(), off.data_ptr(), g.data_ptr(), out.data_ptr(), a["M"], a["D"], a["C"],
                                       a["L"], float(S), BASE, a["gridtype"], 0, a["interp"], a["dtype"], 0.0, 1.0,
                                       torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    for bad in (dict(D=2), dict(C=4), dict(C=1), dict(L=0), dict(L=33), dict(gridtype=2), dict(interp=1), dict(dtype=0)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- kernel 2
def test_pose_ray_grad():
    """|out - ref| <= 2^-40 A: every product and sum is fp64 (at most count + 70 roundings of 2^-53 each)"""
    from laenerf_amd.data import ResidentImages
    rng = np.random.default_rng(4)
    counts = [0, 1, 2, 63, 64, 65, 200]
    N, M = len(counts), sum(counts) + 3
    order = rng.permutation(N)
    rays = np.zeros((N, 3), np.int32)
    off = 0
    for row, c in enumerate(counts):
        rays[row] = (order[row], off, c)
        off += c
    x = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
    g = (rng.standard_normal((M, 3)) * 100).astype(np.float32)
    o = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    out = torch.full((N, 6), float("nan"), dtype=torch.float64, device=DEV)
    ResidentImages.pose_ray_grad(T(rays), T(x), T(g), T(o), out=out)
    again = ResidentImages.pose_ray_grad(T(rays), T(x), T(g), T(o))
    assert torch.equal(out.view(torch.int64), again.view(torch.int64))
    got = out.cpu().numpy()
    ref, A = P.pose_ray_grad_numpy(rays, x, g, o, full=True)
    assert np.all(got[order[0]] == 0)                                         # count 0 writes zeros
    assert np.all(np.abs(got - ref) <= 2.0 ** -40 * A)
    assert np.all(A[order[1:]] > 0)
    # a ray the march truncated (its samples do not fit into M) is dropped, as the compositing kernels drop it
    rays[-1, 2] = M - rays[-1, 1] + 1
    got = ResidentImages.pose_ray_grad(T(rays), T(x), T(g), T(o)).cpu().numpy()
    assert np.all(got[order[-1]] == 0) and np.array_equal(got[order[:-1]], out.cpu().numpy()[order[:-1]])


# ---------------------------------------------------------------------------------------------------------------- kernel 3
def _pose_data(n_img=5, H=8, W=8, seed=3):
    from laenerf_amd.data import ResidentImages
    rng = np.random.default_rng(seed)
    poses = np.zeros((n_img, 4, 4), np.float32)
    for i in range(n_img):
        poses[i, :3, :3] = P.exp_so3(rng.standard_normal(3))
        poses[i, :3, 3] = rng.uniform(-0.9, 0.9, 3)
    poses[0, 1, 3] = -0.0                                                     # a signed zero has to survive
    poses[:, 3, 3] = 1
    img = rng.integers(0, 256, (n_img, H, W, 3), dtype=np.uint8)
    return ResidentImages.from_arrays(img, poses, (10.0, 10.0, W / 2, H / 2), device=DEV), poses


def _words(skip=0, inv_scale=1.0):
    w = np.zeros(16, np.int32)
    w[3] = skip
    w[7] = np.float32(inv_scale).view(np.int32)
    return T(w)


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def test_pose_step():
    """two consecutive steps against pose_numpy: fp64 state within 2^-40 relative, the fp32 matrices within 2^-23 absolute"""
    data, poses = _pose_data()
    assert data.train_poses is None
    tp = data.enable_pose_refinement()
    assert torch.equal(tp.view(torch.int32), data.poses.view(torch.int32)) and tp.data_ptr() != data.poses.data_ptr()
    n_img, hw, N = data.n_img, data.H * data.W, 96
    rng = np.random.default_rng(9)
    lr = torch.tensor([3e-3], dtype=torch.float32, device=DEV)
    ref = (data.pose_master.cpu().numpy(), np.zeros((n_img, 6)), np.zeros((n_img, 6)), np.zeros(n_img, np.int32))
    assert np.array_equal(ref[0].reshape(n_img, 3, 4), poses[:, :3, :4].astype(np.float64))
    for step in range(2):
        img = rng.integers(0, n_img, N)
        img[img == 3] = 2                                                     # image 3 never receives a ray
        inds = img * hw + rng.integers(0, hw, N)
        rg = rng.standard_normal((N, 6)) * 1e3
        if step == 0:
            rg[np.flatnonzero(img == 1)[0], 4] = np.nan                       # image 1's gradient is not finite in the first step
        before = [t.clone() for t in (data.pose_master, data.pose_m, data.pose_v, data.pose_counts, data.train_poses)]
        # the skip word set: nothing is touched
        data.pose_step(T(rg), T(inds), _words(skip=1, inv_scale=2.0 ** -10), lr)
        for t, b in zip((data.pose_master, data.pose_m, data.pose_v, data.pose_counts, data.train_poses), before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
        data.pose_step(T(rg), T(inds), _words(inv_scale=2.0 ** -10), lr)
        ref = P.pose_step_numpy(rg, inds, hw, *ref[:4], inv_scale=2.0 ** -10, lr=3e-3)
        got = [t.cpu().numpy() for t in (data.pose_master, data.pose_m, data.pose_v, data.pose_counts)]
        untouched = [3, 1] if step == 0 else [3]
        for i in untouched:                                                   # bit for bit: master, moments, count, fp32 matrix
            for t, b in zip((data.pose_master, data.pose_m, data.pose_v, data.pose_counts, data.train_poses), before):
                assert torch.equal(t[i:i + 1].view(torch.uint8), b[i:i + 1].view(torch.uint8)), (step, i)
        assert np.array_equal(got[3], ref[3]) and got[3].tolist() == ([1, 0, 1, 0, 1] if step == 0 else [2, 1, 2, 0, 2])
        for k in range(3):
            assert _close(got[k], ref[k], 2.0 ** -40), (step, k)
        tp32 = data.train_poses.cpu().numpy()
        assert np.all(np.abs(tp32[:, :3, :4].reshape(n_img, 12).astype(np.float64) - ref[4].astype(np.float64)) <= 2.0 ** -23)
        assert np.array_equal(tp32[:, 3], poses[:, 3])
        assert np.array_equal(tp32[:, :3, :4].reshape(n_img, 12), got[0].astype(np.float32))
    # the poses did move, by about lr per component and step
    ang, dist = P.pose_error(data.train_poses.cpu().numpy(), poses)
    assert ang[3] == 0 and dist[3] == 0 and np.all(ang[[0, 2, 4]] > 1e-3) and np.all(dist[[0, 2, 4]] > 1e-3)
    assert np.array_equal(data.poses.cpu().numpy(), poses)                    # the caller's input stays
    # lr = 0: counts and moments advance, no pose bit changes (the signed zero included)
    before = data.pose_master.clone()
    data.pose_step(T(rg), T(inds), _words(), torch.zeros(1, device=DEV))
    assert torch.equal(before.view(torch.int64), data.pose_master.view(torch.int64))


def test_sampler_reads_the_refined_poses():
    data, poses = _pose_data()
    a = {k: v.clone() for k, v in data.sample(64, step=5).items() if torch.is_tensor(v)}
    data.enable_pose_refinement()
    b = {k: v.clone() for k, v in data.sample(64, step=5).items() if torch.is_tensor(v)}
    assert all(torch.equal(a[k], b[k]) for k in a)
    data.train_poses[:, :3, 3] += 0.25
    c = data.sample(64, step=5)
    assert torch.equal(c["inds"], a["inds"]) and torch.equal(c["rays_d"], a["rays_d"])
    assert torch.allclose(c["rays_o"], a["rays_o"] + 0.25, rtol=0, atol=1e-6) and not torch.equal(c["rays_o"], a["rays_o"])


# ---------------------------------------------------------------------------------------------------------------- the field op
def test_field_backward_fills_grad_x_and_feeds_autograd():
    """nerf_field(grad_x=...) leaves the kernel's result in the buffer, returns it to an x that requires grad, and changes nothing
    else about the backward"""
    from laenerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, log2_hashmap_size=15).to(DEV).train()
    net.encoder.embeddings.data.uniform_(-0.5, 0.5)
    M = 272
    x = (torch.rand(M, 3, device=DEV) * 2 - 1).contiguous()
    d = torch.nn.functional.normalize(torch.randn(M, 3, device=DEV), dim=-1)
    wr, ws = torch.randn(M, 3, device=DEV), torch.randn(M, device=DEV)

    def run(**kw):
        for p in net.parameters():
            p.grad = None
        xx = x.clone().requires_grad_(kw.pop("req", False))
        with torch.autocast("cuda", dtype=torch.float16):
            sigma, rgb = net(xx, d, **kw)
        ((rgb * wr).sum() + (sigma * ws).sum()).backward()
        return xx.grad, [p.grad.clone() for p in net.parameters()]

    _, base = run()
    buf = torch.full((M, 3), float("nan"), device=DEV)
    gx, grads = run(grad_x=buf, req=True)
    assert gx is not None and torch.equal(gx, buf) and torch.isfinite(buf).all() and buf.abs().sum() > 0
    assert all(torch.equal(a, b) for a, b in zip(base, grads))
    buf2 = torch.zeros(M, 3, device=DEV)
    gx2, _ = run(grad_x=buf2)
    assert gx2 is None and torch.equal(buf2, buf)
    with pytest.raises(RuntimeError, match="grad_x"):
        with torch.autocast("cuda", dtype=torch.float16):
            net(x, d, grad_x=torch.zeros(M, 2, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- the Trainer
ITERS, LR, RAYS = 400, 1e-2, 1024


def _views(n=8, H=64, W=64, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((n, H, W)) < 0.5, 255, img[..., 3])
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    return img, S.lookat_poses(n, seed=seed), (focal, focal, W / 2, H / 2)


def _trainer(net_seed=0, torch_seed=7, seed=1, graph=True, **kw):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    torch.manual_seed(net_seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    img, poses, intr = _views()
    data = ResidentImages.from_arrays(img, poses, intr, device=DEV)
    torch.manual_seed(torch_seed)
    return Trainer(r, opt, data, ITERS, LR, num_rays=RAYS, seed=seed, graph=graph, **kw)


def _state(tr):
    out = {}
    for i, (p, m, v, *_) in enumerate(tr.opt.items):
        out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach().clone(), m.clone(), v.clone()
    out["density_grid"], out["words"], out["data_step"] = tr.r.density_grid.clone(), tr.opt.dev_state.clone(), tr.data.step.clone()
    return out


def _pose_state(tr):
    d = tr.data
    return {"master": d.pose_master.clone(), "m": d.pose_m.clone(), "v": d.pose_v.clone(), "counts": d.pose_counts.clone(),
            "train_poses": d.train_poses.clone(), "refined": tr.refined_poses()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_trainer_pose_lr_zero_is_the_plain_run():
    plain = _trainer().train(32)
    zero = _trainer(pose_refine=True, pose_lr=0.0).train(32)
    assert np.array_equal(plain.losses().view(np.int32), zero.losses().view(np.int32)) and np.isfinite(plain.losses()).all()
    _same(_state(plain), _state(zero))
    assert torch.equal(zero.refined_poses().view(torch.int32), zero.data.poses.view(torch.int32))
    assert int(zero.data.pose_counts.sum()) == 32 - zero.steps_skipped       # mode 'image': one image per step took a (zero) step
    ang, dist = zero.pose_deltas()
    assert not ang.any() and not dist.any()
    assert "pose_refine" not in plain.config() and zero.config()["pose_refine"] is True and zero.config()["pose_lr"] == 0.0
    assert plain.data.train_poses is None and torch.equal(plain.refined_poses(), plain.data.poses)


def test_trainer_pose_graph_equals_eager():
    a = _trainer(pose_refine=True, pose_lr=1e-3, graph=True).train(48)
    b = _trainer(pose_refine=True, pose_lr=1e-3, graph=False).train(48)
    assert a.captures >= 1 and b.captures == 0
    assert np.array_equal(a.losses().view(np.int32), b.losses().view(np.int32))
    _same(_state(a), _state(b))
    _same(_pose_state(a), _pose_state(b))
    ang, dist = a.pose_deltas()
    assert ang.max() > 0 and dist.max() > 0 and np.isfinite(ang).all() and np.isfinite(dist).all()
    assert torch.equal(a.data.poses, b.data.poses) and not torch.equal(a.refined_poses(), a.data.poses)


def test_trainer_pose_resume_equals_uninterrupted(tmp_path):
    kw = dict(pose_refine=True, pose_lr=1e-3)
    full = _trainer(**kw).train(32)
    first = _trainer(**kw).train(16)
    path = first.save_checkpoint(str(tmp_path / "pose.pth"))
    ck = torch.load(path, weights_only=True)
    from laenerf_amd import checkpoint as C
    assert set(ck[C.KEY]["data"]["pose"]) == {"master", "m", "v", "counts"} and ck[C.KEY]["config"]["pose_lr"] == 1e-3
    fresh = _trainer(net_seed=1234, torch_seed=4321, seed=99, **kw)
    ptr = fresh.data.train_poses.data_ptr()
    fresh.load_checkpoint(path)
    assert fresh.data.train_poses.data_ptr() == ptr                           # written in place
    _same(_pose_state(first), _pose_state(fresh))
    fresh.train(16)
    assert np.array_equal(fresh.losses().view(np.int32), full.losses()[-16:].view(np.int32))
    _same(_state(full), _state(fresh))
    _same(_pose_state(full), _pose_state(fresh))
    # a trainer without the refinement refuses the file (the configuration differs), and the other way round
    with pytest.raises(ValueError, match="pose_refine"):
        _trainer().load_checkpoint(path)


def test_trainer_pose_refusals():
    from laenerf_amd.trainer import Trainer
    tr = _trainer()
    tr.r.fused_post_ops = False
    with pytest.raises(ValueError, match="fused_post_ops"):
        Trainer(tr.r, tr.opt, tr.data, ITERS, LR, num_rays=RAYS, pose_refine=True)
    tr.r.fused_post_ops = True
    with pytest.raises(ValueError, match="pose_lr"):
        Trainer(tr.r, tr.opt, tr.data, ITERS, LR, num_rays=RAYS, pose_refine=True, pose_lr=-1.0)
    assert tr.data.train_poses is None                                        # a refused trainer changed nothing on the data


# ---------------------------------------------------------------------------------------------------------------- registration
NOISE_DEG, NOISE_DIST, RADIUS = 0.16, 0.006, 3.2
REG_STEPS, REG_LR, FIT_STEPS = 640, 2e-4, 1024


def _smooth_teacher(n_views, H, W):
    """tools/train_loop.py's teacher (a random network on a sphere-and-boxes occupancy grid) with the table zeroed on every level whose
    cell is smaller than four times the displacement the pose noise causes at the object: NOISE_DIST + RADIUS * angle in world units,
    half of that in the unit cube (bound 1).  -> uint8 RGBA views, true poses, intrinsics, the levels kept"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.rays import get_rays
    from laenerf_amd.renderer import NeRFRenderer
    with torch.random.fork_rng(devices=[DEV]):
        torch.manual_seed(11)
        net = NeRFNetwork(bound=1).to(DEV).eval()
        net.encoder.embeddings.data.uniform_(-1.0, 1.0)
        net.sigma_net.weights.data.mul_(1.5)
    disp = (NOISE_DIST + RADIUS * np.deg2rad(NOISE_DEG)) / 2
    enc = net.encoder
    scales = P.grid_level_scales(enc.num_levels, np.float32(np.log2(enc.per_level_scale)), enc.base_resolution)
    keep = [l for l in range(enc.num_levels) if 1.0 / float(scales[l]) >= 4 * disp]
    off = enc.offsets_host
    for l in range(enc.num_levels):
        if l not in keep:
            net.encoder.embeddings.data[int(off[l]):int(off[l + 1])] = 0
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(DEV).eval()
    r.density_bitfield = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=r.cascade, bound=1.0), 10.0)).to(DEV)
    poses = S.lookat_poses(n_views, radius=RADIUS, seed=0)
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    intr = (focal, focal, W / 2, H / 2)
    out = []
    with torch.no_grad():
        for i in range(n_views):
            ray = get_rays(torch.from_numpy(poses[i:i + 1]).to(DEV), intr, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=0, max_steps=1024)
            ws = res["weights_sum"].float().clamp(0, 1)
            rgb = torch.where(ws[:, None] > 0, res["image"].float() / ws.clamp(min=1e-6)[:, None], torch.zeros_like(res["image"].float()))
            rgba = torch.cat([rgb.clamp(0, 1), ws[:, None]], 1).reshape(H, W, 4)
            out.append((rgba * 255 + 0.5).to(torch.uint8).cpu().numpy())
    return np.stack(out), poses, intr, keep


def test_registration_on_a_smooth_teacher():
    """directional, end to end: a student fitted on the true poses, then frozen (network lr = 0) while a second Trainer refines
    perturbed cameras against it.  Mean rotation and mean translation error end strictly below their start, the loss falls, and the
    same run with pose_lr = 0 moves no camera and ends on a higher loss (the two runs draw the same pixels).
    The noise: NOISE_DEG about a random axis through the camera and NOISE_DIST in a random direction -- at the object RADIUS * angle =
    0.009 and 0.006, of one order, so that neither unknown can absorb the other's error (a translation across the view and a rotation
    about the camera move the image alike).  pose_lr = 2e-4, a twentieth of the error, over 640 steps of one image each (80 per
    camera), decayed to a tenth.  Measured on the MI355X: rotation 0.1600 -> 0.1024 degrees, translation 0.00600 -> 0.00479, last-16
    loss 1.467e-4 refined against 1.552e-4 frozen."""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    img, poses, intr, keep = _smooth_teacher(8, 64, 64)
    assert len(keep) >= 2 and keep == list(range(len(keep)))
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    true_data = ResidentImages.from_arrays(img, poses, intr, bg="random", device=DEV)
    fit = Trainer(r, opt, true_data, FIT_STEPS, LR, num_rays=RAYS, seed=0).train(FIT_STEPS)
    fit_loss = float(fit.losses()[-16:].mean())
    noisy = P.perturb_poses(poses, NOISE_DEG, NOISE_DIST, seed=5)
    ang0, dist0 = (v.mean() for v in P.pose_error(noisy, poses))
    weights = [p.detach().clone() for p in net.parameters()]
    grid_state = (r.density_grid.clone(), r.density_bitfield.clone(), r.mean_count, r.mean_density, r.iter_density, r.local_step)
    rng_state = torch.cuda.get_rng_state(DEV)
    runs = {}
    for name, plr in (("refined", REG_LR), ("frozen", 0.0)):
        r.density_grid.copy_(grid_state[0]); r.density_bitfield.copy_(grid_state[1])
        r.mean_count, r.mean_density, r.iter_density, r.local_step = grid_state[2:]
        torch.cuda.set_rng_state(rng_state, DEV)
        data = ResidentImages.from_arrays(img, noisy, intr, bg="random", device=DEV)
        tr = Trainer(r, opt, data, REG_STEPS, 0.0, num_rays=RAYS, seed=3, pose_refine=True, pose_lr=plr).train(REG_STEPS)
        assert all(torch.equal(a, b.detach()) for a, b in zip(weights, net.parameters()))      # the student is frozen
        ang, dist = (v.mean() for v in P.pose_error(tr.refined_poses().cpu().numpy(), poses))
        losses = tr.losses()
        runs[name] = (ang, dist, float(losses[:16].mean()), float(losses[-16:].mean()))
        print(f"registration {name}: levels kept {keep}, fit loss {fit_loss:.3e}; rotation {np.rad2deg(ang0):.4f} -> {np.rad2deg(ang):.4f} deg, "
              f"translation {dist0:.5f} -> {dist:.5f}, loss first 16 {runs[name][2]:.4e} last 16 {runs[name][3]:.4e}, "
              f"skipped {tr.steps_skipped}")
    ang, dist, first, last = runs["refined"]
    assert ang < ang0 and dist < dist0
    assert last < first
    f_ang, f_dist, _, f_last = runs["frozen"]
    assert f_ang == ang0 and f_dist == dist0
    assert last < f_last
