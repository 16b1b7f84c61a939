"""Depth supervision: the DEPTH flavours of the compositing backward and of the fused training step, the Trainer's and the
distillation's depth term.  Kernel cases: the hand-built table of depth_sup_util (passes of 64 samples, early stops in the first and
second pass and at lane 63, an empty and a dropped ray, a tail of unowned rows, N no multiple of the 4 rays of a workgroup), every
output buffer poisoned with NaN."""
import numpy as np
import pytest
import torch

from depth_sup_util import T_THRESH, build_case, build_grads
from gpu_util import DEV, N as NP, T

pytestmark = pytest.mark.gpu

LAMBDA, SCALE = 0.37, 1024.0


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.fixture(scope="module")
def case():
    from laenerf_amd import build
    build.build()
    c = build_case()
    t = {k: T(c[k]) for k in ("sigmas", "rgbs", "deltas", "rays", "nears", "fars", "bg_rays")}
    t["rows_end"] = torch.tensor([c["rows_end"]], dtype=torch.int32, device=DEV)
    t["rays"].rows_end = t["rows_end"]
    return c, t


@pytest.fixture(scope="module")
def reference(case):
    """fp64 restatement of the backward on the case's inputs, computed once"""
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c, _ = case
    gws, gimg, gD = build_grads(c["N"])
    ref = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, bg=c["bg_rays"], grad_weights_sum=gws,
                                grad_image=gimg, grad_depth=gD)
    t_max = max(float(c["deltas"][o:o + s, 1].astype(np.float64).sum()) for _, o, s in c["rays"] if s and o + s <= c["M"])
    return ref, (gws, gimg, gD), t_max


def _forward(c, t):
    from laenerf_amd.backend import raymarching_backend as B
    n = c["N"]
    ws, dp, im, do, io = _nan(n), _nan(n), _nan(n, 3), _nan(n), _nan(n, 3)
    B.composite_rays_train_forward_blend(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], c["M"], n, T_THRESH, t["nears"], t["fars"],
                                         t["bg_rays"], (0.0, 0.0, 0.0), ws, dp, im, do, io)
    return ws, dp, im, do, io


# ---------------------------------------------------------------------------------------------------------------- a
def test_backward_with_depth_gradient_against_fp64(case, reference):
    """lae_composite_rays_train_backward_blend_ex with grad_depth against the fp64 restatement.  Bound: the kernel family's own (rtol 1e-4, atol
    3e-5 on grad_sigmas, test_gpu_raymarching.py), atol times max(1, max t) * max(1, max |grad_depth|), the magnitude of the new
    operand.  The fp32 restatement deviates from fp64 by 2.0e-8 on these inputs, far below a quarter of it."""
    from laenerf_amd.backend import raymarching_backend as B
    c, t = case
    ref, (gws, gimg, gD), t_max = reference
    ws, dp, im, _, _ = _forward(c, t)
    assert np.allclose(NP(dp), ref["depth"], atol=2e-5) and np.allclose(NP(ws), ref["weights_sum"], atol=2e-6)
    M, n = c["M"], c["N"]
    gs, gc = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend_depth(T(gws), T(gimg), T(gD), t["sigmas"], t["rgbs"], t["deltas"], t["rays"], ws, dp, im, M, n,
                                                T_THRESH, t["bg_rays"], (0.0, 0.0, 0.0), t["rows_end"], gs, gc)
    assert torch.isfinite(gs).all() and torch.isfinite(gc).all()                    # every row of both buffers is written
    atol = 3e-5 * max(1.0, t_max) * max(1.0, float(np.abs(gD).max()))
    err = np.abs(NP(gs).astype(np.float64) - ref["grad_sigmas"])
    print(f"grad_sigmas: max abs error {err.max():.3e}, atol {atol:.3e}, max |grad| {np.abs(ref['grad_sigmas']).max():.3e}")
    assert np.allclose(NP(gs), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    # the depth gradient is there: without it the result is off by far more than the bound
    gs0, gc0 = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend(T(gws), T(gimg), t["sigmas"], t["rgbs"], t["deltas"], t["rays"], ws, im, M, n, T_THRESH,
                                          t["bg_rays"], (0.0, 0.0, 0.0), t["rows_end"], gs0, gc0)
    assert torch.equal(gc, gc0)                                                     # grad_rgbs: the existing backward's bits
    assert not np.allclose(NP(gs0), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    # rows after the stop, of the dropped ray and of the tail are zero
    assert not gs[c["rows_end"]:].any() and not gc[c["rows_end"]:].any()
    # a zero grad_depth gives the existing backward's bits
    gs1, gc1 = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend_depth(T(gws), T(gimg), torch.zeros(n, device=DEV), t["sigmas"], t["rgbs"], t["deltas"],
                                                t["rays"], ws, dp, im, M, n, T_THRESH, t["bg_rays"], (0.0, 0.0, 0.0), t["rows_end"], gs1, gc1)
    assert torch.equal(gs1, gs0) and torch.equal(gc1, gc0)


def test_depth_raw_is_differentiable_through_the_operator(case, reference):
    from laenerf_amd.raymarching import raymarching as rm
    c, t = case
    ref, (gws, gimg, gD), t_max = reference
    s, col = t["sigmas"].clone().requires_grad_(), t["rgbs"].clone().requires_grad_()
    ws, d_raw, d_out, img = rm.composite_rays_train_blend_depth(s, col, t["deltas"], t["rays"], t["nears"], t["fars"], bg_color=t["bg_rays"],
                                                              T_thresh=T_THRESH)
    assert d_raw.requires_grad and not d_out.requires_grad
    torch.autograd.backward([ws, d_raw, img], [T(gws), T(gD), T(gimg)])
    atol = 3e-5 * max(1.0, t_max) * max(1.0, float(np.abs(gD).max()))
    assert np.allclose(NP(s.grad), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    assert np.allclose(NP(col.grad), ref["grad_rgbs"], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- b, c
def _step(c, t, target, depth_sup=None, scale=None, bg_rays=True):
    from laenerf_amd.backend import raymarching_backend as B
    M, n = c["M"], c["N"]
    o = dict(ws=_nan(n), dp=_nan(n), im=_nan(n, 3), do=_nan(n), io=_nan(n, 3), gi=_nan(n, 3), gs=_nan(M), gc=_nan(M, 3), loss=_nan(2),
             part=_nan((n + 3) // 4))
    if depth_sup is not None:
        src, inds, lam, value_only = depth_sup
        o["gd"], o["dpart"] = _nan(n), _nan((n + 3) // 4)
        depth_sup = (src, inds, lam, value_only, o["gd"], o["dpart"])
    B.composite_rays_train_step(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"],
                                t["bg_rays"] if bg_rays else None, (1.0, 1.0, 1.0), t["rows_end"], target, scale, o["ws"], o["dp"], o["im"],
                                o["do"], o["io"], o["gi"], o["gs"], o["gc"], o["loss"], o["part"], depth_sup=depth_sup)
    return o


def _no_sample_rows(c):
    return [n for n, k in enumerate(c["kinds"]) if k == "dropped" or c["rays"][n, 2] == 0]


def _plane(c, with_inds, dtype, seed=5):
    """-> (depth_src, depth_inds or None, z [N] fp32 as the kernel reads it): zeros (no supervision) and a negative value included"""
    rng = np.random.default_rng(seed)
    n = c["N"]
    P = 97 if with_inds else n
    plane = rng.uniform(0.5, 3.0, P).astype(np.float32)
    plane[::4] = 0.0
    plane[1] = -1.0
    inds = rng.integers(0, P, n).astype(np.int64) if with_inds else None
    for row in _no_sample_rows(c):                         # the rays without samples are supervised
        if with_inds:
            inds[c["rays"][row, 0]] = 2 + row % 2
        else:
            plane[c["rays"][row, 0]] = 1.5
    inds = None if inds is None else T(inds)
    src = T(plane).to(dtype)
    z = src.float() if inds is None else src.float()[inds]
    assert int((z > 0).sum()) >= 4 and int((z <= 0).sum()) >= 2
    return src, inds, z


@pytest.mark.parametrize("with_inds", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_fused_step_with_depth_equals_the_two_launches(case, with_inds, dtype):
    from laenerf_amd.backend import raymarching_backend as B
    c, t = case
    M, n = c["M"], c["N"]
    target = torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    scale = torch.tensor([SCALE], device=DEV)
    src, inds, z = _plane(c, with_inds, dtype)
    o = _step(c, t, target, (src, inds, LAMBDA, False), scale)
    for k, v in o.items():
        assert torch.isfinite(v).all(), k                  # every output row is written
    # forward_blend + backward_blend_depth, fed the fused call's own grad_image and grad_depth
    ws, dp, im, do, io = _nan(n), _nan(n), _nan(n, 3), _nan(n), _nan(n, 3)
    B.composite_rays_train_forward_blend(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"],
                                         t["bg_rays"], (1.0, 1.0, 1.0), ws, dp, im, do, io)
    gs, gc = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend_depth(None, o["gi"], o["gd"], t["sigmas"], t["rgbs"], t["deltas"], t["rays"], ws, dp, im, M, n,
                                                T_THRESH, t["bg_rays"], (1.0, 1.0, 1.0), t["rows_end"], gs, gc)
    for a, b in ((ws, o["ws"]), (dp, o["dp"]), (im, o["im"]), (io, o["io"]), (do, o["do"]), (gs, o["gs"]), (gc, o["gc"])):
        assert torch.equal(a, b)
    # the criterion, from torch
    res = (o["dp"] - (z - t["nears"])) * (z > 0)
    g_ref = (res * (2 * LAMBDA / n)) * SCALE
    assert torch.allclose(o["gd"], g_ref, rtol=1e-6, atol=0)
    assert int((o["gd"] != 0).sum()) >= 4 and int((o["gd"] == 0).sum()) >= 2          # both kinds of ray in one launch
    mse = ((o["io"].double() - target.double()) ** 2).mean().item()
    dmse = (res.double() ** 2).mean().item()
    assert o["loss"][1].item() == pytest.approx(mse + LAMBDA * dmse, rel=1e-5)
    assert o["loss"][0].item() == pytest.approx(SCALE * o["loss"][1].item(), rel=1e-6)
    assert LAMBDA * dmse > 0.05 * mse                                                # the depth term is no rounding-level part
    out = _nan(2)
    B.loss_finish(o["dpart"], (n + 3) // 4, n, None, out)
    assert out[1].item() == pytest.approx(dmse, rel=1e-5) and out[0].item() == out[1].item()
    # the empty and the dropped ray add their residual to the value (dmse above holds it) and have no sample gradient
    for row in _no_sample_rows(c):
        idx = int(c["rays"][row, 0])
        assert o["dp"][idx].item() == 0.0 and z[idx].item() > 0 and res[idx].item() != 0 and o["gd"][idx].item() != 0
    assert not o["gs"][c["rows_end"]:].any()


@pytest.mark.parametrize("mode", ["zero_plane", "value_only"])
def test_feature_off_paths_give_the_plain_step(case, mode):
    c, t = case
    n = c["N"]
    target = torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    scale = torch.tensor([SCALE], device=DEV)
    plain = _step(c, t, target, None, scale)
    src, inds, z = _plane(c, True, torch.float16)
    if mode == "zero_plane":
        src = torch.zeros_like(src)
        z = torch.zeros_like(z)
    o = _step(c, t, target, (src, inds, LAMBDA, mode == "value_only"), scale)
    for k in ("ws", "dp", "im", "io", "gi", "gs", "gc"):
        assert torch.equal(plain[k], o[k]), k
    assert not o["gd"].any()
    res = (o["dp"] - (z - t["nears"])) * (z > 0)
    dmse = (res.double() ** 2).mean().item()
    if mode == "zero_plane":
        assert torch.equal(plain["loss"], o["loss"]) and not o["dpart"].any()
    else:
        assert LAMBDA * dmse > 0.05 * plain["loss"][1].item()
        assert o["loss"][1].item() == pytest.approx(plain["loss"][1].item() + LAMBDA * dmse, rel=1e-5)


def test_a_ray_that_misses_the_bounding_box_is_unsupervised(case):
    """near_far_from_aabb gives such a ray near == far == FLT_MAX; a depth plane from a sensor covers it all the same.  Its residual
    would be ~FLT_MAX and the loss infinite: it counts as unsupervised, and every other ray keeps its bits."""
    c, t = case
    n = c["N"]
    target = torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    src, inds, z = _plane(c, False, torch.float32)
    base = _step(c, t, target, (src, None, LAMBDA, False), None)
    miss = [int(c["rays"][row, 0]) for row in _no_sample_rows(c)]               # the rays without samples: they may miss the box
    t2 = dict(t)
    big = torch.finfo(torch.float32).max
    t2["nears"], t2["fars"] = t["nears"].clone(), t["fars"].clone()
    t2["nears"][miss] = big
    t2["fars"][miss] = big
    o = _step(c, t2, target, (src, None, LAMBDA, False), None)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[miss] = False
    assert (base["gd"][miss] != 0).all() and not o["gd"][miss].any()
    assert torch.equal(o["gd"][keep], base["gd"][keep]) and torch.equal(o["gs"], base["gs"]) and torch.equal(o["gc"], base["gc"])
    res = torch.where((z > 0) & keep, o["dp"] - (z - t2["nears"]), torch.zeros_like(z))
    assert torch.isfinite(o["loss"]).all() and torch.isfinite(o["dpart"]).all()
    mse = ((o["io"].double() - target.double()) ** 2).mean().item()
    assert o["loss"][1].item() == pytest.approx(mse + LAMBDA * (res.double() ** 2).mean().item(), rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------- d
def _depth_trainer(depth_weight, depth_grad=True, graph=True, steps=32):
    """a Trainer on the small synthetic scene of test_gpu_trainer.py with a random depth plane (30 % unsupervised pixels)"""
    from test_gpu_trainer import _setup, _state
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    rng = np.random.default_rng(12)
    plane = rng.uniform(2.0, 4.0, (data.n_img, data.H, data.W)).astype(np.float16)
    plane[rng.random(plane.shape) < 0.3] = 0
    data.set_depths(plane)
    torch.manual_seed(7)
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, graph=graph, capacity="exact", depth_weight=depth_weight,
                 depth_grad=depth_grad).train(steps)
    return tr, _state(r, opt)


@pytest.fixture(scope="module")
def trainer_runs():
    return {"graph": _depth_trainer(0.1), "eager": _depth_trainer(0.1, graph=False), "value_only": _depth_trainer(0.1, depth_grad=False),
            "plain": _depth_trainer(None)}


def test_trainer_with_depth_graph_equals_eager(trainer_runs):
    from test_gpu_trainer import _assert_same
    (ta, sa), (tb, sb) = trainer_runs["graph"], trainer_runs["eager"]
    assert ta.captures == 1 and tb.captures == 0                     # steps 16-31 were one replayed graph
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses()) and np.array_equal(ta.depth_losses(), tb.depth_losses())
    assert ta.losses().shape == ta.depth_losses().shape == (32,) and np.isfinite(ta.losses()).all() and (ta.depth_losses() > 0).all()
    # and the depth term trains: the parameters differ from the run without it
    assert any(not torch.equal(x, y) for x, y in zip(sa, trainer_runs["plain"][1]))


def test_trainer_value_only_depth_is_the_run_without_depth(trainer_runs):
    from test_gpu_trainer import _assert_same
    (tv, sv), (tp, sp) = trainer_runs["value_only"], trainer_runs["plain"]
    _assert_same(sv, sp)
    assert tp.depth_losses().size == 0 and (tv.depth_losses() > 0).all()
    mse = tv.losses().astype(np.float64) - 0.1 * tv.depth_losses().astype(np.float64)
    print("value-only: total", tv.losses()[-4:], "depth term", tv.depth_losses()[-4:], "plain", tp.losses()[-4:])
    assert np.allclose(mse, tp.losses(), rtol=1e-5, atol=0)


def test_trainer_refuses_depth_without_a_plane():
    from test_gpu_trainer import _setup
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    with pytest.raises(ValueError):
        Trainer(r, opt, data, 400, 1e-2, depth_weight=1e-3)
    with pytest.raises(ValueError):
        data.set_depths(np.zeros((data.n_img, data.H, data.W + 1), np.float32))


# ---------------------------------------------------------------------------------------------------------------- e
def _sphere_run(depth_grad, groups=4):
    """images without geometric signal (white on a white background), an analytic sphere's depth plane, depth_weight 1"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    n, H, W = 6, 48, 40
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    poses, intr = S.lookat_poses(n, seed=0), (focal, focal, W / 2, H / 2)
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    data = ResidentImages.from_arrays(np.full((n, H, W, 3), 255, np.uint8), poses, intr, bg="white", device=DEV,
                                      depths=S.sphere_depth_planes(poses, intr, H, W, radius=0.6))
    assert float((data.depths > 0).float().mean()) > 0.05
    torch.manual_seed(7)
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, capacity="exact", depth_weight=1.0, depth_grad=depth_grad)
    tr.train(16 * groups)
    return tr.depth_losses().reshape(groups, 16).mean(1)


def test_depth_gradient_pulls_the_geometry_to_the_depth_plane():
    """ordering only: with the gradient the depth term falls, and ends below the value-only run's (DESIGN.md 4g has both sequences)"""
    on, off = _sphere_run(True), _sphere_run(False)
    print("depth term per 16-step group, depth_grad=True :", on.tolist())
    print("depth term per 16-step group, depth_grad=False:", off.tolist())
    assert on[-1] < on[0]
    assert on[-1] < off[-1]


# ---------------------------------------------------------------------------------------------------------------- f
def test_distilled_depth_plane_equals_the_reference_scatter():
    from test_gpu_distill import style_encoder
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.editing.distill import DistillSet, distill_images
    n_img, H, W = 5, 40, 48
    rng = np.random.default_rng(8)
    g = torch.Generator().manual_seed(8)
    views, want = [], np.zeros((n_img, H * W), np.float32)
    for i, K in ((3, 500), (0, 333), (1, 1000)):                       # views 2 and 4 are occluded; the order is not the image order
        idx = np.sort(rng.choice(H * W, K, replace=False))
        depths = rng.uniform(0.5, 4.0, K).astype(np.float32)
        want[i, idx] = depths                                            # gui.py:509-510: d_ = zeros; d_[indices] = depth
        views.append({"pose_idx": i, "indices": torch.from_numpy(idx), "w8s": torch.rand(K, generator=g),
                      "x_term": (torch.rand(K, 3, generator=g) - 0.5) * 0.8,
                      "dirs": torch.nn.functional.normalize(torch.randn(K, 3, generator=g), dim=-1),
                      "pred_imgs": torch.rand(H * W, 3, generator=g), "depths": torch.from_numpy(depths)})
    data = ResidentImages.from_arrays(rng.integers(0, 256, (n_img, H, W, 4), dtype=np.uint8), S.lookat_poses(n_img, seed=1),
                                      (50.0, 50.0, W / 2, H / 2), device=DEV)
    dset = DistillSet.from_views(views, [2, 4], n_img, device=DEV)
    assert dset.depth is not None and dset.depth.shape == (1833,)
    enc = style_encoder()
    out = distill_images(data, enc, dset, depth_sup=True)
    assert out.depths.dtype == torch.float32 and out.depths.shape == (n_img, H, W)
    assert np.array_equal(out.depths.cpu().numpy().reshape(n_img, -1), want)
    assert not out.depths[2].any() and not out.depths[4].any() and data.depths is None
    assert distill_images(data, enc, dset).depths is None
    for v in views:
        del v["depths"]
    with pytest.raises(ValueError):
        distill_images(data, enc, DistillSet.from_views(views, [2, 4], n_img, device=DEV), depth_sup=True)
