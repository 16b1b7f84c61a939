"""The distortion regularizer: the DIST flavours of the compositing forward, backward and fused training step through the C ABI
bindings, and the Trainer's distort_weight.  Kernel cases: the hand-built table of depth_sup_util (passes of 64 samples, early stops in
the first and second pass and at lane 63, an empty and a dropped ray, a tail of unowned rows, N no multiple of the 4 rays of a
workgroup), every output buffer poisoned with NaN.  The fp64 reference is composite_distort_numpy, pinned by test_distort_cpu.py."""
import numpy as np
import pytest
import torch

from depth_sup_util import T_THRESH, build_case, build_grads
from gpu_util import DEV, N as NP, T
from test_distort_cpu import LAMBDA

pytestmark = pytest.mark.gpu

LAMBDA_DEPTH, SCALE = 0.37, 1024.0
BG = (1.0, 1.0, 1.0)


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
    """fp64 restatements on the case's inputs, computed once: the distortion gradient alone and together with the depth gradient"""
    from laenerf_amd.raymarching.raymarching import composite_distort_numpy
    c, _ = case
    gws, gimg, gD = build_grads(c["N"])
    g_dist = np.random.default_rng(31).standard_normal(c["N"]).astype(np.float32)
    kw = dict(bg=c["bg_rays"], grad_weights_sum=gws, grad_image=gimg, grad_dist=g_dist)
    ref = {False: composite_distort_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, **kw),
           True: composite_distort_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, grad_depth=gD, **kw)}
    t_max = max(float(c["deltas"][o:o + s, 1].astype(np.float64).sum()) for _, o, s in c["rays"] if s and o + s <= c["M"])
    return ref, (gws, gimg, gD, g_dist), t_max


def _forward(c, t, bg=(0.0, 0.0, 0.0), dist=True):
    from laenerf_amd.backend import raymarching_backend as B
    n = c["N"]
    ws, dp, im, do, io, ds = _nan(n), _nan(n), _nan(n, 3), _nan(n), _nan(n, 3), _nan(n)
    args = (t["sigmas"], t["rgbs"], t["deltas"], t["rays"], c["M"], n, T_THRESH, t["nears"], t["fars"], t["bg_rays"], bg, ws, dp, im, do, io)
    if dist:
        B.composite_rays_train_forward_blend_dist(*args, ds)
    else:
        B.composite_rays_train_forward_blend(*args)
    return ws, dp, im, do, io, ds


# ---------------------------------------------------------------------------------------------------------------- 1
def test_forward_dist_against_fp64_and_the_other_outputs_keep_their_bits(case, reference):
    """dist against fp64.  Bound: the family's bound on the raw depth (atol 2e-5, test_gpu_depth_sup.py) times max(1, max t): l_ray <=
    W^2 t_max has the depth's magnitude."""
    c, t = case
    ref, _, t_max = reference
    ws, dp, im, do, io, ds = _forward(c, t)
    atol = 2e-5 * max(1.0, t_max)
    err = np.abs(NP(ds).astype(np.float64) - ref[False]["dist"])
    print(f"dist: max abs error {err.max():.3e}, atol {atol:.3e}, max dist {ref[False]['dist'].max():.3e}")
    assert torch.isfinite(ds).all() and np.allclose(NP(ds), ref[False]["dist"], atol=atol)
    none = [int(c["rays"][n, 0]) for n, k in enumerate(c["kinds"]) if k == "dropped" or c["rays"][n, 2] == 0]
    assert len(none) == 2 and not ds[none].any()
    for a, b in zip((ws, dp, im, do, io), _forward(c, t, dist=False)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("with_depth", [False, True])
def test_backward_with_dist_gradient_against_fp64(case, reference, with_depth):
    """lae_composite_rays_train_backward_blend_ex with grad_dist against the fp64 restatement.  Bound: the kernel family's own (rtol 1e-4, atol 3e-5
    on grad_sigmas), atol times max(1, max |q_k|) * max(1, max |grad_dist|), the magnitude of the new operand (q in the colour's
    place; max |q_k| from the fp64 reference), and times the depth test's factor when the depth gradient is on as well."""
    from laenerf_amd.backend import raymarching_backend as B
    c, t = case
    ref, (gws, gimg, gD, g_dist), t_max = reference
    ref = ref[with_depth]
    ws, dp, im, _, _, ds = _forward(c, t)
    M, n = c["M"], c["N"]

    def run(grad_depth, grad_dist):
        gs, gc = _nan(M), _nan(M, 3)
        B.composite_rays_train_backward_blend_dist(T(gws), T(gimg), grad_depth, grad_dist, t["sigmas"], t["rgbs"], t["deltas"], t["rays"],
                                                   ws, dp, ds, im, M, n, T_THRESH, t["bg_rays"], (0.0, 0.0, 0.0), t["rows_end"], gs, gc)
        return gs, gc

    gs, gc = run(T(gD) if with_depth else None, T(g_dist))
    assert torch.isfinite(gs).all() and torch.isfinite(gc).all()                    # every row of both buffers is written
    atol = 3e-5 * max(1.0, float(np.abs(ref["q"]).max())) * max(1.0, float(np.abs(g_dist).max()))
    if with_depth:
        atol *= max(1.0, t_max) * max(1.0, float(np.abs(gD).max()))
    err = np.abs(NP(gs).astype(np.float64) - ref["grad_sigmas"])
    print(f"grad_sigmas (depth {with_depth}): max abs error {err.max():.3e}, atol {atol:.3e}, max |q| {np.abs(ref['q']).max():.3e}, "
          f"max |grad| {np.abs(ref['grad_sigmas']).max():.3e}")
    assert np.allclose(NP(gs), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    assert not gs[c["rows_end"]:].any() and not gc[c["rows_end"]:].any()
    # negative control: without the distortion gradient the result misses the bound; such rays have the existing backward's bits
    gs0, gc0 = run(T(gD) if with_depth else None, torch.zeros(n, device=DEV))
    assert not np.allclose(NP(gs0), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    gs1, gc1 = _nan(M), _nan(M, 3)
    tail = (t["sigmas"], t["rgbs"], t["deltas"], t["rays"], ws)
    rest = (im, M, n, T_THRESH, t["bg_rays"], (0.0, 0.0, 0.0), t["rows_end"], gs1, gc1)
    if with_depth:
        B.composite_rays_train_backward_blend_depth(T(gws), T(gimg), T(gD), *tail, dp, *rest)
    else:
        B.composite_rays_train_backward_blend(T(gws), T(gimg), *tail, *rest)
    assert torch.equal(gs0, gs1) and torch.equal(gc0, gc1)
    assert torch.equal(gc, gc1)                                                     # grad_rgbs does not change with the term


def test_dist_is_differentiable_through_the_operator(case, reference):
    from laenerf_amd.raymarching import raymarching as rm
    c, t = case
    ref, (gws, gimg, gD, g_dist), t_max = reference
    s, col = t["sigmas"].clone().requires_grad_(), t["rgbs"].clone().requires_grad_()
    ws, d_raw, d_out, img, dist = rm.composite_rays_train_blend_distort(s, col, t["deltas"], t["rays"], t["nears"], t["fars"],
                                                                        bg_color=t["bg_rays"], T_thresh=T_THRESH)
    assert dist.requires_grad and d_raw.requires_grad and not d_out.requires_grad
    torch.autograd.backward([ws, img, dist], [T(gws), T(gimg), T(g_dist)])
    atol = 3e-5 * max(1.0, float(np.abs(ref[False]["q"]).max())) * max(1.0, float(np.abs(g_dist).max()))
    assert np.allclose(NP(s.grad), ref[False]["grad_sigmas"], rtol=1e-4, atol=atol)
    assert np.allclose(NP(col.grad), ref[False]["grad_rgbs"], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def _plane(c):
    """a per-ray fp32 depth plane with unsupervised rays (zeros) -> (src, z)"""
    z = np.random.default_rng(5).uniform(0.5, 3.0, c["N"]).astype(np.float32)
    z[::4] = 0.0
    return T(z), T(z)


def _step(c, t, target, depth=None, dist=None, scale=None, bg_rays=True):
    """depth: None or (src, lambda, value_only); dist: None or (lambda, value_only)"""
    from laenerf_amd.backend import raymarching_backend as B
    M, n = c["M"], c["N"]
    o = dict(ws=_nan(n), dp=_nan(n), im=_nan(n, 3), do=_nan(n), io=_nan(n, 3), gi=_nan(n, 3), gs=_nan(M), gc=_nan(M, 3), loss=_nan(2),
             part=_nan((n + 3) // 4))
    depth_sup = dist_sup = None
    if depth is not None:
        o["gd"], o["dpart"] = _nan(n), _nan((n + 3) // 4)
        depth_sup = (depth[0], None, depth[1], depth[2], o["gd"], o["dpart"])
    if dist is not None:
        o["ds"], o["gx"], o["xpart"] = _nan(n), _nan(n), _nan((n + 3) // 4)
        dist_sup = (dist[0], dist[1], o["ds"], o["gx"], o["xpart"])
    B.composite_rays_train_step(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"],
                                t["bg_rays"] if bg_rays else None, BG, t["rows_end"], target, scale, o["ws"], o["dp"], o["im"],
                                o["do"], o["io"], o["gi"], o["gs"], o["gc"], o["loss"], o["part"], depth_sup=depth_sup, dist_sup=dist_sup)
    return o


def _target(n):
    return torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))


@pytest.mark.parametrize("bg_rays", [True, False])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("with_depth", [False, True])
def test_fused_step_with_dist_equals_the_two_launches(case, with_depth, scaled, bg_rays):
    from laenerf_amd.backend import raymarching_backend as B
    c, t = case
    M, n = c["M"], c["N"]
    target = _target(n)
    scale = torch.tensor([SCALE], device=DEV) if scaled else None
    sc = SCALE if scaled else 1.0
    src, z = _plane(c)
    o = _step(c, t, target, (src, LAMBDA_DEPTH, False) if with_depth else None, (LAMBDA, False), scale, bg_rays)
    for k, v in o.items():
        assert torch.isfinite(v).all(), k                  # every output row is written
    # forward_blend_dist + backward_blend_dist, fed the fused call's own grad_image, grad_dist (and grad_depth)
    bgr = t["bg_rays"] if bg_rays else None
    ws, dp, im, do, io, ds = _nan(n), _nan(n), _nan(n, 3), _nan(n), _nan(n, 3), _nan(n)
    B.composite_rays_train_forward_blend_dist(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"], bgr, BG,
                                              ws, dp, im, do, io, ds)
    gs, gc = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend_dist(None, o["gi"], o["gd"] if with_depth else None, o["gx"], t["sigmas"], t["rgbs"], t["deltas"],
                                               t["rays"], ws, dp, ds, im, M, n, T_THRESH, bgr, BG, t["rows_end"], gs, gc)
    for name, a, b in (("ws", ws, o["ws"]), ("dp", dp, o["dp"]), ("im", im, o["im"]), ("io", io, o["io"]), ("do", do, o["do"]),
                       ("ds", ds, o["ds"]), ("gs", gs, o["gs"]), ("gc", gc, o["gc"])):
        assert torch.equal(a, b), name
    # the criterion, from torch / fp64
    assert torch.allclose(o["gx"], torch.full((n,), (LAMBDA / n) * sc, device=DEV), rtol=1e-6, atol=0)
    mse = ((o["io"].double() - target.double()) ** 2).mean().item()
    l_dist = o["ds"].double().sum().item() / n
    dmse = 0.0
    if with_depth:
        res = (o["dp"] - (z - t["nears"])) * (z > 0)
        dmse = (res.double() ** 2).mean().item()
        assert torch.allclose(o["gd"], (res * (2 * LAMBDA_DEPTH / n)) * sc, rtol=1e-6, atol=0)
    assert o["loss"][1].item() == pytest.approx(mse + LAMBDA_DEPTH * dmse + LAMBDA * l_dist, rel=1e-5)
    assert o["loss"][0].item() == pytest.approx(sc * o["loss"][1].item(), rel=1e-6)
    assert LAMBDA * l_dist > 0.05 * mse                                              # the term is no rounding-level part
    out = _nan(2)
    B.loss_finish(o["xpart"], (n + 3) // 4, n, None, out)
    assert out[1].item() == pytest.approx(l_dist, rel=1e-5) and out[0].item() == out[1].item()
    assert not o["gs"][c["rows_end"]:].any()
    # and the term reaches the sample gradients
    plain = _step(c, t, target, (src, LAMBDA_DEPTH, False) if with_depth else None, None, scale, bg_rays)
    assert not torch.equal(plain["gs"], o["gs"]) and torch.equal(plain["gc"], o["gc"])


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("mode", ["zero_lambda", "value_only"])
def test_feature_off_paths_give_the_step_without_the_term(case, mode, with_depth):
    c, t = case
    n = c["N"]
    target = _target(n)
    scale = torch.tensor([SCALE], device=DEV)
    src, _ = _plane(c)
    depth = (src, LAMBDA_DEPTH, False) if with_depth else None
    plain = _step(c, t, target, depth, None, scale)
    o = _step(c, t, target, depth, (0.0 if mode == "zero_lambda" else LAMBDA, mode == "value_only"), scale)
    for k in ("ws", "dp", "im", "io", "gi", "gs", "gc") + (("gd", "dpart") if with_depth else ()):
        assert torch.equal(plain[k], o[k]), k
    assert not o["gx"].any()
    l_dist = o["ds"].double().sum().item() / n
    out = _nan(2)
    from laenerf_amd.backend import raymarching_backend as B
    B.loss_finish(o["xpart"], (n + 3) // 4, n, None, out)
    assert l_dist > 0 and out[1].item() == pytest.approx(l_dist, rel=1e-5)          # the partial sums hold sum(l_ray) regardless
    if mode == "zero_lambda":
        assert torch.equal(plain["loss"], o["loss"])
    else:
        assert o["loss"][1].item() == pytest.approx(plain["loss"][1].item() + LAMBDA * l_dist, rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 5
W_TRAIN = 0.1


def _distort_trainer(distort_weight, distort_grad=True, graph=True, depth_weight=None, steps=32):
    """a Trainer on the small synthetic scene of test_gpu_trainer.py (with a random depth plane when depth_weight is given)"""
    from test_gpu_trainer import _setup, _state
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    if depth_weight is not None:
        rng = np.random.default_rng(12)
        plane = rng.uniform(2.0, 4.0, (data.n_img, data.H, data.W)).astype(np.float16)
        plane[rng.random(plane.shape) < 0.3] = 0
        data.set_depths(plane)
    torch.manual_seed(7)
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, graph=graph, capacity="exact", depth_weight=depth_weight,
                 distort_weight=distort_weight, distort_grad=distort_grad).train(steps)
    return tr, _state(r, opt)


@pytest.fixture(scope="module")
def trainer_runs():
    return {"graph": _distort_trainer(W_TRAIN), "eager": _distort_trainer(W_TRAIN, graph=False),
            "value_only": _distort_trainer(W_TRAIN, distort_grad=False), "plain": _distort_trainer(None)}


def test_trainer_with_distortion_graph_equals_eager(trainer_runs):
    from test_gpu_trainer import _assert_same
    (ta, sa), (tb, sb) = trainer_runs["graph"], trainer_runs["eager"]
    assert ta.captures == 1 and tb.captures == 0                     # steps 16-31 were one replayed graph
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses()) and np.array_equal(ta.distort_losses(), tb.distort_losses())
    assert ta.losses().shape == ta.distort_losses().shape == (32,) and np.isfinite(ta.losses()).all() and (ta.distort_losses() > 0).all()
    # and the term trains: the parameters differ from the run without it
    assert any(not torch.equal(x, y) for x, y in zip(sa, trainer_runs["plain"][1]))


def test_trainer_value_only_distortion_is_the_run_without_it(trainer_runs):
    from test_gpu_trainer import _assert_same
    (tv, sv), (tp, sp) = trainer_runs["value_only"], trainer_runs["plain"]
    _assert_same(sv, sp)
    assert tp.distort_losses().size == 0 and (tv.distort_losses() > 0).all()
    mse = tv.losses().astype(np.float64) - W_TRAIN * tv.distort_losses().astype(np.float64)
    print("value-only: total", tv.losses()[-4:], "distortion term", tv.distort_losses()[-4:], "plain", tp.losses()[-4:])
    assert np.allclose(mse, tp.losses(), rtol=1e-5, atol=0)


def test_trainer_with_depth_and_distortion_graph_equals_eager():
    from test_gpu_trainer import _assert_same
    (ta, sa), (tb, sb) = _distort_trainer(W_TRAIN, depth_weight=0.1), _distort_trainer(W_TRAIN, graph=False, depth_weight=0.1)
    assert ta.captures == 1 and tb.captures == 0
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses()) and np.array_equal(ta.distort_losses(), tb.distort_losses())
    assert np.array_equal(ta.depth_losses(), tb.depth_losses())
    assert (ta.distort_losses() > 0).all() and (ta.depth_losses() > 0).all() and np.isfinite(ta.losses()).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def _disc_run(distort_grad, groups=4):
    """a shaded sphere's silhouette over white, seen from 6 poses (the sizes of test_gpu_depth_sup.py's sphere scene), distort_weight 0.5"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    n, H, W = 6, 48, 40
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    poses, intr = S.lookat_poses(n, seed=0), (focal, focal, W / 2, H / 2)
    d = S.sphere_depth_planes(poses, intr, H, W, radius=0.6)
    hit = d > 0
    shade = np.clip(255.0 * (d - d[hit].min()) / (d[hit].max() - d[hit].min()), 0, 255)
    img = np.where(hit[..., None], np.stack([shade, 255 - shade, np.full_like(shade, 64.0)], -1), 255.0).astype(np.uint8)
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    data = ResidentImages.from_arrays(img, poses, intr, bg="white", device=DEV)
    torch.manual_seed(7)
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, capacity="exact", distort_weight=0.5, distort_grad=distort_grad)
    tr.train(16 * groups)
    return tr.distort_losses().reshape(groups, 16).mean(1)


def test_distortion_gradient_lowers_the_distortion():
    """ordering only: with the gradient the term falls, and ends below the value-only run's (DESIGN.md 4g has both sequences)"""
    on, off = _disc_run(True), _disc_run(False)
    print("distortion term per 16-step group, distort_grad=True :", on.tolist())
    print("distortion term per 16-step group, distort_grad=False:", off.tolist())
    assert on[-1] < on[0]
    assert on[-1] < off[-1]
