"""The colour criteria (mse / l1 / huber / mape) and the opacity-entropy term of the fused training step: the CRIT flavour of
k_composite_train_step through lae_composite_rays_train_step with its criterion term, its two small siblings (lae_colour_loss_forward,
lae_error_map_update_crit) and the Trainer's loss / opacity_weight.  Kernel cases: the hand-built table of depth_sup_util (passes of 64
samples, early stops in the first and second pass and at lane 63, an empty and a dropped ray, a tail of unowned rows, N no multiple of
the 4 rays of a workgroup), every output buffer poisoned with NaN.  The fp64 restatements are pinned by test_criterion_cpu.py.

Entropy tolerance (test_entropy_*): the error of the same float32 expression in numpy against float64, at the kernel's own weights_sum,
times 4 (the device's log2 may be a few ulp off where numpy's is not).  Measured on the case (MI355X): numpy's error 4.90e-8 on h
(h <= 1) and 4.08e-5 on grad_ws (weight 0.5, N = 13, scale 1024: |grad_ws| up to 562), hence the bounds 1.96e-7 and 1.63e-4; the
device's errors were 7.93e-8 and 4.08e-5.  The test prints all six."""
import numpy as np
import pytest
import torch

from depth_sup_util import T_THRESH, build_case
from gpu_util import DEV, N as NP, T
from test_criterion_cpu import DELTA, KINDS, W_OPAC
from test_distort_cpu import LAMBDA

pytestmark = pytest.mark.gpu

LAMBDA_DEPTH, SCALE = 0.37, 1024.0
BG = (1.0, 1.0, 1.0)
KIND_CODE = {"mse": 0, "l1": 1, "huber": 2, "mape": 3}


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


def _plane(c):
    """a per-ray fp32 depth plane with unsupervised rays (zeros)"""
    z = np.random.default_rng(5).uniform(0.5, 3.0, c["N"]).astype(np.float32)
    z[::4] = 0.0
    return T(z)


def _step(c, t, target, depth=None, dist=None, scale=None, bg_rays=True, crit=None):
    """depth: None or (src, lambda, value_only); dist: None or (lambda, value_only); crit: None (the entries before this one) or
    (kind name, None or (lambda, value_only))"""
    from laenerf_amd.backend import raymarching_backend as B
    M, n = c["M"], c["N"]
    o = dict(ws=_nan(n), dp=_nan(n), im=_nan(n, 3), do=_nan(n), io=_nan(n, 3), gi=_nan(n, 3), gs=_nan(M), gc=_nan(M, 3), loss=_nan(2),
             part=_nan((n + 3) // 4))
    depth_sup = dist_sup = crit_sup = None
    if depth is not None:
        o["gd"], o["dpart"] = _nan(n), _nan((n + 3) // 4)
        depth_sup = (depth[0], None, depth[1], depth[2], o["gd"], o["dpart"])
    if dist is not None:
        o["ds"], o["gx"], o["xpart"] = _nan(n), _nan(n), _nan((n + 3) // 4)
        dist_sup = (dist[0], dist[1], o["ds"], o["gx"], o["xpart"])
    if crit is not None:
        opac_sup = None
        if crit[1] is not None:
            o["op"], o["gw"], o["opart"] = _nan(n), _nan(n), _nan((n + 3) // 4)
            opac_sup = (crit[1][0], crit[1][1], o["op"], o["gw"], o["opart"])
        crit_sup = (KIND_CODE[crit[0]], DELTA, opac_sup)
    B.composite_rays_train_step(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"],
                                t["bg_rays"] if bg_rays else None, BG, t["rows_end"], target, scale, o["ws"], o["dp"], o["im"],
                                o["do"], o["io"], o["gi"], o["gs"], o["gc"], o["loss"], o["part"], depth_sup=depth_sup, dist_sup=dist_sup,
                                crit=crit_sup)
    for k, v in o.items():
        assert torch.isfinite(v).all(), k                  # every output row is written
    return o


def _target(n):
    return torch.rand(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))


def _finish(parts, n_elem):
    from laenerf_amd.backend import raymarching_backend as B
    out = _nan(2)
    B.loss_finish(parts, parts.numel(), n_elem, None, out)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("bg_rays", [True, False])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("with_dist", [False, True])
@pytest.mark.parametrize("with_depth", [False, True])
def test_mse_without_the_term_is_the_old_step(case, with_depth, with_dist, scaled, bg_rays):
    """every output of the step with the criterion term (LAE_LOSS_MSE, opac == NULL) against the step without it, the distortion weight 0
    in the cases without distortion -- and there also without the distortion term against the kernels without DIST"""
    c, t = case
    target = _target(c["N"])
    scale = torch.tensor([SCALE], device=DEV) if scaled else None
    depth = (_plane(c), LAMBDA_DEPTH, False) if with_depth else None
    dist = (LAMBDA if with_dist else 0.0, False)
    old = _step(c, t, target, depth, dist, scale, bg_rays)
    new = _step(c, t, target, depth, dist, scale, bg_rays, crit=("mse", None))
    assert old.keys() == new.keys()
    for k in old:
        assert torch.equal(old[k], new[k]), k
    if not with_dist:
        plain = _step(c, t, target, depth, None, scale, bg_rays)
        lean = _step(c, t, target, depth, None, scale, bg_rays, crit=("mse", None))
        assert plain.keys() == lean.keys()
        for k in plain:
            assert torch.equal(plain[k], lean[k]), k


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("mode", ["zero_lambda", "value_only"])
def test_term_off_paths_give_the_step_without_the_term(case, mode, with_depth):
    c, t = case
    n = c["N"]
    target = _target(n)
    scale = torch.tensor([SCALE], device=DEV)
    depth = (_plane(c), LAMBDA_DEPTH, False) if with_depth else None
    plain = _step(c, t, target, depth, (LAMBDA, False), scale)
    o = _step(c, t, target, depth, (LAMBDA, False), scale, crit=("mse", (0.0 if mode == "zero_lambda" else W_OPAC, mode == "value_only")))
    for k in ("ws", "dp", "im", "io", "do", "gi", "gs", "gc", "ds", "gx", "xpart") + (("gd", "dpart") if with_depth else ()):
        assert torch.equal(plain[k], o[k]), k
    assert not o["gw"].any()
    l_op = o["op"].double().sum().item() / n
    assert l_op > 0 and _finish(o["opart"], n)[1].item() == pytest.approx(l_op, rel=1e-5)    # the partial sums hold sum(h) regardless
    if mode == "zero_lambda":
        assert torch.equal(plain["loss"], o["loss"]) and torch.equal(plain["part"], o["part"])
    else:
        assert o["loss"][1].item() == pytest.approx(plain["loss"][1].item() + W_OPAC * l_op, rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def colour_case(case):
    """the MSE call on a first target, and the target of the colour tests built from its blended image: one ray's target is its own
    image_out row (e == 0 on three elements), one ray's is black (the MAPE floor), the rest uniform in [0, 1]"""
    c, t = case
    n = c["N"]
    first = _step(c, t, _target(n), scale=torch.tensor([SCALE], device=DEV))
    target = _target(n).clone()
    target[4] = first["io"][4]
    target[7] = 0.0
    mse = _step(c, t, target, scale=torch.tensor([SCALE], device=DEV))
    return target, mse


@pytest.mark.parametrize("kind", ["l1", "huber", "mape"])
def test_colour_loss_in_the_fused_step(case, colour_case, kind):
    from laenerf_amd.backend import raymarching_backend as B
    from laenerf_amd.raymarching.raymarching import colour_loss_numpy
    c, t = case
    M, n = c["M"], c["N"]
    target, mse = colour_case
    scale = torch.tensor([SCALE], device=DEV)
    o = _step(c, t, target, scale=scale, crit=(kind, None))
    for k in ("ws", "dp", "im", "io", "do"):                                        # the forward is untouched
        assert torch.equal(o[k], mse[k]), k
    # what the targets were built to hold
    e32 = NP(o["io"] - target)
    assert e32.dtype == np.float32 and (e32[4] == 0).all() and (e32 == 0).sum() == 3
    assert (np.abs(e32) > np.float32(DELTA)).any() and ((np.abs(e32) < np.float32(DELTA)) & (e32 != 0)).any()
    assert (NP(target) == 0).sum() >= 3
    assert not torch.equal(o["gi"], mse["gi"]) and not torch.equal(o["gs"], mse["gs"])
    # grad_image: e in float32 (the kernel's branch), the rest in float64
    v, dv = colour_loss_numpy(e32, NP(target), kind, DELTA)
    want = (dv * (1.0 / (3 * n))) * SCALE
    assert np.allclose(NP(o["gi"]).astype(np.float64), want, rtol=1e-6, atol=0)
    assert not NP(o["gi"])[4].any()                                                 # sign(0) = 0
    # the sample gradients: the backward fed the call's own grad_image
    gs, gc = _nan(M), _nan(M, 3)
    B.composite_rays_train_backward_blend(None, o["gi"], t["sigmas"], t["rgbs"], t["deltas"], t["rays"], o["ws"], o["im"], M, n, T_THRESH,
                                          t["bg_rays"], BG, t["rows_end"], gs, gc)
    assert torch.equal(gs, o["gs"]) and torch.equal(gc, o["gc"])
    mean = v.mean()
    print(f"{kind}: loss {o['loss'][1].item():.6e}, float64 mean {mean:.6e}, mse {mse['loss'][1].item():.6e}")
    assert o["loss"][1].item() == pytest.approx(mean, rel=1e-5)
    assert o["loss"][0].item() == pytest.approx(SCALE * o["loss"][1].item(), rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------- 3
def _regimes(ws):
    lo, hi = np.float32(1e-5), np.float32(1) - np.float32(1e-5)
    return ws < lo, ws > hi, (ws > lo) & (ws < hi)


@pytest.mark.parametrize("with_depth_and_dist", [False, True])
def test_entropy_value_gradient_and_the_two_launches(case, with_depth_and_dist):
    from laenerf_amd.backend import raymarching_backend as B
    from laenerf_amd.raymarching.raymarching import opacity_entropy_numpy
    c, t = case
    M, n = c["M"], c["N"]
    target = _target(n)
    scale = torch.tensor([SCALE], device=DEV)
    depth = (_plane(c), LAMBDA_DEPTH, False) if with_depth_and_dist else None
    dist = (LAMBDA, False) if with_depth_and_dist else None
    o = _step(c, t, target, depth, dist, scale, crit=("mse", (W_OPAC, False)))
    plain = _step(c, t, target, depth, dist, scale)
    ws = NP(o["ws"])
    below, above, inside = _regimes(ws)
    assert below.sum() >= 1 and above.sum() >= 1 and inside.sum() >= 4 and below.sum() + above.sum() + inside.sum() == n
    assert ws[int(c["rays"][0, 0])] == 0 and c["rays"][0, 2] == 0                   # the ray without samples
    gw = NP(o["gw"])
    assert not gw[below | above].any() and gw[inside].all()
    # tolerance: 4 x the error of the same float32 expression in numpy against float64, on these inputs
    h64, d64 = opacity_entropy_numpy(ws)
    h32, d32 = opacity_entropy_numpy(ws, dtype=np.float32)
    f32 = np.float32
    g64 = ((W_OPAC / n) * d64) * SCALE
    g32 = ((f32(W_OPAC) / f32(n)) * d32) * f32(SCALE)
    tol_h, tol_g = 4 * np.abs(h32.astype(np.float64) - h64).max(), 4 * np.abs(g32.astype(np.float64) - g64)[inside].max()
    err_h = np.abs(NP(o["op"]).astype(np.float64) - h64).max()
    err_g = np.abs(gw.astype(np.float64) - g64)[inside].max()
    print(f"entropy: numpy float32 error h {tol_h / 4:.3e}, grad_ws {tol_g / 4:.3e}; bounds {tol_h:.3e}, {tol_g:.3e}; device error h "
          f"{err_h:.3e}, grad_ws {err_g:.3e}; max h {h64.max():.3e}, max |grad_ws| {np.abs(g64).max():.3e}")
    assert tol_h > 0 and tol_g > 0 and err_h <= tol_h and err_g <= tol_g
    # the fused call = forward + backward fed (grad_ws, grad_image [, grad_depth, grad_dist])
    gs, gc = _nan(M), _nan(M, 3)
    if with_depth_and_dist:
        B.composite_rays_train_backward_blend_dist(o["gw"], o["gi"], o["gd"], o["gx"], t["sigmas"], t["rgbs"], t["deltas"], t["rays"], o["ws"],
                                                   o["dp"], o["ds"], o["im"], M, n, T_THRESH, t["bg_rays"], BG, t["rows_end"], gs, gc)
    else:
        fw = [_nan(n), _nan(n), _nan(n, 3), _nan(n), _nan(n, 3)]
        B.composite_rays_train_forward_blend(t["sigmas"], t["rgbs"], t["deltas"], t["rays"], M, n, T_THRESH, t["nears"], t["fars"], t["bg_rays"],
                                             BG, *fw)
        for a, b in zip(fw, (o["ws"], o["dp"], o["im"], o["do"], o["io"])):
            assert torch.equal(a, b)
        B.composite_rays_train_backward_blend(o["gw"], o["gi"], t["sigmas"], t["rgbs"], t["deltas"], t["rays"], fw[0], fw[2], M, n, T_THRESH,
                                              t["bg_rays"], BG, t["rows_end"], gs, gc)
    assert torch.equal(gs, o["gs"]) and torch.equal(gc, o["gc"])
    for k_ in ("ws", "dp", "im", "io", "do", "gi", "gc"):                            # the term touches the densities' gradient alone
        assert torch.equal(o[k_], plain[k_]), k_
    assert not torch.equal(o["gs"], plain["gs"])
    # the value
    l_op = h64.sum() / n
    assert _finish(o["opart"], n)[1].item() == pytest.approx(l_op, rel=1e-5)
    assert o["loss"][1].item() == pytest.approx(plain["loss"][1].item() + W_OPAC * l_op, rel=1e-5)
    assert o["loss"][0].item() == pytest.approx(SCALE * o["loss"][1].item(), rel=1e-6)
    mse = ((o["io"].double() - target.double()) ** 2).mean().item()
    assert W_OPAC * l_op > 0.05 * mse                                               # the term is no rounding-level part


def test_entropy_with_huber_against_the_fp64_restatement(case):
    """the whole call against composite_train_step_numpy: the kernel family's bound on grad_sigmas (rtol 1e-4, atol 3e-5,
    test_gpu_depth_sup.py, set for incoming gradients of magnitude 1) times max(1, the largest incoming gradient) -- grad_ws enters the
    bracket as one more constant beside the colour gradient's"""
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    c, t = case
    target = _target(c["N"])
    o = _step(c, t, target, crit=("huber", (W_OPAC, False)))
    ref = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], NP(target), T_THRESH, bg=c["bg_rays"], loss="huber",
                                     huber_delta=DELTA, opacity_weight=W_OPAC)
    r = np.abs(ref["image_out"] - NP(target))
    assert np.abs(r - np.float32(DELTA)).min() > 1e-5                               # no element sits on Huber's knee: fp32 and fp64 branch alike
    atol = 3e-5 * max(1.0, float(np.abs(ref["grad_ws"]).max()), float(np.abs(ref["grad_image"]).max()))
    err = np.abs(NP(o["gs"]).astype(np.float64) - ref["grad_sigmas"]).max()
    print(f"huber + entropy: grad_sigmas max abs error {err:.3e}, atol {atol:.3e}, max |grad| {np.abs(ref['grad_sigmas']).max():.3e}")
    assert np.allclose(NP(o["gs"]), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    assert np.allclose(NP(o["gc"]), ref["grad_rgbs"], rtol=1e-5, atol=1e-6)
    assert o["loss"][1].item() == pytest.approx(float(ref["loss"]), rel=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [39, 4097])
@pytest.mark.parametrize("kind", KINDS)
def test_colour_loss_forward(kind, n):
    from laenerf_amd import _lib, build
    from laenerf_amd.backend import raymarching_backend as B
    from laenerf_amd.raymarching.raymarching import colour_loss_numpy
    build.build()
    g = torch.Generator(device=DEV).manual_seed(n)
    pred, target = torch.rand(n, device=DEV, generator=g), torch.rand(n, device=DEV, generator=g)
    target[::7] = 0.0
    pred[3::11] = target[3::11]
    scale = torch.tensor([SCALE], device=DEV)
    out, grad = _nan(2), _nan(n)
    B.colour_loss_forward(pred, target, n, KIND_CODE[kind], DELTA, scale, out, grad)
    assert torch.isfinite(grad).all() and torch.isfinite(out).all()
    e32 = NP(pred - target)
    v, dv = colour_loss_numpy(e32, NP(target), kind, DELTA)
    assert out[1].item() == pytest.approx(v.mean(), rel=1e-5) and out[0].item() == pytest.approx(SCALE * out[1].item(), rel=1e-6)
    assert np.allclose(NP(grad).astype(np.float64), (dv * (1.0 / n)) * SCALE, rtol=1e-6, atol=0)
    if kind == "mse":
        out0, grad0 = _nan(2), _nan(n)
        _lib.check(_lib.load().lae_mse_loss_forward(pred.data_ptr(), target.data_ptr(), n, scale.data_ptr(), out0.data_ptr(), grad0.data_ptr(),
                                                    _lib.stream()), "mse_loss_forward")
        assert torch.equal(out, out0) and torch.equal(grad, grad0)
    else:
        from laenerf_amd.losses import colour_loss_scaled
        p = pred.clone().requires_grad_()
        loss = colour_loss_scaled(p, target, scale, kind, DELTA)
        loss.backward()
        assert torch.equal(loss.detach(), out[0]) and torch.equal(loss.unscaled, out[1]) and torch.equal(p.grad, grad)


def test_error_map_update_crit():
    from laenerf_amd import _lib, build
    from laenerf_amd.backend import raymarching_backend as B
    from laenerf_amd.data import ema_update
    build.build()
    n, n_img, H, W = 13, 2, 8, 8
    rng = np.random.default_rng(9)
    pred, gt = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)
    gt[2] = 0.0
    pred[5] = gt[5]
    inds = (rng.integers(0, n_img, n) * H * W + rng.integers(0, H * W, n)).astype(np.int64)
    cells = rng.permutation(16384)[:n].astype(np.int32)
    inds[3] = n_img * H * W + 1                                                      # an image out of range
    cells[8] = 16384                                                                 # a cell out of range
    ok = np.ones(n, bool); ok[[3, 8]] = False
    before = rng.uniform(0, 1, (n_img, 16384)).astype(np.float32)
    tp, tg, ti, tc = T(pred), T(gt), T(inds), T(cells)

    def run(kind):
        m = T(before)
        B.error_map_update(m, n_img, H, W, ti, tc, tp, tg, n, kind=KIND_CODE[kind], param=DELTA)
        return m

    old = T(before)
    _lib.check(_lib.load().lae_error_map_update(old.data_ptr(), n_img, H, W, ti.data_ptr(), tc.data_ptr(), tp.data_ptr(), tg.data_ptr(), n,
                                                _lib.stream()), "error_map_update")
    assert torch.equal(run("mse"), old)
    for kind in ("huber", "l1", "mape"):
        got = NP(run(kind))
        want = ema_update(before, inds[ok], cells[ok], pred[ok], gt[ok], H, W, loss=kind, huber_delta=DELTA)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kind       # skipped rows included: nothing else changed
        assert (got != before).sum() == ok.sum() and not np.array_equal(got, NP(old))


# ---------------------------------------------------------------------------------------------------------------- 5
W_TRAIN = 0.05


def _trainer(graph=True, steps=32, depth_weight=None, **kw):
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
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, graph=graph, capacity="exact", depth_weight=depth_weight, **kw).train(steps)
    return tr, _state(r, opt)


@pytest.fixture(scope="module")
def plain_run():
    return _trainer()


def _assert_graph_equals_eager(kw, terms):
    from test_gpu_trainer import _assert_same
    (ta, sa), (tb, sb) = _trainer(**kw), _trainer(graph=False, **kw)
    assert ta.captures == 1 and tb.captures == 0                     # steps 16-31 were one replayed graph
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses()) and ta.losses().shape == (32,) and np.isfinite(ta.losses()).all()
    for name in terms:
        a, b = getattr(ta, name)(), getattr(tb, name)()
        assert np.array_equal(a, b) and a.shape == (32,) and (a > 0).all(), name
    return ta, sa


def test_trainer_with_huber_graph_equals_eager(plain_run):
    ta, sa = _assert_graph_equals_eager(dict(loss="huber"), ())
    assert ta.opacity_losses().size == 0
    assert any(not torch.equal(x, y) for x, y in zip(sa, plain_run[1])) and not np.array_equal(ta.losses(), plain_run[0].losses())


def test_trainer_with_entropy_graph_equals_eager(plain_run):
    ta, sa = _assert_graph_equals_eager(dict(opacity_weight=W_TRAIN), ("opacity_losses",))
    assert any(not torch.equal(x, y) for x, y in zip(sa, plain_run[1]))


def test_trainer_with_every_term_graph_equals_eager():
    _assert_graph_equals_eager(dict(loss="huber", opacity_weight=W_TRAIN, depth_weight=0.1, distort_weight=0.1),
                               ("opacity_losses", "depth_losses", "distort_losses"))


def test_trainer_mse_spelled_out_is_the_default(plain_run):
    from test_gpu_trainer import _assert_same
    tm, sm = _trainer(loss="mse", huber_delta=0.3, opacity_grad=False)
    _assert_same(sm, plain_run[1])
    assert np.array_equal(tm.losses(), plain_run[0].losses()) and tm.opacity_losses().size == 0


def test_trainer_value_only_entropy_is_the_run_without_it(plain_run):
    from test_gpu_trainer import _assert_same
    tv, sv = _trainer(opacity_weight=W_TRAIN, opacity_grad=False)
    tp, sp = plain_run
    _assert_same(sv, sp)
    assert tp.opacity_losses().size == 0 and tv.opacity_losses().shape == (32,) and (tv.opacity_losses() > 0).all()
    mse = tv.losses().astype(np.float64) - W_TRAIN * tv.opacity_losses().astype(np.float64)
    assert np.allclose(mse, tp.losses(), rtol=1e-5, atol=0)


def test_error_map_follows_the_criterion():
    """one eager step with error_map='ema': the map after a Huber step equals the numpy restatement on the step's own image and batch,
    and differs from the MSE step's"""
    from laenerf_amd.data import ema_update
    maps = {}
    for kind in ("huber", "mse"):
        from test_gpu_trainer import _setup
        from laenerf_amd.trainer import Trainer
        r, opt, data = _setup()
        torch.manual_seed(7)
        tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, graph=False, capacity="exact", error_map="ema", loss=kind)
        seen = {}
        inner = data.update_error_map

        def spy(pred, batch, **kw):
            seen.update(before=data.error_map.clone(), pred=pred.detach().float().clone(), kw=kw,
                        batch={k: batch[k].clone() for k in ("inds", "cells", "gt")})
            return inner(pred, batch, **kw)

        data.update_error_map = spy
        tr.train(1)
        assert seen["kw"] == {"loss": kind, "huber_delta": 0.1}
        b = seen["batch"]
        want = ema_update(NP(seen["before"]), NP(b["inds"]), NP(b["cells"]), NP(seen["pred"]), NP(b["gt"]), data.H, data.W, loss=kind,
                          huber_delta=0.1)
        maps[kind] = NP(data.error_map)
        assert np.array_equal(maps[kind].view(np.uint32), want.view(np.uint32)), kind
        assert (maps[kind] != NP(seen["before"])).sum() > 1000
    assert not np.array_equal(maps["huber"], maps["mse"])


def test_resume_with_huber_and_entropy_continues_bit_for_bit(tmp_path):
    import checkpoint_util as U
    from laenerf_amd.trainer import Trainer
    kw = dict(loss="huber", opacity_weight=W_TRAIN)

    def make(net_seed, torch_seed, seed):
        r, opt, data = U.setup(net_seed)
        torch.manual_seed(torch_seed)
        return Trainer(r, opt, data, U.ITERS, U.LR, num_rays=U.RAYS, seed=seed, graph=True, capacity="bucket", **kw)

    full = make(0, 7, 1).train(32)
    want = U.snapshot(full)
    first = make(0, 7, 1).train(16)
    path = first.save_checkpoint(str(tmp_path / "run.pth"))
    cfg = torch.load(path, weights_only=True)["laenerf_amd"]["config"]
    assert cfg["loss"] == "huber" and cfg["huber_delta"] == 0.1 and cfg["opacity_weight"] == W_TRAIN and cfg["opacity_grad"] is True
    resumed = make(1234, 4321, 99)
    resumed.load_checkpoint(path)
    resumed.train(16)
    U.assert_same_state(want, resumed)
    U.assert_same_tail(full, resumed, 16)
    assert np.array_equal(resumed.opacity_losses(), full.opacity_losses()[-16:]) and resumed.opacity_losses().shape == (16,)
    # a default trainer refuses the file under strict_config, naming the keys
    with pytest.raises(ValueError, match="loss"):
        U.fresh_for_resume().load_checkpoint(path)


# ---------------------------------------------------------------------------------------------------------------- 6
def _haze_run(opacity_grad, groups=4):
    """test_gpu_distort.py's shaded sphere over white, opacity_weight 0.05"""
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
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, capacity="exact", opacity_weight=0.05, opacity_grad=opacity_grad)
    tr.train(16 * groups)
    return tr.opacity_losses().reshape(groups, 16).mean(1)


def test_entropy_gradient_lowers_the_entropy():
    """ordering only: after the same groups the mean entropy with the gradient lies below the value-only run's"""
    on, off = _haze_run(True), _haze_run(False)
    print("opacity entropy per 16-step group, opacity_grad=True :", on.tolist())
    print("opacity entropy per 16-step group, opacity_grad=False:", off.tolist())
    assert on[-1] < off[-1]


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("opacity_weight", [None, W_TRAIN])
def test_shade_train_without_fused_post_ops_states_the_same_criterion(opacity_weight):
    """the operator-by-operator path (colour_loss_scaled on the blended image, the entropy with torch operators) against the fused
    kernel on the same samples: the same sums in another order, to the 2e-6 relative test_gpu_e2e.py allows the MSE for that; the
    entropy's log2 differs by a few ulp between the two, far below it at this weight"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(5)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    net.encoder.embeddings.data.uniform_(-0.3, 0.3)
    r = NeRFRenderer(net, bound=1).to(DEV)
    r.density_bitfield = T(S.pack_bits_np(S.sphere_density_grid(), 10.0))
    o, d = S.lego_like_rays(500, seed=6)
    gt = torch.rand(500, 3, device=DEV)
    scale = torch.tensor([512.0], device=DEV)
    net.train()
    out = []
    for fused in (True, False):
        r.fused_post_ops = fused
        net.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            marched = r.march_train(T(o), T(d), perturb=False)
            res = r.shade_train(marched, bg_color=1, gt=gt, scaler=scale, loss="huber", huber_delta=DELTA, opacity_weight=opacity_weight)
        res["loss"].backward()
        g = net.encoder.embeddings.grad
        assert torch.isfinite(g).all() and g.abs().sum().item() > 0
        out.append((res["loss"].item(), res["loss"].unscaled.item(), res["image"].detach().clone(), g.clone()))
    (l1, u1, i1, g1), (l0, u0, i0, g0) = out
    want = torch.nn.functional.huber_loss(i1, gt, delta=DELTA).item() / DELTA
    if opacity_weight is None:
        assert u1 == pytest.approx(want, rel=1e-5)
    else:
        assert u1 > want
    assert u0 == pytest.approx(u1, rel=2e-6) and l0 == pytest.approx(l1, rel=2e-6) and l1 == pytest.approx(512.0 * u1, rel=1e-6)
    assert torch.allclose(i0, i1, rtol=1e-5, atol=1e-6)
    cos = torch.nn.functional.cosine_similarity(g0.float().flatten(), g1.float().flatten(), dim=0).item()
    print(f"unfused against fused, opacity {opacity_weight}: loss {u0:.6e} / {u1:.6e}, cosine of the table gradients {cos:.6f}")
    assert cos > 0.99                                      # the same direction; the fp16 backward keeps the two from being bit-equal
