"""The colour criteria and the opacity entropy of the fused training step, as far as no GPU is needed: the float64 restatement
(colour_loss_numpy, opacity_entropy_numpy, composite_train_step_numpy) against the reference's own huber_loss / mape_loss (recorded by
tests/golden/make_golden_criteria.py) and against CPU torch autograd in float64, the Trainer's config() keys, and the argument checks
of every layer."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from depth_sup_util import T_THRESH, build_case
from step_args import null_step

KINDS = ("mse", "l1", "huber", "mape")
DELTA = 0.1
W_OPAC = 0.5                # the weight of the fused-step tests (test_gpu_criterion.py): the term is no rounding-level part of the loss


# ---------------------------------------------------------------------------------------------------------------- 1
def test_restatement_reproduces_the_references_huber_and_mape():
    """the reference ran in float32: 1e-6 relative"""
    from laenerf_amd.raymarching.raymarching import colour_loss_numpy
    g = golden("criteria")
    pred, target = g["pred"], g["target"]
    e32 = pred - target
    assert pred.dtype == np.float32 and 200 <= pred.size <= 1000 and pred.min() >= 0 and pred.max() <= 1 and target.min() >= 0
    assert (e32 == 0).sum() >= 8 and (np.abs(e32) == np.float32(DELTA)).sum() >= 8 and (target == 0).sum() >= 8
    assert (np.abs(e32) > np.float32(DELTA)).sum() >= 50 and (np.abs(e32) < np.float32(DELTA)).sum() >= 50
    assert float(g["delta"]) == DELTA
    e = pred.astype(np.float64) - target.astype(np.float64)
    for name in ("huber", "mape"):
        v, _ = colour_loss_numpy(e, target, name, DELTA)
        nz = g[name] != 0
        print(f"{name}: max relative difference {(np.abs(v - g[name])[nz] / np.abs(g[name][nz])).max():.3e}")
        assert np.allclose(v, g[name], rtol=1e-6, atol=0)
        assert not v[e == 0].any()


def test_element_loss_derivatives_and_sign_of_zero():
    from laenerf_amd.raymarching.raymarching import colour_loss_numpy
    rng = np.random.default_rng(2)
    t = rng.uniform(0, 1, 500)
    e = rng.uniform(-0.5, 0.5, 500)
    e = e[np.abs(np.abs(e) - np.float32(DELTA)) > 1e-4]            # away from Huber's knee, where the one-sided slopes differ
    t = t[:e.size]
    h = 1e-7
    for name in KINDS:
        v, dv = colour_loss_numpy(e, t, name, DELTA)
        fd = (colour_loss_numpy(e + h, t, name, DELTA)[0] - colour_loss_numpy(e - h, t, name, DELTA)[0]) / (2 * h)
        far = np.abs(e) > 2 * h
        assert np.allclose(dv[far], fd[far], rtol=1e-6, atol=1e-8), name
        v0, dv0 = colour_loss_numpy(np.zeros(3), np.array([0.0, 0.5, 1.0]), name, DELTA)
        assert not v0.any() and not dv0.any(), name                  # sign(0) = 0
    with pytest.raises(ValueError):
        colour_loss_numpy(e, t, "l2")


# ---------------------------------------------------------------------------------------------------------------- 2
def _torch_step(c, target, loss, opacity_weight, scale, z=None, depth_weight=0.0):
    """the step written with torch operators in float64 on the CPU -> (loss value, d / d sigmas, d / d rgbs); the forward as
    composite_depth_numpy states it (early stop after the first sample with T_post < T_thresh, that sample included)"""
    from laenerf_amd.raymarching.raymarching import OPAC_LO
    sig = torch.tensor(c["sigmas"], dtype=torch.float64, requires_grad=True)
    col = torch.tensor(c["rgbs"], dtype=torch.float64, requires_grad=True)
    dl = torch.tensor(c["deltas"], dtype=torch.float64)
    N = c["N"]
    ws, img, D = [torch.zeros((), dtype=torch.float64)] * N, [torch.zeros(3, dtype=torch.float64)] * N, [torch.zeros((), dtype=torch.float64)] * N
    for index, off, steps in (tuple(int(v) for v in r) for r in c["rays"]):
        if steps == 0 or off + steps > c["M"]:
            continue
        alpha = 1 - torch.exp(-sig[off:off + steps] * dl[off:off + steps, 0])
        T_post = torch.cumprod(1 - alpha, 0)
        below = (T_post.detach() < T_THRESH).nonzero()
        n = int(below[0]) + 1 if below.numel() else steps
        T_pre = torch.cat([torch.ones(1, dtype=torch.float64), T_post[:n - 1]])
        w = alpha[:n] * T_pre
        t = torch.cumsum(dl[off:off + n, 1], 0)
        ws[index], img[index], D[index] = w.sum(), (w[:, None] * col[off:off + n]).sum(0), (w * t).sum()
    ws, img, D = torch.stack(ws), torch.stack(img), torch.stack(D)
    out = img + (1 - ws)[:, None] * torch.tensor(c["bg_rays"], dtype=torch.float64)
    tgt = torch.tensor(target, dtype=torch.float64)
    d = float(np.float32(DELTA))
    if loss == "mse":
        total = F.mse_loss(out, tgt)
    elif loss == "l1":
        total = F.l1_loss(out, tgt)
    elif loss == "huber":
        total = F.huber_loss(out, tgt, delta=d) / d
    else:
        total = ((out - tgt).abs() / (tgt.abs() + float(np.float32(1e-2)))).mean()
    if z is not None:
        zz, nr = torch.tensor(z, dtype=torch.float64), torch.tensor(c["nears"], dtype=torch.float64)
        total = total + depth_weight * (((D - (zz - nr)) * (zz > 0)) ** 2).mean()
    if opacity_weight is not None:
        lo = float(np.float32(OPAC_LO))
        o = ws.clamp(lo, float(np.float32(1) - np.float32(OPAC_LO)))
        total = total + opacity_weight * (-(o * torch.log2(o) + (1 - o) * torch.log2(1 - o))).mean()
    (total * scale).backward()
    return float(total.detach()), sig.grad.numpy(), col.grad.numpy()


@pytest.mark.parametrize("opacity_weight", [None, W_OPAC])
@pytest.mark.parametrize("loss", KINDS)
def test_restatement_against_torch_autograd_fp64(loss, opacity_weight):
    """value and gradients of composite_train_step_numpy against autograd.  Tolerance: the file's rtol 1e-12 on the value, as
    test_distort_cpu.py compares float64 against float64; on the gradients rtol 1e-12 plus an absolute term, because a sample's
    gradient is a difference of sums over up to 200 samples of magnitude up to the largest gradient G: 200 roundings of 2.2e-16
    relative to G, with the two orders of summation (sequential here, cumprod / cumsum in torch) -> atol = 1e-12 * G."""
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    c = build_case()
    rng = np.random.default_rng(4)
    target = rng.uniform(0, 1, (c["N"], 3))
    target[3] = 0.0
    z = rng.uniform(0.5, 3.0, c["N"]); z[::3] = 0.0
    scale = 8.0
    f = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], target, T_THRESH, bg=c["bg_rays"], z=z, nears=c["nears"],
                                   depth_weight=0.37, scale=scale, loss=loss, huber_delta=DELTA, opacity_weight=opacity_weight)
    value, gs, gc = _torch_step(c, target, loss, opacity_weight, scale, z=z, depth_weight=0.37)
    assert np.isclose(f["loss"], value, rtol=1e-12, atol=0), (f["loss"], value)
    for name, a, b in (("grad_sigmas", f["grad_sigmas"], gs), ("grad_rgbs", f["grad_rgbs"], gc)):
        big = np.abs(b).max()
        err = np.abs(a - b).max()
        print(f"{loss} opacity {opacity_weight} {name}: max abs difference {err:.3e}, largest gradient {big:.3e}")
        assert big > 1e-3 and np.allclose(a, b, rtol=1e-12, atol=1e-12 * big), name
    if loss == "huber":                                     # both branches occur on the blended image
        r = np.abs(f["image_out"] - target)
        assert (r > np.float32(DELTA)).any() and (r < np.float32(DELTA)).any()
    if opacity_weight is not None:
        ws = f["weights_sum"]
        assert (ws < 1e-5).any() and (ws > 1 - 1e-5).any() and ((ws > 1e-5) & (ws < 1 - 1e-5)).sum() >= 4
        assert not f["grad_ws"][(ws < 1e-5) | (ws > 1 - 1e-5)].any() and f["grad_ws"][(ws > 1e-5) & (ws < 1 - 1e-5)].all()
        if loss == "mse":
            assert opacity_weight * f["opac_mean"] > 0.05 * f["colour"]          # the share test_gpu_criterion.py asserts on the device
        assert np.isclose(f["loss"], f["colour"] + 0.37 * f["depth_mse"] + opacity_weight * f["opac_mean"], rtol=1e-14)


def test_restatement_off_paths_and_the_mse_of_the_existing_restatement():
    from laenerf_amd.raymarching.raymarching import composite_distort_numpy, composite_train_step_numpy
    c = build_case()
    target = np.random.default_rng(4).uniform(0, 1, (c["N"], 3))
    args = (c["sigmas"], c["rgbs"], c["deltas"], c["rays"])
    old = composite_distort_numpy(*args, T_THRESH, bg=c["bg_rays"], target=target, distort_weight=0.25, scale=8.0)
    new = composite_train_step_numpy(*args, target, T_THRESH, bg=c["bg_rays"], distort_weight=0.25, scale=8.0)
    assert new["loss"] == old["loss"] and np.array_equal(new["grad_sigmas"], old["grad_sigmas"]) and np.array_equal(new["grad_rgbs"], old["grad_rgbs"])
    assert not new["grad_ws"].any()
    on = composite_train_step_numpy(*args, target, T_THRESH, bg=c["bg_rays"], distort_weight=0.25, scale=8.0, opacity_weight=W_OPAC)
    off = composite_train_step_numpy(*args, target, T_THRESH, bg=c["bg_rays"], distort_weight=0.25, scale=8.0, opacity_weight=W_OPAC,
                                     opacity_grad=False)
    assert off["loss"] == on["loss"] > old["loss"] and np.array_equal(off["grad_sigmas"], old["grad_sigmas"])
    assert np.abs(on["grad_sigmas"] - old["grad_sigmas"]).max() > 1e-3 and np.array_equal(on["grad_rgbs"], old["grad_rgbs"])


def test_ema_update_restates_the_criterion_per_ray():
    from laenerf_amd.data import ema_update
    rng = np.random.default_rng(6)
    pred, gt = rng.uniform(0, 1, (5, 3)).astype(np.float32), rng.uniform(0, 1, (5, 3)).astype(np.float32)
    m = np.ones((2, 16384), np.float32)
    inds, cells = np.array([0, 1, 2, 3, 4]) + 100, np.array([7, 8, 9, 10, 11])
    new = ema_update(m, inds, cells, pred, gt, 10, 10, loss="l1")
    want = np.float32(0.1) + np.float32(0.9) * (np.abs(pred - gt).astype(np.float64).mean(1))
    assert np.allclose(new[1, cells], want, rtol=1e-6) and new.sum() < m.sum()
    assert np.array_equal(ema_update(m, inds, cells, pred, gt, 10, 10), ema_update(m, inds, cells, pred, gt, 10, 10, loss="mse"))


# ---------------------------------------------------------------------------------------------------------------- 3
def _cpu_trainer(**kw):
    """a Trainer over stand-ins: its constructor and config() touch no device"""
    from laenerf_amd.trainer import Trainer
    r = types.SimpleNamespace(fused_post_ops=True, density_grid=torch.zeros(1), aabb_train=torch.zeros(6), min_near=0.2, bound=1,
                              grid_size=128, density_thresh=10.0, density_scale=1)
    opt = types.SimpleNamespace(param_groups=[{}], device_lr=False)
    data = types.SimpleNamespace(error_map=None, n_img=6, H=48, W=40, C=4, mode="image", bg="random", color_space="srgb")
    return Trainer(r, opt, data, 100, 1e-2, **kw)


NEW_KEYS = ("loss", "huber_delta", "opacity_weight", "opacity_grad")


def test_config_carries_the_new_keys_only_off_the_defaults():
    from laenerf_amd.checkpoint import check_config
    default = _cpu_trainer().config()
    assert not any(k in default for k in NEW_KEYS)
    assert not any(k in _cpu_trainer(loss="mse", huber_delta=0.3, opacity_grad=False).config() for k in NEW_KEYS)
    # a file written before these arguments existed has none of the keys: no difference for a default trainer, in either direction
    before = {k: v for k, v in default.items()}
    assert check_config(before, _cpu_trainer().config()) == []
    huber = _cpu_trainer(loss="huber").config()
    assert huber["loss"] == "huber" and huber["huber_delta"] == 0.1 and "opacity_weight" not in huber
    assert [n for n, _, _ in check_config(before, huber)] == ["huber_delta", "loss"]
    assert check_config(huber, _cpu_trainer(loss="huber", huber_delta=0.1).config()) == []
    assert [n for n, _, _ in check_config(huber, _cpu_trainer(loss="huber", huber_delta=0.2).config())] == ["huber_delta"]
    l1 = _cpu_trainer(loss="l1").config()
    assert l1["loss"] == "l1" and "huber_delta" not in l1
    op = _cpu_trainer(opacity_weight=0.01, opacity_grad=False).config()
    assert op["opacity_weight"] == 0.01 and op["opacity_grad"] is False and "loss" not in op
    assert [n for n, _, _ in check_config(default, op)] == ["opacity_grad", "opacity_weight"]


# ---------------------------------------------------------------------------------------------------------------- 4
BAD_WEIGHTS = [-1.0, float("inf"), float("nan")]
BAD_DELTAS = [0.0, -0.1, float("inf"), float("nan")]


def test_library_entries_refuse_invalid_arguments_before_any_launch(hip_lib):
    step, colour, emap = hip_lib.lae_composite_rays_train_step, hip_lib.lae_colour_loss_forward, hip_lib.lae_error_map_update_crit
    crit = lambda kind=0, delta=0.1, lam=0.1, opac=None: (kind, delta, lam, 0, opac, None, None)   # the criterion term; no depth, no distortion
    assert null_step(step, crit=crit()) == -3                                # NULL pointers
    for kind in (-1, 4):
        assert null_step(step, crit=crit(kind=kind)) == -1
    for d in BAD_DELTAS:
        assert null_step(step, crit=crit(kind=2, delta=d)) == -1
        assert null_step(step, crit=crit(kind=1, delta=d)) == -3             # the parameter is Huber's alone
        assert colour(None, None, 4, 2, d, None, None, None, None) == -3     # NULL comes first there, as in lae_mse_loss_forward
        assert emap(None, 1, 4, 4, None, None, None, None, 4, 2, d, None) == -1
    buf = (torch.zeros(4).data_ptr(),) * 4
    for d in BAD_DELTAS:
        assert colour(buf[0], buf[1], 4, 2, d, None, buf[2], buf[3], None) == -1
    assert colour(buf[0], buf[1], 4, 7, 0.1, None, buf[2], buf[3], None) == -1 and colour(buf[0], buf[1], 0, 0, 0.1, None, buf[2], buf[3], None) == -1
    for w in BAD_WEIGHTS:                                                    # the weight counts only with the term (opac != NULL)
        assert null_step(step, crit=crit(lam=w, opac=buf[0])) == -1
        assert null_step(step, crit=crit(lam=w)) == -3
    assert null_step(step, N=0, crit=crit()) == 0                            # N == 0: nothing to do
    assert null_step(step, N=0, crit=crit(kind=9)) == -1                     # the kind is checked first
    assert emap(None, 1, 4, 4, None, None, None, None, 0, 3, 0.0, None) == 0 and emap(None, 1, 4, 4, None, None, None, None, 4, 3, 0.0, None) == -3


def test_python_layers_refuse_invalid_arguments():
    from laenerf_amd.losses import colour_loss_scaled
    from laenerf_amd.raymarching import raymarching as rm
    for w in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="opacity_weight"):
            rm.composite_rays_train_blend_mse(*([None] * 7), opacity_weight=w)
        with pytest.raises(ValueError, match="opacity_weight"):
            _cpu_trainer(opacity_weight=w)
    for d in BAD_DELTAS:
        with pytest.raises(ValueError, match="huber_delta"):
            rm.composite_rays_train_blend_mse(*([None] * 7), loss="huber", huber_delta=d)
        with pytest.raises(ValueError, match="huber_delta"):
            _cpu_trainer(loss="huber", huber_delta=d)
        with pytest.raises(ValueError, match="huber_delta"):
            colour_loss_scaled(None, None, loss="huber", huber_delta=d)
    for layer in (lambda: rm.composite_rays_train_blend_mse(*([None] * 7), loss="l2"), lambda: _cpu_trainer(loss="l2"),
                  lambda: colour_loss_scaled(None, None, loss="l2")):
        with pytest.raises(ValueError, match="loss must be"):
            layer()
    with pytest.raises(ValueError, match="fused_post_ops"):
        from laenerf_amd.trainer import Trainer
        Trainer(types.SimpleNamespace(fused_post_ops=False), None, types.SimpleNamespace(error_map=None), 100, 1e-2, opacity_weight=0.01)
    with pytest.raises(RuntimeError):
        rm.finish_opacity_loss(types.SimpleNamespace())
    from laenerf_amd.renderer import NeRFRenderer
    with pytest.raises(RuntimeError, match="needs gt"):
        NeRFRenderer.shade_train(types.SimpleNamespace(fused_post_ops=True), None, gt=None, loss="huber")
