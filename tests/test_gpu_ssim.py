"""SSIM on the device: lae_ssim and the two patch kernels against the float64 restatements (metrics.ssim_numpy, ssim_grad_numpy),
evaluate_one_epoch(ssim=True) and the Trainer's D-SSIM term (ssim_weight).

The bounds.  Kernel and restatement compute the same quantities in float64 from the same fp32 inputs; they differ in the order of
the sums, in fused multiply-adds and possibly in the last bit of exp() in the window.  With u = 2^-53 and inputs in [0, 1]:
  * a window sum is two 11-term dot products with non-negative weights that sum to 1.  Each pass is off by at most 12 u (11 additions
    and a product per term), the second also carries the first's error, a product x x, y y or x y adds one rounding, and the weights
    themselves may differ by 2 u relatively: each of the five sums is within 32 u of its exact value on either side, so the two
    sides are within d = 64 u of each other.
  * S = (A1 / B1) (A2 / B2) with |A1| <= B1 and |A2| <= B2.  A1 and B1 move by at most 2 d (mx + my) each, so A1 / B1 moves by at
    most 4 d (mx + my) / B1.  A2 and B2 are sums of two differences `window sum - product of means`, each off by at most 3 d, so each
    moves by at most 6 d and A2 / B2 by at most 12 d / B2.  Forming A, B, the quotients and the product adds a few roundings of
    values <= 1.  Hence |S_kernel - S_restatement| <= d (4 max((mx + my) / B1) + 12 / min B2) + 64 u =: e_S, with the maxima taken
    from the restatement's own terms.  B2 >= C2 = (0.03 L)^2 and (mx + my) / B1 <= 1 / sqrt(2 C1), so for L >= 0.25 this is at
    most 64 u (4 / 3.6e-3 + 12 / 5.6e-5) + 64 u = 1.6e-9 whatever the image; on the near-flat pair under the data rule C2 is tiny and
    min B2, the pair's own variance, is what bounds it.
  * the mean of S is a sum of values |S| <= 1 + e_S in a fixed tree on the device and pairwise in numpy: both within 64 u.
  * the map is S rounded once to fp32: e_S + 2^-24 (|S| + e_S).
  * the gradient.  With k1 = max 1 / B1 and k2 = max 1 / B2 (k1 + k2 >= 1): A1, A2, B1, B2 each move by at most 6 d; then
    Dxy = 2 A1 / (B1 B2) moves by at most 12 d (2 k1 k2 + k2^2), Dxx = -S / B2 by at most 12 d (k1 + k2) k2 + 6 d k2^2 and
    Dm = 2 my (A2 - A1) / (B1 B2) - S (2 mx / B1 - 2 mx / B2) by at most d (26 k1 k2 + 36 (k1 + k2)^2 + 2 (k1 + k2) + 12 (k1^2 + k2^2)):
    each by at most e_D = 64 d (k1 + k2)^2.  A pixel's gradient is (sum w Dm + 2 x sum w Dxx + y sum w Dxy) / N with weights w >= 0
    that sum to at most 1 and x, y <= 1: at most 4 e_D / N, and the 121-term sums add less than another e_D / N.  Times |gout| /
    n_patch, plus the one fp32 rounding of the stored value."""
import numpy as np
import pytest
import torch

import patch_train_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu

u = 2.0 ** -53
d = 64 * u


def _terms(x, y, L):
    from laenerf_amd.metrics import _ssim_terms
    _, _, _, L, A1, A2, B1, B2, mx, my = _ssim_terms(x, y, L)
    return L, B1, B2, mx, my


def _e_S(x, y, L):
    _, B1, B2, mx, my = _terms(x, y, L)
    return d * (4 * ((mx + my) / B1).max() + 12 / B2.min()) + 64 * u


def _e_G(pred, gt, L, gout, P):
    """the float64 bound of a gradient element for a batch of patches [n_patch, P, P, 3] and an upstream gradient gout"""
    n_patch = pred.shape[0]
    k = max((1 / B1).max() + (1 / B2).max() for _, B1, B2, _, _ in (_terms(pred[p], gt[p], L) for p in range(n_patch)))
    return abs(gout) / n_patch * 5 * 64 * d * k * k / (3 * (P - 10) ** 2)


def _inputs(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        x, y = rng.random((H, W, 3)), rng.random((H, W, 3))
    elif kind == "flat":
        x = 0.7 + 1e-3 * (2 * rng.random((H, W, 3)) - 1)
        y = 0.7 + 1e-3 * (2 * rng.random((H, W, 3)) - 1)
    else:
        x = rng.random((H, W, 3))
        y = x
    return x.astype(np.float32), y.astype(np.float32)


def _tile():
    from laenerf_amd.metrics import SSIM_TILE_H, SSIM_TILE_W
    return SSIM_TILE_H, SSIM_TILE_W


def _valid_shapes():
    TH, TW = _tile()
    return [(1, 1), (TH - 1, TW - 1), (TH - 1, TW + 1), (TH, TW), (TH + 1, TW - 1), (TH + 1, TW + 1), (2 * TH + 5, TW + 9)]    # the last: 3 x 2 tiles


@pytest.mark.parametrize("case", range(7))
def test_metric_against_restatement(case):
    from laenerf_amd.metrics import ssim, ssim_numpy, ssim_scratch_doubles
    nh, nw = _valid_shapes()[case]
    H, W = nh + 10, nw + 10
    for kind in ("uniform", "flat", "same"):
        x, y = _inputs(kind, H, W, seed=case * 10 + len(kind))
        tx, ty = torch.from_numpy(x).to(DEV).reshape(-1, 3), torch.from_numpy(y).to(DEV).reshape(-1, 3)
        for L in (None, 1.0, 0.25):
            want, S = ssim_numpy(x, y, L, full=True)
            e_S = _e_S(x, y, L)
            if kind == "uniform" and L is not None:
                assert e_S <= 1.6e-9                                                   # the image-independent form of the bound
            outs = []
            for _ in range(2):
                out = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
                smap = torch.full((nh, nw, 3), float("nan"), dtype=torch.float32, device=DEV)
                scratch = torch.full((ssim_scratch_doubles(H, W),), float("nan"), dtype=torch.float64, device=DEV)
                assert ssim(tx, ty, H, W, data_range=L, out=out, map=smap, scratch=scratch) is out
                outs.append((out.cpu().numpy(), smap.cpu().numpy()))
            (got, gmap), (got2, gmap2) = outs
            assert got.tobytes() == got2.tobytes() and gmap.tobytes() == gmap2.tobytes()        # two calls, the same bits
            err, merr = abs(got[0] - want), np.abs(gmap.astype(np.float64) - S)
            print(f"{H}x{W} {kind} L={L}: ssim {want:.12f} err {err:.3e} bound {e_S + 64 * u:.3e} map err {merr.max():.3e}")
            assert err <= e_S + 64 * u
            assert (merr <= e_S + 2.0 ** -24 * (np.abs(S) + e_S)).all()
            if kind == "same":
                assert abs(got[0] - 1.0) <= e_S + 64 * u
            # without the map and with scratch of its own: the same bits
            assert ssim(tx, ty, H, W, data_range=L).cpu().numpy().tobytes() == got.tobytes()


def test_metric_refusals_and_constant_images():
    from laenerf_amd.metrics import ssim
    x = torch.rand(10 * 40, 3, device=DEV)
    with pytest.raises(ValueError):
        ssim(x, x, 10, 40)
    with pytest.raises(ValueError):
        ssim(x, x, 40, 10)
    a, b = torch.full((13 * 12, 3), 0.3, device=DEV), torch.full((13 * 12, 3), 0.6, device=DEV)
    smap = torch.zeros(3, 2, 3, device=DEV)
    assert torch.isnan(ssim(a, b, 13, 12, map=smap)).all() and torch.isnan(smap).all()       # the data's range is 0: 0 / 0
    assert torch.isfinite(ssim(a, b, 13, 12, data_range=1.0)).all()


def _patch_batch(n_patch, P, seed):
    rng = np.random.default_rng(seed)
    pred = rng.random((n_patch, P, P, 3))
    gt = np.clip(pred + 0.1 * rng.standard_normal(pred.shape), 0, 1)
    return pred.astype(np.float32), gt.astype(np.float32)


@pytest.mark.parametrize("n_patch,P", [(1, 11), (3, 16), (2, 32), (1, 64)])
def test_patch_forward_and_backward_against_restatements(n_patch, P):
    from laenerf_amd import _lib
    from laenerf_amd.metrics import ssim_grad_numpy, ssim_numpy
    pred, gt = _patch_batch(n_patch, P, seed=P)
    tp, tg = torch.from_numpy(pred).to(DEV).reshape(-1, 3), torch.from_numpy(gt).to(DEV).reshape(-1, 3)
    lib = _lib.load()
    for L, gout in ((1.0, -0.37), (0.25, 2.5)):
        want = np.array([ssim_numpy(pred[p], gt[p], L) for p in range(n_patch)])
        e_S = max(_e_S(pred[p], gt[p], L) for p in range(n_patch))
        e_G = _e_G(pred, gt, L, gout, P)
        ref = np.stack([ssim_grad_numpy(pred[p], gt[p], L) for p in range(n_patch)]) * (gout / n_patch)
        g_dev = torch.tensor([gout], dtype=torch.float32, device=DEV)
        ref = ref * (float(g_dev.item()) / gout)                                         # the fp32 scalar the kernel reads
        outs = []
        for _ in range(2):
            per_patch = torch.full((n_patch,), float("nan"), dtype=torch.float64, device=DEV)
            grad = torch.full((n_patch * P * P, 3), float("nan"), dtype=torch.float32, device=DEV)
            _lib.check(lib.lae_ssim_patch_forward(tp.data_ptr(), tg.data_ptr(), n_patch, P, L, per_patch.data_ptr(), _lib.stream()), "fwd")
            _lib.check(lib.lae_ssim_patch_backward(tp.data_ptr(), tg.data_ptr(), n_patch, P, L, g_dev.data_ptr(), grad.data_ptr(),
                                                   _lib.stream()), "bwd")
            outs.append((per_patch.cpu().numpy(), grad.cpu().numpy()))
        (got, ggrad), (got2, ggrad2) = outs
        assert got.tobytes() == got2.tobytes() and ggrad.tobytes() == ggrad2.tobytes()          # two calls, the same bits
        gerr = np.abs(ggrad.astype(np.float64).reshape(ref.shape) - ref)
        print(f"n={n_patch} P={P} L={L}: fwd err {np.abs(got - want).max():.3e} bound {e_S + 64 * u:.3e}; "
              f"grad max {np.abs(ref).max():.3e} err {gerr.max():.3e} fp64 bound {e_G:.3e}")
        assert (np.abs(got - want) <= e_S + 64 * u).all()
        assert np.isfinite(ggrad).all()
        assert (gerr <= e_G + 2.0 ** -24 * (np.abs(ref) + e_G)).all()


def test_ssim_patch_loss_autograd_reaches_pred_only():
    from laenerf_amd.losses import ssim_patch_loss
    from laenerf_amd.metrics import ssim_grad_numpy, ssim_numpy
    n_patch, P = 3, 16
    pred, gt = _patch_batch(n_patch, P, seed=5)
    tp = torch.from_numpy(pred).to(DEV).reshape(-1, 3).requires_grad_(True)
    tg = torch.from_numpy(gt).to(DEV).reshape(-1, 3).requires_grad_(True)
    loss = ssim_patch_loss(tp, tg, P)
    want = np.array([ssim_numpy(pred[p], gt[p], 1.0) for p in range(n_patch)])
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.per_patch.dtype == torch.float64
    e_S = max(_e_S(pred[p], gt[p], 1.0) for p in range(n_patch)) + 64 * u
    assert np.abs(loss.per_patch.cpu().numpy() - want).max() <= e_S
    assert abs(float(loss.detach()) - (1.0 - want.mean())) <= e_S + 2.0 ** -23           # the mean rounded to fp32, then 1 - it
    (3.0 * loss).backward()
    assert tg.grad is None and tp.grad is not None and tp.grad.shape == tp.shape
    ref = -3.0 / n_patch * np.stack([ssim_grad_numpy(pred[p], gt[p], 1.0) for p in range(n_patch)]).reshape(-1, 3)
    e_G = _e_G(pred, gt, 1.0, 3.0, P)
    assert (np.abs(tp.grad.cpu().numpy() - ref) <= e_G + 2.0 ** -24 * (np.abs(ref) + e_G)).all()
    with pytest.raises(ValueError):
        ssim_patch_loss(tp, tg, 10)


# ---------------------------------------------------------------------------------------------------------------- evaluate_one_epoch
def test_evaluate_one_epoch_scores_ssim_and_leaves_the_rest_alone():
    """PSNR, LPIPS and the masked MSE of a call with ssim=True are bit-equal to a call without.  The calls run under torch's request
    for deterministic convolution algorithms: without it two IDENTICAL calls (ssim=False both) differ in LPIPS by up to 3.7e-9 on this
    scene (measured, six calls; the AlexNet trunk's MIOpen convolutions, the effect metrics._deterministic_convs is there for), while
    PSNR is bit-equal either way."""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.metrics import LPIPS, eval_view_numpy, ssim_numpy
    from laenerf_amd.trainer import Trainer
    from test_gpu_trainer import _assert_same, _images, _setup, _state
    H, W = 48, 40
    img, poses, intr = _images(n=3, H=H, W=W, seed=9)
    r, opt, data = _setup()
    torch.manual_seed(8)
    tr = Trainer(r, opt, data, 300, 1e-2, num_rays=4096, seed=3, capacity="exact", ema_decay=0.95)
    tr.train(32)
    test = ResidentImages.from_arrays(img, poses, intr, device=DEV)
    masks = [torch.zeros(H, W, dtype=torch.uint8, device=DEV), None, torch.full((H, W), 255, dtype=torch.uint8, device=DEV)]
    lp = LPIPS.random(0, device=DEV)
    before = _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None]
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        plain = tr.evaluate_one_epoch(test, lpips=lp, masks=masks)
        res = tr.evaluate_one_epoch(test, lpips=lp, masks=masks, ssim=True)
        fixed = tr.evaluate_one_epoch(test, ssim=True, ssim_data_range=1.0)
    finally:
        torch.backends.cudnn.deterministic = was
    _assert_same(before, _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None])      # the weights are restored
    assert plain["ssim"] is None and plain["mean_ssim"] is None
    for key in ("psnr", "lpips", "masked_mse"):
        assert plain[key].tobytes() == res[key].tobytes(), key
    for key in ("mean_psnr", "mean_lpips", "mean_masked_mse"):
        assert plain[key] == res[key], key
    assert res["ssim"].shape == (3,) and res["ssim"].dtype == np.float64 and res["mean_ssim"] == float(np.mean(res["ssim"]))
    with tr._eval_weights():
        preds = [tr._render_view(test, i, scale_depth=False)[0].cpu().numpy() for i in range(3)]
    for i in range(3):
        x = preds[i].reshape(H, W, 3)
        y = eval_view_numpy(preds[i], img[i])["gt"].reshape(H, W, 3)
        for got, L in ((res["ssim"][i], None), (fixed["ssim"][i], 1.0)):
            want = ssim_numpy(x, y, L)
            print(f"view {i} L={L}: ssim {want:.9f} err {abs(got - want):.3e} bound {_e_S(x, y, L) + 64 * u:.3e}")
            assert abs(got - want) <= _e_S(x, y, L) + 64 * u
    with pytest.raises(ValueError, match="ssim_data_range"):
        tr.evaluate_one_epoch(test, ssim=True, ssim_data_range=0.0)


# ---------------------------------------------------------------------------------------------------------------- the Trainer
STEPS, PS = 48, 16


@pytest.fixture(scope="module")
def eager_run():
    """48 eager steps with the D-SSIM term alone (the third group is the one a graph trainer replays, test_gpu_patch_train.py)"""
    tr = U.make_trainer(graph=False, patch_size=PS, lpips=None, ssim_weight=0.2)
    tr.train(STEPS)
    return U.state(tr), tr.losses(), tr.ssim_losses()


def test_graph_ssim_trainer_equals_eager(eager_run):
    state, losses, ds = eager_run
    tg = U.make_trainer(graph=True, patch_size=PS, lpips=None, ssim_weight=0.2)
    tg.train(STEPS)
    U.assert_same(U.state(tg), state)
    assert np.array_equal(tg.losses(), losses) and np.array_equal(tg.ssim_losses(), ds)
    assert ds.shape == (STEPS,) and np.isfinite(ds).all() and (ds >= 0).all() and (ds <= 2).all() and np.isfinite(losses).all()
    assert tg.captures >= 1 and tg.lpips is None and (tg.perceptual_losses() == 0).all()
    assert tg.n_rays == (U.RAYS // (PS * PS)) * PS * PS and tg.config()["ssim_weight"] == 0.2
    print("ssim trainer: D-SSIM first", ds[:4], "last", ds[-4:], "captures", tg.captures, "warm", tg.warm_groups)


def test_saved_and_resumed_ssim_run_equals_the_uninterrupted_one(eager_run, tmp_path):
    state, losses, ds = eager_run
    first = U.make_trainer(graph=True, patch_size=PS, lpips=None, ssim_weight=0.2)
    first.train(16)
    path = first.save_checkpoint(str(tmp_path / "ssim.pth"))
    resumed = U.make_trainer(net_seed=1234, torch_seed=4321, seed=99, graph=True, patch_size=PS, lpips=None, ssim_weight=0.2)
    resumed.load_checkpoint(path)
    resumed.train(STEPS - 16)
    U.assert_same(U.state(resumed), state)
    assert np.array_equal(resumed.losses(), losses[16:]) and np.array_equal(resumed.ssim_losses(), ds[16:])
    other = U.make_trainer(patch_size=PS, lpips=None, ssim_weight=0.3)
    with pytest.raises(ValueError, match="ssim_weight"):
        other.load_checkpoint(path)


def test_both_terms_and_a_trainer_without_ssim_weight_refuses_the_file(tmp_path):
    tr = U.make_trainer(graph=False, ssim_weight=0.2)                   # P = 32, lpips = LPIPS.random(0)
    tr.train(16)
    perc, ds = tr.perceptual_losses(), tr.ssim_losses()
    assert perc.shape == ds.shape == (16,) and (perc > 0).all() and np.isfinite(perc).all()
    assert np.isfinite(ds).all() and (ds >= 0).all() and (ds <= 2).all() and (ds > 0).any()
    path = tr.save_checkpoint(str(tmp_path / "both.pth"))
    plain = U.make_trainer()
    assert "ssim_weight" not in plain.config()
    with pytest.raises(ValueError, match="ssim_weight"):
        plain.load_checkpoint(path)
