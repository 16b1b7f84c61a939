"""Patch-based training with an LPIPS term, the parts that need no GPU: the numpy restatement of the patch draw, the float64
restatements of the LPIPS head and of its gradient against torch's float64 autograd, the pack restatement, the C ABI's refusals and
the Trainer's argument refusals."""
import ctypes
import types

import numpy as np
import pytest
import torch

SEED = 0x5EED_1234_ABCD


# ---------------------------------------------------------------------------------------------------------------- draw_patches
def test_draw_patches_bounds_and_layout():
    from laenerf_amd.data import draw_patches
    H, W, P, n_img, n_patch = 33, 40, 32, 3, 64
    for mode in ("image", "all"):
        for step in range(8):
            img, row, col, inds = draw_patches(SEED, step, n_patch, P, n_img, H, W, mode)
            assert img.shape == row.shape == col.shape == (n_patch,) and inds.shape == (n_patch * P * P,)
            assert (row == 0).all()                              # H - P = 1: the only top row is 0
            assert col.min() >= 0 and col.max() <= 7             # W - P = 8, exclusive
            pix = inds % (H * W)
            assert (pix // W).max() == 31 and (pix % W).max() <= 38      # image row 32 and column 39 are never drawn
            assert ((inds // (H * W)) == np.repeat(img, P * P)).all()
            # row-major inside the patch: ray r of patch q is pixel (row + (r % P^2) / P, col + r % P)
            r = np.arange(n_patch * P * P)
            q, rem = r // (P * P), r % (P * P)
            assert np.array_equal(inds, img[q] * H * W + (row[q] + rem // P) * W + (col[q] + rem % P))
            if mode == "image":
                assert len(set(img.tolist())) == 1
    assert len({tuple(draw_patches(SEED, s, 4, P, n_img, H, W, "all")[2]) for s in range(4)}) == 4    # the step changes the draw


def test_draw_patches_image_is_the_plain_samplers():
    from laenerf_amd.data import draw_indices, draw_patches
    for step in (0, 1, 77):
        img = draw_patches(SEED, step, 5, 32, 7, 48, 40, "image")[0]
        assert np.array_equal(img, draw_indices(SEED, step, 5, 7, 48, 40, "image")[0])
        # mode 'all': patch q draws the image ray q of the plain sampler would draw
        img = draw_patches(SEED, step, 5, 32, 7, 48, 40, "all")[0]
        assert np.array_equal(img, draw_indices(SEED, step, 5, 7, 48, 40, "all")[0])


def test_draw_patches_hits_every_row():
    from laenerf_amd.data import draw_patches
    _, row, col, _ = draw_patches(SEED, 3, 10000, 32, 2, 40, 44, "image")      # H - P = 8, W - P = 12
    assert sorted(set(row.tolist())) == list(range(8))
    assert sorted(set(col.tolist())) == list(range(12))


def test_draw_patches_refuses_bad_sizes():
    from laenerf_amd.data import draw_patches
    for P in (1, 33, 40):
        with pytest.raises(ValueError):
            draw_patches(SEED, 0, 1, P, 2, 33, 40)


# ---------------------------------------------------------------------------------------------------------------- the head
SHAPES = [(5, 1), (16, 6), (70, 9)]       # (C, hw) per layer
B = 2


def _feats(rng, zero_pixel=False):
    feats = [np.maximum(rng.standard_normal((2 * B, C, hw)), 0.0) + 0.0 for C, hw in SHAPES]    # exact zeros as after a ReLU
    for f in feats:
        f[:, 0, :] += 0.5                                         # no all-zero pixel
    if zero_pixel:
        feats[1][0, :, 2] = 0.0                                   # pair 0, side 0
        feats[1][3, :, 4] = 0.0                                   # pair 1, side 1
    weights = [rng.random(C) for C, _ in SHAPES]
    return feats, weights


def _torch_head(feats, weights):
    """the lpips formula written with torch operators (lpips' normalize_tensor, NetLinLayer, spatial_average), float64"""
    total = 0
    for f, w in zip(feats, weights):
        f0, f1 = f[0::2], f[1::2]
        n0 = torch.sqrt((f0 * f0).sum(1, keepdim=True))
        n1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
        d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
        total = total + (d * w.view(1, -1, 1)).sum(1).mean(-1)
    return total


# float64 bound for a gradient entry: each of the two reductions behind it adds at most C roundings of 2^-53, relative to the
# largest term; a factor 64 covers the handful of further operations and the cancellation between the expression's two terms,
# whose magnitudes stay within that factor of the largest gradient entry for these features (no near-zero norm)
def _f64_tol(C, ref):
    return 64 * C * 2.0 ** -53 * np.abs(ref).max()


@pytest.mark.parametrize("both", [False, True])
def test_head_restatements_against_torch_float64_autograd(both):
    from laenerf_amd.metrics import lpips_head_grad_numpy, lpips_head_numpy
    rng = np.random.default_rng(5)
    feats, weights = _feats(rng)
    gout = np.array([0.7, -1.3])
    tf = [torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in feats]
    tw = [torch.tensor(w, dtype=torch.float64) for w in weights]
    val = _torch_head(tf, tw)
    got = lpips_head_numpy(feats, weights)
    assert got.shape == (B,) and got.dtype == np.float64
    np.testing.assert_allclose(got, val.detach().numpy(), rtol=64 * 70 * 2.0 ** -53, atol=0)
    (val * torch.tensor(gout)).sum().backward()
    grads = lpips_head_grad_numpy(feats, weights, gout, both=both)
    for (C, _), g, t in zip(SHAPES, grads, tf):
        ref = t.grad.numpy().copy()
        assert g.shape == ref.shape and g.dtype == np.float64
        if not both:
            assert (g[0::2] == 0).all()
            ref[0::2] = 0
        assert np.abs(g - ref).max() <= _f64_tol(C, ref), (C, np.abs(g - ref).max(), _f64_tol(C, ref))


def test_zero_norm_pixels_get_zero_gradient_where_torch_gives_nan():
    from laenerf_amd.metrics import lpips_head_grad_numpy, lpips_head_numpy
    rng = np.random.default_rng(6)
    feats, weights = _feats(rng, zero_pixel=True)
    gout = np.array([1.0, 1.0])
    tf = [torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in feats]
    val = _torch_head(tf, [torch.tensor(w, dtype=torch.float64) for w in weights])
    np.testing.assert_allclose(lpips_head_numpy(feats, weights), val.detach().numpy(), rtol=64 * 70 * 2.0 ** -53)   # the value is fine
    val.sum().backward()
    t = tf[1].grad.numpy()
    assert np.isnan(t[0, :, 2]).all() and np.isnan(t[3, :, 4]).all()              # torch: sqrt'(0) * 0
    g = lpips_head_grad_numpy(feats, weights, gout, both=True)
    assert all(np.isfinite(x).all() for x in g)
    assert (g[1][0, :, 2] == 0).all() and (g[1][3, :, 4] == 0).all()              # the rule: zero on the zero-norm side
    assert np.abs(g[1][1, :, 2]).max() > 0 and np.abs(g[1][2, :, 4]).max() > 0    # the other side of those pixels is computed
    ok = ~np.isnan(t)
    assert np.abs(g[1][ok] - t[ok]).max() <= _f64_tol(16, t[ok])


def test_gradient_agrees_with_a_central_finite_difference():
    from laenerf_amd.metrics import lpips_head_grad_numpy, lpips_head_numpy
    rng = np.random.default_rng(7)
    feats, weights = _feats(rng)
    gout = np.array([0.9, 1.7])
    grads = lpips_head_grad_numpy(feats, weights, gout, both=True)
    # h = 1e-5: the truncation error h^2 f''' / 6 ~ 1e-10 and the rounding error 2^-53 |V| / h ~ 1e-11, both far below 1e-7 of the
    # largest entry; positive features are probed (a ReLU zero sits on no kink of the head, but +h / -h keep it simple)
    h = 1e-5
    for l, (f, g) in enumerate(zip(feats, grads)):
        flat = f.reshape(-1)
        for idx in rng.choice(flat.size, size=12, replace=False):
            old = flat[idx]
            flat[idx] = old + h
            up = (lpips_head_numpy(feats, weights) * gout).sum()
            flat[idx] = old - h
            dn = (lpips_head_numpy(feats, weights) * gout).sum()
            flat[idx] = old
            assert abs((up - dn) / (2 * h) - g.reshape(-1)[idx]) <= 1e-7 * np.abs(g).max(), (l, idx)


# ---------------------------------------------------------------------------------------------------------------- the pack
def test_pack_restatement_equals_eval_views():
    from laenerf_amd.metrics import eval_view_numpy, patch_pack_numpy
    rng = np.random.default_rng(8)
    P = 32
    pred, gt = rng.random((P * P, 3), dtype=np.float32), rng.random((P * P, 3), dtype=np.float32)
    want = eval_view_numpy(pred, gt)["lpips_in"]                   # [2, 3, HW]: gt, pred, normalize=True
    got = patch_pack_numpy(pred, gt, P, normalize=True)
    assert got.shape == (2, 3, P, P) and got.dtype == np.float32
    assert np.array_equal(got.reshape(2, 3, -1).view(np.uint32), want.view(np.uint32))
    # three patches: pair p = images 2p (gt) and 2p + 1 (pred); normalize=False leaves out the 2v - 1
    pred3, gt3 = rng.random((3 * P * P, 3), dtype=np.float32), rng.random((3 * P * P, 3), dtype=np.float32)
    x = patch_pack_numpy(pred3, gt3, P, normalize=False)
    shift, scale = np.float32(-0.088), np.float32(0.448)
    assert x.shape == (6, 3, P, P)
    assert x[3, 1, 5, 7] == (pred3[P * P + 5 * P + 7, 1] - shift) / scale and x[4, 1, 0, 31] == (gt3[2 * P * P + 31, 1] - shift) / scale


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_new_entry_points_refuse_bad_arguments_before_a_launch(hip_lib):
    one = ctypes.c_void_p(16)

    def sample(P, N, H=33, W=40, images=one):
        return hip_lib.lae_sample_train_batch_patch(images, 0, 3, H, W, 4, one, 1.0, 1.0, 1.0, 1.0, N, P, one, 0.2, 0, one, 0, 1, 0, one, one,
                                                    one, one, one, one, one, None)
    assert sample(33, 33 * 33) == -1 and sample(1, 4) == -1 and sample(40, 1600, 64, 40) == -1      # P = H, P = 1, P = W
    assert sample(32, 1000) == -1 and sample(32, 0) == -1                                          # not n_patch * P^2
    assert sample(32, 2048, images=None) == -3
    arr = (ctypes.c_void_p * 1)(16)
    u = lambda v: (ctypes.c_uint32 * 1)(v)
    assert hip_lib.lae_lpips_head_grad(1, arr, arr, u(64), u(4), 0, one, arr, 0, None) == 0         # no pair: nothing to do
    assert hip_lib.lae_lpips_head_grad(1, arr, arr, u(513), u(4), 1, one, arr, 0, None) == -1
    assert hip_lib.lae_lpips_head_grad(6, arr, arr, u(64), u(4), 1, one, arr, 0, None) == -1
    assert hip_lib.lae_lpips_head_grad(1, arr, arr, u(64), u(4), 1, None, arr, 0, None) == -3
    assert hip_lib.lae_patch_pack(one, one, 1, 0, 0, one, None) == -1 and hip_lib.lae_patch_pack(None, one, 1, 32, 0, one, None) == -3
    assert hip_lib.lae_patch_unpack_grad(one, 1, 0, 0, one, None) == -1 and hip_lib.lae_patch_unpack_grad(one, 1, 32, 0, None, None) == -3


# ---------------------------------------------------------------------------------------------------------------- the Trainer
def test_trainer_refuses_patch_arguments_before_touching_the_data():
    from laenerf_amd.metrics import LPIPS
    from laenerf_amd.trainer import Trainer
    lp = LPIPS.random(0)
    renderer = types.SimpleNamespace(fused_post_ops=True)
    data = types.SimpleNamespace(H=64, W=64, n_img=4, error_map=None, gains=None, depths=None, pixel_weights=None, second_target=None)
    before = dict(vars(data))
    new = lambda **kw: Trainer(renderer, None, data, 100, 1e-2, num_rays=2048, **kw)
    with pytest.raises(ValueError, match="max-pool"):
        new(patch_size=16, lpips=lp)
    with pytest.raises(ValueError, match="lpips"):
        new(patch_size=32)
    with pytest.raises(ValueError, match="lpips"):
        new(patch_size=32, lpips=torch.nn.Identity())
    with pytest.raises(ValueError, match="holds no patch"):
        Trainer(renderer, None, data, 100, 1e-2, num_rays=1000, patch_size=32, lpips=lp)
    with pytest.raises(ValueError, match="smaller than the images"):
        new(patch_size=64, lpips=lp)
    with pytest.raises(ValueError, match="perceptual_weight"):
        new(patch_size=32, lpips=lp, perceptual_weight=-1.0)
    with pytest.raises(ValueError, match="patch_headroom"):
        new(patch_size=32, lpips=lp, patch_headroom=0.5)
    for kw in ({"error_map": "ema"}, {"error_map": "fixed"}, {"depth_weight": 0.1}, {"distort_weight": 0.01}, {"opacity_weight": 0.01},
               {"pixel_weights": True}, {"second_weight": 0.5}, {"pose_refine": True}, {"exposure_refine": True}):
        with pytest.raises(ValueError, match="cannot be combined with " + next(iter(kw))):
            new(patch_size=32, lpips=lp, **kw)
    assert vars(data) == before
