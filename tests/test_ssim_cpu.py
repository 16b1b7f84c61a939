"""SSIM, the parts that need no GPU: the float64 restatement against torchmetrics' sequence of steps, its gradient against central
differences, the definition's properties, the C ABI's refusals and the Trainer's argument rules for ssim_weight."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SHAPES = [(11, 11), (12, 27), (40, 21)]


def _pair(rng, H, W):
    x = rng.random((H, W, 3))
    return x, np.clip(x + 0.1 * rng.standard_normal((H, W, 3)), 0, 1)


def _torchmetrics_steps(x, y, data_range):
    """structural_similarity_index_measure(preds, target, data_range=...) with its defaults (gaussian kernel, sigma 1.5, kernel size
    11, k1 0.01, k2 0.03, elementwise mean), step by step as torchmetrics' _ssim_update takes them, in float64: reflect pad by 5, ONE
    grouped conv2d of the five stacked planes with the 2-D window, crop 5 on every side, mean"""
    p = torch.from_numpy(x).permute(2, 0, 1)[None]
    t = torch.from_numpy(y).permute(2, 0, 1)[None]
    if data_range is None:
        data_range = max(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    dist = torch.arange((1 - 11) / 2, (1 + 11) / 2, 1, dtype=torch.float64)          # torchmetrics' _gaussian
    g = torch.exp(-torch.pow(dist / 1.5, 2) / 2)
    g = (g / g.sum())[None]
    kernel = torch.matmul(g.t(), g).expand(3, 1, 11, 11).contiguous()
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    o = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=3)
    mu_p, mu_t = o[0:1], o[1:2]
    s_p, s_t, s_pt = o[2:3] - mu_p * mu_p, o[3:4] - mu_t * mu_t, o[4:5] - mu_p * mu_t
    full = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_p + s_t + c2))
    return float(full[..., 5:-5, 5:-5].reshape(1, -1).mean())


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("data_range", [None, 1.0, 0.25])
def test_restatement_equals_torchmetrics_steps(H, W, data_range):
    from laenerf_amd.metrics import ssim_numpy
    x, y = _pair(np.random.default_rng(H * 100 + W), H, W)
    got, want = ssim_numpy(x, y, data_range), _torchmetrics_steps(x, y, data_range)
    print(H, W, data_range, got, abs(got - want))
    assert abs(got - want) <= 1e-13
    val, S = ssim_numpy(x, y, data_range, full=True)
    assert S.shape == (H - 10, W - 10, 3) and val == float(S.mean())


def test_gradient_restatement_against_central_differences():
    from laenerf_amd.metrics import ssim_grad_numpy, ssim_numpy
    x, y = _pair(np.random.default_rng(3), 13, 12)
    for L in (1.0, 0.25):
        G = ssim_grad_numpy(x, y, L)
        N = np.zeros_like(x)
        h = 1e-6
        for i in np.ndindex(x.shape):
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            N[i] = (ssim_numpy(xp, y, L) - ssim_numpy(xm, y, L)) / (2 * h)
        print(L, np.abs(G).max(), np.abs(G - N).max())
        assert G.shape == x.shape and np.abs(G - N).max() <= 1e-8
    with pytest.raises(ValueError):
        ssim_grad_numpy(x, y, None)


def test_properties():
    from laenerf_amd.metrics import ssim_numpy
    rng = np.random.default_rng(4)
    for H, W in SHAPES:
        x, y = _pair(rng, H, W)
        for L in (None, 1.0):
            assert abs(ssim_numpy(x, x, L) - 1.0) <= 1e-15
            assert ssim_numpy(x, y, L) == ssim_numpy(y, x, L)
            assert ssim_numpy(x, y, L) < 1.0
    for shape in ((10, 11, 3), (11, 10, 3), (3, 40, 3)):
        with pytest.raises(ValueError):
            ssim_numpy(np.zeros(shape), np.zeros(shape))
    assert np.isnan(ssim_numpy(np.full((11, 13, 3), 0.3), np.full((11, 13, 3), 0.6)))      # the data's range is 0: 0 / 0
    assert np.isfinite(ssim_numpy(np.full((11, 13, 3), 0.3), np.full((11, 13, 3), 0.6), 1.0))
    with pytest.raises(ValueError):
        ssim_numpy(x, y, 0.0)


def test_scratch_size_and_tile_constants_follow_the_header(hip_lib):
    import os
    import re
    from conftest import ROOT
    from laenerf_amd import metrics as M
    hdr = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    const = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1))
    assert (M.SSIM_TILE_H, M.SSIM_TILE_W, M.SSIM_MINMAX_BLOCKS) == (const("LAE_SSIM_TILE_H"), const("LAE_SSIM_TILE_W"), const("LAE_SSIM_MINMAX_BLOCKS"))
    hip_lib.lae_ssim_scratch_doubles.restype = ctypes.c_uint64
    for H, W in ((11, 11), (26, 42), (27, 43), (800, 800), (1080, 1920), (5, 5)):
        assert hip_lib.lae_ssim_scratch_doubles(H, W) == M.ssim_scratch_doubles(H, W), (H, W)
    assert "ssim.hip" in __import__("laenerf_amd.build", fromlist=["SOURCES"]).SOURCES


def test_entry_points_refuse_bad_arguments_before_a_launch(hip_lib):
    one = ctypes.c_void_p(16)
    d = ctypes.c_double
    ssim = lambda H=16, W=16, L=1.0, x=one, out=one: hip_lib.lae_ssim(x, one, H, W, d(L), one, out, None, None)
    assert ssim(H=10) == -1 and ssim(W=10) == -1 and ssim(H=40000) == -1 and ssim(L=float("nan")) == -1 and ssim(L=float("inf")) == -1
    assert ssim(x=None) == -3 and ssim(out=None) == -3
    fwd = lambda n=1, P=16, L=1.0, pred=one: hip_lib.lae_ssim_patch_forward(pred, one, n, P, d(L), one, None)
    bwd = lambda n=1, P=16, L=1.0, gout=one: hip_lib.lae_ssim_patch_backward(one, one, n, P, d(L), gout, one, None)
    for f in (fwd, bwd):
        assert f(P=10) == -1 and f(P=4097) == -1 and f(L=0.0) == -1 and f(L=-1.0) == -1 and f(L=float("nan")) == -1 and f(n=70000) == -1
        assert f(n=0) == 0
    assert fwd(pred=None) == -3 and bwd(gout=None) == -3


def test_python_wrappers_refuse_bad_arguments():
    from laenerf_amd.losses import ssim_patch_loss
    from laenerf_amd.metrics import ssim
    x = torch.zeros(12 * 12, 3)
    with pytest.raises(ValueError, match="at least 11"):
        ssim(x, x, 10, 12)
    with pytest.raises(ValueError, match="pred"):
        ssim(x.double(), x, 12, 12)
    with pytest.raises(ValueError, match="gt"):
        ssim(x, x[:100], 12, 12)
    with pytest.raises(ValueError, match="data_range"):
        ssim(x, x, 12, 12, data_range=0.0)
    with pytest.raises(ValueError, match="map"):
        ssim(x, x, 12, 12, map=torch.zeros(5))
    with pytest.raises(ValueError, match="scratch"):
        ssim(x, x, 12, 12, scratch=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="at least 11"):
        ssim_patch_loss(x, x, 10)
    with pytest.raises(ValueError, match="n_patch"):
        ssim_patch_loss(x, x, 11)
    with pytest.raises(ValueError, match="data_range"):
        ssim_patch_loss(x, x, 12, data_range=None)


def test_trainer_argument_rules_for_ssim_weight():
    from laenerf_amd.metrics import LPIPS
    from laenerf_amd.trainer import Trainer
    lp = LPIPS.random(0)
    renderer = types.SimpleNamespace(fused_post_ops=True)
    data = types.SimpleNamespace(H=64, W=64, n_img=4, error_map=None, gains=None, depths=None, pixel_weights=None, second_target=None)
    before = dict(vars(data))
    new = lambda **kw: Trainer(renderer, None, data, 100, 1e-2, num_rays=2048, **kw)
    with pytest.raises(ValueError, match="ssim_weight needs patch_size > 1"):
        new(ssim_weight=0.2)
    with pytest.raises(ValueError, match="patch_size >= 11"):
        new(patch_size=10, ssim_weight=0.2)
    with pytest.raises(ValueError, match="max-pool"):
        new(patch_size=16, ssim_weight=0.2, lpips=lp)                 # with both terms the rule stays P >= 32
    with pytest.raises(ValueError, match="lpips"):
        new(patch_size=32, ssim_weight=0.2, lpips=torch.nn.Identity())
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ssim_weight must be finite"):
            new(patch_size=16, ssim_weight=bad)
    with pytest.raises(ValueError, match="cannot be combined with depth_weight"):
        new(patch_size=16, ssim_weight=0.2, depth_weight=0.1)
    with pytest.raises(ValueError, match="max-pool"):                  # without ssim_weight nothing changed
        new(patch_size=16, lpips=lp)
    with pytest.raises(ValueError, match="lpips"):
        new(patch_size=32)
    assert vars(data) == before
    # P = 16 with lpips=None passes every argument rule: what stops the constructor is the stand-in objects, not a ValueError
    try:
        new(patch_size=16, ssim_weight=0.2)
    except ValueError as e:                                            # pragma: no cover
        pytest.fail(f"patch_size=16 with ssim_weight and lpips=None was refused: {e}")
    except (AttributeError, TypeError):
        pass
