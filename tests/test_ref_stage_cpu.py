"""The Ref-NPR second stage's host side (laenerf_amd/editing/ref_stage.py), without a GPU: the colour-patch taps against
F.interpolate, the float64 restatement against the reference's torch lines, the phase gate, the dense scatter of the registration
and every refusal."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from laenerf_amd.editing.ref_stage import (GT, REF, RefEditSet, RefStyleTrainer, pack_ref_arrays, ref_phase, ref_stage_numpy,
                                           reference_ref_terms)
from laenerf_amd.editing.style_trainer import StyleTrainer, image_terms_on
from ref_stage_util import H_REF, W_REF, make_mask, make_ref_view, make_ref_views

U = 2.0 ** -24                              # fp32 unit roundoff


def _bare_view(H, W, seed, border):
    idx = make_mask(H, W, seed, border)
    K = idx.numel()
    return dict(x_term=torch.zeros(K, 3), indices=idx, w8s=torch.ones(K), indices_ray_reg=torch.zeros(0, dtype=torch.long),
                ref_targets=torch.zeros(0, 3), target_weights=torch.zeros(0))


@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("hw", [(70, 83), (32, 48)])
def test_taps_equal_interpolate_of_the_scattered_canvas(hw, border):
    """The taps, applied in float64, against F.interpolate in float64 of the same canvas.  What differs is the fp32 arithmetic of the
    tap weights.  Per axis the source coordinate src = scale * (dst + 0.5) - 0.5 < n_in carries three fp32 roundings (the scale, the
    product, the difference): |d src| <= 3 u n_in.  The bilinear interpolant is continuous and piecewise linear in src with slope
    at most max|canvas| = 1 (also across a change of int(src)), so the two axes move an output by at most 3 u (H + W); l1 = src - i0
    is exact, l0 = 1 - l1, the product ly * lx and the merge of duplicates add one rounding each on weights <= 1 over four taps:
    8 u more."""
    H, W = hw
    view = _bare_view(H, W, 5 + H, border)
    a = pack_ref_arrays([view], (H, W))
    ph, pw = H // 16, W // 16
    assert tuple(a["patch_hw"]) == (ph, pw) and a["tap_row"].shape == (1, ph * pw, 4)
    K = view["indices"].numel()
    vals = torch.rand(K, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    canvas = torch.zeros(H * W, 3, dtype=torch.float64)
    canvas[view["indices"]] = vals
    want = F.interpolate(canvas.view(H, W, 3).permute(2, 0, 1)[None], size=(ph, pw), mode="bilinear", align_corners=False, antialias=False)[0]
    rows, tw = a["tap_row"][0].astype(np.int64), a["tap_w"][0].astype(np.float64)
    got = (tw[..., None] * np.where((rows >= 0)[..., None], vals.numpy()[np.maximum(rows, 0)], 0.0)).sum(1)            # [n_out, 3]
    dev = float(np.abs(got.T.reshape(3, ph, pw) - want.numpy()).max())
    tol = 3 * U * (H + W) + 8 * U
    print(f"{H}x{W} border={border}: max deviation {dev:.3g}, bound {tol:.3g}")
    assert dev <= tol
    # fp32 F.interpolate, the arithmetic the reference runs: the same bound plus its own roundings of the same kind
    want32 = F.interpolate(canvas.float().view(H, W, 3).permute(2, 0, 1)[None], size=(ph, pw), mode="bilinear", align_corners=False, antialias=False)[0]
    assert float(np.abs(got.T.reshape(3, ph, pw) - want32.double().numpy()).max()) <= 2 * tol
    # no row under two outputs; row_tap is the inverse of tap_row
    flat = rows.reshape(-1)
    hit = flat[flat >= 0]
    assert hit.size > 0 and np.unique(hit).size == hit.size
    rt = a["row_tap"]
    assert np.array_equal(np.sort(np.nonzero(rt >= 0)[0]), np.sort(hit)) and np.array_equal(flat[rt[rt >= 0]], np.nonzero(rt >= 0)[0])
    # duplicates merged: no source pixel twice under one output, the weights of every output sum to one
    assert np.abs(tw.sum(1) - 1.0).max() <= 8 * U
    assert (rows < 0).any()                                        # the holes: taps whose source pixel is off the mask
    if border:
        xi, yi = view["indices"] // W, view["indices"] % W
        assert xi.min() == 0 and xi.max() == H - 1 and yi.min() == 0 and yi.max() == W - 1


def test_pack_refuses_an_image_without_a_relu5_grid():
    v = _bare_view(15, 40, 1, True)
    with pytest.raises(ValueError, match="relu5"):
        pack_ref_arrays([v], (15, 40))
    with pytest.raises(ValueError, match="relu5"):
        pack_ref_arrays([_bare_view(40, 15, 1, True)], (40, 15))


def test_dense_scatter_of_the_registration():
    views = make_ref_views(seed=2)                                  # R = 0, R = K, 0 < R < K
    a = pack_ref_arrays(views, (H_REF, W_REF))
    o = 0
    for v, view in enumerate(views):
        K, rows = view["x_term"].shape[0], view["indices_ray_reg"].numpy()
        t, w = a["ref_target"][o:o + K], a["ref_weight"][o:o + K]
        assert a["ref_count"][v] == rows.size
        off = np.setdiff1d(np.arange(K), rows)
        assert not t[off].any() and not w[off].any()
        assert np.array_equal(t[rows], view["ref_targets"].numpy()) and np.array_equal(w[rows], view["target_weights"].numpy())
        assert np.array_equal(a["w8s16"][o:o + K], view["w8s"].numpy().astype(np.float16))
        o += K
    assert a["ref_count"][0] == 0 and a["ref_count"][1] == views[1]["x_term"].shape[0]
    assert not a["ref_weight"][:views[0]["x_term"].shape[0]].any()
    neg = dict(views[2], target_weights=-views[2]["target_weights"])             # clamp_min(target_weights, 0)
    assert not pack_ref_arrays([neg], (H_REF, W_REF))["ref_weight"].any()


@pytest.mark.parametrize("mode", [GT, REF])
def test_restatement_equals_the_reference_lines(mode):
    """ref_stage_numpy (float64) against the reference's torch lines (fp32): a sum of n non-negative fp32 terms of a few roundings
    each deviates by at most about (n + 4) u relatively; 1e-5 covers the 3 K = 13 000 terms here with room"""
    view = make_ref_view(3, reg="some")
    K = view["x_term"].shape[0]
    g = torch.Generator().manual_seed(4)
    cp = torch.rand(3, H_REF // 16, W_REF // 16, generator=g)
    a = pack_ref_arrays([view], (H_REF, W_REF), {"color_patch": cp[None]})
    pred = torch.rand(K, 3, generator=g).half()
    pc, reg, patch = reference_ref_terms(pred, view["w8s"], mode, target=view["targets"], ref_targets=view["ref_targets"],
                                         target_weights=view["target_weights"], indices_ray_reg=view["indices_ray_reg"],
                                         indices=view["indices"], image_hw=(H_REF, W_REF), color_patch=cp)
    r = ref_stage_numpy(pred.numpy(), a["w8s16"], mode, target=view["targets"].numpy(), ref_target=a["ref_target"], ref_weight=a["ref_weight"],
                        R=a["ref_count"][0], tap_row=a["tap_row"][0], tap_w=a["tap_w"][0], color_patch=a["color_patch"][0])
    assert np.array_equal(pc.numpy().view(np.uint16), r["predw"].view(np.uint16))
    assert abs(float(reg) - r["terms"][0]) <= 1e-5 * r["terms"][0]
    if mode == REF:
        assert r["terms"][1] > 0 and abs(float(patch) - r["terms"][1]) <= 1e-5 * r["terms"][1]
    else:
        assert float(patch) == 0.0 and r["terms"][1] == 0.0


def test_restatement_gradient_is_the_derivative_of_its_terms():
    view = make_ref_view(5, H=32, W=48, reg="some")
    K = view["x_term"].shape[0]
    g = torch.Generator().manual_seed(6)
    cp = torch.rand(3, 2, 3, generator=g)
    a = pack_ref_arrays([view], (32, 48), {"color_patch": cp[None]})
    pred = torch.rand(K, 3, generator=g).half()
    for mode in (GT, REF):
        pc = (pred.float() * torch.from_numpy(a["w8s16"]).float()[:, None]).half().double().requires_grad_(True)
        if mode == GT:
            loss = 0.7 * ((pc - view["targets"].double()) ** 2).mean()
        else:
            rows = view["indices_ray_reg"]
            w = torch.clamp_min(view["target_weights"], 0).double()
            canvas = torch.zeros(32 * 48, 3, dtype=torch.float64).index_put((view["indices"],), pc).view(32, 48, 3)
            tw, tr = torch.from_numpy(a["tap_w"][0]).double(), torch.from_numpy(a["tap_row"][0]).long()
            patch = (tw[..., None] * torch.where((tr >= 0)[..., None], pc[tr.clamp_min(0)], torch.zeros((), dtype=torch.float64))).sum(1)
            loss = 0.7 * (((view["ref_targets"].double() - pc[rows]) ** 2) * w[:, None]).mean() + 1.3 * ((patch.T.reshape(3, 2, 3) - cp.double()) ** 2).mean()
            assert canvas.shape == (32, 48, 3)
        loss.backward()
        r = ref_stage_numpy(pred.numpy(), a["w8s16"], mode, target=view["targets"].numpy(), ref_target=a["ref_target"], ref_weight=a["ref_weight"],
                            R=a["ref_count"][0], tap_row=a["tap_row"][0], tap_w=a["tap_w"][0], color_patch=a["color_patch"][0], g_terms=(0.7, 1.3))
        want = pc.grad.numpy() * a["w8s16"].astype(np.float64)[:, None]
        assert np.abs(r["g_pred"] - want).max() <= 1e-12 * np.abs(want).max()


def test_phase_gate_follows_image_terms_on():
    for warm in (-1, 0, 16, 40, 1000):
        for s in list(range(0, 96)) + [1007, 1008, 1023, 1024]:
            assert ref_phase(s, warm) == (REF if image_terms_on(s, warm) else GT)
    assert [ref_phase(s, 16) for s in (0, 16, 31, 32, 63)] == [GT, GT, GT, REF, REF]


def _params(**kw):
    p = dict(weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3, offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2,
             style_weight=0, tv_weight=0, smooth_trans_weight=0, depth_disc_weight=0, intensity_weight=0, mse_loss=6.0, cos_loss_factor=0.0,
             color_patch_loss=0.0, feature_size=32, warmup_iterations=16)
    p.update(kw)
    return SimpleNamespace(**p)


def test_refusals():
    views = make_ref_views(seed=7)
    es = RefEditSet.from_views(views, (H_REF, W_REF), device="cpu")
    assert es.tmpl_z is None and es.ref["w8s16"].dtype == torch.float16 and "smooth" in es.image
    o, K = int(es.offsets_host[2]), int(es.counts_host[2])
    h, w = views[2]["style_guide"].shape
    off = int(es.image_host["img_off"][2])
    assert np.array_equal(es.image_host["smooth"][off:off + h * w].reshape(h, w), (1.0 - views[2]["style_guide"]).numpy())
    enc = object()                                                  # every refusal comes before the network is touched
    for kw, what in ((dict(style_weight=1.0), "style_weight"), (dict(smooth_trans_weight=1e-3), "smooth_trans_weight"),
                     (dict(intensity_weight=0.1), "intensity_weight"), (dict(cos_loss_factor=2.5), "supervision"),
                     (dict(color_patch_loss=30.0), "supervision")):
        with pytest.raises(NotImplementedError, match=what):
            RefStyleTrainer(enc, es, _params(**kw), iters=16)
    P = 64
    sup = {"tmpl_z": torch.zeros(3, 3, P, dtype=torch.int32), "style_feat": torch.rand(3, 8, P), "feature_size": 32,
           "color_patch": torch.rand(3, 3, H_REF // 16, W_REF // 16)}
    es2 = RefEditSet.from_views(views, (H_REF, W_REF), supervision=sup, device="cpu")
    with pytest.raises(NotImplementedError, match="semantic encoder"):
        RefStyleTrainer(enc, es2, _params(cos_loss_factor=2.5), iters=16)
    with pytest.raises(TypeError):
        from laenerf_amd.editing import EditSet
        RefStyleTrainer(enc, EditSet.from_views(views, image_hw=(H_REF, W_REF), device="cpu"), _params(), iters=16)
    bad = dict(sup, tmpl_z=torch.full((3, 3, P), P, dtype=torch.int32))
    with pytest.raises(ValueError, match="tmpl_z"):
        RefEditSet.from_views(views, (H_REF, W_REF), supervision=bad, device="cpu")
    with pytest.raises(NotImplementedError):
        es.save("unused.npz")
    assert RefStyleTrainer._N_TERMS == 6 and StyleTrainer._N_TERMS == 4
