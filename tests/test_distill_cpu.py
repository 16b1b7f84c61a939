"""The dataset rewrite of LAENeRF's distillation stage (include/laenerf.h lae_distill_compose / lae_error_map_seed) as restated by
`compose_distill_numpy` / `error_map_seed_numpy`, against the reference's expressions (nerf/gui.py:419-469 distill_dataset) in
float64 torch and against torch's bilinear interpolate on the CPU; the step count of --train_steps_distill; DistillSet's packing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from laenerf_amd.editing.distill import DistillSet, compose_distill_numpy, distill_steps, error_map_seed_numpy


def case(seed, n_img=3, H=20, W=24, C=3, P=8, mask=0xff, K=(150, 90), thresh=0.5, dtype=np.float32):
    """rows of len(K) views (images 0 and 2 when n_img = 3: image 1 occluded), random logits / offsets / edit, w with values exactly
    at the threshold"""
    rng = np.random.default_rng(seed)
    images = rng.random((n_img, H, W, C)).astype(dtype)
    view_img = [0, 2][:len(K)]
    img, pix, w, pred_full, views = [], [], [], [], []
    for v, k in zip(view_img, K):
        idx = np.sort(rng.choice(H * W, size=k, replace=False))
        wv = rng.random(k).astype(np.float32)
        wv[: k // 10] = np.float32(thresh)                                  # at the threshold: the pixel keeps the ground truth
        pf = (rng.random((H * W, 3)) * 0.9).astype(np.float32)
        img.append(np.full(k, v, np.int32)); pix.append(idx.astype(np.int32)); w.append(wv); pred_full.append(pf)
        views.append((v, idx, wv, pf))
    R = sum(K)
    n_active = bin(mask & ((1 << P) - 1)).count("1")
    d = dict(images=images, img_idx=np.concatenate(img), pix=np.concatenate(pix), w=np.concatenate(w),
             pred=np.concatenate([pf[idx] for _, idx, _, pf in views]),
             w_logits=(rng.standard_normal((R, 16)) * 3).astype(np.float16), o_raw=(rng.standard_normal((R, 16)) * 0.7).astype(np.float16),
             active_mask=mask & ((1 << P) - 1), palette_mod=rng.random((n_active, 3)).astype(np.float32),
             p_weights=(rng.random(n_active) * 2).astype(np.float32), p_bias=(rng.standard_normal(n_active) * 0.2).astype(np.float32),
             palette_og=rng.random((n_active, 3)).astype(np.float32))
    dist = np.zeros(R, np.float32)
    interp = np.sort(rng.choice(R, size=R // 3, replace=False))
    dist[interp] = rng.random(interp.size).astype(np.float32)
    d["dist"], d["views"], d["interp"] = dist, views, interp
    return d


def reference_chain(c, blend_thresh=0.5, no_bg=False, smooth=False):
    """gui.py:433-469 per view in float64 torch (its .half() casts left out: the rule computes in fp32)"""
    out = torch.from_numpy(c["images"].astype(np.float64))
    n_img, H, W, C = out.shape
    cols = [j for j in range(16) if (c["active_mask"] >> j) & 1]
    dd = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    pm, po, pw, pb = dd(c["palette_mod"]), dd(c["palette_og"]), dd(c["p_weights"])[None], dd(c["p_bias"])[None]
    r0 = 0
    for v, idx, wv, pf in c["views"]:
        k = idx.size
        sl = slice(r0, r0 + k)
        weights_og = torch.softmax(torch.from_numpy(c["w_logits"][sl][:, cols].astype(np.float64)), -1)
        offsets = torch.tanh(torch.from_numpy(c["o_raw"][sl][:, :3].astype(np.float64)))
        weights = torch.clamp_min(pb + pw * weights_og, 0)
        weights /= weights.sum(-1)[..., None]
        pred_colors = torch.clamp(offsets + weights @ pm, 0, 1)
        if smooth:
            ii = np.nonzero(np.isin(np.arange(r0, r0 + k), c["interp"]))[0]
            dw = dd(c["dist"][sl][ii])
            palet_interp = dw[..., None, None] * po[None] + (1 - dw[..., None, None]) * pm[None]
            weight_interp = weights_og[ii] * dw[..., None] + weights[ii] * (1 - dw[..., None])
            pred_colors[ii] = torch.clamp(torch.einsum("bi,bik->bk", weight_interp, palet_interp) + offsets[ii], 0, 1)
        w8s = torch.zeros(H * W, 1, dtype=torch.float64)
        w8s[idx, 0] = dd(wv)
        style = torch.zeros(H * W, 3, dtype=torch.float64)
        style[idx] = pred_colors
        style = w8s * style if no_bg else (1 - w8s) * dd(pf) + w8s * style
        mask = w8s <= blend_thresh
        gt = out[v].reshape(H * W, C)[:, :3]
        out[v].reshape(H * W, C)[:, :3] = torch.clamp(~mask * style + mask * gt, 0, 1)
        r0 += k
    return out.numpy()


def compose(c, **kw):
    return compose_distill_numpy(c["images"], c["img_idx"], c["pix"], c["w"], c["pred"], c["w_logits"], c["o_raw"], c["active_mask"],
                                 c["palette_mod"], c["p_weights"], c["p_bias"], **kw)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("no_bg", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("mask", [0xff, 0b10110101])
def test_compose_numpy_equals_the_reference_expressions(C, no_bg, smooth, mask):
    c = case(7 + C + 2 * no_bg + 4 * smooth, C=C, mask=mask)
    got = compose(c, no_bg=no_bg, dist=c["dist"] if smooth else None, palette_og=c["palette_og"] if smooth else None)
    want = reference_chain(c, no_bg=no_bg, smooth=smooth)
    assert got.dtype == np.float32
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=0, atol=1e-6)
    # w == blend_thresh, pixels off the rows, the alpha channel and the occluded image: the input, exactly
    at = c["w"] == np.float32(0.5)
    flat_in, flat_out = c["images"].reshape(3, -1, C), got.reshape(3, -1, C)
    assert np.array_equal(flat_out[c["img_idx"][at], c["pix"][at]], flat_in[c["img_idx"][at], c["pix"][at]])
    assert np.array_equal(got[1], c["images"][1])
    if C == 4:
        assert np.array_equal(got[..., 3], c["images"][..., 3])
    written = np.zeros(flat_in.shape[:2], bool)
    written[c["img_idx"][c["w"] > 0.5], c["pix"][c["w"] > 0.5]] = True
    assert np.array_equal(flat_out[~written], flat_in[~written])
    assert not np.array_equal(flat_out[written], flat_in[written])


def test_compose_numpy_rounds_fp16_images_from_the_fp32_value():
    c = case(3)
    c16 = dict(c, images=c["images"].astype(np.float16))
    got16 = compose(c16)
    got32 = compose(dict(c, images=c16["images"].astype(np.float32)))
    assert got16.dtype == np.float16
    assert np.array_equal(got16, got32.astype(np.float16))


def test_compose_numpy_where_every_edited_weight_clamps_away():
    """sum(w') = 0: the weights count as zero (the reference: 0 / 0 = NaN) -> colour = clamp(o)"""
    c = case(5)
    c["p_bias"] = np.full_like(c["p_bias"], -10.0)
    got = compose(c)
    assert np.isfinite(got).all()
    sel = c["w"] > 0.5
    o = np.tanh(c["o_raw"][sel, :3].astype(np.float32).astype(np.float64)).astype(np.float32)
    wr = c["w"][sel][:, None]
    want = np.clip((np.float32(1) - wr) * c["pred"][sel] + wr * np.clip(np.float32(0) + o, 0, 1), 0, 1)
    assert np.array_equal(got.reshape(3, -1, 3)[c["img_idx"][sel], c["pix"][sel]], want)


@pytest.mark.parametrize("H,W", [(800, 800), (96, 96), (75, 210), (1080, 1920)])
def test_error_map_seed_numpy_equals_torch_interpolate(H, W):
    rng = np.random.default_rng(H + W)
    x = np.zeros((H, W), np.float32)
    m = rng.random((H, W)) < 0.3
    x[m] = rng.random(int(m.sum())).astype(np.float32)
    got = error_map_seed_numpy(x)
    want = torch.clamp(F.interpolate(torch.from_numpy(x)[None, None], (128, 128), mode="bilinear", align_corners=False) + 15e-2, 0, 1)
    assert got.shape == (16384,) and got.dtype == np.float32
    np.testing.assert_allclose(got, want.flatten().numpy(), rtol=0, atol=1e-6)
    many = error_map_seed_numpy(np.stack([x, x[::-1].copy()]))
    assert np.array_equal(many[0], got) and many.shape == (2, 16384)


def test_distill_steps_follow_the_reference_gui():
    assert distill_steps(3000) == 3008
    assert distill_steps(3008) == 3024
    assert distill_steps(0) == 16
    assert distill_steps(15) == 16 and distill_steps(16) == 32


def views_of(c, smooth):
    views = []
    r0 = 0
    for v, idx, wv, pf in c["views"]:
        k = idx.size
        d = dict(pose_idx=v, indices=torch.from_numpy(idx.astype(np.int64)), w8s=torch.from_numpy(wv),
                 pred_imgs=torch.from_numpy(pf), x_term=torch.rand(k, 3), dirs=torch.rand(k, 3))
        if smooth:
            ii = np.nonzero(np.isin(np.arange(r0, r0 + k), c["interp"]))[0]
            d["indices_interp"] = torch.from_numpy(ii)
            d["dist_weights"] = torch.from_numpy(c["dist"][r0 + ii])
        views.append(d)
        r0 += k
    return views


@pytest.mark.parametrize("smooth", [False, True])
def test_distill_set_packs_views(smooth):
    c = case(11)
    views = views_of(c, smooth)
    s = DistillSet.from_views(views, [1], 3, device="cpu")
    assert s.V == 2 and s.R == 240 and s.n_img == 3 and s.occluded == [1]
    assert s.offsets_host.tolist() == [0, 150] and s.counts_host.tolist() == [150, 90] and s.view_img_host.tolist() == [0, 2]
    assert np.array_equal(s.img_idx.numpy(), c["img_idx"]) and np.array_equal(s.pix.numpy(), c["pix"])
    assert np.array_equal(s.w.numpy(), c["w"]) and np.array_equal(s.pred.numpy(), c["pred"])     # pred_imgs[indices]
    assert np.array_equal(s.x_term.numpy(), torch.cat([v["x_term"] for v in views]).numpy())
    if smooth:
        assert np.array_equal(s.dist.numpy(), c["dist"])                  # dist_weights at indices_interp, 0 elsewhere
    else:
        assert s.dist is None
    with pytest.raises(ValueError):                                      # a view whose image is listed as occluded
        DistillSet.from_views(views, [0], 3, device="cpu")
    with pytest.raises(ValueError):                                      # the same image twice
        DistillSet.from_views([views[0], views[0]], [], 3, device="cpu")
    with pytest.raises(ValueError):                                      # an image outside the set
        DistillSet.from_views(views, [], 2, device="cpu")
