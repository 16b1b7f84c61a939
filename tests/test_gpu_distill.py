"""-m gpu: LAENeRF's distillation stage (laenerf_amd.editing.distill; nerf/gui.py:357-541, 1420-1430, 1935-1990): the compose and seed
kernels against their numpy restatements bit for bit and against the reference's half-precision chain / torch's interpolate, the
pixels the rewrite must not touch, graph replay with a new edit, the grid rule that lets the stage reuse Trainer, and the whole stage
end to end (fit -> edit grid -> extraction -> palette network -> distillation)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, N, T

pytestmark = pytest.mark.gpu


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def rows_case(seed, n_img=4, H=40, W=48, C=3, P=8, mask=0xff, K=(700, 333, 1000), thresh=0.5, clamp_all=False):
    """rows of len(K) views on images 0, 1, 3 (image 2 occluded), random logits / offsets / edit / weights (some exactly at the
    threshold), distance weights on a third of the rows"""
    rng = np.random.default_rng(seed)
    view_img = [0, 1, 3][:len(K)]
    img, pix, w = [], [], []
    for v, k in zip(view_img, K):
        img.append(np.full(k, v, np.int32))
        pix.append(np.sort(rng.choice(H * W, size=k, replace=False)).astype(np.int32))
        wv = rng.random(k).astype(np.float32)
        wv[: k // 10] = np.float32(thresh)
        w.append(wv)
    R = sum(K)
    n_active = bin(mask & ((1 << P) - 1)).count("1")
    Rp = (R + 15) // 16 * 16
    dist = np.zeros(R, np.float32)
    ii = rng.choice(R, size=R // 3, replace=False)
    dist[ii] = rng.random(ii.size).astype(np.float32)
    c = dict(images=rng.random((n_img, H, W, C)).astype(np.float32), img_idx=np.concatenate(img), pix=np.concatenate(pix),
             w=np.concatenate(w), pred=(rng.random((R, 3)) * 0.9).astype(np.float32),
             w_logits=(rng.standard_normal((Rp, 16)) * 3).astype(np.float16), o_raw=(rng.standard_normal((Rp, 16)) * 0.7).astype(np.float16),
             active_mask=mask & ((1 << P) - 1), P=P, palette_mod=rng.random((n_active, 3)).astype(np.float32),
             palette_og=rng.random((n_active, 3)).astype(np.float32), p_weights=(rng.random(n_active) * 2).astype(np.float32),
             p_bias=(rng.standard_normal(n_active) * 0.2).astype(np.float32), dist=dist, K=list(K), view_img=view_img, H=H, W=W)
    if clamp_all:
        c["p_bias"] = np.full(n_active, -10.0, np.float32)                # every edited weight clamps to 0: sum(w') == 0
    return c


def device_set(c, x_term=None, dirs=None):
    from laenerf_amd.editing import DistillSet
    R = c["w"].size
    x_term = torch.zeros(R, 3) if x_term is None else x_term
    dirs = torch.zeros(R, 3) if dirs is None else dirs
    return DistillSet(torch.from_numpy(c["img_idx"]), torch.from_numpy(c["pix"]), torch.from_numpy(c["w"]), torch.from_numpy(c["pred"]),
                      x_term, dirs, torch.from_numpy(c["dist"]), c["K"], c["view_img"], [2], c["images"].shape[0], device=DEV)


def fake_enc(c):
    return SimpleNamespace(num_color_bases=c["P"], _active_mask=c["active_mask"])


def kernel(c, images, smooth=False, no_bg=False, palette=None):
    from laenerf_amd.editing.distill import compose_launch
    s = device_set(c)
    compose_launch(s, T(c["w_logits"]), T(c["o_raw"]), fake_enc(c), T(c["palette_mod"]) if palette is None else palette, T(c["palette_og"]),
                   T(c["p_weights"]), T(c["p_bias"]), images, 0.5, no_bg, s.dist if smooth else None)
    return images


def numpy_rule(c, images, smooth=False, no_bg=False):
    from laenerf_amd.editing import compose_distill_numpy
    return compose_distill_numpy(images, c["img_idx"], c["pix"], c["w"], c["pred"], c["w_logits"], c["o_raw"], c["active_mask"],
                                 c["palette_mod"], c["p_weights"], c["p_bias"], blend_thresh=0.5, no_bg=no_bg,
                                 dist=c["dist"] if smooth else None, palette_og=c["palette_og"] if smooth else None)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("smooth,no_bg", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("mask,clamp_all", [(0xff, False), (0b10110101, False), (0xff, True)])
def test_compose_equals_compose_distill_numpy(dtype, C, smooth, no_bg, mask, clamp_all):
    c = rows_case(int(C + 2 * smooth + 4 * no_bg + mask % 7), C=C, mask=mask, clamp_all=clamp_all)
    base = c["images"].astype(dtype)
    got = N(kernel(c, T(base.copy()), smooth, no_bg)) if dtype == np.float32 else kernel(c, T(base.copy()), smooth, no_bg).cpu().numpy()
    want = numpy_rule(c, base, smooth, no_bg)
    assert got.dtype == want.dtype == dtype
    assert np.array_equal(got.view(np.uint32 if dtype == np.float32 else np.uint16), want.view(np.uint32 if dtype == np.float32 else np.uint16))
    assert np.isfinite(got).all()


# The kernel against the reference's half-precision chain (gui.py:433-469: softmax / tanh outputs in fp16, the normalised weights
# and the palette cast to fp16 for the product, fp16 sums).  The difference is fp16 rounding of values in [0, 1]: half an ulp at 1
# is 2.4e-4, a product over 8 bases and the offset add accumulate a few of them.  Measured once on the MI355X: 9.05e-4 (max over
# the cases below); the bound is 2e-3.
REF_HALF_MEASURED = 9.05e-4
REF_HALF_TOL = 2e-3


def reference_half_chain(c, images, smooth):
    """gui.py:433-469 with the reference's dtypes, per view, on the device"""
    out = images.clone()
    n_img, H, W, C = out.shape
    cols = [j for j in range(16) if (c["active_mask"] >> j) & 1]
    pm, po = T(c["palette_mod"]), T(c["palette_og"])
    pw, pb = T(c["p_weights"])[None], T(c["p_bias"])[None]
    r0 = 0
    for v, k in zip(c["view_img"], c["K"]):
        sl = slice(r0, r0 + k)
        idx = T(c["pix"][sl]).long()
        weights_og = torch.softmax(T(c["w_logits"][sl])[:, cols], -1)                 # fp16, as tcnn's output under the softmax
        offsets = torch.tanh(T(c["o_raw"][sl])[:, :3])
        weights = torch.clamp_min(pb + pw * weights_og, 0)
        weights /= weights.sum(-1)[..., None].half()
        pred_colors = torch.clamp(offsets.half() + weights.half() @ pm.half(), 0, 1)
        if smooth:
            ii = torch.nonzero(T(c["dist"][sl]) != 0, as_tuple=True)[0]
            dw = T(c["dist"][sl])[ii]
            palet_interp = dw[..., None, None] * po[None, ...] + (1 - dw[..., None, None]) * pm[None, ...]
            weight_interp = weights_og[ii] * dw[..., None] + weights[ii] * (1 - dw[..., None])
            pred_colors[ii] = torch.clamp(torch.einsum("bi,bik->bk", weight_interp.half(), palet_interp.half()) + offsets[ii], 0, 1)
        w8s = torch.zeros(H * W, 1, device=DEV)
        w8s[idx, 0] = T(c["w"][sl])
        style = torch.zeros(H * W, 3, device=DEV)
        style[idx] = pred_colors.float()
        pred_img = torch.zeros(H * W, 3, device=DEV)
        pred_img[idx] = T(c["pred"][sl])
        style = (1 - w8s) * pred_img + w8s * style
        mask = w8s <= 0.5
        gt = out[v].reshape(H * W, C)[:, :3]
        out[v].reshape(H * W, C)[:, :3] = torch.clamp(~mask * style + mask * gt, 0, 1)
        r0 += k
    return out


def test_compose_is_close_to_the_reference_half_chain():
    worst = 0.0
    for seed, smooth, mask in ((1, False, 0xff), (2, True, 0xff), (3, False, 0b10110101), (4, True, 0b01101110)):
        c = rows_case(seed, mask=mask)
        got = kernel(c, T(c["images"].copy()), smooth)
        want = reference_half_chain(c, T(c["images"]), smooth)
        worst = max(worst, (got - want).abs().max().item())
    print("distill compose vs the reference's half chain: max |diff|", worst)
    assert worst <= REF_HALF_TOL


def style_encoder(P=8, seed=3):
    from laenerf_amd.editing import LAENeRF
    torch.manual_seed(seed)
    m = LAENeRF(SimpleNamespace(bound=1, num_palette_bases=P, style_weight=0), dir_encoding="sphere_harmonics").to(DEV)
    m.encoder.embeddings.data.uniform_(-1.0, 1.0)
    return m


def network_case(seed, C=4, u8=True):
    """rows_case on a real palette network: rows with points and directions, ResidentImages of uint8 (or fp32) images"""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd import synthetic as S
    c = rows_case(seed, C=C)
    g = torch.Generator().manual_seed(seed)
    R = c["w"].size
    x = (torch.rand(R, 3, generator=g) - 0.5) * 0.8
    d = F.normalize(torch.randn(R, 3, generator=g), dim=-1)
    s = device_set(c, x, d)
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, size=c["images"].shape, dtype=np.uint8) if u8 else c["images"]
    data = ResidentImages.from_arrays(imgs, S.lookat_poses(imgs.shape[0], seed=seed), (50.0, 50.0, c["W"] / 2, c["H"] / 2), device=DEV)
    return c, s, data


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_distill_images_touches_only_edit_pixels(dtype):
    from laenerf_amd.editing import distill_images
    from laenerf_amd.editing.distill import _network_outputs
    c, s, data = network_case(5)
    enc = style_encoder()
    before = data.images.clone()
    g = torch.Generator(device=DEV).manual_seed(1)
    pal = torch.rand(8, 3, device=DEV, generator=g)
    out = distill_images(data, enc, s, palette=pal, dtype=dtype)
    assert torch.equal(data.images, before)                               # the caller's images are untouched
    assert out is not data and out.images.dtype == dtype and out.images.shape == data.images.shape
    assert out.mode == data.mode and out.bg == data.bg and out.color_space == data.color_space and torch.equal(out.poses, data.poses)
    assert out.intrinsics == data.intrinsics and out.bound == data.bound and out.error_map is None
    base = (before.float() / 255).to(dtype)                               # uint8 -> value / 255 in fp32 -> dtype
    wl, ol = _network_outputs(enc, s.x_term, s.dirs)
    want = numpy_rule(dict(c, w_logits=wl.cpu().numpy(), o_raw=ol.cpu().numpy(), palette_mod=pal.cpu().numpy(),
                           p_weights=np.ones(8, np.float32), p_bias=np.zeros(8, np.float32)), base.cpu().numpy())
    got = out.images.cpu().numpy()
    assert np.array_equal(got.view(np.uint16 if dtype == torch.float16 else np.uint32),
                          want.view(np.uint16 if dtype == torch.float16 else np.uint32))
    written = torch.zeros(data.n_img, data.H * data.W, dtype=torch.bool, device=DEV)
    sel = s.w > 0.5
    written[s.img_idx[sel].long(), s.pix[sel].long()] = True
    flat_out, flat_in = out.images.reshape(data.n_img, -1, 4), base.reshape(data.n_img, -1, 4)
    assert torch.equal(bits(flat_out[~written]), bits(flat_in[~written]))    # at or below the threshold, off the rows: bit-identical
    assert torch.equal(bits(out.images[..., 3]), bits(base[..., 3]))        # alpha: bit-identical
    assert not torch.equal(flat_out[written], flat_in[written])
    with pytest.raises(ValueError):
        distill_images(data, enc, s, dtype=torch.uint8)


def test_error_map_seed_equals_numpy_and_torch_interpolate():
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.editing import distill_images, error_map_seed_numpy
    for H, W in ((40, 48), (96, 96), (200, 130)):
        c = rows_case(H, H=H, W=W, C=3, K=(H * W // 3, H * W // 5, 2 * H * W // 3))
        g = torch.Generator().manual_seed(H)
        s = device_set(c, torch.rand(c["w"].size, 3, generator=g) - 0.5, F.normalize(torch.randn(c["w"].size, 3, generator=g), dim=-1))
        data = ResidentImages.from_arrays(c["images"], S.lookat_poses(4, seed=1), (50.0, 50.0, W / 2, H / 2), device=DEV)
        out = distill_images(data, style_encoder(), s, error_maps=True)
        em = out.error_map.cpu().numpy()
        assert em.shape == (4, 16384)
        assert (em[2] == 1.0).all()                                        # the occluded view keeps its ones
        dense = np.zeros((4, H * W), np.float32)
        dense[c["img_idx"], c["pix"]] = c["w"]
        for v in c["view_img"]:
            want = error_map_seed_numpy(dense[v].reshape(H, W))
            assert np.array_equal(em[v].view(np.uint32), want.view(np.uint32)), (H, W, v)
            ref = torch.clamp(F.interpolate(torch.from_numpy(dense[v].reshape(H, W))[None, None], (128, 128), mode="bilinear",
                                            align_corners=False) + 15e-2, 0, 1)
            np.testing.assert_allclose(em[v], ref.flatten().numpy(), rtol=0, atol=1e-6)


def test_compose_replays_from_a_graph_with_a_new_palette():
    from laenerf_amd.editing.distill import compose_launch
    c = rows_case(21, C=4)
    s = device_set(c)
    args = (T(c["w_logits"]), T(c["o_raw"]), fake_enc(c))
    pal, og, pw, pb = T(c["palette_mod"].copy()), T(c["palette_og"]), T(c["p_weights"]), T(c["p_bias"])
    base = T(c["images"].astype(np.float16))
    buf = base.clone()
    launch = lambda images: compose_launch(s, *args, pal, og, pw, pb, images, 0.5, False, s.dist)
    launch(buf)                                                           # warm-up
    first = buf.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(buf)
    pal.copy_(T(np.random.default_rng(3).random(c["palette_mod"].shape).astype(np.float32)))
    buf.copy_(base)
    g.replay()
    eager = base.clone()
    launch(eager)                                                         # the new palette, eagerly
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(eager))
    assert not torch.equal(bits(eager), bits(first))


def test_second_mark_untrained_grid_with_the_same_poses_is_a_no_op():
    """what lets distill_nerf hand the fitted renderer to a new Trainer: its first call marks the grid again from the same poses"""
    import importlib
    tl = importlib.import_module("tools.train_loop")
    images, poses, intr = tl.teacher_views(torch.device(DEV), 8, 64, 64)
    tr = tl.make_trainer(torch.device(DEV), images, poses, intr, iters=96)
    tr.train(96)
    grid = tr.r.density_grid.clone()
    assert bool((grid > 0).any())
    tr.r.mark_untrained_grid(tr.data.poses, tr.data.intrinsics)
    assert torch.equal(bits(tr.r.density_grid), bits(grid))


# End to end, measured once on the MI355X (calibration run): PSNR of the distilled NeRF against the distilled images 46.69 dB; over
# the 7939 edit pixels the mean |render - distilled target| is 0.0137 against 0.0449 for |render - original image| (ratio 0.31:
# one base of eight moved to its complement changes an edit pixel by ~0.045 per channel); PSNR outside the region 49.33 dB after the
# distillation against 62.08 dB before.  The drop is the learning rate's restart at 1e-2 on a converged fit (the reference's new
# LambdaLR does the same): 49 dB is an RMS error of 0.0034.  Bars: 4 dB under the PSNR, a ratio of 0.5, 16 dB of drop and 44 dB.
E2E_PSNR_MEASURED = 46.69
E2E_EDIT_RATIO_MEASURED = 0.31
E2E_OUTSIDE_MEASURED = (62.08, 49.33)


def render_views(r, data, views):
    out = []
    r.model.eval()
    with torch.no_grad():
        for i in views:
            o, d, img = data.view_rays(int(i))
            with torch.autocast("cuda", dtype=torch.float16):
                pred = r.render_eval(o, d, bg_color=1.0, image_hw=(data.H, data.W))["image"]
            gt = img[:, :3] * img[:, 3:] + (1 - img[:, 3:]) if img.shape[-1] == 4 else img
            out.append((pred.float().reshape(-1, 3), gt))
    r.model.train()
    return out


def masked_psnr(pairs, masks):
    se = sum(float((((p - g) ** 2).sum(-1) * m).sum()) for (p, g), m in zip(pairs, masks))
    n = sum(float(m.sum()) * 3 for m in masks)
    return -10 * np.log10(se / n)


def test_distill_an_edit_into_the_nerf_end_to_end():
    import importlib
    from laenerf_amd import raymarching
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.editing import DistillSet, EditSet, StyleTrainer, distill_nerf, extract_views
    from laenerf_amd.editing.distill import _network_outputs
    from test_gpu_style_train import make_model
    tl = importlib.import_module("tools.train_loop")
    dev = torch.device(DEV)
    images, poses, intr = tl.teacher_views(dev, 16, 96, 96)
    tr = tl.make_trainer(dev, images, poses, intr, iters=768)
    tr.train(768)
    r, data = tr.r, tr.data
    # edit grid: the occupied cells of the x >= 0 half-space
    coords = raymarching.morton3D_invert(torch.arange(128 ** 3, dtype=torch.int32, device=dev))
    half = (coords[:, 0] >= 64).float()[None].expand(r.cascade, -1).contiguous()
    edit = r.density_bitfield & raymarching.packbits(half, 0.5)
    r.eval()
    imgs_f = data.images.float() / 255
    views, occluded = extract_views(r, data.poses, data.intrinsics, data.H, data.W, edit, imgs_f)
    r.train()
    assert len(views) >= 8
    es = EditSet.from_views(views, device=DEV)
    enc, params = make_model(seed=21, spread=1e-4)
    StyleTrainer(enc, es, params, iters=256, distill_palette_steps=-1, seed=0).train(256)
    # a strong edit: the base with the largest mean weight over the rows moved to its complement
    ds = DistillSet.from_views(views, occluded, data.n_img, device=DEV)
    wl, _ = _network_outputs(enc, ds.x_term, ds.dirs)
    k = int(torch.softmax(wl[:ds.R, :8].float(), -1).mean(0).argmax())
    pal = enc.color_palette.detach().clone()
    pal[k] = 1 - pal[k]
    masks_edit = []
    for i in range(data.n_img):
        m = torch.zeros(data.H * data.W, device=dev)
        sel = (ds.img_idx == i) & (ds.w > 0.5)
        m[ds.pix[sel].long()] = 1
        masks_edit.append(m)
    view_ids = list(range(data.n_img))
    before = render_views(r, data, view_ids)
    psnr_out_before = masked_psnr(before, [1 - m for m in masks_edit])
    distilled, tr2 = distill_nerf(r, tr.opt, data, enc, views, occluded, steps=288, lr=1e-2, error_maps=True, palette=pal)
    assert tr2.global_step == 304 and np.isfinite(tr2.losses()).all()
    assert distilled.error_map is not None and not bool((distilled.error_map == 1).all())
    psnr = tr2.evaluate(view_ids, data=distilled, bg_color=1.0)
    after = render_views(r, distilled, view_ids)
    orig = render_views(r, ResidentImages.from_arrays(images, poses, intr, device=DEV), view_ids)
    d_target = sum(float(((p - g).abs().sum(-1) * m).sum()) for (p, g), m in zip(after, masks_edit))
    d_orig = sum(float(((p - g).abs().sum(-1) * m).sum()) for (p, _), (_, g), m in zip(after, orig, masks_edit))
    n_edit = sum(float(m.sum()) * 3 for m in masks_edit)
    psnr_out_after = masked_psnr([(p, g) for (p, _), (_, g) in zip(after, orig)], [1 - m for m in masks_edit])
    print(f"distill e2e: PSNR vs distilled {psnr:.2f} dB; edit pixels |render - target| {d_target / n_edit:.4f}, |render - original| "
          f"{d_orig / n_edit:.4f} ({n_edit / 3:.0f} px); outside PSNR {psnr_out_before:.2f} -> {psnr_out_after:.2f} dB; base {k}")
    assert n_edit > 1000
    assert psnr >= E2E_PSNR_MEASURED - 4.0
    assert d_target < 0.5 * d_orig
    assert psnr_out_after >= psnr_out_before - 16.0 and psnr_out_after >= E2E_OUTSIDE_MEASURED[1] - 5.0
