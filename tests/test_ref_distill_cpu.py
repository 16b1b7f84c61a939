"""The data set of the Ref-NPR distillation as far as no GPU is needed: `ref_distill_numpy` (the restatement of lae_ref_distill_init /
lae_ref_distill_scatter) against the reference's dataloader_nerf (editing/single_view_edit_dataset.py:466-513) restated with dense
torch indexing on two tiny views, the row packing and its checks, and the library entries' argument checks."""
import numpy as np
import pytest
import torch

H = W = 8


def tiny_views(seed=0, C=4):
    """two 8 x 8 views of a 3-image set (image 1 has no view): K extracted pixels each, a handful of them registered; one negative
    target weight (clamped), one exact-zero alpha under a registered pixel"""
    rng = np.random.default_rng(seed)
    images = rng.uniform(0, 1, (3, H, W, C)).astype(np.float32)
    if C == 4:
        images[..., 3] = np.where(rng.random((3, H, W)) < 0.3, 0.0, images[..., 3])
    views = []
    for pose, K, R in ((2, 20, 5), (0, 11, 4)):
        idx = np.sort(rng.permutation(H * W)[:K]).astype(np.int64)
        reg = np.sort(rng.permutation(K)[:R]).astype(np.int64)
        tw = rng.uniform(0, 1, R).astype(np.float32)
        tw[0] = -0.25
        if C == 4:
            images[pose].reshape(-1, 4)[idx[reg[1]], 3] = 0.0
        views.append(dict(pose_idx=pose, indices=torch.from_numpy(idx), indices_ray_reg=torch.from_numpy(reg),
                          ref_targets=torch.from_numpy(rng.uniform(0, 1, (R, 3)).astype(np.float32)), target_weights=torch.from_numpy(tw),
                          depths=torch.from_numpy(rng.uniform(1, 4, K).astype(np.float32)),
                          colours=torch.from_numpy(rng.uniform(0, 1, (K, 3)).astype(np.float32))))
    return images, views


def reference_dataloader_nerf(train_image, v):
    """what single_view_edit_dataset.py:466-513 builds for one view, restated with dense torch indexing in its order of operations
    (scatter, then add 1 - alpha); `colours` stands for the network's output.  The reference clamps target_weights where they are made
    (:226, as pack_ref_arrays restates); the clamp is applied here.  -> (target image, weight plane, style image, depth plane)"""
    img = torch.from_numpy(train_image)
    alpha = img[..., -1]
    pix = v["indices"]
    reg_pix = pix[v["indices_ray_reg"]]
    weight = torch.zeros(H * W)
    weight[reg_pix] = v["target_weights"].clamp_min(0)
    weight = weight.view(H, W) + (1 - alpha)
    target = torch.zeros(H * W, img.shape[-1])
    target[:, -1] = alpha.reshape(-1)
    target[reg_pix, :3] = v["ref_targets"]
    style = torch.zeros(H * W, img.shape[-1])
    style[pix, -1] = alpha.reshape(-1)[pix]
    style[pix, :3] = v["colours"].float()
    depth = torch.zeros(H * W)
    depth[pix] = v["depths"]
    return target.view(H, W, -1).numpy(), weight.numpy(), style.view(H, W, -1).numpy(), depth.view(H, W).numpy()


def _packed(views, n_img=3):
    from laenerf_amd.editing.ref_distill import pack_ref_rows
    rows = {k: t.numpy() for k, t in pack_ref_rows(views, n_img, H * W).items()}
    ext_img = np.concatenate([np.full(v["indices"].numel(), v["pose_idx"], np.int32) for v in views])
    ext_pix = np.concatenate([v["indices"].numpy() for v in views]).astype(np.int32)
    ext_rgb = np.concatenate([v["colours"].numpy() for v in views])
    ext_depth = np.concatenate([v["depths"].numpy() for v in views])
    return rows, (ext_img, ext_pix, ext_rgb, ext_depth)


def test_restatement_against_the_references_loop():
    from laenerf_amd.editing.ref_distill import ref_distill_numpy
    images, views = tiny_views()
    rows, ext = _packed(views)
    got = ref_distill_numpy(images, rows["reg_img"], rows["reg_pix"], rows["reg_rgb"], rows["reg_w"], *ext, dtype=np.float32)
    for v in views:
        want = reference_dataloader_nerf(images[v["pose_idx"]], v)
        for name, a, b in zip(("images", "pixel_weights", "second_target", "depths"), got, want):
            assert np.array_equal(a[v["pose_idx"]], b), (name, v["pose_idx"])
    # the image no view points at keeps the background rule
    im, w, s2, d = (g[1] for g in got)
    assert not im[..., :3].any() and np.array_equal(im[..., 3], images[1, ..., 3]) and np.array_equal(w, np.float32(1) - images[1, ..., 3])
    assert not s2.any() and not d.any()
    # what the case was built to hold: a clamped weight, a registered pixel under alpha 0 (weight = w + 1)
    assert (rows["reg_w"] < 0).sum() == 2 and got[1].max() > 1
    # fp16 stores are the fp32 values rounded once
    half = ref_distill_numpy(images, rows["reg_img"], rows["reg_pix"], rows["reg_rgb"], rows["reg_w"], *ext)
    for a, b in zip(half[:3], got[:3]):
        assert a.dtype == np.float16 and np.array_equal(a, b.astype(np.float16))
    assert half[3].dtype == np.float32 and np.array_equal(half[3], got[3])


def test_three_channel_data_uint8_alpha_and_skipped_rows():
    from laenerf_amd.editing.ref_distill import ref_distill_numpy
    images, views = tiny_views(C=3)
    rows, ext = _packed(views)
    im, w, s2, d = ref_distill_numpy(images, rows["reg_img"], rows["reg_pix"], rows["reg_rgb"], rows["reg_w"], *ext, dtype=np.float32)
    assert (im[..., 3] == 1).all() and (s2[..., 3].reshape(3, -1)[ext[0], ext[1]] == 1).all()        # a = 1, not the blue channel
    assert w.reshape(3, -1)[rows["reg_img"], rows["reg_pix"]].tolist() == np.maximum(rows["reg_w"], 0).tolist() and (w >= 0).all()
    img4, views4 = tiny_views(C=4)
    u8 = (img4 * 255).astype(np.uint8)
    rows4, ext4 = _packed(views4)
    a8 = ref_distill_numpy(u8, rows4["reg_img"], rows4["reg_pix"], rows4["reg_rgb"], rows4["reg_w"], *ext4, dtype=np.float32)
    af = ref_distill_numpy(u8.astype(np.float32) / np.float32(255), rows4["reg_img"], rows4["reg_pix"], rows4["reg_rgb"], rows4["reg_w"],
                           *ext4, dtype=np.float32)
    for x, y in zip(a8, af):
        assert np.array_equal(x, y)
    # rows outside the planes are skipped
    bad_img, bad_pix = rows4["reg_img"].copy(), ext4[1].copy()
    bad_img[0], bad_pix[0] = 3, H * W
    skipped = ref_distill_numpy(u8, bad_img, rows4["reg_pix"], rows4["reg_rgb"], rows4["reg_w"], ext4[0], bad_pix, ext4[2], ext4[3], dtype=np.float32)
    kept = ref_distill_numpy(u8, rows4["reg_img"][1:], rows4["reg_pix"][1:], rows4["reg_rgb"][1:], rows4["reg_w"][1:], ext4[0][1:], ext4[1][1:],
                             ext4[2][1:], ext4[3][1:], dtype=np.float32)
    for x, y in zip(skipped, kept):
        assert np.array_equal(x, y)


def test_packing_checks():
    from laenerf_amd.editing.ref_distill import pack_ref_rows
    _, views = tiny_views()
    rows = pack_ref_rows(views, 3, H * W)
    assert rows["reg_img"].dtype == torch.int32 and rows["reg_pix"].dtype == torch.int32 and rows["reg_img"].tolist() == [2] * 5 + [0] * 4
    assert torch.equal(rows["reg_pix"][:5].long(), views[0]["indices"][views[0]["indices_ray_reg"]])
    assert pack_ref_rows([], 3, H * W)["reg_img"].numel() == 0
    twice = [dict(views[0]), dict(views[0])]
    with pytest.raises(ValueError, match="given twice"):
        pack_ref_rows(twice, 3, H * W)
    with pytest.raises(ValueError, match="outside the 2 images"):
        pack_ref_rows(views, 2, H * W)
    dup = dict(views[0]); dup["indices"] = views[0]["indices"].clone(); dup["indices"][1] = dup["indices"][0]
    with pytest.raises(AssertionError, match="same pixel"):
        pack_ref_rows([dup], 3, H * W)
    short = dict(views[0]); short["target_weights"] = views[0]["target_weights"][:-1]
    with pytest.raises(ValueError, match="one entry per row"):
        pack_ref_rows([short], 3, H * W)
    off = dict(views[0]); off["indices"] = views[0]["indices"] + H * W
    with pytest.raises(ValueError, match="outside the image"):
        pack_ref_rows([off], 3, H * W)


def test_library_entries_refuse_invalid_arguments_before_any_launch(hip_lib):
    init, scatter = hip_lib.lae_ref_distill_init, hip_lib.lae_ref_distill_scatter
    p = torch.zeros(16).data_ptr()
    assert init(None, 2, 0, 64, 4, 1, None, None, None, None, None) == 0            # nothing to do
    assert init(None, 2, 2, 64, 4, 1, None, None, None, None, None) == -3
    for C in (1, 2, 5):
        assert init(p, 2, 2, 64, C, 1, p, p, p, p, None) == -1
    for dt in (0, 3):                                                               # the planes are fp16 / fp32, never uint8
        assert init(p, 2, 2, 64, 4, dt, p, p, p, p, None) == -1
    assert init(p, 7, 2, 64, 4, 1, p, p, p, p, None) == -1
    rows = lambda r1=4, r2=4: [r1, p, p, p, p, r2, p, p, p, p]
    assert scatter(0, None, None, None, None, 0, None, None, None, None, None, 2, 2, 64, 4, 1, None, None, None, None, None) == 0
    assert scatter(*rows(), None, 2, 2, 64, 4, 1, p, p, p, p, None) == -3
    assert scatter(4, None, p, p, p, 0, None, None, None, None, p, 2, 2, 64, 4, 1, p, p, p, p, None) == -3
    assert scatter(*rows(), p, 2, 2, 64, 5, 1, p, p, p, p, None) == -1
    assert scatter(*rows(), p, 2, 2, 64, 4, 0, p, p, p, p, None) == -1
    assert scatter(*rows(), p, 9, 2, 64, 4, 1, p, p, p, p, None) == -1
