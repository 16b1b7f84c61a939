"""Host side of training from posed images (laenerf_amd.data / laenerf_amd.trainer): the batch RNG's restatement, the
transforms.json loader and the learning-rate table.  No GPU needed."""
import json
import math

import numpy as np
import pytest


def test_philox4x32_10_known_answers():
    # the Philox4x32-10 known-answer vectors published with the generator (Random123 kat_vectors)
    from laenerf_amd.data import philox4x32_10
    cases = [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ]
    for ctr, key, want in cases:
        got = philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert [int(x) for x in got] == want


def test_draw_rule_ranges_and_modes():
    from laenerf_amd.data import draw_background, draw_indices
    img, pix = draw_indices(7, 3, 1000, 5, 37, 29, mode="image")
    assert (img == img[0]).all() and 0 <= img[0] < 5
    assert pix.min() >= 0 and pix.max() < 37 * 29
    img_a, pix_a = draw_indices(7, 3, 1000, 5, 37, 29, mode="all")
    assert np.array_equal(pix_a, pix) and len(set(img_a.tolist())) == 5     # the pixel word does not depend on the mode
    assert not np.array_equal(draw_indices(7, 4, 1000, 5, 37, 29)[1], pix)  # a new step, a new batch
    bg = draw_background(7, 3, 1000)
    assert bg.dtype == np.float32 and bg.shape == (1000, 3) and bg.min() >= 0 and bg.max() < 1
    assert np.array_equal(bg * 2 ** 24, np.floor(bg * 2 ** 24))            # 24-bit grid


def _write_scene(tmp_path, rgba, with_fl, downscale_size=(12, 10)):
    from PIL import Image
    W, H = downscale_size
    rng = np.random.default_rng(0)
    frames, pixels = [], []
    for i in range(3):
        arr = rng.integers(0, 256, size=(H, W, 4 if rgba else 3), dtype=np.uint8)
        Image.fromarray(arr, "RGBA" if rgba else "RGB").save(tmp_path / f"r_{i}.png")
        pose = np.eye(4)
        pose[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        pose[:3, 3] = rng.normal(size=3) * 4
        frames.append({"file_path": f"./r_{i}", "transform_matrix": pose.tolist()})
        pixels.append(arr)
    tf = {"frames": frames}
    if with_fl:
        tf.update(fl_x=13.5, fl_y=14.0, cx=5.5)
    else:
        tf["camera_angle_x"] = 0.69
    (tmp_path / "transforms.json").write_text(json.dumps(tf))
    return tf, np.stack(pixels)


@pytest.mark.parametrize("rgba", [True, False])
def test_from_transforms_poses_intrinsics_images(tmp_path, rgba):
    from laenerf_amd.data import ResidentImages
    tf, pixels = _write_scene(tmp_path, rgba, with_fl=False)
    d = ResidentImages.from_transforms(str(tmp_path), scale=0.5, offset=(0.1, -0.2, 0.3), device="cpu")
    assert d.C == (4 if rgba else 3) and d.images.dtype.is_floating_point is False
    assert d.images.shape == (3, 10, 12, d.C)
    assert np.array_equal(d.images.numpy(), pixels)                 # uint8 kept as decoded, alpha channel included
    for i, fr in enumerate(tf["frames"]):
        p = np.array(fr["transform_matrix"], dtype=np.float32)
        want = np.array([[p[1, 0], -p[1, 1], -p[1, 2], p[1, 3] * 0.5 + 0.1],
                         [p[2, 0], -p[2, 1], -p[2, 2], p[2, 3] * 0.5 - 0.2],
                         [p[0, 0], -p[0, 1], -p[0, 2], p[0, 3] * 0.5 + 0.3],
                         [0, 0, 0, 1]], dtype=np.float32)
        assert np.array_equal(d.poses[i].numpy(), want)
    fl = 12 / (2 * math.tan(0.69 / 2))
    assert d.intrinsics == pytest.approx((fl, fl, 6.0, 5.0), rel=0, abs=0)


def test_from_transforms_focal_downscale_and_float(tmp_path):
    from PIL import Image
    from laenerf_amd.data import ResidentImages
    _, pixels = _write_scene(tmp_path, True, with_fl=True)
    d = ResidentImages.from_transforms(str(tmp_path / "transforms.json"), downscale=2, dtype="float32", device="cpu")
    assert d.images.shape == (3, 5, 6, 4) and d.images.dtype.is_floating_point
    assert d.intrinsics == (13.5 / 2, 14.0 / 2, 5.5 / 2, 5 / 2)     # cy defaults to H/2 of the downscaled image
    box = np.asarray(Image.fromarray(pixels[1], "RGBA").resize((6, 5), Image.BOX), dtype=np.uint8)
    assert np.array_equal(d.images[1].numpy(), box.astype(np.float32) / 255)


def test_learning_rate_table():
    from laenerf_amd.trainer import lr_schedule
    lr, iters = 1e-2, 300
    t = lr_schedule(lr, iters, 400, n_groups=4)
    assert t.dtype == np.float32 and t.shape == (400, 4)
    want = np.array([np.float32(lr * 0.1 ** min(it / iters, 1)) for it in range(400)], dtype=np.float32)
    for g in range(4):
        assert np.array_equal(t[:, g], want)
    assert t[-1, 0] == np.float32(lr * 0.1)


def test_bucket_capacity_padding():
    from laenerf_amd.trainer import bucket_capacity
    prev = 0
    for M in range(128, 1 << 21, 128 * 37):
        c = bucket_capacity(M)
        assert c >= M and c % 128 == 0 and (c - M) <= 0.125 * M + 128
        assert c >= prev
        prev = c
    # one octave: 8 steps of 1/8 (the last bucket is the next power of two)
    assert {bucket_capacity(M) for M in range(1 << 16, 1 << 17, 128)} == {(1 << 16) + j * (1 << 13) for j in range(9)}
