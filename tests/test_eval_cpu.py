"""Host side of evaluation: the LPIPS weight loader, the Trainer's EMA gate and decay sequence, the masked-MSE / uint8 rules of
lae_eval_view's numpy restatement, load_masks."""
import json
import os

import numpy as np
import pytest
import torch


def _alex_sd(seed=0):
    from laenerf_amd.metrics import alexnet_trunk
    torch.manual_seed(seed)
    sd = {f"features.{k}": v for k, v in alexnet_trunk().state_dict().items()}
    sd["classifier.1.weight"] = torch.zeros(4, 4)                 # torchvision's classifier: ignored
    return sd


def _lin_sd(seed=0):
    from laenerf_amd.metrics import ALEX_CHANNELS
    g = torch.Generator().manual_seed(seed)
    return {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for k, c in enumerate(ALEX_CHANNELS)}


def test_lpips_loader_takes_torchvision_and_lpips_layouts(tmp_path):
    from laenerf_amd.metrics import load_lpips_alex
    sd, ld = _alex_sd(), _lin_sd()
    torch.save(sd, tmp_path / "alex.pth")
    torch.save(ld, tmp_path / "lin.pth")
    for a, b in ((sd, ld), (str(tmp_path / "alex.pth"), str(tmp_path / "lin.pth"))):
        m = load_lpips_alex(a, b)
        for i in (0, 3, 6, 8, 10):
            assert torch.equal(m.trunk[i].weight, sd[f"features.{i}.weight"]) and torch.equal(m.trunk[i].bias, sd[f"features.{i}.bias"])
        for k in range(5):
            assert torch.equal(m.lins[k], ld[f"lin{k}.model.1.weight"].reshape(-1))
        assert not any(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("change, match", [
    (lambda sd, ld: sd.pop("features.6.bias"), "missing 'features.6.bias'"),
    (lambda sd, ld: sd.__setitem__("features.3.weight", torch.zeros(192, 64, 3, 3)), "features.3.weight has shape"),
    (lambda sd, ld: sd.__setitem__("features.1.weight", torch.zeros(1)), "unexpected key 'features.1.weight'"),
    (lambda sd, ld: ld.pop("lin4.model.1.weight"), "missing 'lin4.model.1.weight'"),
    (lambda sd, ld: ld.__setitem__("lin2.model.1.weight", torch.zeros(1, 256, 1, 1)), "lin2.model.1.weight has shape"),
])
def test_lpips_loader_rejects_wrong_keys_and_shapes(change, match):
    from laenerf_amd.metrics import load_lpips_alex
    sd, ld = _alex_sd(), _lin_sd()
    change(sd, ld)
    with pytest.raises(ValueError, match=match):
        load_lpips_alex(sd, ld)


def test_lpips_random_is_seeded_and_shaped():
    from laenerf_amd.metrics import LPIPS, ALEX_CHANNELS
    a, b, c = LPIPS.random(3), LPIPS.random(3), LPIPS.random(4)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    assert not torch.equal(a.trunk[0].weight, c.trunk[0].weight)
    assert [int(w.numel()) for w in a.lins] == list(ALEX_CHANNELS) and all(float(w.min()) >= 0 for w in a.lins)
    feats = a.features(torch.zeros(2, 3, 800, 800))             # the taps at 800 x 800: 199^2, 99^2, 49^2 x 3
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 199, 199), (192, 99, 99), (384, 49, 49), (256, 49, 49), (256, 49, 49)]


def test_ema_gate_and_decay_sequence():
    from laenerf_amd.optim import ema_update_steps, ema_one_minus_decay
    assert ema_update_steps(0, 64, 6) == [6, 12, 18, 24, 30, 36, 42, 48, 54, 60]
    assert ema_update_steps(16, 16, 5) == [20, 25, 30]                  # inside one captured 16-step group
    assert ema_update_steps(0, 3, 4) == [] and ema_update_steps(0, 100, 100) == [100]
    # torch_ema: decay_t = min(decay, (1 + n) / (10 + n)) for the n-th update (n counted from 1); EMA.update() passes
    # float(1 - decay_t) through ctypes (fp32 rounding of the fp64 value)
    got = [ema_one_minus_decay(0.95, n) for n in range(1, 200)]
    want = [np.float32(1.0 - min(0.95, (1 + n) / (10 + n))) for n in range(1, 200)]
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    assert got[0] == np.float32(1 - 2 / 11) and got[-1] == np.float32(1 - 0.95)
    n_switch = next(n for n in range(1, 200) if (1 + n) / (10 + n) >= 0.95)   # from here on decay_t = decay
    assert n_switch == 170 and ema_one_minus_decay(0.95, 169) != ema_one_minus_decay(0.95, 170)
    assert ema_one_minus_decay(0.9, 1, use_num_updates=False) == np.float32(1.0 - 0.9)


def test_eval_view_rules_on_hand_computed_values():
    from laenerf_amd.metrics import eval_view_numpy, psnr_from_sse
    pred = np.array([[0.5, 0.25, 1.5], [-0.2, 1.0, 0.999], [0.1, 0.2, 0.3]], np.float32)
    gt = np.array([[255, 0, 0, 255], [0, 255, 0, 0], [255, 255, 255, 0]], np.uint8)    # alpha 1, 0, 0
    depth = np.array([0.5, 2.0, -1.0], np.float32)
    mask = np.array([0, 7, 0], np.uint8)                                                # m = 1 - clip(mask, 0, 1) = 1, 0, 1
    r = eval_view_numpy(pred, gt, depth=depth, bg=1.0, mask=mask)
    assert np.array_equal(r["gt"], np.array([[1, 0, 0], [1, 1, 1], [1, 1, 1]], np.float32))          # blended over white
    d = pred.astype(np.float64) - r["gt"]
    assert r["sse"] == pytest.approx(float((d ** 2).sum()), rel=1e-15)
    raw = gt[:, :3].astype(np.float32) * (np.float32(1) / np.float32(255))
    dm = (pred.astype(np.float64) - raw) ** 2
    assert r["masked_sse"] == pytest.approx(float(dm[0].sum() + dm[2].sum()), rel=1e-15)             # no blend; pixel 1 is out
    # uint8: clip to [0, 1], * 255, truncate
    assert r["rgb_u8"].tolist() == [[127, 63, 255], [0, 255, 254], [25, 51, 76]]
    assert r["depth_u8"].tolist() == [127, 255, 0]
    # LPIPS input: index 0 the blended gt, 1 pred, ((2x - 1) - shift) / scale per channel
    assert r["lpips_in"].shape == (2, 3, 3)
    assert r["lpips_in"][0, 0, 0] == np.float32((np.float32(1.0) + np.float32(0.030)) / np.float32(0.458))
    assert r["lpips_in"][1, 2, 0] == np.float32((np.float32(2.0) + np.float32(0.188)) / np.float32(0.450))
    assert psnr_from_sse([3 * 0.01], 3).tolist() == [pytest.approx(20.0)]


def test_load_masks_on_a_generated_scene(tmp_path):
    from PIL import Image
    from laenerf_amd.metrics import load_masks
    (tmp_path / "test").mkdir()
    frames = []
    for i in range(4):
        Image.fromarray(np.full((6, 8, 3), 40 * i, np.uint8)).save(tmp_path / "test" / f"r_{i}.png")
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": np.eye(4).tolist()})
    frames.append({"file_path": "./test/missing", "transform_matrix": np.eye(4).tolist()})   # no image: skipped
    m0 = np.zeros((6, 8, 4), np.uint8); m0[2:4, 3:6, 3] = 255                               # RGBA: the alpha channel
    Image.fromarray(m0).save(tmp_path / "test" / "r_0_mask.png")
    m1 = np.zeros((6, 8, 3), np.uint8); m1[0, 0, 0] = 9; m1[1, 1, 2] = 9                    # RGB: cv2's last channel = red
    Image.fromarray(m1).save(tmp_path / "test" / "r_1_mask.png")
    m3 = np.zeros((3, 4), np.uint8); m3[1:, 2:] = 200                                       # half size, gray: resized
    Image.fromarray(m3).save(tmp_path / "test" / "r_3_mask.png")
    with open(tmp_path / "transforms_test.json", "w") as f:
        json.dump({"camera_angle_x": 0.69, "frames": frames}, f)
    masks = load_masks(str(tmp_path), "test")
    assert len(masks) == 4 and masks[2] is None
    assert masks[0].dtype == torch.uint8 and np.array_equal(masks[0].numpy(), m0[..., 3])
    want1 = np.zeros((6, 8), np.uint8); want1[0, 0] = 9
    assert np.array_equal(masks[1].numpy(), want1)
    assert masks[3].shape == (6, 8) and masks[3][0, 0] == 0 and masks[3][5, 7] == 200
    assert load_masks(os.path.join(str(tmp_path), "transforms_test.json"), H=12, W=16)[0].shape == (12, 16)
