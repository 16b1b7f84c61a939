"""CPU: the host side of LAENeRF's stylization (nerf/utils.py:997-1033): the edit set's image arrays, the VGG-19 weight loader, the
style crop rule, the warm-up gate, the preserve_color schedule and the trainer's refusals."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from style_mode_util import BOXES, H_IMG, W_IMG, make_image_views
from laenerf_amd.editing import style_trainer as ST


def _set(views=None, **kw):
    from laenerf_amd.editing import EditSet
    return EditSet.from_views(views if views is not None else make_image_views(), image_hw=(H_IMG, W_IMG), device="cpu", **kw)


def test_pixel_row_map_follows_indices_and_the_exclusive_crop():
    views = make_image_views()
    es = _set(views)
    im = es.image_host
    for v, view in enumerate(views):
        x0, x1, y0, y1 = (int(t) for t in view["cut_min_max_xy"])
        assert im["box"][v].tolist() == [x0, x1, y0, y1]
        h, w = x1 - x0, y1 - y0
        o = int(im["img_off"][v])
        pm = im["pix2row"][o:o + h * w].reshape(h, w)
        # the reference's scatter + crop: canvas[indices[r]] = r, then canvas[x0:x1, y0:y1]
        canvas = np.full(H_IMG * W_IMG, -1, np.int64)
        canvas[view["indices"].numpy()] = np.arange(view["indices"].numel())
        assert np.array_equal(pm, canvas.reshape(H_IMG, W_IMG)[x0:x1, y0:y1])
        r2p = im["row2pix"][es.offsets_host[v]:es.offsets_host[v] + es.counts_host[v]]
        inside = r2p >= 0
        assert np.array_equal(pm.reshape(-1)[r2p[inside]], np.nonzero(inside)[0])
        xi, yi = view["indices"].numpy() // W_IMG, view["indices"].numpy() % W_IMG
        assert np.array_equal(inside, (xi < x1) & (yi < y1))               # the last edit row and column fall outside
        assert np.array_equal(im["cut_gt"][o:o + h * w].reshape(h, w, 3), view["cut_gt"].numpy())
        assert np.array_equal(im["tv_h"][o:o + h * w].reshape(h, w)[:h - 1], view["cut_tv_h"].numpy())
        assert np.array_equal(im["tv_v"][o:o + h * w].reshape(h, w)[:, :w - 1], view["cut_tv_v"].numpy())
        assert np.array_equal(im["smooth"][o:o + h * w].reshape(h, w), view["cut_smooth_trans"].numpy())
        # the per-view maxima the depth-discontinuity term divides by (0 for an empty one: the one-pixel-high crop)
        want_h = float(view["cut_tv_h"].max()) if view["cut_tv_h"].numel() else 0.0
        want_v = float(view["cut_tv_v"].max()) if view["cut_tv_v"].numel() else 0.0
        assert im["vmax"][v].tolist() == [np.float32(want_h), np.float32(want_v)]
    assert es.max_crop_pixels == max((b[1] - b[0]) * (b[3] - b[2]) for b in BOXES)


def test_image_arrays_survive_save_and_load(tmp_path):
    from laenerf_amd.editing import EditSet
    es = _set(seed=7)
    es.save(tmp_path / "set.npz")
    back = EditSet.load(tmp_path / "set.npz", device="cpu")
    assert back.image_hw == es.image_hw and back.seed == es.seed
    assert set(back.image_host) == set(es.image_host)
    for k, a in es.image_host.items():
        assert np.array_equal(back.image_host[k], a), k
        if k != "image_hw":
            assert torch.equal(back.image[k], es.image[k])


def test_sets_without_image_arrays_load_as_before(tmp_path):
    from laenerf_amd.editing import EditSet
    views = make_image_views()
    plain = EditSet.from_views(views, device="cpu")
    assert plain.image is None
    # a file written the way earlier versions wrote it
    np.savez(tmp_path / "old.npz", x_term=plain.x_term.numpy(), dirs=plain.dirs.numpy(), targets=plain.targets.numpy(),
             counts=plain.counts_host.astype(np.int32), depth_factor=plain.depth_factor.numpy(), seed=np.uint64(3))
    back = EditSet.load(tmp_path / "old.npz", device="cpu")
    assert back.image is None and back.seed == 3 and torch.equal(back.x_term, plain.x_term)


def test_image_packing_rejects_bad_views():
    from laenerf_amd.editing import EditSet
    views = make_image_views()
    bad = dict(views[0])
    bad["cut_min_max_xy"] = torch.tensor([3, 3, 2, 9])                     # an empty crop: the reference's resize fails on it
    with pytest.raises(ValueError):
        EditSet.from_views([bad] + views[1:], image_hw=(H_IMG, W_IMG), device="cpu")
    partial = [dict(v) for v in views]
    del partial[1]["cut_smooth_trans"]
    with pytest.raises(ValueError):
        EditSet.from_views(partial, image_hw=(H_IMG, W_IMG), device="cpu")


def _vgg_state_dict(last=14, seed=0):
    from laenerf_amd.editing.style_network import vgg19_features
    torch.manual_seed(seed)
    net = vgg19_features(36)
    sd = {f"features.{k}": v for k, v in net.state_dict().items()}
    sd["classifier.0.weight"] = torch.zeros(4, 4)                            # torchvision's file also holds the classifier
    return sd


def test_vgg19_loader_maps_the_torchvision_layout(tmp_path):
    from laenerf_amd.editing import load_vgg19_features
    sd = _vgg_state_dict()
    torch.save(sd, tmp_path / "vgg19.pth")
    for src in (sd, str(tmp_path / "vgg19.pth")):
        net = load_vgg19_features(src, 14)
        assert len(net) == 15 and not any(p.requires_grad for p in net.parameters())
        for i in (0, 2, 5, 7, 10, 12, 14):
            assert torch.equal(net[i].weight, sd[f"features.{i}.weight"]) and torch.equal(net[i].bias, sd[f"features.{i}.bias"])
        assert isinstance(net[4], torch.nn.MaxPool2d) and isinstance(net[13], torch.nn.ReLU) and not net[13].inplace
    x = torch.rand(3, 32, 32)
    assert load_vgg19_features(sd, 14)(x).shape == (256, 8, 8)


def test_vgg19_loader_rejects_bad_keys_and_shapes():
    from laenerf_amd.editing import load_vgg19_features
    sd = _vgg_state_dict()
    missing = dict(sd)
    del missing["features.12.bias"]
    with pytest.raises(ValueError):
        load_vgg19_features(missing, 14)
    load_vgg19_features(missing, 10)                                        # layers past last_layer are not needed
    shape = dict(sd)
    shape["features.5.weight"] = torch.zeros(128, 32, 3, 3)
    with pytest.raises(ValueError):
        load_vgg19_features(shape, 14)
    extra = dict(sd)
    extra["features.3.weight"] = torch.zeros(1)                             # a ReLU has no weights
    with pytest.raises(ValueError):
        load_vgg19_features(extra, 14)


def _torchvision_random_crop(img, size, gen):
    """torchvision 0.15.2 RandomCrop(size, pad_if_needed=True).forward restated: pad width, then height, by the deficit on both ends
    (F.pad(img, [d, 0]) / [0, d]), then get_params' two torch.randint draws"""
    _, h, w = img.shape
    if w < size:
        img = torch.nn.functional.pad(img, (size - w, size - w, 0, 0))
    _, h, w = img.shape
    if h < size:
        img = torch.nn.functional.pad(img, (0, 0, size - h, size - h))
    _, h, w = img.shape
    if h == size and w == size:
        return img
    i = torch.randint(0, h - size + 1, size=(1,), generator=gen).item()
    j = torch.randint(0, w - size + 1, size=(1,), generator=gen).item()
    return img[:, i:i + size, j:j + size]


@pytest.mark.parametrize("hw", [(20, 30), (40, 52), (12, 64), (64, 9), (32, 32), (31, 33)])
def test_style_crop_follows_random_crop(hw):
    from laenerf_amd.editing.style_network import random_crop
    img = torch.rand(3, *hw)
    for seed in range(3):
        got = random_crop(img, 32, generator=torch.Generator().manual_seed(seed))
        want = _torchvision_random_crop(img, 32, torch.Generator().manual_seed(seed))
        assert torch.equal(got, want), (hw, seed)


def test_style_layers_of_different_shapes_are_refused():
    from laenerf_amd.editing import StyleNetwork
    from laenerf_amd.editing.style_network import vgg19_features
    from style_mode_util import striped_style
    with pytest.raises(ValueError):
        StyleNetwork(striped_style(), vgg19_features(14), style_layers=(3, 10), size=32)
    net = StyleNetwork(striped_style(), vgg19_features(14), size=32, generator=torch.Generator().manual_seed(0))
    assert net.gram_style.shape == (3, 256, 256)


def test_warmup_gate_is_per_group():
    on = [ST.image_terms_on(s, 1000) for s in range(1100)]
    assert not any(on[:1008]) and all(on[1008:])
    assert not any(ST.image_terms_on(s, 0) for s in range(16)) and ST.image_terms_on(16, 0)
    assert ST.image_terms_on(0, -1)


@pytest.mark.parametrize("V", [3, 20, 40])
def test_preserve_color_schedule_consumes_one_view_per_group(V):
    g = torch.Generator().manual_seed(5)
    sched, colour = ST.draw_schedule(g, V, 64, preserve_color=True)
    assert sched.size == 64 and colour.size == 4
    g = torch.Generator().manual_seed(5)
    for k in range(4):
        flat = []
        while len(flat) < 17:
            flat.extend(torch.randperm(V, generator=g)[:17 - len(flat)].tolist())
        assert colour[k] == flat[0] and sched[16 * k:16 * (k + 1)].tolist() == flat[1:]
    # without preserve_color: unchanged
    assert np.array_equal(ST.draw_schedule(torch.Generator().manual_seed(5), V, 64), ST.view_schedule(V, 64, seed=5))


def test_refusals_need_image_arrays_and_a_style_network():
    from laenerf_amd.editing import EditSet, StyleTrainer
    plain = EditSet.from_views(make_image_views(), device="cpu")
    for name in ("style_weight", "tv_weight", "depth_disc_weight", "smooth_trans_weight"):
        with pytest.raises(NotImplementedError, match="image arrays"):
            StyleTrainer(None, plain, SimpleNamespace(**{name: 1}), 100)
    es = _set()
    for p in (SimpleNamespace(style_weight=1), SimpleNamespace(preserve_color=True), SimpleNamespace(tv_weight=1, preserve_color=True)):
        with pytest.raises(NotImplementedError, match="style network"):
            StyleTrainer(None, es, p, 100)
    with pytest.raises(NotImplementedError):
        StyleTrainer(None, es, SimpleNamespace(intensity_weight=1), 100)
    nosmooth = EditSet.from_views(make_image_views(smooth=False), image_hw=(H_IMG, W_IMG), device="cpu")
    with pytest.raises(NotImplementedError, match="cut_smooth_trans"):
        StyleTrainer(None, nosmooth, SimpleNamespace(smooth_trans_weight=1e-3), 100)
