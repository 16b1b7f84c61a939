"""Trainer(pixel_weights=True, second_weight=...): mask- / confidence-weighted training and the second colour target inside the captured
16-step groups, on the scene and the sizes of test_gpu_criterion.py's _trainer (6 RGBA images of 48 x 40, log2_hashmap_size=16, 2048
rays, 32 steps: 16 eager, 16 replayed).  The held-out ordering alone runs on a scene that has a held-out answer: the teacher views of
tools/train_loop.py at a quarter of its size."""
import os
import sys

import numpy as np
import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

W_SECOND, W_DEPTH = 0.5, 0.1


def _planes(data, seed=21):
    """weights in [0, 2] with 20 % exact zeros (fp16), a 4-channel second target (fp16), the depth plane of the depth tests"""
    rng = np.random.default_rng(seed)
    shape = (data.n_img, data.H, data.W)
    w = rng.uniform(0, 2, shape).astype(np.float16)
    w[rng.random(shape) < 0.2] = 0
    second = rng.uniform(0, 1, shape + (4,)).astype(np.float16)
    depth = rng.uniform(2.0, 4.0, shape).astype(np.float16)
    depth[rng.random(shape) < 0.3] = 0
    return w, second, depth


def _trainer(graph=True, steps=32, planes=True, ones=False, images=None, **kw):
    from test_gpu_trainer import _setup, _state
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    if images is not None:
        data.images.copy_(torch.from_numpy(images).to(DEV))
    if planes:
        w, second, depth = _planes(data)
        data.set_pixel_weights(np.ones_like(w) if ones else w)
        data.set_second_target(second)
        data.set_depths(depth)
    torch.manual_seed(7)
    tr = Trainer(r, opt, data, 400, 1e-2, num_rays=2048, seed=1, graph=graph, capacity="exact", **kw).train(steps)
    return tr, _state(r, opt)


FULL = dict(pixel_weights=True, second_weight=W_SECOND, depth_weight=W_DEPTH)


@pytest.fixture(scope="module")
def plain_run():
    return _trainer(planes=False)


def test_graph_replay_equals_eager_with_weights_second_target_and_depth(plain_run):
    from test_gpu_trainer import _assert_same
    (ta, sa), (tb, sb) = _trainer(**FULL), _trainer(graph=False, **FULL)
    assert ta.captures == 1 and tb.captures == 0                      # steps 16-31 were one replayed graph
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses()) and ta.losses().shape == (32,) and np.isfinite(ta.losses()).all()
    for name in ("second_losses", "depth_losses"):
        a, b = getattr(ta, name)(), getattr(tb, name)()
        assert np.array_equal(a, b) and a.shape == (32,) and (a > 0).all(), name
    assert (ta.losses() > W_SECOND * ta.second_losses()).all()         # the total holds the term
    assert any(not torch.equal(x, y) for x, y in zip(sa, plain_run[1]))
    assert plain_run[0].second_losses().size == 0


def test_a_plane_of_ones_is_the_default_run(plain_run):
    from test_gpu_trainer import _assert_same
    to, so = _trainer(ones=True, pixel_weights=True)
    _assert_same(so, plain_run[1])
    assert np.array_equal(to.losses(), plain_run[0].losses()) and to.second_losses().size == 0
    # ... and planes on the data that the trainer was not asked to use change nothing
    tn, sn = _trainer()
    _assert_same(sn, plain_run[1])


def _make(net_seed, torch_seed, seed, graph=True, **kw):
    """a Trainer on checkpoint_util's scene with the three planes on its data"""
    import checkpoint_util as U
    from laenerf_amd.trainer import Trainer
    r, opt, data = U.setup(net_seed)
    w, second, depth = _planes(data)
    data.set_pixel_weights(w); data.set_second_target(second); data.set_depths(depth)
    torch.manual_seed(torch_seed)
    return Trainer(r, opt, data, U.ITERS, U.LR, num_rays=U.RAYS, seed=seed, graph=graph, capacity="bucket", **kw)


def test_all_four_auxiliary_terms_at_once_replay_equals_eager():
    """depth, distortion, opacity entropy and the second target (with pixel weights) in one step, 48 steps: 16 host-sized, a group run
    eagerly because its capacity is new, a group captured and replayed; the same state and the same per-step records as eager"""
    import checkpoint_util as U
    kw = dict(FULL, distort_weight=0.01, opacity_weight=0.01, loss="mse")
    a, b = _make(0, 7, 1, graph=True, **kw).train(48), _make(0, 7, 1, graph=False, **kw).train(48)
    assert a.captures >= 1 and b.captures == 0                         # the captured path cannot be skipped silently
    U.assert_same_state(a, b)
    for name in ("losses", "depth_losses", "distort_losses", "opacity_losses", "second_losses"):
        x, y = getattr(a, name)(), getattr(b, name)()
        assert x.shape == (48,) and np.isfinite(x).all() and np.array_equal(x, y), name


def test_resume_with_weights_and_second_target_continues_bit_for_bit(tmp_path):
    import checkpoint_util as U
    make = _make

    full = make(0, 7, 1, **FULL).train(32)
    want = U.snapshot(full)
    first = make(0, 7, 1, **FULL).train(16)
    path = first.save_checkpoint(str(tmp_path / "run.pth"))
    cfg = torch.load(path, weights_only=True)["laenerf_amd"]["config"]
    assert cfg["pixel_weights"] is True and cfg["second_weight"] == W_SECOND and cfg["depth_weight"] == W_DEPTH
    resumed = make(1234, 4321, 99, **FULL)
    resumed.load_checkpoint(path)
    resumed.train(16)
    U.assert_same_state(want, resumed)
    U.assert_same_tail(full, resumed, 16)
    assert np.array_equal(resumed.second_losses(), full.second_losses()[-16:]) and resumed.second_losses().shape == (16,)
    # a trainer without the options refuses the file under strict_config, naming the keys
    with pytest.raises(ValueError, match="pixel_weights"):
        make(1234, 4321, 99, depth_weight=W_DEPTH).load_checkpoint(path)
    # a default trainer's file carries neither key: files written before the options existed load as they did
    plain = U.make_trainer().train(16)
    p2 = plain.save_checkpoint(str(tmp_path / "plain.pth"))
    cfg2 = torch.load(p2, weights_only=True)["laenerf_amd"]["config"]
    assert "pixel_weights" not in cfg2 and "second_weight" not in cfg2
    U.fresh_for_resume().load_checkpoint(p2)


def test_masked_pixels_cannot_matter():
    """two data sets that differ only in the colours (and alphas) of pixels whose weight is 0, trained 32 steps from the same seeds:
    bit-identical parameters, optimizer state and losses.  No tolerance: w = 0 makes w * e and the gradient exact zeros."""
    from test_gpu_trainer import _assert_same, _images
    img, _, _ = _images()
    w = _planes(type("D", (), dict(n_img=img.shape[0], H=img.shape[1], W=img.shape[2])))[0]
    masked = w == 0
    assert 0.1 < masked.mean() < 0.3
    other = img.copy()
    other[masked] = np.random.default_rng(3).integers(0, 256, size=(int(masked.sum()), 4), dtype=np.uint8)
    assert (other[masked] != img[masked]).any() and np.array_equal(other[~masked], img[~masked])
    kw = dict(pixel_weights=True, depth_weight=W_DEPTH)
    (ta, sa), (tb, sb) = _trainer(images=img, **kw), _trainer(images=other, **kw)
    assert ta.captures == 1 and tb.captures == 1
    _assert_same(sa, sb)
    assert np.array_equal(ta.losses(), tb.losses())
    # without the weights the two sets train apart
    (_, sc), (_, sd) = _trainer(images=img, steps=16, graph=False, depth_weight=W_DEPTH), _trainer(images=other, steps=16, graph=False,
                                                                                                 depth_weight=W_DEPTH)
    assert any(not torch.equal(x, y) for x, y in zip(sc, sd))


def test_masking_the_outliers_raises_the_held_out_psnr():
    """ordering only: 10 % of the training pixels overwritten with opaque random colours (tools/train_loop.py --outliers 0.1, held-out
    views clean); the run with weight 0 on them (--mask-outliers 0.1) ends strictly above the unweighted run at the same seeds.  16
    views of 64 x 64 and 256 steps instead of the tool's 28 views of 128 x 128 and 1024 steps"""
    import train_loop as TL
    from laenerf_amd import build
    from laenerf_amd.data import ResidentImages
    build.build()
    dev = torch.device(DEV)
    images, poses, intr = TL.teacher_views(dev, 16, 64, 64)
    held = 4
    rng = np.random.default_rng(17)
    hit = rng.random(images[held:].shape[:3]) < 0.1
    noise = rng.integers(0, 256, size=images[held:].shape, dtype=np.uint8)
    noise[..., 3] = 255
    images[held:][hit] = noise[hit]
    test = ResidentImages.from_arrays(images[:held], poses[:held], intr, device=dev)
    out = {}
    for name, mask in (("unweighted", None), ("masked", np.where(hit, 0.0, 1.0).astype(np.float16))):
        tr = TL.make_trainer(dev, images[held:], poses[held:], intr, iters=256, n_rays=2048, pixel_weights=mask)
        tr.train(256)
        assert tr.captures >= 1 and np.isfinite(tr.losses()).all()
        out[name] = tr.evaluate(range(held), data=test, bg_color=1.0)
    print(f"held-out PSNR over white, 10 % outliers: unweighted {out['unweighted']:.2f} dB, masked {out['masked']:.2f} dB")
    assert out["masked"] > out["unweighted"]


def test_refused_combinations_raise():
    from test_gpu_trainer import _setup
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    w, second, _ = _planes(data)
    with pytest.raises(ValueError, match="weight plane"):
        Trainer(r, opt, data, 400, 1e-2, pixel_weights=True)
    with pytest.raises(ValueError, match="second target"):
        Trainer(r, opt, data, 400, 1e-2, second_weight=0.5)
    data.set_pixel_weights(w); data.set_second_target(second)
    for kw in (dict(pixel_weights=True), dict(second_weight=0.5)):
        for loss in ("l1", "huber", "mape"):
            with pytest.raises(ValueError, match="loss='mse'"):
                Trainer(r, opt, data, 400, 1e-2, loss=loss, **kw)
        with pytest.raises(ValueError, match="error_map='ema'"):
            Trainer(r, opt, data, 400, 1e-2, error_map="ema", **kw)
    with pytest.raises(ValueError, match="second_weight"):
        Trainer(r, opt, data, 400, 1e-2, second_weight=-1.0)
    with pytest.raises(ValueError, match="floating"):
        data.set_pixel_weights(np.zeros((data.n_img, data.H, data.W), np.uint8))
    assert data.pixel_weights.device == data.images.device and data.second_target.device == data.images.device


def test_shade_train_without_fused_post_ops_states_the_same_criterion():
    """the torch-operator path against the fused kernel on the same samples: the same sums in another order, to the 2e-6 relative
    test_gpu_criterion.py allows its unfused criterion"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    from gpu_util import T
    torch.manual_seed(5)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    net.encoder.embeddings.data.uniform_(-0.3, 0.3)
    r = NeRFRenderer(net, bound=1).to(DEV)
    r.density_bitfield = T(S.pack_bits_np(S.sphere_density_grid(), 10.0))
    o, d = S.lego_like_rays(500, seed=6)
    g = torch.Generator(device=DEV).manual_seed(3)
    gt, bg = torch.rand(500, 3, device=DEV, generator=g), torch.rand(500, 3, device=DEV, generator=g)
    plane, second = 2 * torch.rand(900, device=DEV, generator=g), torch.rand(900, 4, device=DEV, generator=g).half()
    inds = torch.randint(0, 900, (500,), device=DEV, generator=g)
    scale = torch.tensor([512.0], device=DEV)
    net.train()
    out = []
    for fused in (True, False):
        r.fused_post_ops = fused
        with torch.autocast("cuda", dtype=torch.float16):
            marched = r.march_train(T(o), T(d), perturb=False)
            res = r.shade_train(marched, bg_color=bg, gt=gt, scaler=scale, pixel_weights=plane, pixel_inds=inds, second_target=second,
                                second_weight=W_SECOND)
        out.append((res["loss"].item(), res["loss"].unscaled.item()))
    (l1, u1), (l0, u0) = out
    print(f"unfused against fused: loss {u0:.6e} / {u1:.6e}")
    assert u0 == pytest.approx(u1, rel=2e-6) and l0 == pytest.approx(l1, rel=2e-6) and l1 == pytest.approx(512.0 * u1, rel=1e-6)
