"""laenerf_amd.trainer.Trainer: the reference's loop (refresh every 16 steps, decaying learning rate, random background)
eagerly and as one captured graph per 16-step group."""
import numpy as np
import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu


def _images(n=6, H=48, W=40, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((n, H, W)) < 0.5, 255, img[..., 3])
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    return img, S.lookat_poses(n, seed=seed), (focal, focal, W / 2, H / 2)


def _setup(lr=1e-2, net_seed=0, device_lr=True):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(net_seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(lr), betas=(0.9, 0.99), eps=1e-15, device_lr=device_lr)
    img, poses, intr = _images()
    data = ResidentImages.from_arrays(img, poses, intr, device=DEV)
    return r, opt, data


def _state(r, opt):
    out = [p.detach().clone() for p, *_ in opt.items]
    out += [m.clone() for _, m, *_ in opt.items] + [v.clone() for _, _, v, *_ in opt.items]
    out += [r.density_grid.clone(), r.density_bitfield.clone(), opt.dev_state.clone()]
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


def test_eager_trainer_equals_hand_written_loop():
    from laenerf_amd.trainer import Trainer, lr_schedule
    iters, steps, lr, seed = 200, 48, 1e-2, 5
    r, opt, data = _setup(lr)
    torch.manual_seed(99)
    tr = Trainer(r, opt, data, iters, lr, num_rays=2048, seed=seed, graph=False, capacity="exact").train(steps)
    got, got_losses = _state(r, opt), tr.losses()

    r2, opt2, data2 = _setup(lr, device_lr=False)
    data2.seed = seed
    table = lr_schedule(lr, iters, steps)
    torch.manual_seed(99)
    r2.mark_untrained_grid(data2.poses, data2.intrinsics)
    losses = []
    r2.model.train()
    for s in range(steps):
        if s % 16 == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                r2.update_extra_state()
        opt2.set_lr(float(table[s, 0]))
        b = data2.sample(2048, step=s)
        with torch.autocast("cuda", dtype=torch.float16):
            res = r2.render_train(b["rays_o"], b["rays_d"], bg_color=b["bg"], perturb=True, gt=b["gt"], scaler=opt2)
        opt2.backward(res["loss"])
        opt2.step()
        losses.append(res["loss"].unscaled.clone())
    _assert_same(got, _state(r2, opt2))
    assert np.array_equal(got_losses, torch.stack(losses).cpu().numpy())
    assert r.mean_count == r2.mean_count > 0


def test_graph_trainer_equals_eager_trainer():
    from laenerf_amd.trainer import Trainer
    runs = []
    for graph in (True, False):
        r, opt, data = _setup()
        torch.manual_seed(7)
        tr = Trainer(r, opt, data, 400, 1e-2, num_rays=4096, seed=1, graph=graph, capacity="bucket")
        caps = []
        for i in range(5):                       # 16 eager steps, then four groups (a refresh before each)
            if i == 2:
                # a higher occupancy threshold from the refresh at step 32 on: the samples of group 32-47 drop, so the group
                # at 48 gets another capacity (a new graph) -- the same change in both runs
                r.density_thresh = 10.0
            tr.train(16)
            caps.append(tr._m_cap() if r.mean_count > 0 else None)
        runs.append((_state(r, opt), tr.losses(), tr, caps))
    (sa, la, ta, ca), (sb, lb, tb, cb) = runs
    _assert_same(sa, sb)
    assert np.array_equal(la, lb) and np.isfinite(la).all()
    assert ta.captures >= 1 and ta.warm_groups + ta.captures == ta.cache_misses and tb.captures == 0
    assert ca == cb and len(set(ca[1:])) >= 2                 # at least one change of capacity between groups
    print("graph trainer: capacities", ca, "captures", ta.captures, "warm groups", ta.warm_groups)


def test_bucket_against_exact_first_bucketed_step():
    from laenerf_amd.trainer import Trainer
    losses = {}
    for cap in ("bucket", "exact"):
        r, opt, data = _setup()
        torch.manual_seed(3)
        tr = Trainer(r, opt, data, 400, 1e-2, num_rays=4096, seed=2, graph=False, capacity=cap)
        tr.train(17)
        losses[cap] = tr.losses()
        if cap == "bucket":
            assert tr._m_cap() >= tr._m()
    np.testing.assert_array_equal(losses["bucket"][:16], losses["exact"][:16])
    assert abs(losses["bucket"][16] - losses["exact"][16]) <= 1e-5 * abs(losses["exact"][16])


# Held-out PSNR over white of the scene fit below, measured once on the MI355X (calibration run): 47.72 dB.
FIT_PSNR_MEASURED = 47.72


def test_scene_fit_reaches_psnr():
    """tools/train_loop.py's scene at a smaller scale: 20 RGBA 96x96 views of a teacher network, 4 held out; a fresh student
    trained 768 steps with random backgrounds (graph mode, bucketed capacity) is evaluated over white.  Measured: 47.72 dB
    (FIT_PSNR_MEASURED); the bound is 3 dB below it."""
    import importlib
    tl = importlib.import_module("tools.train_loop")
    images, poses, intr = tl.teacher_views(torch.device(DEV), 20, 96, 96)
    tr = tl.make_trainer(torch.device(DEV), images[4:], poses[4:], intr, iters=768)
    tr.train(768)
    from laenerf_amd.data import ResidentImages
    psnr = tr.evaluate(range(4), data=ResidentImages.from_arrays(images[:4], poses[:4], intr, device=DEV), bg_color=1.0)
    print("scene fit: held-out PSNR", psnr, "captures", tr.captures, "skipped", tr.steps_skipped)
    assert psnr >= max(28.0, FIT_PSNR_MEASURED - 3.0)
