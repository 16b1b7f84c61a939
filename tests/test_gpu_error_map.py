"""lae_sample_train_batch_weighted / lae_error_map_update (ResidentImages with an error map, Trainer(error_map=...)) against
their numpy restatement, lae_get_rays, the uniform sampler, torch and the reference's get_rays(error_map=...)."""
import numpy as np
import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

N_IMG = 4


def _scene(C, dtype, H, W, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        img = torch.from_numpy(rng.integers(0, 256, size=(N_IMG, H, W, C), dtype=np.uint8))
    else:
        img = torch.from_numpy(rng.random((N_IMG, H, W, C), dtype=np.float32)).to(dtype)
    return img, S.lookat_poses(N_IMG, seed=seed), (0.9 * W, 0.9 * W, W / 2 + 0.3, H / 2 - 0.7)


def _map(seed=0):
    """weights with zeros, ties (a coarse grid of values) and one hot cell"""
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, 6, size=(N_IMG, 16384)) / 4).astype(np.float32)
    m[:, 777] = 1e6
    m[1, :] = 0                                                      # one image of zeros only
    m[1, 5:9] = 2.0
    return m


def _as_f32(img):
    return img.float() / 255 if img.dtype == torch.uint8 else img.float()


def _get_rays(d, im, px):
    from laenerf_amd import _lib
    n = len(px)
    P = d.poses[torch.from_numpy(im).to(DEV)].contiguous()
    ro = torch.empty(n, 1, 3, device=DEV); rd = torch.empty_like(ro)
    ne = torch.empty(n, 1, device=DEV); fa = torch.empty_like(ne)
    inds = torch.from_numpy(px).to(DEV).contiguous()
    _lib.check(_lib.load().lae_get_rays(_lib.ptr(P), n, *d.intrinsics, d.H, d.W, _lib.ptr(inds), 1, 1, 0, 0.0, 0.0, _lib.ptr(ro),
                                        _lib.ptr(rd), _lib.ptr(d.aabb), d.min_near, _lib.ptr(ne), _lib.ptr(fa), _lib.stream()),
               "get_rays")
    return ro.view(n, 3), rd.view(n, 3), ne.view(n), fa.view(n)


@pytest.mark.parametrize("HW", [(37, 53), (300, 211)])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
def test_weighted_batch_matches_restatement(HW, C, dtype):
    from laenerf_amd.data import ResidentImages, cell_pixels, draw_background, draw_cells, draw_indices
    H, W = HW
    img, poses, intr = _scene(C, dtype, H, W)
    seed, n = 0x0BAD_5EED_1234, 3000
    d = ResidentImages.from_arrays(img, poses, intr, bg="random" if C == 4 else "white", seed=seed, device=DEV, error_map=True)
    emap = _map()
    d.error_map.copy_(torch.from_numpy(emap))
    first = {}
    for s in range(256):                                             # a step for every image (image 1: zero weights only)
        first.setdefault(int(draw_indices(seed, s, 1, N_IMG, H, W)[0][0]), s)
    assert len(first) == N_IMG
    images_seen = set()
    for step in sorted(first.values()) + [1000]:
        b = d.sample(n, step=step)
        assert int(d.step.item()) == step + 1
        im, _ = draw_indices(seed, step, n, N_IMG, H, W)
        images_seen.add(int(im[0]))
        cells = draw_cells(seed, step, emap[im[0]], n)
        assert np.array_equal(b["cells"].cpu().numpy(), cells), step
        px = cell_pixels(seed, step, cells, H, W)
        assert np.array_equal(b["inds"].cpu().numpy(), im * H * W + px), step
        for got, want in zip((b["rays_o"], b["rays_d"], b["nears"], b["fars"]), _get_rays(d, im, px)):
            assert torch.equal(got, want), step
        pix = _as_f32(img).reshape(-1, C)[torch.from_numpy(im * H * W + px)]
        if C == 4:
            bg = torch.from_numpy(draw_background(seed, step, n))
            assert torch.equal(b["bg"].cpu(), bg)
            want = pix[:, :3] * pix[:, 3:] + bg * (1 - pix[:, 3:])
        else:
            assert b["bg"] == 1
            want = pix
        assert torch.equal(b["gt"].cpu(), want), step
    print("images drawn:", sorted(images_seen))


def test_cells_distinct_and_full_selection():
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(3, torch.uint8, 64, 64)
    d = ResidentImages.from_arrays(img, poses, intr, seed=3, device=DEV, error_map=True)
    d.error_map.copy_(torch.from_numpy(_map(1)))
    for step in range(6):
        c = d.sample(4096, step=step)["cells"].cpu().numpy()
        assert len(np.unique(c)) == 4096 and (np.diff(c) > 0).all()
    for step in range(N_IMG + 3):
        c = d.sample(16384, step=step)["cells"].cpu().numpy()
        assert np.array_equal(c, np.arange(16384))


def test_image_equals_uniform_sampler():
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(4, torch.uint8, 40, 30)
    u = ResidentImages.from_arrays(img, poses, intr, seed=11, device=DEV)
    w = ResidentImages.from_arrays(img, poses, intr, seed=11, device=DEV, error_map=True)
    HW = 40 * 30
    for step in range(0, 200, 7):
        a = u.sample(512, step=step)["inds"] // HW
        b = w.sample(512, step=step)["inds"] // HW
        assert torch.equal(a, b) and len(torch.unique(b)) == 1
        assert torch.equal(u.sample(512, step=step)["bg"], w.sample(512, step=step)["bg"])     # words 2..4 unchanged


def test_update_bit_exact_and_against_torch():
    from laenerf_amd.data import ResidentImages, ema_update
    H, W = 48, 40
    img, poses, intr = _scene(4, torch.uint8, H, W)
    d = ResidentImages.from_arrays(img, poses, intr, seed=8, device=DEV, error_map=True)
    emap = _map(2) + 0.5
    d.error_map.copy_(torch.from_numpy(emap))
    b = d.sample(4096, step=12)
    g = torch.Generator(device=DEV).manual_seed(0)
    pred = torch.rand(4096, 3, device=DEV, generator=g)
    before = d.error_map.clone()
    d.update_error_map(pred, b)
    got = d.error_map.cpu().numpy()
    want = ema_update(before.cpu().numpy(), b["inds"].cpu().numpy(), b["cells"].cpu().numpy(), pred.cpu().numpy(),
                      b["gt"].cpu().numpy(), H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the reference's torch expressions on the device (nerf/utils.py:597, 609-631).  The gather / EMA / scatter, given the
    # kernel's per-ray error, agree within 1 ulp.  torch's device MSE-mean itself rounds differently from the stated
    # ((d0^2 + d1^2) + d2^2) / 3 (measured: up to 3 ulps of the error, 2 ulps of the map); that gap is bounded, not hidden
    index = b["inds"][:1] // (H * W)
    inds = b["cells"].long()[None]
    dd = pred.cpu().numpy() - b["gt"].cpu().numpy()
    ours = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]) / np.float32(3)
    torch_err = torch.nn.MSELoss(reduction="none")(pred, b["gt"]).mean(-1)

    def ema(error):
        em = before[index]
        em.scatter_(1, inds, 0.1 * em.gather(1, inds) + 0.9 * error[None])
        ref = before.clone()
        ref[index] = em
        return (d.error_map.view(torch.int32).long() - ref.view(torch.int32).long()).abs()[index[0]][inds[0]].cpu().numpy()

    same = ema(torch.from_numpy(ours).to(DEV))
    full = ema(torch_err)
    err_ulps = np.abs(ours.view(np.int32).astype(np.int64) - torch_err.cpu().numpy().view(np.int32).astype(np.int64))
    print("update vs torch on the device: map ulps with the kernel's error", np.bincount(same), "with torch's error",
          np.bincount(full), "error ulps", np.bincount(err_ulps))
    assert same.max() <= 1
    assert err_ulps.max() <= 4 and full.max() <= 2


def test_captured_sample_and_update_equal_eager():
    from laenerf_amd.data import ResidentImages
    H, W = 64, 48
    img, poses, intr = _scene(4, torch.uint8, H, W)
    g = torch.Generator(device=DEV).manual_seed(1)
    preds = torch.rand(5, 2048, 3, device=DEV, generator=g)
    runs = []
    for graph in (False, True):
        d = ResidentImages.from_arrays(img, poses, intr, seed=21, device=DEV, error_map=True)
        d.error_map.copy_(torch.from_numpy(_map(3) + 0.25))
        pred = torch.empty(2048, 3, device=DEV)
        outs = []
        if graph:
            d.sample(2048, step=0)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            m0 = d.error_map.clone()
            with torch.cuda.graph(gr):
                b = d.sample(2048)
                d.update_error_map(pred, b)
            d.error_map.copy_(m0)
            d.step.fill_(100)
            for i in range(5):
                pred.copy_(preds[i])
                gr.replay()
                outs.append({k: v.clone() for k, v in b.items() if torch.is_tensor(v)})
        else:
            d.step.fill_(100)
            for i in range(5):
                b = d.sample(2048)
                d.update_error_map(preds[i], b)
                outs.append({k: v.clone() for k, v in b.items() if torch.is_tensor(v)})
        runs.append((outs, d.error_map.clone(), int(d.step.item())))
    (oa, ma, sa), (ob, mb, sb) = runs
    assert sa == sb == 105
    for a, b in zip(oa, ob):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(ma.view(torch.int32), mb.view(torch.int32))


def test_chi_square_against_reference_get_rays():
    """inclusion counts per weight class: the kernel's draws against laenerf_amd.rays.get_rays(error_map=...) (torch's
    multinomial on the device) from the same map"""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.rays import get_rays
    H, W, n, draws = 128, 128, 2048, 300
    img, poses, intr = _scene(3, torch.uint8, H, W)
    cls = np.arange(16384) % 4
    row = np.array([1.0, 2.0, 4.0, 8.0], np.float32)[cls]
    d = ResidentImages.from_arrays(img[:1], poses[:1], intr, seed=5, device=DEV, error_map=True)
    d.error_map.copy_(torch.from_numpy(row[None]))
    ours = np.zeros(4)
    for s in range(draws):
        ours += np.bincount(cls[d.sample(n, step=s)["cells"].cpu().numpy()], minlength=4)
    theirs = np.zeros(4)
    torch.manual_seed(0)
    for s in range(draws):
        r = get_rays(d.poses[:1], intr, H, W, n, error_map=d.error_map[:1])
        theirs += np.bincount(cls[r["inds_coarse"][0].cpu().numpy()], minlength=4)
    x = float((((ours - theirs) ** 2) / (ours + theirs)).sum())
    print("class counts", ours, theirs, "chi2", x)
    assert x < 3 + 8 * np.sqrt(6)


def _loop_state(r, opt, data):
    from test_gpu_trainer import _state
    return _state(r, opt) + [data.error_map.clone()]


def test_eager_ema_trainer_equals_hand_written_loop():
    from test_gpu_trainer import _assert_same, _setup
    from laenerf_amd.trainer import Trainer, lr_schedule
    iters, steps, lr, seed = 200, 48, 1e-2, 5
    r, opt, data = _setup(lr)
    torch.manual_seed(99)
    tr = Trainer(r, opt, data, iters, lr, num_rays=2048, seed=seed, graph=False, capacity="exact", error_map="ema").train(steps)
    got, got_losses = _loop_state(r, opt, data), tr.losses()

    r2, opt2, data2 = _setup(lr, device_lr=False)
    data2.seed = seed
    data2.enable_error_map()
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
        data2.update_error_map(res["image"], b)
        opt2.backward(res["loss"])
        opt2.step()
        losses.append(res["loss"].unscaled.clone())
    _assert_same(got, _loop_state(r2, opt2, data2))
    assert np.array_equal(got_losses, torch.stack(losses).cpu().numpy())
    assert not torch.equal(data.error_map, torch.ones_like(data.error_map))


@pytest.mark.parametrize("mode", ["ema", "fixed"])
def test_graph_trainer_equals_eager_with_error_map(mode):
    from test_gpu_trainer import _assert_same, _setup
    from laenerf_amd.trainer import Trainer
    runs = []
    for graph in (True, False):
        r, opt, data = _setup()
        seeded = torch.rand(data.n_img, 16384, generator=torch.Generator().manual_seed(4)) + 0.05
        data.enable_error_map().copy_(seeded.to(DEV))
        torch.manual_seed(7)
        tr = Trainer(r, opt, data, 400, 1e-2, num_rays=4096, seed=1, graph=graph, capacity="bucket", error_map=mode)
        caps = []
        for i in range(5):
            if i == 2:
                r.density_thresh = 10.0                  # as test_gpu_trainer: a capacity change between groups
            tr.train(16)
            caps.append(tr._m_cap() if r.mean_count > 0 else None)
        runs.append((_loop_state(r, opt, data), tr.losses(), tr, caps))
        if mode == "fixed":
            assert torch.equal(data.error_map, seeded.to(DEV))
        else:
            assert not torch.equal(data.error_map, seeded.to(DEV))
    (sa, la, ta, ca), (sb, lb, tb, cb) = runs
    _assert_same(sa, sb)
    assert np.array_equal(la, lb) and np.isfinite(la).all()
    assert ta.captures >= 1 and tb.captures == 0
    assert ca == cb and len(set(ca[1:])) >= 2


def test_scene_fit_with_error_map_matches_uniform():
    """test_gpu_trainer's teacher-scene fit with error_map='ema' against the same fit with uniform pixels: the held-out PSNR
    lands within 1 dB (the bar is an estimate, not a measurement)"""
    import importlib
    from laenerf_amd.data import ResidentImages
    tl = importlib.import_module("tools.train_loop")
    images, poses, intr = tl.teacher_views(torch.device(DEV), 20, 96, 96)
    test = ResidentImages.from_arrays(images[:4], poses[:4], intr, device=DEV)
    psnr = {}
    for mode in (None, "ema"):
        tr = tl.make_trainer(torch.device(DEV), images[4:], poses[4:], intr, iters=768, error_map=mode)
        tr.train(768)
        psnr[mode] = tr.evaluate(range(4), data=test, bg_color=1.0)
    print("scene fit: held-out PSNR uniform", psnr[None], "ema", psnr["ema"])
    assert psnr["ema"] >= psnr[None] - 1.0
