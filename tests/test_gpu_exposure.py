"""Exposure / white-balance refinement on the GPU: the gained samplers against the plain ones and against the float32 restatement,
lae_exposure_step / lae_exposure_publish against the float64 restatements of laenerf_amd/exposure.py, the Trainer's exposure_refine path
(bit-equalities), and a run that recovers perturbed exposures against a frozen student."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, T
from laenerf_amd import exposure as E

pytestmark = pytest.mark.gpu

N_IMG, SH, SW, N_RAYS = 5, 12, 10, 97                     # 97 rays: a tail in the last wave and the last block


# ---------------------------------------------------------------------------------------------------------------- the samplers
def _stack(dtype, C, seed=0):
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (N_IMG, SH, SW, 4), dtype=np.uint8)
    u8[..., 3] = np.where(rng.random((N_IMG, SH, SW)) < 0.3, 255, u8[..., 3])
    img = u8 if dtype == "u8" else (u8.astype(np.float32) / np.float32(255)).astype(np.float16 if dtype == "f16" else np.float32)
    return img[..., :C].copy()


def _data(img, bg, linear, weighted):
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    d = ResidentImages.from_arrays(img, S.lookat_poses(N_IMG, seed=0), (14.0, 14.0, SW / 2, SH / 2), device=DEV, bg=bg, seed=17,
                                   color_space="linear" if linear else "srgb", mode="image" if weighted else "all", error_map=weighted)
    if weighted:
        d.error_map.copy_(T(np.random.default_rng(1).uniform(0.1, 2.0, tuple(d.error_map.shape)).astype(np.float32)))
    return d


def _snap(b):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}


def _same_batch(a, b, skip=()):
    for k, v in a.items():
        if k in skip:
            continue
        if torch.is_tensor(v):
            assert torch.equal(v.view(torch.uint8), b[k].view(torch.uint8)), k
        else:
            assert v == b[k], k


CASES = [(dt, C, bg, lin) for dt in ("u8", "f16", "f32") for C in (3, 4) for bg in ("white", "random") for lin in (0, 1)]


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("dtype,C,bg,linear", CASES)
def test_sampler_with_gains_of_one_is_the_plain_sampler(dtype, C, bg, linear, weighted):
    d = _data(_stack(dtype, C), bg, linear, weighted)
    plain = _snap(d.sample(N_RAYS, step=3))
    assert "fg" not in plain
    gains = d.enable_exposure_refinement()
    assert gains.dtype == torch.float32 and tuple(gains.shape) == (N_IMG, 3) and bool((gains == 1).all())
    got = _snap(d.sample(N_RAYS, step=3))
    _same_batch(plain, got)
    assert got["fg"].shape == (N_RAYS, 3) and int(d.step) == 4
    if C == 3:
        assert torch.equal(got["fg"], got["gt"])
    if not weighted:
        assert len(torch.unique(got["inds"] // (SH * SW))) > 1                # mode 'all': several images in one batch


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("dtype,C,bg,linear", CASES)
def test_sampler_with_random_gains_matches_the_restatement(dtype, C, bg, linear, weighted):
    """gt and fg bit for bit against gained_targets_numpy.  Its colour input is the plain sampler's gt on the stack's RGB channels alone
    (C = 3: the texel after the optional srgb_to_linear, no blend; the draw does not depend on C), alpha the texel's fourth channel, the
    background the plain sampler's own."""
    img = _stack(dtype, C)
    d = _data(img, bg, linear, weighted)
    plain = _snap(d.sample(N_RAYS, step=5))
    colour = _data(img[..., :3].copy(), bg, linear, weighted).sample(N_RAYS, step=5)
    assert torch.equal(colour["inds"], plain["inds"])
    d.enable_exposure_refinement()
    g = np.random.default_rng(9).uniform(0.5, 2.0, (N_IMG, 3)).astype(np.float32)
    d.gains.copy_(T(g))
    got = _snap(d.sample(N_RAYS, step=5))
    _same_batch(plain, got, skip=("gt",))
    inds = plain["inds"].cpu().numpy()
    alpha = None
    if C == 4:
        a = img.reshape(-1, 4)[inds, 3]
        alpha = a.astype(np.float32) / np.float32(255) if dtype == "u8" else a.astype(np.float32)
    bg_np = plain["bg"].cpu().numpy() if torch.is_tensor(plain["bg"]) else 1.0
    gt, fg = E.gained_targets_numpy(colour["gt"].cpu().numpy(), g[inds // (SH * SW)], alpha, bg_np)
    assert np.array_equal(got["gt"].cpu().numpy().view(np.int32), gt.view(np.int32))
    assert np.array_equal(got["fg"].cpu().numpy().view(np.int32), fg.view(np.int32))
    assert not torch.equal(got["gt"], plain["gt"])


# ---------------------------------------------------------------------------------------------------------------- the step kernels
def _step_data(n_img=5, H=8, W=8):
    from laenerf_amd import synthetic as S
    from laenerf_amd.data import ResidentImages
    img = np.random.default_rng(3).integers(0, 256, (n_img, H, W, 3), dtype=np.uint8)
    return ResidentImages.from_arrays(img, S.lookat_poses(n_img, seed=0), (10.0, 10.0, W / 2, H / 2), device=DEV)


def _words(skip=0):
    w = np.zeros(16, np.int32)
    w[3] = skip
    w[7] = np.float32(2.0 ** -10).view(np.int32)                              # 1 / loss scale: must not enter
    return T(w)


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def _ex_tensors(d):
    return d.exposure_master, d.exposure_m, d.exposure_v, d.exposure_counts, d.gains


@pytest.mark.parametrize("mode", ["rgb", "gray"])
@pytest.mark.parametrize("N,plane_dtype", [(96, None), (96, np.float16), (97, None), (97, np.float32)])
@pytest.mark.parametrize("kind", ["mse", "l1", "huber", "mape"])
def test_exposure_step_and_publish(kind, N, plane_dtype, mode):
    """two consecutive steps against exposure_numpy: counts equal, fp64 state within 2^-40 relative (the bound of test_pose_step for the
    same kind of arithmetic), gains within one fp32 ulp of float32(exp2(.)) of the restated master"""
    d = _step_data()
    d.enable_exposure_refinement(mode)
    n_img, hw = d.n_img, d.H * d.W
    rng = np.random.default_rng(N + 3 * (mode == "gray"))
    lr = torch.tensor([3e-3], dtype=torch.float32, device=DEV)
    plane = None if plane_dtype is None else rng.uniform(0.0, 2.0, (n_img, d.H, d.W)).astype(plane_dtype)
    plane_t = None if plane is None else T(plane)
    ref = (np.zeros((n_img, 3)), np.zeros((n_img, 3)), np.zeros((n_img, 3)), np.zeros(n_img, np.int32))
    kw = dict(loss=kind, huber_delta=0.1)
    for step in range(2):
        img = rng.integers(0, n_img, N)
        img[img == 3] = 2                                                     # image 3 never receives a ray
        inds = img * hw + rng.integers(0, hw, N)
        gt, fg = rng.uniform(0, 1.5, (N, 3)).astype(np.float32), rng.uniform(0, 1.5, (N, 3)).astype(np.float32)
        pred = (gt + rng.uniform(-0.3, 0.3, (N, 3))).astype(np.float32)
        if step == 0:
            pred[np.flatnonzero(img == 1)[0], 1] = np.nan                     # image 1's gradient is not finite in the first step
        batch = {"gt": T(gt), "fg": T(fg), "inds": T(inds)}
        before = [t.clone() for t in _ex_tensors(d)]
        d.exposure_step(T(pred), batch, _words(skip=1), lr, pixel_weights=plane_t, **kw)      # the skip word set: no bit moves
        for t, b in zip(_ex_tensors(d), before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
        d.exposure_step(T(pred), batch, _words(), lr, pixel_weights=plane_t, **kw)
        ref = E.exposure_step_numpy(pred, gt, fg, inds, hw, *ref, weights=plane, mode=mode, lr=3e-3, **kw)
        got = [t.cpu().numpy() for t in _ex_tensors(d)]
        for i in ([3, 1] if step == 0 else [3]):                              # untouched: master, moments and count bit for bit
            for t, b in zip(_ex_tensors(d)[:4], before[:4]):
                assert torch.equal(t[i:i + 1].view(torch.uint8), b[i:i + 1].view(torch.uint8)), (step, i)
        assert np.array_equal(got[3], ref[3]) and got[3].tolist() == ([1, 0, 1, 0, 1] if step == 0 else [2, 1, 2, 0, 2])
        for k in range(3):
            assert _close(got[k], ref[k], 2.0 ** -40), (step, k, np.abs(got[k] - ref[k]).max())
        g_ref = E.exposure_publish_numpy(ref[0])
        assert np.all(np.abs(got[4].astype(np.float64) - g_ref.astype(np.float64)) <= np.spacing(g_ref).astype(np.float64)), step
        g_own = E.exposure_publish_numpy(got[0])                               # ... and of the kernel's own master
        assert np.all(np.abs(got[4].astype(np.float64) - g_own.astype(np.float64)) <= np.spacing(g_own).astype(np.float64)), step
        if mode == "gray":
            assert np.array_equal(got[0][:, 0], got[0][:, 1]) and np.array_equal(got[0][:, 0], got[0][:, 2])
    # the gains did move (each step by up to about lr, in either direction: two steps may partly cancel, never exactly), and their
    # per-channel geometric mean is 1
    assert np.all(got[0][[0, 2, 4]] != 0) and np.abs(got[0]).max() > 1e-3 and not got[0][3].any()
    assert np.all(np.abs(np.log2(got[4].astype(np.float64)).mean(0)) < 1e-6)
    # lr = 0: counts and moments advance, no master bit changes
    before = [t.clone() for t in _ex_tensors(d)]
    d.exposure_step(T(pred), batch, _words(), torch.zeros(1, device=DEV), pixel_weights=plane_t, **kw)
    assert torch.equal(before[0].view(torch.int64), d.exposure_master.view(torch.int64))
    assert torch.equal(before[4].view(torch.int32), d.gains.view(torch.int32))
    assert d.exposure_counts.tolist() == [3, 2, 3, 0, 3] and not torch.equal(before[1], d.exposure_m)
    # center = False publishes 2^master
    d.exposure_step(T(pred), batch, _words(skip=1), lr, pixel_weights=plane_t, center=False, **kw)
    raw = E.exposure_publish_numpy(d.exposure_master.cpu().numpy(), center=False)
    assert np.all(np.abs(d.gains.cpu().numpy() - raw) <= np.spacing(raw))


def test_a_single_image_keeps_a_gain_of_one_and_zeros_publish_ones():
    d = _step_data(n_img=1)
    d.enable_exposure_refinement()
    rng = np.random.default_rng(2)
    N, hw = 97, d.H * d.W
    lr = torch.tensor([1e-2], dtype=torch.float32, device=DEV)
    for _ in range(3):
        gt = rng.uniform(0, 1, (N, 3)).astype(np.float32)
        batch = {"gt": T(gt), "fg": T(gt), "inds": T(rng.integers(0, hw, N))}
        d.exposure_step(T((gt + 0.1).astype(np.float32)), batch, _words(), lr)
        assert bool((d.gains == 1).all())
    assert int(d.exposure_counts[0]) == 3 and bool((d.exposure_master.abs() > 1e-2).all())
    d5 = _step_data()
    d5.enable_exposure_refinement()
    d5.gains.fill_(7.0)
    batch = {"gt": T(gt), "fg": T(gt), "inds": T(rng.integers(0, 5 * hw, N))}
    d5.exposure_step(T(gt), batch, _words(skip=1), lr)                        # a skipped step still publishes: zeros give exact ones
    assert d5.gains.cpu().numpy().tobytes() == np.ones((5, 3), np.float32).tobytes()
    with pytest.raises(ValueError, match="enable_exposure_refinement"):
        _step_data().exposure_step(T(gt), batch, _words(), lr)
    with pytest.raises(ValueError, match="mode"):
        _step_data().enable_exposure_refinement("hsv")


# ---------------------------------------------------------------------------------------------------------------- the Trainer
ITERS, LR, RAYS = 400, 1e-2, 1024


def _views(n=8, H=64, W=64, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((n, H, W)) < 0.5, 255, img[..., 3])
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    return img, S.lookat_poses(n, seed=seed), (focal, focal, W / 2, H / 2)


def _trainer(net_seed=0, torch_seed=7, seed=1, graph=True, data_kw=None, **kw):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    torch.manual_seed(net_seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    img, poses, intr = _views()
    data = ResidentImages.from_arrays(img, poses, intr, device=DEV, **(data_kw or {}))
    torch.manual_seed(torch_seed)
    return Trainer(r, opt, data, ITERS, LR, num_rays=RAYS, seed=seed, graph=graph, **kw)


def _state(tr):
    out = {}
    for i, (p, m, v, *_) in enumerate(tr.opt.items):
        out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach().clone(), m.clone(), v.clone()
    out["density_grid"], out["words"], out["data_step"] = tr.r.density_grid.clone(), tr.opt.dev_state.clone(), tr.data.step.clone()
    return out


def _ex_state(tr):
    d = tr.data
    return {"master": d.exposure_master.clone(), "m": d.exposure_m.clone(), "v": d.exposure_v.clone(),
            "counts": d.exposure_counts.clone(), "gains": d.gains.clone(), "reported": tr.gains()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


def test_trainer_exposure_lr_zero_is_the_plain_run():
    plain = _trainer().train(32)
    zero = _trainer(exposure_refine=True, exposure_lr=0.0).train(32)
    assert np.array_equal(plain.losses().view(np.int32), zero.losses().view(np.int32)) and np.isfinite(plain.losses()).all()
    _same(_state(plain), _state(zero))
    assert zero.gains().cpu().numpy().tobytes() == np.ones((8, 3), np.float32).tobytes() and not zero.exposures().any()
    assert int(zero.data.exposure_counts.sum()) == 32 - zero.steps_skipped   # mode 'image': one image per step took a (zero) step
    assert bool(zero.data.exposure_m.abs().sum() > 0)
    cfg = zero.config()
    assert "exposure_refine" not in plain.config() and cfg["exposure_refine"] is True and cfg["exposure_lr"] == 0.0
    assert cfg["exposure_mode"] == "rgb" and cfg["exposure_center"] is True
    assert plain.data.gains is None and bool((plain.gains() == 1).all()) and not plain.exposures().any()


def test_trainer_exposure_graph_equals_eager():
    a = _trainer(exposure_refine=True, exposure_lr=1e-2, graph=True).train(48)
    b = _trainer(exposure_refine=True, exposure_lr=1e-2, graph=False).train(48)
    assert a.captures >= 1 and b.captures == 0
    assert np.array_equal(a.losses().view(np.int32), b.losses().view(np.int32))
    _same(_state(a), _state(b))
    _same(_ex_state(a), _ex_state(b))
    ex = a.exposures()
    assert np.isfinite(ex).all() and np.abs(ex).max() > 1e-2 and np.all(np.abs(ex.mean(0)) < 1e-12)
    assert np.all(np.abs(a.gains().cpu().numpy() - np.exp2(ex).astype(np.float32)) <= np.spacing(np.exp2(ex).astype(np.float32)))


@pytest.mark.parametrize("combo", ["pose-huber-opacity-ema", "weights-depth-distort-fixed-gray"])
def test_trainer_exposure_combines_with_the_other_terms(combo):
    """graph replay equals eager with everything else switched on as well, the exposure state included"""
    if combo == "pose-huber-opacity-ema":
        kw = dict(pose_refine=True, pose_lr=1e-3, loss="huber", opacity_weight=1e-3, error_map="ema", ema_decay=0.95)
        data_kw = None
    else:
        rng = np.random.default_rng(4)
        data_kw = dict(pixel_weights=rng.uniform(0.5, 1.5, (8, 64, 64)).astype(np.float16),
                       depths=rng.uniform(1.0, 3.0, (8, 64, 64)).astype(np.float32))
        kw = dict(pixel_weights=True, depth_weight=1e-3, distort_weight=1e-3, error_map="fixed", exposure_mode="gray")
    a = _trainer(exposure_refine=True, exposure_lr=1e-2, graph=True, data_kw=data_kw, **kw).train(48)      # 48: a group may run warm
    b = _trainer(exposure_refine=True, exposure_lr=1e-2, graph=False, data_kw=data_kw, **kw).train(48)
    assert a.captures >= 1 and np.isfinite(a.losses()).all()
    assert np.array_equal(a.losses().view(np.int32), b.losses().view(np.int32))
    _same(_state(a), _state(b))
    _same(_ex_state(a), _ex_state(b))
    ex = a.exposures()
    assert np.abs(ex).max() > 1e-2
    if "gray" in combo:
        assert np.array_equal(ex[:, 0], ex[:, 1]) and np.array_equal(ex[:, 0], ex[:, 2])


def test_trainer_exposure_resume_equals_uninterrupted(tmp_path):
    kw = dict(exposure_refine=True, exposure_lr=1e-2)
    full = _trainer(**kw).train(32)
    first = _trainer(**kw).train(16)
    path = first.save_checkpoint(str(tmp_path / "exposure.pth"))
    ck = torch.load(path, weights_only=True)
    from laenerf_amd import checkpoint as C
    assert set(ck[C.KEY]["data"]["exposure"]) == {"master", "m", "v", "counts", "gains"} and ck[C.KEY]["config"]["exposure_lr"] == 1e-2
    fresh = _trainer(net_seed=1234, torch_seed=4321, seed=99, **kw)
    ptrs = [t.data_ptr() for t in _ex_tensors(fresh.data)]
    fresh.load_checkpoint(path)
    assert [t.data_ptr() for t in _ex_tensors(fresh.data)] == ptrs           # written in place
    _same(_ex_state(first), _ex_state(fresh))
    fresh.train(16)
    assert np.array_equal(fresh.losses().view(np.int32), full.losses()[-16:].view(np.int32))
    _same(_state(full), _state(fresh))
    _same(_ex_state(full), _ex_state(fresh))
    # a trainer without the refinement refuses the file (the configuration differs), and the other way round
    plain = _trainer()
    with pytest.raises(ValueError, match="exposure_refine"):
        plain.load_checkpoint(path)
    assert plain.data.gains is None
    plain_path = plain.train(16).save_checkpoint(str(tmp_path / "plain.pth"))
    assert "exposure" not in torch.load(plain_path, weights_only=True)[C.KEY]["data"]
    with pytest.raises(ValueError, match="exposure_refine"):
        _trainer(**kw).load_checkpoint(plain_path)


def test_trainer_exposure_refusals():
    from laenerf_amd.trainer import Trainer
    tr = _trainer()
    args = (tr.r, tr.opt, tr.data, ITERS, LR)
    tr.data.set_second_target(np.zeros((8, 64, 64, 3), np.float32))
    with pytest.raises(ValueError, match="second_weight"):
        Trainer(*args, num_rays=RAYS, exposure_refine=True, second_weight=0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="exposure_lr"):
            Trainer(*args, num_rays=RAYS, exposure_refine=True, exposure_lr=bad)
    with pytest.raises(ValueError, match="exposure_mode"):
        Trainer(*args, num_rays=RAYS, exposure_refine=True, exposure_mode="hsv")
    assert tr.data.gains is None and tr.data.exposure_master is None         # a refused trainer changed nothing on the data
    assert "fg" not in tr.data.sample(64)


# ---------------------------------------------------------------------------------------------------------------- end to end
STOPS, EX_LR, EX_STEPS, FIT_STEPS = 0.5, 1e-2, 640, 1024


def _teacher_views(n_views, H, W):
    """tools/train_loop.py's teacher (a random network on a sphere-and-boxes occupancy grid) -> uint8 RGBA views, poses, intrinsics"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.rays import get_rays
    from laenerf_amd.renderer import NeRFRenderer
    with torch.random.fork_rng(devices=[DEV]):
        torch.manual_seed(11)
        net = NeRFNetwork(bound=1).to(DEV).eval()
        net.encoder.embeddings.data.uniform_(-1.0, 1.0)
        net.sigma_net.weights.data.mul_(1.5)
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(DEV).eval()
    r.density_bitfield = torch.from_numpy(S.pack_bits_np(S.sphere_density_grid(cascade=r.cascade, bound=1.0), 10.0)).to(DEV)
    poses = S.lookat_poses(n_views, radius=3.2, seed=0)
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    intr = (focal, focal, W / 2, H / 2)
    out = []
    with torch.no_grad():
        for i in range(n_views):
            ray = get_rays(torch.from_numpy(poses[i:i + 1]).to(DEV), intr, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=0, max_steps=1024)
            ws = res["weights_sum"].float().clamp(0, 1)
            rgb = torch.where(ws[:, None] > 0, res["image"].float() / ws.clamp(min=1e-6)[:, None], torch.zeros_like(res["image"].float()))
            rgba = torch.cat([rgb.clamp(0, 1), ws[:, None]], 1).reshape(H, W, 4)
            out.append((rgba * 255 + 0.5).to(torch.uint8).cpu().numpy())
    return np.stack(out), poses, intr


def test_exposures_are_recovered_against_a_frozen_student():
    """directional, end to end: a student fitted on the true images, then frozen (network lr = 0) while a second Trainer trains on copies
    whose exposure was perturbed by up to half a stop (perturb_exposures, zero mean).  With refinement the RMS of exposures() + u -- what
    is left of the perturbation after the learned gain -- ends strictly below the RMS of u and the loss falls; the same run with
    exposure_lr = 0 moves no gain and ends on a higher loss (the two runs draw the same pixels).
    exposure_lr = 1e-2 over 640 steps of one image each (80 per image), decayed to a tenth: Adam moves a gain by about lr per step, so
    an image can cover 80 * 1e-2 * 0.39 (the mean of the decay) = 0.31 stops, the RMS of a uniform draw in [-0.5, 0.5] (0.29).
    Measured on the MI355X: RMS of the exposure error 0.2742 -> 0.0720 stops refined (0.2742 frozen); loss first 16 8.04e-4, last 16
    1.93e-4 refined against 7.73e-4 frozen; the fit's own last-16 loss on the true images 1.10e-4."""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    img, poses, intr = _teacher_views(8, 64, 64)
    torch.manual_seed(0)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1, density_thresh=10).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    true_data = ResidentImages.from_arrays(img, poses, intr, bg="random", device=DEV)
    fit = Trainer(r, opt, true_data, FIT_STEPS, LR, num_rays=RAYS, seed=0).train(FIT_STEPS)
    fit_loss = float(fit.losses()[-16:].mean())
    shifted, u = E.perturb_exposures(img, STOPS, seed=5)
    rms = lambda a: float(np.sqrt(np.mean(a * a)))
    rms0 = rms(u)
    assert rms0 > 0.1
    weights = [p.detach().clone() for p in net.parameters()]
    grid_state = (r.density_grid.clone(), r.density_bitfield.clone(), r.mean_count, r.mean_density, r.iter_density, r.local_step)
    rng_state = torch.cuda.get_rng_state(DEV)
    runs = {}
    for name, elr in (("refined", EX_LR), ("frozen", 0.0)):
        r.density_grid.copy_(grid_state[0]); r.density_bitfield.copy_(grid_state[1])
        r.mean_count, r.mean_density, r.iter_density, r.local_step = grid_state[2:]
        torch.cuda.set_rng_state(rng_state, DEV)
        data = ResidentImages.from_arrays(shifted, poses, intr, bg="random", device=DEV)
        tr = Trainer(r, opt, data, EX_STEPS, 0.0, num_rays=RAYS, seed=3, exposure_refine=True, exposure_lr=elr).train(EX_STEPS)
        assert all(torch.equal(a, b.detach()) for a, b in zip(weights, net.parameters()))      # the student is frozen
        losses = tr.losses()
        runs[name] = (rms(tr.exposures() + u), float(losses[:16].mean()), float(losses[-16:].mean()), tr.gains().cpu().numpy())
        print(f"exposure {name}: fit loss {fit_loss:.3e}; rms stops {rms0:.4f} -> {runs[name][0]:.4f}, loss first 16 {runs[name][1]:.4e} "
              f"last 16 {runs[name][2]:.4e}, skipped {tr.steps_skipped}")
    left, first, last, _ = runs["refined"]
    assert left < rms0
    assert last < first
    f_left, _, f_last, f_gains = runs["frozen"]
    assert f_left == rms0 and f_gains.tobytes() == np.ones((8, 3), np.float32).tobytes()      # the frozen run moved no gain
    assert last < f_last
