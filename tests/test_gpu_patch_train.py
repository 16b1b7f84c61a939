"""Patch-based training with an LPIPS term on the GPU: the patch sampler against its numpy restatement, lae_get_rays and torch's
blend; pack / unpack against their restatements; the head's gradient through the C ABI against the float64 restatement;
losses.lpips_patch_loss against the chain written with torch operators; the Trainer's patch mode (graph replay, resume, refusals)."""
import numpy as np
import pytest
import torch

import patch_train_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu

N_IMG, H, W, P, N_PATCH = 3, 33, 40, 32, 2
SEED = 0x1234_5678_9ABC


# ---------------------------------------------------------------------------------------------------------------- the sampler
def _scene(C, dtype, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        img = torch.from_numpy(rng.integers(0, 256, size=(N_IMG, H, W, C), dtype=np.uint8))
    else:
        img = torch.from_numpy(rng.random((N_IMG, H, W, C), dtype=np.float32)).to(dtype)
    return img, S.lookat_poses(N_IMG, seed=seed), (31.5, 33.0, W / 2 + 0.3, H / 2 - 0.7)


@pytest.mark.parametrize("mode", ["image", "all"])
@pytest.mark.parametrize("bg", ["white", "random"])
@pytest.mark.parametrize("C,dtype", [(4, torch.uint8), (3, torch.float16)])
def test_patch_batch_matches_restatement_get_rays_and_blend(mode, bg, C, dtype):
    from laenerf_amd import _lib
    from laenerf_amd.data import ResidentImages, draw_background, draw_patches
    img, poses, intr = _scene(C, dtype)
    step, n = 41, N_PATCH * P * P
    d = ResidentImages.from_arrays(img, poses, intr, mode=mode, bg=bg, seed=SEED, device=DEV)
    b = d.sample(n, step=step, patch_size=P)
    assert b["patch_size"] == P and int(d.step.item()) == step + 1
    im, row, col, inds = draw_patches(SEED, step, N_PATCH, P, N_IMG, H, W, mode)
    assert np.array_equal(b["inds"].cpu().numpy(), inds)
    assert (row == 0).all() and col.max() <= 7
    # rays, nears, fars: lae_get_rays on the drawn pixels, one pose per ray
    im_ray, px = inds // (H * W), inds % (H * W)
    Pm = d.poses[torch.from_numpy(im_ray).to(DEV)].contiguous()
    ro = torch.empty(n, 1, 3, device=DEV); rd = torch.empty_like(ro)
    ne = torch.empty(n, 1, device=DEV); fa = torch.empty_like(ne)
    pix = torch.from_numpy(px).to(DEV).contiguous()
    _lib.check(_lib.load().lae_get_rays(_lib.ptr(Pm), n, *intr, H, W, _lib.ptr(pix), 1, 1, 0, 0.0, 0.0, _lib.ptr(ro), _lib.ptr(rd),
                                        _lib.ptr(d.aabb), d.min_near, _lib.ptr(ne), _lib.ptr(fa), _lib.stream()), "get_rays")
    for got, want in ((b["rays_o"], ro.view(n, 3)), (b["rays_d"], rd.view(n, 3)), (b["nears"], ne.view(n)), (b["fars"], fa.view(n))):
        assert torch.equal(got, want)
    # gt: torch's CPU expression on the same background (words 2..4 of ray r, as the plain sampler)
    f = img.float() / 255 if img.dtype == torch.uint8 else img.float()
    texel = f.reshape(-1, C)[torch.from_numpy(inds)]
    if bg == "random":
        back = torch.from_numpy(draw_background(SEED, step, n))
        assert torch.equal(b["bg"].cpu(), back)
    else:
        assert b["bg"] == 1
        back = 1
    want = texel[:, :3] * texel[:, 3:] + back * (1 - texel[:, 3:]) if C == 4 else texel
    assert torch.equal(b["gt"].cpu(), want)


def test_captured_patch_sampler_draws_fresh_batches():
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(4, torch.uint8)
    d = ResidentImages.from_arrays(img, poses, intr, seed=77, device=DEV)
    s, n = 1000, N_PATCH * P * P
    keys = ("rays_o", "rays_d", "nears", "fars", "gt", "bg", "inds")
    eager = []
    for i in range(3):
        eager.append({k: v.clone() for k, v in d.sample(n, step=s + i, patch_size=P).items() if torch.is_tensor(v)})
        assert int(d.step.item()) == s + i + 1                   # one per call
    assert not torch.equal(eager[0]["inds"], eager[1]["inds"])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = d.sample(n, patch_size=P)
    d.step.fill_(s)
    for i in range(3):
        g.replay()
        for k in keys:
            assert torch.equal(out[k], eager[i][k]), (i, k)
    assert int(d.step.item()) == s + 3


def test_patch_sampler_refusals():
    from laenerf_amd import _lib
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(4, torch.uint8)
    d = ResidentImages.from_arrays(img, poses, intr, seed=1, device=DEV)
    o = d._buffers(33 * 33)
    p = _lib.ptr

    def call(P_, N_):
        return _lib.load().lae_sample_train_batch_patch(
            p(d.images), 0, N_IMG, H, W, 4, p(d.poses), *d.intrinsics, N_, P_, p(d.aabb), d.min_near, d.seed, p(d.step), 0, 1, 0,
            p(o["rays_o"]), p(o["rays_d"]), p(o["nears"]), p(o["fars"]), p(o["gt"]), p(o["bg"]), p(o["inds"]), _lib.stream())
    d.step.fill_(5)
    assert call(H, H * H) == -1 and call(1, 16) == -1 and call(32, 1000) == -1 and call(32, 1025) == -1
    assert int(d.step.item()) == 5                               # refused before any launch: the counter did not move
    for P_, n in ((H, H * H), (32, 1000), (40, 1600)):
        with pytest.raises(ValueError):
            d.sample(n, patch_size=P_)
    d2 = ResidentImages.from_arrays(img, poses, intr, seed=1, device=DEV, error_map=True)
    with pytest.raises(ValueError, match="error map"):
        d2.sample(1024, patch_size=32)
    d3 = ResidentImages.from_arrays(img, poses, intr, seed=1, device=DEV)
    d3.enable_exposure_refinement()
    with pytest.raises(ValueError, match="exposure gains"):
        d3.sample(1024, patch_size=32)


# ---------------------------------------------------------------------------------------------------------------- pack / unpack
@pytest.mark.parametrize("n_patch", [1, 3])
@pytest.mark.parametrize("normalize", [False, True])
def test_pack_and_unpack_are_byte_equal_to_their_restatements(n_patch, normalize):
    from laenerf_amd.losses import patch_pack
    from laenerf_amd.metrics import patch_pack_numpy
    rng = np.random.default_rng(11 + n_patch)
    pred = rng.random((n_patch * P * P, 3), dtype=np.float32) * 1.2 - 0.1
    gt = rng.random((n_patch * P * P, 3), dtype=np.float32)
    tp = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    x = patch_pack(tp, torch.from_numpy(gt).to(DEV), P, normalize)
    want = patch_pack_numpy(pred, gt, P, normalize)
    assert x.shape == (2 * n_patch, 3, P, P)
    assert np.array_equal(x.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the transpose: torch autograd of the restatement written with torch operators (CPU, fp32)
    gx = torch.from_numpy(rng.standard_normal((2 * n_patch, 3, P, P)).astype(np.float32))
    cp = torch.from_numpy(pred).requires_grad_(True)
    xr = U.torch_pack(cp, torch.from_numpy(gt), P, normalize)
    assert np.array_equal(xr.detach().numpy().view(np.uint32), want.view(np.uint32))
    xr.backward(gx)
    x.backward(gx.to(DEV))
    assert np.array_equal(tp.grad.cpu().numpy().view(np.uint32), cp.grad.numpy().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- the head's gradient
LAYERS = [(5, 1), (64, 49), (70, 9), (192, 257), (384, 1)]       # (C, hw): a partial wave, several blocks, a tail, hw = 1


@pytest.mark.parametrize("both", [0, 1])
@pytest.mark.parametrize("n_pairs", [1, 3])
def test_head_gradient_is_one_fp32_rounding_of_the_float64_restatement(n_pairs, both):
    from laenerf_amd.metrics import lpips_head_grad_numpy
    rng = np.random.default_rng(100 + n_pairs)
    feats = [np.maximum(rng.standard_normal((2 * n_pairs, C, hw)), 0).astype(np.float32) for C, hw in LAYERS]   # exact zeros from a ReLU
    for f in (feats[1], feats[3]):
        f[0, :, 3] = 0                                           # one all-zero pixel on side 0 ...
        f[2 * n_pairs - 1, :, 5] = 0                             # ... and one on side 1
    weights = [rng.random(C).astype(np.float32) for C, _ in LAYERS]
    gout = rng.standard_normal(n_pairs)
    if n_pairs > 1:
        gout[1] = 0.0
    tf = [torch.from_numpy(f).to(DEV) for f in feats]
    tw = [torch.from_numpy(w).to(DEV) for w in weights]
    tg = torch.from_numpy(gout).to(DEV)
    got = [g.cpu().numpy() for g in U.head_grad_abi(tf, tw, tg, both)]
    again = [g.cpu().numpy() for g in U.head_grad_abi(tf, tw, tg, both)]
    ref = lpips_head_grad_numpy(feats, weights, gout, both=bool(both))
    floor = 2.0 ** -149                                          # the spacing of fp32 subnormals: results below 2^-126
    for (C, hw), g, g2, r in zip(LAYERS, got, again, ref):
        assert np.isfinite(g).all(), (C, hw)                     # every element written (the buffers were NaN), none NaN
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32)), (C, hw)
        err = np.abs(g.astype(np.float64) - r)
        assert (err <= 2.0 ** -23 * np.abs(r) + floor).all(), (C, hw, float((err / np.maximum(np.abs(r), 1e-300)).max()))
        if not both:
            assert (g[0::2] == 0).all()
        assert np.abs(g[1::2]).max() > 0 or n_pairs == 1 and gout[0] == 0
    for g in (got[1], got[3]):
        assert (g[2 * n_pairs - 1, :, 5] == 0).all() and (g[0, :, 3] == 0).all()      # the zero-norm rule
    if n_pairs > 1:
        assert all((g[2:4] == 0).all() for g in got)             # gout = 0


# ---------------------------------------------------------------------------------------------------------------- lpips_patch_loss
def test_lpips_patch_loss_value_and_gradient():
    """The kernel chain (pack, trunk, lae_lpips_head / _grad, unpack) against the same chain written with torch operators.  Their
    difference is the trunk's fp32 arithmetic: the torch chain in fp32 on the device is measured against the torch chain in float64
    (CPU) on the same inputs, and the kernel chain is allowed four times that error.
    Measured on the MI355X (max |difference| of the gradient on pred_rows, whose largest entry is 1.7e-3 / 4.2e-3):
      normalize=False: torch fp32 chain 3.98e-9, kernel chain 3.29e-9;  normalize=True: torch fp32 chain 8.34e-9, kernel chain 6.80e-9."""
    from laenerf_amd.losses import lpips_patch_loss, patch_pack
    lp = U.lpips()
    rng = np.random.default_rng(21)
    n = 2 * P * P
    gt = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).to(DEV)
    pred0 = (gt + torch.from_numpy(0.2 * rng.standard_normal((n, 3)).astype(np.float32)).to(DEV)).clamp(0, 1)
    for normalize in (False, True):
        pred = pred0.clone().requires_grad_(True)
        loss = lpips_patch_loss(pred, gt, P, lp, normalize)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.per_patch.dtype == torch.float64 and loss.per_patch.shape == (2,)
        # LPIPS.forward on the packed input: the same bits where its convolutions are asked to be deterministic as the loss asks;
        # as it is called by default, its own two calls on one input were measured to differ in the last taps' last bits (4e-9),
        # so there the bound is a convolution's worst-case fp32 rounding, K * 2^-24 with the trunk's largest fan-in K = 384 * 9
        x = patch_pack(pred0, gt, P, normalize)
        was = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            want = lp(x)
        finally:
            torch.backends.cudnn.deterministic = was
        assert torch.equal(loss.per_patch, want) and torch.equal(loss.detach(), want.mean().float())
        assert abs(float(lp(x).mean()) - float(loss.detach())) <= 384 * 9 * 2.0 ** -24 * float(loss.detach())
        assert float(loss) > 0
        loss.backward()
        g = pred.grad.double().cpu()
        v64, g64 = U.torch_chain(lp, pred0, gt, P, normalize, torch.float64, "cpu")
        v32, g32 = U.torch_chain(lp, pred0, gt, P, normalize, torch.float32, DEV)
        e32 = float((g32.double().cpu() - g64).abs().max())
        e = float((g - g64).abs().max())
        print(f"lpips_patch_loss normalize={normalize}: value {float(loss):.6f} (float64 {float(v64):.6f}); gradient max |g64| "
              f"{float(g64.abs().max()):.3e}, torch fp32 chain error {e32:.3e}, kernel chain error {e:.3e}")
        assert torch.isfinite(g).all() and e32 > 0
        assert e <= 4 * e32
        assert abs(float(loss) - float(v64)) <= 4 * max(abs(float(v32) - float(v64)), 2.0 ** -24 * float(v64))


# ---------------------------------------------------------------------------------------------------------------- the Trainer
STEPS = 32


def _run(steps=STEPS, **kw):
    tr = U.make_trainer(**kw)
    tr.train(steps)
    return tr


@pytest.fixture(scope="module")
def eager_run():
    """48 eager patch steps, shared: (state, losses, perceptual losses, trainer).  The first 32 are the steps the checks are about;
    the group at step 16 has a capacity no earlier step reached, so a graph trainer runs it eagerly (workspaces cannot grow inside
    a capture) and only the group at step 32 is captured and replayed: 16 more steps put a replay into the comparison."""
    tr = _run(steps=STEPS + 16, graph=False)
    return U.state(tr), tr.losses(), tr.perceptual_losses(), tr


def test_graph_patch_trainer_equals_eager(eager_run):
    state, losses, perc, te = eager_run
    tg = _run(steps=STEPS + 16, graph=True)
    assert np.array_equal(tg.losses()[:STEPS], losses[:STEPS]) and np.array_equal(tg.perceptual_losses()[:STEPS], perc[:STEPS])
    U.assert_same(U.state(tg), state)
    assert np.array_equal(tg.losses(), losses) and np.array_equal(tg.perceptual_losses(), perc)
    assert losses.shape == perc.shape == (STEPS + 16,) and np.isfinite(losses).all()
    assert np.isfinite(perc).all() and (perc > 0).all()
    assert tg.truncated_steps() == 0 and te.truncated_steps() == 0
    assert tg.r.peak_count > 0 and tg.r.peak_count == te.r.peak_count
    assert tg.captures >= 1 and te.captures == 0
    print("patch trainer: peak", tg.r.peak_count, "mean", tg.r.mean_count, "limit", tg._m(), "captures", tg.captures, "warm", tg.warm_groups,
          "peak/mean", tg.peak_to_mean())


def test_zero_perceptual_weight_equals_the_chain_skipped():
    a = U.make_trainer(graph=False, perceptual_weight=0.0)
    a.train(STEPS)
    b = U.make_trainer(graph=False, perceptual_weight=0.0)
    b.skip_perceptual = True
    b.train(STEPS)
    U.assert_same(U.state(a), U.state(b))
    assert np.array_equal(a.losses(), b.losses())
    assert (a.perceptual_losses() > 0).all() and (b.perceptual_losses() == 0).all()


def test_saved_and_resumed_patch_run_equals_the_uninterrupted_one(tmp_path):
    full = U.make_trainer(graph=True, ema_decay=0.95, epoch_len=5)
    full.train(STEPS)
    first = U.make_trainer(graph=True, ema_decay=0.95, epoch_len=5)
    first.train(16)
    path = first.save_checkpoint(str(tmp_path / "patch.pth"))
    cfg = first.config()
    assert cfg["patch_size"] == U.P and cfg["perceptual_weight"] == 1e-3 and cfg["perceptual_normalize"] is False and cfg["patch_headroom"] == 2.0
    resumed = U.make_trainer(net_seed=1234, torch_seed=4321, seed=99, graph=True, ema_decay=0.95, epoch_len=5)
    resumed.load_checkpoint(path)
    assert resumed.r.peak_count == first.r.peak_count
    resumed.train(STEPS - 16)
    U.assert_same(U.state(resumed), U.state(full))
    assert np.array_equal(resumed.losses(), full.losses()[16:]) and np.array_equal(resumed.perceptual_losses(), full.perceptual_losses()[16:])
    assert resumed.r.peak_count == full.r.peak_count and resumed.truncated_steps() == full.truncated_steps() == 0
    # a trainer without patches refuses the file (the configuration differs)
    plain = U.make_trainer(patch_size=1)
    with pytest.raises(ValueError, match="patch_size"):
        plain.load_checkpoint(path)


def test_refused_combinations_leave_the_data_untouched():
    from laenerf_amd.trainer import Trainer
    r, opt, data = U.setup()
    lp = U.lpips()
    seed, aabb = data.seed, data.aabb.clone()
    for kw in ({"error_map": "ema"}, {"error_map": "fixed"}, {"depth_weight": 0.1}, {"distort_weight": 0.01}, {"opacity_weight": 0.01},
               {"pixel_weights": True}, {"second_weight": 0.5}, {"pose_refine": True}, {"exposure_refine": True}, {"patch_size": 16},
               {"lpips": None}, {"patch_size": 64}):
        args = {"patch_size": U.P, "lpips": lp, **kw}
        with pytest.raises(ValueError):
            Trainer(r, opt, data, U.ITERS, U.LR, num_rays=U.RAYS, seed=5, **args)
        assert data.error_map is None and data.gains is None and data.train_poses is None and data.depths is None
        assert data.seed == seed and torch.equal(data.aabb, aabb) and r.count_limit is None
    for loss in ("l1", "huber", "mape"):                          # every colour criterion works with patches
        tr = U.make_trainer(graph=False, loss=loss)
        tr.train(2)
        assert np.isfinite(tr.losses()).all() and (tr.perceptual_losses() > 0).all()


def test_default_trainer_is_the_hand_written_loop():
    """Trainer() without the new arguments: the losses and parameters of the loop written out by hand (the check of
    test_gpu_trainer.py, here on the 64 x 64 scene and 32 steps), and nothing of the patch mode switched on"""
    from laenerf_amd.trainer import lr_schedule
    tr = U.make_trainer(patch_size=1, graph=False, torch_seed=99, seed=5)
    assert tr.r.count_limit is None and tr.lpips is None and tr.n_rays == U.RAYS and "patch_size" not in tr.config()
    tr.train(STEPS)
    assert tr.perceptual_losses().size == 0 and tr.truncated_steps() == 0

    r2, opt2, data2 = U.setup(device_lr=False)
    data2.seed = 5
    table = lr_schedule(U.LR, U.ITERS, STEPS)
    torch.manual_seed(99)
    r2.mark_untrained_grid(data2.poses, data2.intrinsics)
    losses = []
    r2.model.train()
    for s in range(STEPS):
        if s % 16 == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                r2.update_extra_state()
        opt2.set_lr(float(table[s, 0]))
        b = data2.sample(U.RAYS, step=s)
        with torch.autocast("cuda", dtype=torch.float16):
            res = r2.render_train(b["rays_o"], b["rays_d"], bg_color=b["bg"], perturb=True, gt=b["gt"], scaler=opt2)
        opt2.backward(res["loss"])
        opt2.step()
        losses.append(res["loss"].unscaled.clone())
    for i, ((p, m, v, *_), (p2, m2, v2, *_)) in enumerate(zip(tr.opt.items, opt2.items)):
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), i
    assert torch.equal(tr.r.density_grid, r2.density_grid)
    assert np.array_equal(tr.losses(), torch.stack(losses).cpu().numpy())
