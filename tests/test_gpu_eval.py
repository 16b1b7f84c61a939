"""Evaluation on the device: lae_eval_view and the LPIPS head against numpy / fp64 restatements, the Trainer's gated EMA
inside captured groups, evaluate_one_epoch / test."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV
from lpips_util import head_fp64, lpips_fp64
from test_gpu_trainer import _images, _setup, _state, _assert_same

pytestmark = pytest.mark.gpu


def _gt(rng, dtype, n, H, W, C):
    if dtype == torch.uint8:
        img = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
        if C == 4:
            img[..., 3] = np.where(rng.random((n, H, W)) < 0.3, 255, np.where(rng.random((n, H, W)) < 0.3, 0, img[..., 3]))
        return img
    img = rng.random((n, H, W, C)).astype(np.float32)
    return img.astype(np.float16) if dtype == torch.float16 else img


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("with_mask", [False, True])
def test_eval_view_against_numpy(dtype, C, with_mask):
    from laenerf_amd.metrics import eval_view, eval_view_numpy
    H, W = 37, 53                                         # odd: a partial last quad; view 1 of the stack is not 16-byte aligned
    rng = np.random.default_rng(C * 10 + int(with_mask))
    imgs = torch.from_numpy(_gt(rng, dtype, 2, H, W, C)).to(DEV)
    for view in (0, 1):
        pred_np = (rng.random((H * W, 3)) * 1.2 - 0.1).astype(np.float32)
        depth_np = (rng.random(H * W) * 1.4 - 0.2).astype(np.float32)
        mask_np = np.where(rng.random(H * W) < 0.5, 0, rng.integers(1, 256, H * W)).astype(np.uint8) if with_mask else None
        pred, depth = torch.from_numpy(pred_np).to(DEV), torch.from_numpy(depth_np).to(DEV)
        mask = torch.from_numpy(mask_np).to(DEV) if with_mask else None
        gt = imgs[view]
        outs = []
        for _ in range(2):
            o = {"sse": torch.zeros(1, dtype=torch.float64, device=DEV), "gt_out": torch.empty(H * W, 3, device=DEV),
                 "rgb_u8": torch.empty(H * W, 3, dtype=torch.uint8, device=DEV), "depth_u8": torch.empty(H * W, dtype=torch.uint8, device=DEV),
                 "lpips_in": torch.empty(2, 3, H, W, device=DEV)}
            if with_mask:
                o["masked_sse"] = torch.zeros(1, dtype=torch.float64, device=DEV)
            eval_view(pred, gt, depth=depth, bg=1.0, mask=mask, **o)
            outs.append({k: v.cpu().numpy() for k, v in o.items()})
        a, b = outs
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k                         # two runs, the same bits
        ref = eval_view_numpy(pred_np, gt.cpu().numpy(), depth=depth_np, bg=1.0, mask=mask_np)
        assert a["gt_out"].tobytes() == ref["gt"].tobytes()
        # ... and the same bits as Trainer.evaluate's torch expression of the blend
        img = gt.reshape(-1, C)
        img = img.float() / 255 if img.dtype == torch.uint8 else img.float()
        tgt = img[:, :3] * img[:, 3:] + 1.0 * (1 - img[:, 3:]) if C == 4 else img
        assert torch.equal(torch.from_numpy(a["gt_out"]).to(DEV), tgt)
        assert abs(a["sse"][0] - ref["sse"]) <= 1e-12 * ref["sse"]
        if with_mask:
            assert abs(a["masked_sse"][0] - ref["masked_sse"]) <= 1e-12 * ref["masked_sse"]
        assert np.array_equal(a["rgb_u8"], ref["rgb_u8"]) and np.array_equal(a["depth_u8"], ref["depth_u8"])
        assert a["lpips_in"].reshape(2, 3, -1).tobytes() == ref["lpips_in"].tobytes()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(800, 800), (37, 53)])
def test_lpips_head_against_fp64_restatement(B, hw):
    from laenerf_amd.metrics import LPIPS
    lp = LPIPS.random(1, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(B * 7 + hw[0])
    x = (torch.rand(2 * B, 3, *hw, device=DEV, generator=g) * 2 - 1) * 2
    feats = lp.features(x)
    got = lp.head(feats).cpu().numpy()
    want = head_fp64(feats, lp.lins).cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)) and np.all(want > 0)
    assert lp.head(feats).cpu().numpy().tobytes() == got.tobytes()
    # identical images -> exactly 0.  The pairs' features are made identical here: MIOpen may give two equal images of one
    # batch features that differ in the last bit (observed at 37 x 53: 2.2e-16)
    same = [f.clone() for f in feats]
    for f in same:
        f[1::2] = f[0::2]
    assert np.all(lp.head(same).cpu().numpy() == 0.0)


def test_lpips_whole_chain_against_fp64():
    from laenerf_amd.metrics import LPIPS, eval_view
    lp = LPIPS.random(2, device=DEV)
    H, W = 64, 72
    rng = np.random.default_rng(3)
    gt = torch.from_numpy(rng.random((H, W, 3)).astype(np.float32)).to(DEV)
    pred = (gt + torch.from_numpy(rng.normal(0, 0.05, (H, W, 3)).astype(np.float32)).to(DEV)).reshape(-1, 3).contiguous()
    lp_in = torch.empty(2, 3, H, W, device=DEV)
    eval_view(pred, gt, lpips_in=lp_in)
    got = float(lp(lp_in).item())
    want = float(lpips_fp64(lp, gt.permute(2, 0, 1)[None], pred.reshape(H, W, 3).permute(2, 0, 1)[None]).item())
    assert abs(got - want) <= 1e-3 * want


def _hand_loop_with_ema(steps, lr, seed, iters, epoch_len, decay, torch_seed):
    """test_gpu_trainer's hand-written eager loop + EMA.update() after exactly the steps that close an epoch"""
    from laenerf_amd.optim import EMA
    from laenerf_amd.trainer import lr_schedule
    r, opt, data = _setup(lr, device_lr=False)
    torch.manual_seed(torch_seed)
    data.seed = seed
    ema = EMA(r.parameters(), decay=decay)
    table = lr_schedule(lr, iters, steps)
    r.mark_untrained_grid(data.poses, data.intrinsics)
    r.model.train()
    for s in range(steps):
        if s % 16 == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                r.update_extra_state()
        opt.set_lr(float(table[s, 0]))
        b = data.sample(4096, step=s)
        with torch.autocast("cuda", dtype=torch.float16):
            res = r.render_train(b["rays_o"], b["rays_d"], bg_color=b["bg"], perturb=True, gt=b["gt"], scaler=opt)
        opt.backward(res["loss"])
        opt.step()
        if (s + 1) % epoch_len == 0:
            ema.update()
    return r, opt, ema


def test_trainer_ema_in_captured_groups_equals_eager_and_hand_loop():
    from laenerf_amd.optim import ema_update_steps
    from laenerf_amd.trainer import Trainer
    steps, lr, seed, iters = 64, 1e-2, 4, 300
    runs = []
    for graph in (True, False):
        r, opt, data = _setup(lr)
        torch.manual_seed(5)
        tr = Trainer(r, opt, data, iters, lr, num_rays=4096, seed=seed, graph=graph, capacity="exact", ema_decay=0.95)
        assert tr.epoch_len == data.n_img == 6
        tr.train(steps)
        runs.append((r, opt, tr))
    (ra, oa, ta), (rb, ob, tb) = runs
    assert ta.captures >= 1 and tb.captures == 0
    ups = ema_update_steps(0, steps, 6)
    assert sum(1 for s in ups if s > 16) >= 3                       # epochs closing inside the captured groups
    _assert_same(_state(ra, oa) + ta.ema.shadow_params, _state(rb, ob) + tb.ema.shadow_params)
    rc, oc, ema = _hand_loop_with_ema(steps, lr, seed, iters, 6, 0.95, torch_seed=5)
    _assert_same([p.detach() for p in ra.parameters() if p.requires_grad], [p.detach() for p in rc.parameters() if p.requires_grad])
    _assert_same(ta.ema.shadow_params, ema.shadow_params)
    assert ta.ema.state_dict()["num_updates"] == tb.ema.state_dict()["num_updates"] == ema.num_updates == len(ups)


def _captured_group_nodes(tr):
    """nodes of one 16-step group captured the way Trainer._run_group does (no replay)"""
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))     # the runtime torch has mapped
    g = torch.cuda.CUDAGraph(keep_graph=True)
    m_cap = tr._m_cap()
    local = tr.r.local_step
    with torch.cuda.graph(g, pool=tr._pool):
        for k in range(16):
            tr._step(k, m_cap)
    tr.r.local_step = local
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return n.value


def test_no_ema_adds_no_launch_to_a_captured_group():
    from laenerf_amd.trainer import Trainer
    counts = {}
    for decay in (None, 0.95):
        r, opt, data = _setup()
        torch.manual_seed(6)
        tr = Trainer(r, opt, data, 300, 1e-2, num_rays=4096, seed=2, capacity="exact", ema_decay=decay)
        tr.train(48)
        counts[decay] = _captured_group_nodes(tr)
    assert counts[0.95] == counts[None] + 16                        # one gated launch per step, nothing without an EMA


def test_evaluate_one_epoch_restores_weights_and_next_group_is_unchanged():
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.metrics import LPIPS
    from laenerf_amd.trainer import Trainer
    img, poses, intr = _images(n=3, H=48, W=40, seed=9)
    states = []
    for evaluate in (True, False):
        r, opt, data = _setup()
        torch.manual_seed(8)
        tr = Trainer(r, opt, data, 300, 1e-2, num_rays=4096, seed=3, capacity="exact", ema_decay=0.95)
        tr.train(48)
        if evaluate:
            before = _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None]
            test = ResidentImages.from_arrays(img, poses, intr, device=DEV)
            masks = [torch.zeros(48, 40, dtype=torch.uint8, device=DEV), None, torch.full((48, 40), 255, dtype=torch.uint8, device=DEV)]
            res = tr.evaluate_one_epoch(test, lpips=LPIPS.random(0, device=DEV), masks=masks)
            assert res["psnr"].shape == (3,) and np.isfinite(res["psnr"]).all() and np.all(res["lpips"] > 0)
            assert np.isnan(res["masked_mse"][1]) and res["masked_mse"][2] == 0 and res["masked_mse"][0] > 0
            assert res["mean_masked_mse"] == pytest.approx(res["masked_mse"][0] / 2, rel=1e-12)
            rgb, depth = tr.test(test)
            assert rgb.shape == (3, 48, 40, 3) and depth.shape == (3, 48, 40) and rgb.dtype == depth.dtype == torch.uint8
            _assert_same(before, _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None])
        tr.train(16)                                                 # the next captured group
        states.append(_state(r, opt) + tr.ema.shadow_params + [tr.ema.device_count()[:1].clone()])
    _assert_same(*states)


def test_evaluate_one_epoch_psnr_matches_evaluate_with_ema_weights():
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.trainer import Trainer
    r, opt, data = _setup()
    torch.manual_seed(10)
    tr = Trainer(r, opt, data, 300, 1e-2, num_rays=4096, seed=6, ema_decay=0.95)
    tr.train(48)
    img, poses, intr = _images(n=3, H=48, W=40, seed=12)
    for dtype in ("uint8", "float16"):
        images = img if dtype == "uint8" else (img.astype(np.float32) / 255).astype(np.float16)
        test = ResidentImages.from_arrays(images, poses, intr, device=DEV)
        res = tr.evaluate_one_epoch(test)
        tr.ema.store(); tr.ema.copy_to()
        want = [tr.evaluate([i], data=test, bg_color=1.0) for i in range(3)]
        tr.ema.restore()
        assert np.all(np.abs(res["psnr"] - np.array(want)) <= 1e-4), (res["psnr"], want)
        assert res["mean_psnr"] == pytest.approx(float(np.mean(res["psnr"])))
