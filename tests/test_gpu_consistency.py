"""lae_consistency_pair (through metrics.consistency_pair) against the float64 restatement metrics.consistency_numpy on the
two-view fixture of tests/consistency_util.py, and Trainer.evaluate_consistency against its hand-written loop.

Tolerances (tests/test_consistency_cpu.py measures the figures they rest on and asserts them on the CPU):
  validity   identical to float64 wherever the float64 margin is >= 1e-3; the pixels inside that band may be at most 2 % of the image
             (the fixture has none).  1e-3 is over a hundred times the float32 flow error (8.6e-6 px): an exclusion band, not a
             tolerance on the result.
  warped     measured max |float32 restatement - float64 restatement| on the fixture: 2.93e-7 (asserted <= 3.0e-7 on the CPU).
             Allowed: 8 x 3.0e-7 = 2.4e-6 -- the kernel contracts to fma and may order the bilinear sum differently, each a few ulp
             of a value that is at most 1.
  sse        count * 3 * (2 tol_w max|Fw - F_b| + tol_w^2) against the float64 sum of the restated err over the kernel's own valid.
  lpips_in   tol_w / min(LPIPS_SCALE), with the kernel's valid.
  identity   with a = b at most H pixels with geometry may be invalid (the float32 restatement loses 4 at 24 x 40 and 8 at 37 x 53:
             pixels whose landing point rounds just below their own row or column, next to a pixel without geometry or past the
             frame's edge) and the largest err is <= 1e-10: a coordinate error under 1e-5 px times a neighbour colour difference
             under 0.2 is 2e-6 per channel; squared, times 3.
The LPIPS chain runs at 37 x 53 only: AlexNet's second max-pool has no output for an image under 31 px (24 x 40)."""
import numpy as np
import pytest
import torch

import consistency_util as U
from gpu_util import DEV
from test_consistency_cpu import MARGIN, MARGIN_CAP, MEASURED_W

pytestmark = pytest.mark.gpu

TOL_W = 8 * MEASURED_W
OUTS = ("sse", "count", "valid", "warped", "lpips_in")


def _dev(f, **over):
    f = dict(f, **over)
    t = {k: torch.from_numpy(np.array(f[k])).to(DEV) for k in ("frame_a", "frame_b", "depth_a", "opacity_a", "depth_b",
                                                                         "opacity_b", "pose_a", "pose_b")}
    return [t["frame_a"], t["frame_b"], t["depth_a"], t["opacity_a"], t["depth_b"], t["opacity_b"], t["pose_a"], t["pose_b"],
            f["intrinsics"], f["H"], f["W"]]


def _outs(H, W):
    return {"sse": torch.full((1,), -1.0, dtype=torch.float64, device=DEV), "count": torch.full((1,), -1.0, dtype=torch.float64, device=DEV),
            "valid": torch.full((H * W,), 7, dtype=torch.uint8, device=DEV), "warped": torch.full((H * W, 3), -1.0, device=DEV),
            "lpips_in": torch.full((2, 3, H, W), -1.0, device=DEV)}


def _run(a, H, W, **kw):
    from laenerf_amd.metrics import consistency_pair
    o = _outs(H, W)
    consistency_pair(*a, **o, **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}


def _identity(f):
    return dict(frame_b=f["frame_a"], depth_b=f["depth_a"], opacity_b=f["opacity_a"], pose_b=f["pose_a"])


@pytest.mark.parametrize("shape", U.SHAPES)
def test_pair_against_float64_restatement(shape):
    from laenerf_amd.metrics import LPIPS_SCALE, consistency_numpy
    H, W = shape
    f, r = U.fixture(H, W), U.restated(H, W)
    got = _run(_dev(f), H, W)
    valid = got["valid"].reshape(H, W)
    assert set(np.unique(valid)) <= {0, 1}
    valid = valid.astype(bool)
    band = r["margin"] < MARGIN
    print("valid", valid.sum(), "of", H * W, "restated", r["valid"].sum(), "band", band.sum(), "differ", (valid != r["valid"]).sum())
    assert band.mean() <= MARGIN_CAP
    assert np.array_equal(valid[~band], r["valid"][~band])
    warped = got["warped"].reshape(H, W, 3)
    both = valid & r["valid"]
    dw = np.abs(warped.astype(np.float64) - r["warped"])[both].max()
    print("max |warped - float64|", dw, "allowed", TOL_W)
    assert dw <= TOL_W
    assert np.all(warped[~valid] == 0)
    # count: the popcount of the kernel's own valid, exactly; sse: the float64 sum of the restated err over the same pixels
    assert got["count"][0] == valid.sum()
    want = float(r["err"][valid].sum())
    dmax = np.abs(r["warped"] - f["frame_b"].astype(np.float64))[valid].max()
    tol = valid.sum() * 3 * (2 * TOL_W * dmax + TOL_W ** 2)
    print("sse", got["sse"][0], "restated", want, "allowed", tol, "warp_mse", got["sse"][0] / got["count"][0])
    assert abs(got["sse"][0] - want) <= tol
    lp_want = consistency_numpy(*U.args(f), valid=valid)["lpips_in"]
    dl = np.abs(got["lpips_in"].astype(np.float64) - lp_want).max()
    print("max |lpips_in - float64|", dl, "allowed", TOL_W / min(LPIPS_SCALE))
    assert dl <= TOL_W / min(LPIPS_SCALE)
    assert np.array_equal(got["lpips_in"][0][:, ~valid], got["lpips_in"][1][:, ~valid])


def test_lpips_of_the_pair_against_fp64():
    from laenerf_amd.metrics import LPIPS
    from lpips_util import lpips_fp64
    H, W = 37, 53
    f = U.fixture(H, W)
    got = _run(_dev(f), H, W)
    lp = LPIPS.random(3, device=DEV)
    val = float(lp(torch.from_numpy(got["lpips_in"]).to(DEV)).item())
    valid = torch.from_numpy(got["valid"].reshape(H, W).astype(bool)).to(DEV)
    fb = torch.from_numpy(f["frame_b"].copy()).to(DEV)
    x0 = torch.where(valid[..., None], torch.from_numpy(got["warped"].reshape(H, W, 3)).to(DEV), fb)
    want = float(lpips_fp64(lp, x0.permute(2, 0, 1)[None], fb.permute(2, 0, 1)[None]).item())
    print("lpips", val, "fp64", want)
    assert want > 0 and abs(val - want) <= 1e-3 * want


@pytest.mark.parametrize("shape", U.SHAPES)
def test_uint8_frames_equal_the_fp32_run_on_their_values(shape):
    H, W = shape
    f = U.fixture(H, W)
    a8, b8 = ((f[k] * 255 + 0.5).astype(np.uint8) for k in ("frame_a", "frame_b"))
    g8 = _run(_dev(f, frame_a=a8, frame_b=b8), H, W)
    to_f = lambda u: (torch.from_numpy(u).to(DEV).float() * (1 / 255)).cpu().numpy()         # the kernel's to_f
    gf = _run(_dev(f, frame_a=to_f(a8), frame_b=to_f(b8)), H, W)
    for k in OUTS:
        assert g8[k].tobytes() == gf[k].tobytes(), k
    assert g8["count"][0] > 0 and g8["sse"][0] > 0


@pytest.mark.parametrize("shape", U.SHAPES)
def test_identity_pair(shape):
    H, W = shape
    f = U.fixture(H, W)
    got = _run(_dev(f, **_identity(f)), H, W)
    valid = got["valid"].reshape(H, W).astype(bool)
    geom = f["opacity_a"] >= 0.5
    lost = geom & ~valid
    print("identity: valid", valid.sum(), "of", geom.sum(), "lost at (row, col)", np.argwhere(lost).tolist())
    assert not valid[~geom].any()
    assert lost.sum() <= H
    err = ((got["warped"].reshape(H, W, 3).astype(np.float64) - f["frame_a"].astype(np.float64)) ** 2).sum(-1)
    print("identity: max err", err[valid].max(), "sse", got["sse"][0])
    assert err[valid].max() <= 1e-10
    assert got["sse"][0] <= 1e-10 * valid.sum()


@pytest.mark.parametrize("shape", U.SHAPES)
def test_two_runs_and_a_graph_replay_give_the_same_bits(shape):
    from laenerf_amd.metrics import CONSISTENCY_SCRATCH_DOUBLES, consistency_pair
    H, W = shape
    a = _dev(U.fixture(H, W))
    first, second = _run(a, H, W), _run(a, H, W)
    for k in OUTS:
        assert first[k].tobytes() == second[k].tobytes(), k
    scratch = torch.empty(CONSISTENCY_SCRATCH_DOUBLES, dtype=torch.float64, device=DEV)
    o = _outs(H, W)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        consistency_pair(*a, **o, scratch=scratch)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        consistency_pair(*a, **o, scratch=scratch)
    for k, v in _outs(H, W).items():
        o[k].copy_(v)                                               # the sentinels back in
    g.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert o[k].cpu().numpy().tobytes() == first[k].tobytes(), k


def test_optional_outputs_and_rejection():
    from laenerf_amd import _lib
    from laenerf_amd.metrics import consistency_pair
    H, W = 37, 53
    f = U.fixture(H, W)
    a = _dev(f)
    full = _run(a, H, W)
    sse, count = consistency_pair(*a)
    assert sse.cpu().numpy().tobytes() == full["sse"].tobytes() and count.cpu().numpy().tobytes() == full["count"].tobytes()
    # an empty pair: count == 0 and sse == 0, nothing divided on the device
    zero = np.zeros((H, W), np.float32)
    e = _run(_dev(f, opacity_b=zero, depth_b=zero), H, W)
    assert e["count"][0] == 0 and e["sse"][0] == 0 and not e["valid"].any() and np.isfinite(e["lpips_in"]).all()
    assert np.array_equal(e["lpips_in"][0], e["lpips_in"][1])

    def bad(i, t, **kw):
        b = list(a)
        if i is not None:
            b[i] = t
        with pytest.raises((ValueError, RuntimeError)):
            consistency_pair(*b, **kw)
    bad(0, a[0].half())                                             # dtype of a frame
    bad(1, (a[1] * 255).to(torch.uint8))                            # two frame dtypes
    bad(2, a[2].double())                                           # dtype of a depth
    bad(3, a[3][:-1])                                               # shape
    bad(6, a[6][:3])                                                # a 3 x 4 pose
    bad(0, a[0].cpu())                                              # a CPU tensor
    bad(7, a[7].cpu())
    bad(None, None, valid=torch.empty(H * W, dtype=torch.bool, device=DEV))
    bad(None, None, warped=torch.empty(H * W, 4, device=DEV))
    bad(None, None, sse=torch.zeros(1, device=DEV))
    bad(None, None, min_opacity=0.0)
    bad(9, 1)                                                       # H = 1
    # the entry point itself, before any launch: NULL -> -3, another dtype / a 1-pixel-wide frame -> -1
    lib = _lib.load()
    p = [t.data_ptr() for t in a[:8]]
    s = torch.empty(16384, dtype=torch.float64, device=DEV)
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    call = lambda fa, dt, w, sse_p: lib.lae_consistency_pair(fa, p[1], dt, p[2], p[3], p[4], p[5], p[6], p[7], 40.0, 40.0, W / 2, H / 2, H, w,
                                                             0.5, s.data_ptr(), sse_p, out[1:].data_ptr(), None, None, None, None)
    assert call(None, 2, W, out.data_ptr()) == -3 and call(p[0], 2, W, None) == -3
    assert call(p[0], 1, W, out.data_ptr()) == -1 and call(p[0], 2, 1, out.data_ptr()) == -1
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [0.0, 0.0]


# ---------------------------------------------------------------- Trainer.evaluate_consistency
def _trained(seed=3, steps=48):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.trainer import Trainer
    from test_gpu_trainer import _images, _setup
    r, opt, data = _setup()
    torch.manual_seed(8)
    tr = Trainer(r, opt, data, 300, 1e-2, num_rays=4096, seed=seed, capacity="exact", ema_decay=0.95)
    tr.train(steps)
    img, poses, intr = _images(n=4, H=32, W=32, seed=9)
    return r, opt, tr, ResidentImages.from_arrays(img, poses, intr, device=DEV)


def _hand_loop(tr, test, step, min_opacity, frames=None):
    """render_eval of every view + consistency_pair of every pair (i, i + step), written out"""
    from laenerf_amd.metrics import consistency_pair
    from laenerf_amd.rays import get_rays
    n, H, W = test.n_img, test.H, test.W
    views = []
    with tr._eval_weights(), torch.no_grad():
        for i in range(n):
            ray = get_rays(test.poses[i:i + 1], test.intrinsics, H, W)
            with torch.autocast("cuda", dtype=torch.float16):
                res = tr.r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=False, image_hw=(H, W))
            views.append((res["image"].float().contiguous(), res["depth"].float().contiguous(), res["weights_sum"].float().contiguous()))
    sums = torch.zeros(n - step, 2, dtype=torch.float64, device=DEV)
    for i in range(n - step):
        (fa, da, aa), (fb, db, ab) = views[i], views[i + step]
        if frames is not None:
            fa, fb = frames[i], frames[i + step]
        consistency_pair(fa, fb, da, aa, db, ab, test.poses[i], test.poses[i + step], test.intrinsics, H, W, min_opacity=min_opacity,
                         sse=sums[i, 0:1], count=sums[i, 1:2])
    return sums.cpu().numpy(), torch.stack([v[0] for v in views]).reshape(n, H, W, 3)


def test_evaluate_consistency_equals_the_hand_loop():
    from laenerf_amd.metrics import LPIPS
    r, opt, tr, test = _trained()
    n, H, W = test.n_img, test.H, test.W
    lp = LPIPS.random(0, device=DEV)
    renders = None
    for step in (1, 2):
        for mo in (0.5, 0.05):
            res = tr.evaluate_consistency(test, step=step, min_opacity=mo, lpips=lp if (step, mo) == (1, 0.05) else None)
            s, renders = _hand_loop(tr, test, step, mo)
            print("step", step, "min_opacity", mo, "valid_share", res["valid_share"], "warp_mse", res["warp_mse"], "lpips", res["lpips"])
            assert res["warp_mse"].shape == res["valid_share"].shape == (n - step,)
            assert (s[:, 1] / (H * W)).tobytes() == res["valid_share"].tobytes()
            with np.errstate(all="ignore"):
                assert np.where(s[:, 1] == 0, np.nan, s[:, 0] / s[:, 1]).tobytes() == res["warp_mse"].tobytes()
            assert res["empty_pairs"] == int((s[:, 1] == 0).sum())
            if res["empty_pairs"] < n - step:
                assert res["mean_warp_mse"] == float(np.mean(res["warp_mse"][s[:, 1] > 0]))
            if res["lpips"] is not None:
                assert res["lpips"].shape == (n - step,) and np.all(res["lpips"] >= 0) and res["mean_lpips"] == float(np.mean(res["lpips"]))
            else:
                assert res["mean_lpips"] is None
    # frames: the model's own fp32 renders give the default's bits; a constant image warps onto itself
    base = tr.evaluate_consistency(test, step=1, min_opacity=0.05)
    assert (base["valid_share"] > 0).any()                          # the comparisons below are about something
    own = tr.evaluate_consistency(test, step=1, min_opacity=0.05, frames=renders)
    assert own["warp_mse"].tobytes() == base["warp_mse"].tobytes() and own["valid_share"].tobytes() == base["valid_share"].tobytes()
    for const in (torch.full((n, H, W, 3), 0.3, device=DEV), torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=DEV)):
        c = tr.evaluate_consistency(test, step=1, min_opacity=0.05, frames=const)
        assert c["valid_share"].tobytes() == base["valid_share"].tobytes()
        assert np.all(c["warp_mse"][c["valid_share"] > 0] == 0) and np.all(np.isnan(c["warp_mse"][c["valid_share"] == 0]))
    for bad_step in (n, n + 3, 0):
        with pytest.raises(ValueError):
            tr.evaluate_consistency(test, step=bad_step)
    for bad_frames in (renders[:-1], renders.half(), renders.reshape(n, H * W, 3)):
        with pytest.raises(ValueError):
            tr.evaluate_consistency(test, frames=bad_frames)
    test.color_space = "linear"
    with pytest.raises(ValueError):
        tr.evaluate_consistency(test)


def test_evaluate_consistency_restores_weights_and_next_group_is_unchanged(tmp_path):
    from test_gpu_trainer import _assert_same, _state
    states = []
    for evaluate in (True, False):
        r, opt, tr, test = _trained()
        if evaluate:
            before = _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None]
            res = tr.evaluate_consistency(test, step=1, min_opacity=0.05, out_dir=str(tmp_path))
            assert res["warp_mse"].shape == (3,)
            assert sorted(p.name for p in tmp_path.iterdir()) == [f"ngp_{i:04d}_warp.png" for i in range(3)]
            _assert_same(before, _state(r, opt) + [sh.half.clone() for *_, sh, _ in opt.items if sh is not None])
        tr.train(16)                                                 # the next captured group
        states.append(_state(r, opt) + tr.ema.shadow_params + [tr.ema.device_count()[:1].clone()])
    _assert_same(*states)
