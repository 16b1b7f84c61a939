"""composite_depth_numpy, the sequential restatement the GPU depth-supervision tests compare against: its backward against a central
finite difference of its own forward in fp64, and the precondition on the committed inputs that makes an fp32 / fp64 comparison
meaningful (no early stop close enough to the threshold to fall on another sample in fp32)."""
import numpy as np
import torch

from depth_sup_util import T_THRESH, build_case, build_grads
from step_args import null_step


def _objective(c, rays, sig, rgb, gws, gimg, gD):
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    f = composite_depth_numpy(sig, rgb, c["deltas"], rays, T_THRESH, n_rays=c["N"])
    out = f["image"] + (1 - f["weights_sum"])[:, None] * c["bg_rays"].astype(np.float64)
    return float((gws * f["weights_sum"]).sum() + (gimg * out).sum() + (gD * f["depth"]).sum())


def test_backward_equals_finite_difference_of_the_forward_fp64():
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c = build_case()
    gws, gimg, gD = (g.astype(np.float64) for g in build_grads(c["N"]))
    sig, rgb = c["sigmas"].astype(np.float64), c["rgbs"].astype(np.float64)
    full = composite_depth_numpy(sig, rgb, c["deltas"], c["rays"], T_THRESH, bg=c["bg_rays"], grad_weights_sum=gws, grad_image=gimg,
                                 grad_depth=gD)
    rng = np.random.default_rng(0)
    h, checked, stopped_rows = 1e-5, 0, 0
    for n in range(c["N"]):
        index, off, steps = (int(v) for v in c["rays"][n])
        if steps == 0:
            continue
        dropped = off + steps > c["M"]
        steps_in = min(steps, c["M"] - off)
        last = int(full["stop"][index])
        ks = {0, steps_in - 1, max(last, 0), min(last + 1, steps_in - 1), min(63, steps_in - 1), min(64, steps_in - 1)}
        ks |= {int(k) for k in rng.integers(0, steps_in, 4)}
        one = c["rays"][n:n + 1]
        for k in sorted(ks):
            i = off + k
            for arr, grad, col in ((sig, full["grad_sigmas"], None), (rgb, full["grad_rgbs"], int(rng.integers(0, 3)))):
                sel = i if col is None else (i, col)
                keep = arr[sel]
                arr[sel] = keep + h
                up = _objective(c, one, sig, rgb, gws, gimg, gD)
                arr[sel] = keep - h
                dn = _objective(c, one, sig, rgb, gws, gimg, gD)
                arr[sel] = keep
                fd = (up - dn) / (2 * h)
                assert abs(fd - grad[sel]) <= 1e-8 + 1e-6 * abs(grad[sel]), (n, k, col, fd, grad[sel])
                checked += 1
            if dropped or k > last:
                assert full["grad_sigmas"][i] == 0 and not full["grad_rgbs"][i].any()
                stopped_rows += 1
    assert checked >= 150 and stopped_rows >= 4
    # the depth gradient is not a rounding-level term of this check
    without = composite_depth_numpy(sig, rgb, c["deltas"], c["rays"], T_THRESH, bg=c["bg_rays"], grad_weights_sum=gws, grad_image=gimg)
    assert np.abs(full["grad_sigmas"] - without["grad_sigmas"]).max() > 1e-3


def test_committed_case_takes_every_path_and_no_stop_is_marginal():
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c = build_case()
    f = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH)
    assert f["margin"] >= 1e-3, f["margin"]
    stop = {k: int(f["stop"][c["rays"][n, 0]]) for n, k in enumerate(c["kinds"]) if k != "plain"}
    assert 0 < stop["stop_first"] < 63 and 64 <= stop["stop_second"] < 128 and stop["stop_lane63"] == 63 and stop["dropped"] == -1
    for n, k in enumerate(c["kinds"]):
        if k == "plain" and c["rays"][n, 2] > 0:                       # these rays run to their last sample
            assert int(f["stop"][c["rays"][n, 0]]) == c["rays"][n, 2] - 1
    assert c["N"] % 4 != 0 and c["M"] > c["rows_end"] and sorted(c["rays"][:, 2])[-1] >= 200


def test_criterion_restatement_matches_its_definition():
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c = build_case()
    rng = np.random.default_rng(4)
    z = rng.uniform(0.5, 3.0, c["N"]); z[::3] = 0.0; z[1] = -1.0
    target = rng.uniform(0, 1, (c["N"], 3))
    f = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, bg=c["bg_rays"], target=target, z=z,
                              nears=c["nears"], depth_weight=0.25, scale=8.0)
    res = (f["depth"] - (z - c["nears"].astype(np.float64))) * (z > 0)
    assert np.allclose(f["res"], res, rtol=0, atol=1e-15) and not f["res"][::3].any() and f["res"][1] == 0
    assert np.isclose(f["loss"], ((f["image_out"] - target) ** 2).mean() + 0.25 * (res ** 2).mean(), rtol=1e-14)
    assert np.allclose(f["grad_depth"], 8.0 * 0.25 * 2 * res / c["N"], rtol=1e-14)
    off = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, bg=c["bg_rays"], target=target, z=z,
                                nears=c["nears"], depth_weight=0.25, scale=8.0, depth_grad=False)
    assert not off["grad_depth"].any() and off["loss"] == f["loss"]
    # a ray that misses the bounding box (near == far == FLT_MAX) is unsupervised: without the rule its residual is ~FLT_MAX
    big = np.finfo(np.float32).max
    nears, fars = c["nears"].copy(), c["fars"].copy()
    hit = int(np.nonzero(z > 0)[0][0])
    nears[hit] = fars[hit] = big
    kw = dict(bg=c["bg_rays"], target=target, z=z, nears=nears, depth_weight=0.25, scale=8.0, dtype=np.float32)
    miss = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, fars=fars, **kw)
    assert miss["res"][hit] == 0 and miss["grad_depth"][hit] == 0 and np.isfinite(miss["loss"])
    assert np.allclose(np.delete(miss["res"], hit), np.delete(f["res"], hit), rtol=1e-5, atol=1e-6)
    with np.errstate(over="ignore"):
        assert not np.isfinite(    composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, **kw)["loss"])


def test_new_entries_refuse_invalid_arguments_before_any_launch(hip_lib):
    step, bwd = hip_lib.lae_composite_rays_train_step, hip_lib.lae_composite_rays_train_backward_blend_ex
    term = lambda dtype=1, lam=0.1: (None, dtype, None, lam, 0, None, None)                        # the depth term, its pointers NULL
    assert null_step(step, depth=term()) == -3                            # NULL pointers
    assert null_step(step, depth=term(dtype=0)) == -1                     # uint8 planes are not depth planes
    assert null_step(step, depth=term(dtype=7)) == -1
    for lam in (-1.0, float("nan"), float("inf")):
        assert null_step(step, depth=term(lam=lam)) == -1
    assert null_step(step, N=0, depth=term()) == 0                        # N == 0: nothing to do
    assert bwd(*([None] * 8), 8, 4, 1e-4, None, 0.0, 0.0, 0.0, *([None] * 9)) == -3
    assert bwd(*([None] * 8), 0, 4, 1e-4, None, 0.0, 0.0, 0.0, *([None] * 9)) == 0
    p = torch.zeros(4).data_ptr()                                         # every other pointer given: grad_depth needs depth
    assert bwd(*([p] * 8), 8, 4, 1e-4, None, 0.0, 0.0, 0.0, p, None, p, p, p, None, None, None, None) == -3
