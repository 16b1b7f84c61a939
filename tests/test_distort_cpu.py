"""composite_distort_numpy, the sequential fp64 restatement the GPU distortion tests compare against: its value and dl/dw against the
reference's own eff_distloss (recorded by tests/golden/make_golden_distort.py) and against the O(n^2) pairwise definition, its
grad_sigmas against a central finite difference of its own forward (which pins the Q = 2 l shortcut of the backward), and the argument
checks of every layer, none of which needs a GPU."""
import types

import numpy as np
import pytest
import torch

from conftest import golden
from depth_sup_util import T_THRESH, build_case
from step_args import null_step

LAMBDA = 0.25               # the weight of the fused-step tests (test_gpu_distort.py): the term is no rounding-level part of the loss


def _restate(c, **kw):
    from laenerf_amd.raymarching.raymarching import composite_distort_numpy
    return composite_distort_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, **kw)


# ---------------------------------------------------------------------------------------------------------------- a
def test_value_and_dl_dw_equal_the_reference_and_the_pairwise_definition():
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c = build_case()
    g = golden("distort_case")
    f = _restate(c)
    samples = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, samples=True)["samples"]
    assert sorted(samples) == [int(r) for r in g["rows"]] and len(g["rows"]) == 11
    at = 0
    for row, value, count in zip(g["rows"], g["value"], g["count"]):
        index, off, _ = (int(v) for v in c["rays"][row])
        w, t, _ = samples[int(row)]
        assert len(w) == count
        assert np.isclose(f["dist"][index], value, rtol=1e-12, atol=0), (row, f["dist"][index], value)
        assert np.allclose(f["q"][off:off + count], g["grad_w"][at:at + count], rtol=1e-12, atol=0)
        at += count
        d0 = c["deltas"][off:off + count, 0].astype(np.float64)
        pairwise = (d0 * w * w).sum() / 3 + (w[:, None] * w[None, :] * np.abs(t[:, None] - t[None, :])).sum()
        assert np.isclose(f["dist"][index], pairwise, rtol=1e-12, atol=0)
    assert at == g["grad_w"].size
    # rays without samples contribute nothing; the mean runs over all rays; q is zero on the rows no ray uses
    none = [int(c["rays"][n, 0]) for n, k in enumerate(c["kinds"]) if k == "dropped" or c["rays"][n, 2] == 0]
    assert len(none) == 2 and not f["dist"][none].any() and (np.delete(f["dist"], none) > 0).all()
    assert np.isclose(f["dist_mean"], f["dist"].sum() / c["N"], rtol=1e-15) and not f["q"][c["rows_end"]:].any()


# ---------------------------------------------------------------------------------------------------------------- b
def test_grad_sigmas_equal_finite_differences_of_the_forward_fp64():
    from laenerf_amd.raymarching.raymarching import composite_distort_numpy
    c = build_case()
    rng = np.random.default_rng(3)
    g_dist = rng.standard_normal(c["N"])
    sig = c["sigmas"].astype(np.float64)
    full = composite_distort_numpy(sig, c["rgbs"], c["deltas"], c["rays"], T_THRESH, grad_dist=g_dist)
    assert full["margin"] >= 1e-3                       # no early stop can flip under the perturbation below
    assert not full["grad_rgbs"].any()                  # the term does not touch the colours
    h, checked = 1e-6, 0
    for n in range(c["N"]):
        index, off, steps = (int(v) for v in c["rays"][n])
        if steps == 0 or off + steps > c["M"]:
            continue
        last = int(full["stop"][index])
        ks = {0, steps - 1, last, min(last + 1, steps - 1), min(63, steps - 1), min(64, steps - 1)} | {int(k) for k in rng.integers(0, steps, 4)}
        one = c["rays"][n:n + 1]
        for k in sorted(ks):
            i = off + k
            keep = sig[i]
            vals = []
            for s in (h, -h):
                sig[i] = keep + s
                vals.append(composite_distort_numpy(sig, c["rgbs"], c["deltas"], one, T_THRESH, n_rays=c["N"])["dist"][index])
            sig[i] = keep
            fd = g_dist[index] * (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - full["grad_sigmas"][i]) <= 1e-9 + 1e-6 * abs(full["grad_sigmas"][i]), (n, k, fd, full["grad_sigmas"][i])
            if k > last:
                assert full["grad_sigmas"][i] == 0
            checked += 1
    assert checked >= 60 and np.abs(full["grad_sigmas"]).max() > 1e-3


def test_criterion_restatement_and_the_weight_of_the_gpu_tests():
    c = build_case()
    rng = np.random.default_rng(4)
    target = rng.uniform(0, 1, (c["N"], 3))
    z = rng.uniform(0.5, 3.0, c["N"]); z[::3] = 0.0
    f = _restate(c, bg=c["bg_rays"], target=target, distort_weight=LAMBDA, scale=8.0)
    assert np.isclose(f["loss"], f["mse"] + LAMBDA * f["dist_mean"], rtol=1e-14) and f["depth_mse"] == 0
    assert np.allclose(f["grad_dist"], 8.0 * LAMBDA / c["N"], rtol=1e-15)
    assert LAMBDA * f["dist_mean"] > 0.05 * f["mse"]
    both = _restate(c, bg=c["bg_rays"], target=target, z=z, nears=c["nears"], depth_weight=0.37, distort_weight=LAMBDA, scale=8.0)
    assert np.isclose(both["loss"], both["mse"] + 0.37 * both["depth_mse"] + LAMBDA * both["dist_mean"], rtol=1e-14) and both["depth_mse"] > 0
    off = _restate(c, bg=c["bg_rays"], target=target, distort_weight=LAMBDA, scale=8.0, distort_grad=False)
    plain = _restate(c, bg=c["bg_rays"], target=target, scale=8.0)
    assert not off["grad_dist"].any() and off["loss"] == f["loss"] and np.array_equal(off["grad_sigmas"], plain["grad_sigmas"])
    assert np.abs(f["grad_sigmas"] - plain["grad_sigmas"]).max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------- c
BAD_WEIGHTS = [-1.0, float("inf"), float("nan")]


def test_library_entries_refuse_invalid_arguments_before_any_launch(hip_lib):
    step, bwd, fwd = (hip_lib.lae_composite_rays_train_step, hip_lib.lae_composite_rays_train_backward_blend_ex,
                      hip_lib.lae_composite_rays_train_forward_blend)
    term = lambda lam=0.1: (lam, 0, None, None, None)                     # the distortion term, its pointers NULL; no depth term
    assert null_step(step, dist=term()) == -3                             # NULL pointers
    for w in BAD_WEIGHTS:
        assert null_step(step, dist=term(lam=w)) == -1
    assert null_step(step, N=0, dist=term()) == 0                         # N == 0: nothing to do
    assert null_step(step, N=0, dist=term(lam=-1.0)) == -1                # the weight is checked first
    assert bwd(*([None] * 8), 8, 4, 1e-4, None, 0.0, 0.0, 0.0, *([None] * 9)) == -3
    assert bwd(*([None] * 8), 0, 4, 1e-4, None, 0.0, 0.0, 0.0, *([None] * 9)) == 0
    p = torch.zeros(4).data_ptr()                                         # every other pointer given: grad_dist needs depth and dist
    assert bwd(*([p] * 8), 8, 4, 1e-4, None, 0.0, 0.0, 0.0, p, None, p, p, None, None, p, p, None) == -3
    assert bwd(*([p] * 8), 8, 4, 1e-4, None, 0.0, 0.0, 0.0, p, None, p, p, None, p, p, None, None) == -3
    assert fwd(*([None] * 4), 8, 4, 1e-4, None, None, None, 0.0, 0.0, 0.0, *([None] * 7)) == -3
    assert fwd(*([None] * 4), 8, 0, 1e-4, None, None, None, 0.0, 0.0, 0.0, *([None] * 7)) == 0


@pytest.mark.parametrize("w", BAD_WEIGHTS)
def test_python_layers_refuse_an_invalid_weight(w):
    from laenerf_amd.raymarching import raymarching as rm
    from laenerf_amd.trainer import Trainer
    with pytest.raises(ValueError):
        rm.composite_rays_train_blend_mse(*([None] * 7), distort_weight=w)
    with pytest.raises(ValueError):
        Trainer(types.SimpleNamespace(fused_post_ops=True), None, types.SimpleNamespace(error_map=None), 100, 1e-2, distort_weight=w)


def test_the_term_needs_gt_and_fused_post_ops():
    from laenerf_amd.renderer import NeRFRenderer
    from laenerf_amd.trainer import Trainer
    for fused, gt in ((False, object()), (True, None)):
        with pytest.raises(RuntimeError, match="distortion"):
            NeRFRenderer.shade_train(types.SimpleNamespace(fused_post_ops=fused), None, gt=gt, distort_weight=0.01)
    with pytest.raises(ValueError, match="fused_post_ops"):
        Trainer(types.SimpleNamespace(fused_post_ops=False), None, types.SimpleNamespace(error_map=None), 100, 1e-2, distort_weight=0.01)
    with pytest.raises(RuntimeError):
        from laenerf_amd.raymarching.raymarching import finish_distort_loss
        finish_distort_loss(types.SimpleNamespace())
