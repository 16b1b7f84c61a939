"""the restatements of tests/optim_util.py, pinned without a GPU: adam_step_f64 against torch.optim.Adam in float64, scaler_begin
against a trace written out by hand, and the exact first-step cases against the kernel's statement order in numpy float32"""
import numpy as np
import pytest
import torch

import optim_util as OU


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adam_step_f64_is_torch_adam(weight_decay):
    """5 steps of torch.optim.Adam (single-tensor path) on CPU float64 tensors, the same fp32-rounded hyper-parameters: 1e-15 absolute
    (5.6e-17 measured at n = 4096, lr 1e-2, betas (0.9, 0.99), eps 1e-15, weight_decay 0.01)"""
    n, lr, betas, eps = 4096, 1e-2, (0.9, 0.99), 1e-15
    rng = np.random.default_rng(11)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    t = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    opt = torch.optim.Adam([t], lr=OU.f32(lr), betas=(OU.f32(betas[0]), OU.f32(betas[1])), eps=OU.f32(eps), weight_decay=OU.f32(weight_decay),
                           foreach=False)
    rp, rm, rv = p.astype(np.float64), np.zeros(n), np.zeros(n)
    worst = 0.0
    for step in range(1, 6):
        g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
        t.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        rp, rm, rv = OU.adam_step_f64(rp, rm, rv, g, lr, betas[0], betas[1], eps, weight_decay, step, 1.0)
        st = opt.state[t]
        worst = max(worst, np.abs(t.detach().numpy() - rp).max(), np.abs(st["exp_avg"].numpy() - rm).max(),
                    np.abs(st["exp_avg_sq"].numpy() - rv).max())
    print(f"adam_step_f64 vs torch.optim.Adam float64, weight_decay {weight_decay}: {worst:.2e}")
    assert worst <= 1e-15
    assert np.abs(rp - p).max() > 1e-3                       # it moved: the comparison is not of two copies of the input


def test_adam_step_f64_unscales_with_the_fp32_reciprocal():
    rng = np.random.default_rng(2)
    p, m, v = rng.standard_normal(64), 1e-3 * rng.standard_normal(64), 1e-6 * rng.random(64)
    g = rng.standard_normal(64).astype(np.float32)
    inv = np.float32(1.0 / 3.0)
    a = OU.adam_step_f64(p, m, v, g, 1e-2, 0.9, 0.99, 1e-15, 0.01, 7, inv)
    b = OU.adam_step_f64(p, m, v, g.astype(np.float64) * float(inv), 1e-2, 0.9, 0.99, 1e-15, 0.01, 7, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _state(scale, tracker=0, step=0, skipped=0):
    return dict(scale=scale, growth_tracker=tracker, found_inf=0, skip=0, step=step, inv_bc1=0.0, bc2_sqrt=0.0, inv_scale=0.0, skipped=skipped)


def test_scaler_begin_follows_a_hand_written_trace():
    """growth_interval 3, growth 2, backoff 0.5, scale 8: growth after three finite steps, an inf on the step that would have grown,
    two infs in a row; every expected word written out"""
    found = [0, 0, 0, 0, 0, 1, 1, 0, 0, 0]
    #        (scale, tracker, skip, step, inv_scale, skipped) after each begin
    want = [(8.0, 1, 0, 1, 0.125, 0),
            (8.0, 2, 0, 2, 0.125, 0),
            (16.0, 0, 0, 3, 0.125, 0),          # third finite step: grows; this step's gradients were scaled by 8
            (16.0, 1, 0, 4, 0.0625, 0),
            (16.0, 2, 0, 5, 0.0625, 0),
            (8.0, 0, 1, 5, 0.0625, 1),          # inf on the step that would have grown: skipped, backed off, tracker cleared
            (4.0, 0, 1, 5, 0.125, 2),           # a second inf in a row
            (4.0, 1, 0, 6, 0.25, 2),
            (4.0, 2, 0, 7, 0.25, 2),
            (8.0, 0, 0, 8, 0.25, 2)]
    s = _state(8.0)
    for f, w in zip(found, want):
        s = OU.scaler_begin(s, f, 3, 2.0, 0.5, 1)
        assert (s["scale"], s["growth_tracker"], s["skip"], s["step"], s["inv_scale"], s["skipped"]) == w
        assert s["found_inf"] == 0
    # use_scaler = 0: the word is cleared, nothing is skipped, the scale and the tracker stay, 1 / scale is 1
    s = _state(1.0)
    for k, f in enumerate([0, 1, 1, 0]):
        s = OU.scaler_begin(s, f, 3, 2.0, 0.5, 0)
        assert (s["scale"], s["growth_tracker"], s["found_inf"], s["skip"], s["step"], s["inv_scale"], s["skipped"]) == (1.0, 0, 0, 0, k + 1, 1.0, 0)
    # 1 / scale is the fp64 reciprocal rounded to fp32; the bias corrections are filled in only when the betas are given
    s = OU.scaler_begin(_state(3.0), 0, 3, 2.0, 0.5, 1)
    assert s["inv_scale"] == float(np.float32(1.0 / 3.0)) and s["inv_bc1"] == 0.0
    s = OU.scaler_begin(_state(3.0), 0, 3, 2.0, 0.5, 1, betas=(0.5, 0.75))
    assert (s["inv_bc1"], s["bc2_sqrt"]) == (2.0, 0.5)
    s = OU.scaler_begin(_state(3.0, step=10 ** 7 - 1), 0, 3, 2.0, 0.5, 1, betas=(0.9, 0.99))
    assert (s["step"], s["inv_bc1"], s["bc2_sqrt"]) == (10 ** 7, 1.0, 1.0)


@pytest.mark.parametrize("n", [9, 1025, 16003])
@pytest.mark.parametrize("kind", ["half", "float", "weight_decay"])
def test_exact_cases_are_exact_in_fp32(kind, n):
    """the closed forms of the exact first step are what fp32 arithmetic gives, operation by operation (this pins the cases, not the
    kernel): p' = p - lr sign(u), m' = u / 2, v' = u^2 / 4"""
    E = OU.EXACT
    wd = kind == "weight_decay"
    c = OU.exact_case(n, kind == "half", weight_decay=wd)
    s = OU.scaler_begin(_state(E["scale"]), 0, 2000, 2.0, 0.5, 1, betas=(E["beta1"], E["beta2"]))
    assert (s["inv_scale"], s["inv_bc1"], s["bc2_sqrt"], s["step"]) == (2.0 ** -7, 2.0, 0.5, 1)
    lr_over_bc1 = np.float32(np.float64(np.float32(E["lr"])) * np.float64(np.float32(s["inv_bc1"])))
    z = np.zeros(n, np.float32)
    p, m, v = OU.adam1_f32(c["p"], z, z, c["g"], s["inv_scale"], lr_over_bc1, s["bc2_sqrt"], E["beta1"], E["beta2"], E["eps"],
                           E["weight_decay"] if wd else 0.0)
    k = c["keep"]
    assert k.all() or wd
    for got, want in ((p, c["p1"]), (m, c["m1"]), (v, c["v1"])):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32))
    # the float64 restatement agrees exactly too (nothing rounds; with weight decay u^2 rounds in v' alone)
    rp, rm, rv = OU.adam_step_f64(c["p"], z, z, c["g"], E["lr"], E["beta1"], E["beta2"], E["eps"], E["weight_decay"] if wd else 0.0, 1, s["inv_scale"])
    assert np.array_equal(rp[k], c["p1"][k].astype(np.float64)) and np.array_equal(rm[k], c["m1"][k].astype(np.float64))
    assert wd or np.array_equal(rv, c["v1"].astype(np.float64))
    # the case has what the test needs: both signs, the whole exponent range, neighbours that differ, no zero gradient
    assert (c["g"] != 0).all() and (c["sign_g"] > 0).any() and (c["sign_g"] < 0).any()
    if n >= 1025:
        e = np.unique(np.log2(np.abs(c["g"].astype(np.float64))).astype(int))
        assert (e.min(), e.max(), len(e)) == {"half": (-24, 15, 40), "float": (-40, 40, 81), "weight_decay": (1, 4, 4)}[kind]
    assert len(np.unique(c["p"][:OU.P_PERIOD])) == min(n, OU.P_PERIOD)
    if wd and n >= 1025:
        flipped = (np.sign(c["u"]) != c["sign_g"])[k].mean()
        print(f"weight decay flips the sign of the update on {flipped:.3f} of the elements, {int((~k).sum())} dropped")
        assert flipped > 1 / 3
