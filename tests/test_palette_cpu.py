"""no GPU: the float64 restatement of the palette stage (laenerf_amd/editing/palette_reference.py) against torch float64 autograd of
the reference formulation -- the recomposition of editing/style_encoder.py:148-158 and the losses of :183-205 -- and the conditions
of the case generators of tests/palette_util.py.  The restatement's fp16 roundings are switched off for the comparison with
autograd (round16=False); what is left is the same real-valued function, so the tolerance is 1e-12 of the largest entry."""
import numpy as np
import pytest
import torch

import palette_util as U
from laenerf_amd.editing import (palet_reg_numpy, palette_backward_numpy, palette_forward_numpy, palette_recompose_bits,
                                 style_loss_numpy)
from laenerf_amd.editing.palette_reference import half

REL = 1e-12
CPU_CASES = [(8, 0xFF, 257), (8, 0b10110101, 257), (16, 0xFFFF, 257), (16, 0x8000, 257), (3, 0b100, 257), (1, 1, 257), (8, 0xFF, 1)]


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= REL * max(np.abs(b).max(), 1e-300)


def torch_forward(c):
    """style_encoder.py:148-158 in float64; the palette leaf holds palette.half()'s values (the cast's backward is the identity)"""
    wl = torch.tensor(c.w_logits.astype(np.float64), requires_grad=True)
    ol = torch.tensor(c.o_raw.astype(np.float64), requires_grad=True)
    pal = torch.tensor(half(c.palette), requires_grad=True)
    active = torch.tensor([(c.mask >> k) & 1 == 1 for k in range(c.P)])
    w_hat = torch.softmax(wl[:, :c.P][:, active], -1)
    o_hat = torch.tanh(ol[:, :3])
    pred = torch.clamp(w_hat @ pal[active] + o_hat, 0, 1)
    return wl, ol, pal, pred, w_hat, o_hat


@pytest.mark.parametrize("P,mask,M", CPU_CASES)
def test_plain_backward_equals_float64_autograd(P, mask, M):
    c = U.random_case(P, mask, M)
    wl, ol, pal, pred, w_hat, o_hat = torch_forward(c)
    f = palette_forward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, round16=False)
    assert close(f.pred, pred.detach().numpy()) and close(f.w_hat, w_hat.detach().numpy()) and close(f.o_hat, o_hat.detach().numpy())
    assert np.array_equal(f.pre, f.pre_exact)
    gp, gw, go = (torch.tensor(v.astype(np.float64)) for v in (c.g_pred, c.g_w, c.g_o))
    ((pred * gp).sum() + (w_hat * gw).sum() + (o_hat * go).sum()).backward()
    b = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "plain", g_pred=c.g_pred, g_w=c.g_w, g_o=c.g_o, round16=False)
    assert close(b.g_w_logits, wl.grad.numpy()) and close(b.g_o_raw, ol.grad.numpy()) and close(b.g_palette, pal.grad.numpy())
    assert (np.abs(b.g_w_logits) <= b.mag_w).all() and (np.abs(b.g_o_raw) <= b.mag_o).all() and (np.abs(b.g_palette) <= b.mag_palette).all()
    # each upstream gradient alone (the kernel takes NULL for the others)
    for kw in ({"g_pred": c.g_pred}, {"g_w": c.g_w}, {"g_o": c.g_o}):
        one = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "plain", round16=False, **kw)
        rest = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "plain", round16=False,
                                      **{k: v for k, v in (("g_pred", c.g_pred), ("g_w", c.g_w), ("g_o", c.g_o)) if k not in kw})
        assert close(one.g_w_logits + rest.g_w_logits, b.g_w_logits) and close(one.g_palette + rest.g_palette, b.g_palette)


@pytest.mark.parametrize("with_pred32", [False, True])
@pytest.mark.parametrize("P,mask,M", CPU_CASES)
def test_loss_backward_equals_float64_autograd(P, mask, M, with_pred32):
    """MSE + weights_loss + offset_loss (style_encoder.py:188-192, :204-205) times upstream * scale; the rows whose two largest
    logits are equal pin the row arg-max to the first maximum (torch.max(dim) returns the first index too)."""
    c = U.random_case(P, mask, M)
    wl, ol, pal, pred, w_hat, o_hat = torch_forward(c)
    wu, wn, co = (float(np.float32(v)) for v in U.LOSS_W)
    target = torch.tensor(c.target.astype(np.float64))
    loss = torch.nn.functional.mse_loss(pred, target) + torch.sum(w_hat, dim=0).max() * wu + (1 - w_hat.max(dim=-1).values).sum() * wn \
        + torch.pow(o_hat, 2).sum() * co
    total = loss * (U.UPSTREAM * U.SCALE)
    if with_pred32:
        total = total + (pred * torch.tensor(c.g_pred32.astype(np.float64))).sum()
    total.backward()
    b = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "loss", upstream=U.UPSTREAM, scale=U.SCALE, target=c.target,
                               lw=U.LOSS_W, g_pred32=c.g_pred32 if with_pred32 else None, round16=False)
    assert close(b.g_w_logits, wl.grad.numpy()) and close(b.g_o_raw, ol.grad.numpy()) and close(b.g_palette, pal.grad.numpy())
    if len(c.tie_rows):
        assert (b.kmax[c.tie_rows] == np.argmax(c.w_logits[:, c.cols].astype(np.float64), -1)[c.tie_rows]).all()
    # the criterion's value: the terms, then the three fp16 roundings of nerf/utils.py:990-995
    f = palette_forward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, round16=False)
    s = style_loss_numpy(f.pred, c.target, f.w_hat, f.o_hat, U.LOSS_W, U.SCALE)
    terms = [torch.nn.functional.mse_loss(pred, target), torch.sum(w_hat, dim=0).max() * wu, (1 - w_hat.max(dim=-1).values).sum() * wn,
             torch.pow(o_hat, 2).sum() * co]
    assert close(s.fin[2:6], [t.item() for t in terms])
    assert s.fin[1] == s.fin[2] + float(half(s.fin[3] + s.fin[4])) + float(half(s.fin[5])) and s.fin[0] == s.fin[1] * U.SCALE
    assert s.fin[6] == s.jmax == int(torch.sum(w_hat, dim=0).argmax()) and s.fin[7] == U.SCALE and s.fin[8] == 0.0


def test_m_live_rows_take_no_part():
    c = U.random_case(8, 0xFF, 257)
    kw = dict(upstream=U.UPSTREAM, scale=U.SCALE, lw=U.LOSS_W, round16=False)
    part = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, 8, 0xFF, "loss", target=c.target, M_live=200, **kw)
    head = palette_backward_numpy(c.w_logits[:200], c.o_raw[:200], c.palette, 8, 0xFF, "loss", target=c.target[:200], **kw)
    assert np.array_equal(part.g_w_logits[:200], head.g_w_logits) and np.array_equal(part.g_palette, head.g_palette)
    assert not part.g_w_logits[200:].any() and not part.g_o_raw[200:].any()


def torch_palet_loss(p, wv, wd):
    """style_encoder.py:195-202"""
    pal = torch.tensor(p.astype(np.float64), requires_grad=True)
    dists = (torch.pow(pal[:, None, :] - pal, 2)).sum(-1)
    dist_loss = (1 - dists / dists.max()).mean()
    valid_loss = (torch.floor(pal) * pal).sum()
    value = valid_loss * wv + dist_loss * wd
    value.backward()
    return value.item(), pal.grad.numpy()


@pytest.mark.parametrize("name", sorted(U.reg_palettes()))
def test_regulariser_equals_float64_autograd(name):
    """every palette, the tied ones included: torch's full-reduction max spreads d(max) evenly over the tied maxima"""
    p, _ = U.reg_palettes()[name]
    wv, wd = (float(np.float32(v)) for v in U.REG_W)
    tv, tg = torch_palet_loss(p, wv, wd)
    v, g, vm, gm = palet_reg_numpy(p, *U.REG_W, with_magnitude=True)
    if name == "p1":                                   # the reference's own 0/0
        assert np.isnan(tv) and np.isnan(v) and np.isnan(tg).all() and np.isnan(g).all()
        return
    assert abs(v - tv) <= REL * abs(tv) and close(g, tg)
    assert abs(v) <= vm and (np.abs(g) <= gm * (1 + 1e-12)).all()
    assert g.shape == p.shape and np.isfinite(g).all()


def test_column_tie_goes_to_the_first_column_where_torch_splits():
    """the uniform term's arg-max on tied column sums: torch's full-reduction .max() spreads the gradient evenly over the tied
    columns, which the softmax backward then cancels; the kernel -- and the restatement -- give all of it to the FIRST column."""
    t = U.tied_columns_case(na=8, M=12)
    c = type("C", (), dict(t, cols=list(range(8)), na=8))
    wl, ol, pal, pred, w_hat, o_hat = torch_forward(c)
    wu = float(np.float32(U.LOSS_W[0]))
    sums = torch.sum(w_hat, dim=0)
    assert float((sums.max() - sums.min()).detach()) == 0.0
    (sums.max() * wu).backward()
    assert np.abs(wl.grad.numpy()).max() <= 1e-17                                  # even split: wu / 8 in every column, cancelled
    b = palette_backward_numpy(t["w_logits"], t["o_raw"], t["palette"], 8, 0xFF, "loss", upstream=1.0, scale=1.0,
                               target=palette_forward_numpy(t["w_logits"], t["o_raw"], t["palette"], 8, 0xFF).pred, lw=(U.LOSS_W[0], 0.0, 0.0))
    want = np.zeros((12, 16))
    want[:, :8] = -wu / 64.0
    want[:, 0] = wu * (1.0 - 1.0 / 8.0) / 8.0
    assert close(b.g_w_logits, want)
    s = style_loss_numpy(np.zeros((12, 3)), np.zeros((12, 3)), np.full((12, 8), 0.125), np.zeros((12, 3)), U.LOSS_W)
    assert s.jmax == 0


@pytest.mark.parametrize("P,mask,M", U.EXACT_CASES)
def test_recompose_bits_equals_the_restatement_on_exact_cases(P, mask, M):
    c = U.exact_case(P, mask, M)
    pred, pre = palette_recompose_bits(c.w_hat.astype(np.float32), c.o_hat.astype(np.float16), c.palette, P, mask)
    assert pred.dtype == np.float16 and np.array_equal(pre.astype(np.float64), c.pre) and np.array_equal(pred.astype(np.float64), c.pred)


def test_recompose_bits_is_within_the_restatements_roundings_on_random_cases():
    c = U.random_case(16, 0xFFFF, 257)
    pred, pre = palette_recompose_bits(c.fwd.w_hat.astype(np.float32), c.fwd.o_hat.astype(np.float16), c.palette, 16, 0xFFFF)
    # same inputs up to the fp32 rounding of w_hat: at most one fp16 ulp apart (2^-10 below 2)
    assert np.abs(pre.astype(np.float64) - c.fwd.pre).max() <= 2.0 ** -10 and np.abs(pre.astype(np.float64)).max() < 2


def test_generators_meet_their_conditions():
    redrawn = 0
    for P, mask, M in U.RANDOM_CASES:
        c = U.random_case(P, mask, M)                  # asserts the clamp fractions, the fragile-row redraw, the arg-max gap
        redrawn += c.n_redrawn
        assert c.w_logits.dtype == np.float16 and c.w_logits.shape == (M, 16) and c.g_w.shape == (M, c.na)
    assert redrawn > 0                                 # some rows did sit within 2^-9 of a clamp edge
    for P, mask, M in U.EXACT_CASES:
        U.exact_case(P, mask, M)                       # asserts exact representability and the clamp-edge rows
    assert set(U.reg_palettes()) == {"cube", "dyadic6", "rand", "p2", "p16", "masked", "p1"}
    assert {(P, mask) for P, mask, _ in U.RANDOM_CASES} == set(U.MASKS) == {(P, mask) for P, mask, _ in U.EXACT_CASES}
    assert {M for _, _, M in U.RANDOM_CASES} == set(U.M_SIZES) | {U.M_WRAP}
    assert (U.M_WRAP + 255) // 256 == 66 and U.M_WRAP % 256 == 1
