"""-m gpu: the four kernels of the palette stage (csrc/palette.hip: k_palette_fwd, k_palette_bwd<false|true>, k_style_loss_partial /
_final, k_palette_grad_reduce) through `style_backend`, against laenerf_amd/editing/palette_reference.py -- equality where the
arithmetic is exact, a float64 restatement with derived bounds elsewhere.  Cases: tests/palette_util.py (seeded numpy; their
conditions are asserted on the CPU, tests/test_palette_cpu.py pins the restatement to torch float64 autograd).

How the pins fit together.  The forward's w_hat and o_hat are pinned to the float64 softmax / tanh; pred is pinned BIT for bit to
`palette_recompose_bits` of the kernel's own w_hat and o_hat (every row, clamp edges included).  The backward kernels recompute
softmax and tanh with the same device code, so the backward restatement starts from the forward's outputs: its clamp mask is then
right on every row and no row is excluded, and what is left between kernel and restatement is fp32 rounding of known depth.

Bounds (u = 2^-24, the fp32 unit roundoff; every `mag` is the restatement's sum of term magnitudes of that entry):

  w_hat      |w - w64| <= W_ULPS u w64.  Not derivable here: it is the accuracy of the device expf (numerator and sum) plus the
             roundings of the sum, the reciprocal and the product; the ROCm tree documents no error bound for expf / tanhf.  Measured
             on these fixed inputs: 6.98 u at the worst (M = 16641, P = 16; 3.1 - 4.7 u at the other sizes); allowed 4x = 28 u.
  o_hat      within one fp16 ulp of RN_half(tanh64) (a device tanhf a few fp32 ulps off can only move the fp16 rounding by one step).
             Measured: no entry of the 110 000 differs from RN_half(tanh64) at all.
  g_w_logits one fp16 ulp of the reference entry (the store) + K_W u mag_w, mag_w = w_k (A_k + sum_j w_j A_j) with A_k the sum of the
             magnitudes of gw_k's terms.  Operation count: gw_k = g_in + 3 products + 3 adds: each term passes <= 4 roundings -> 4 u A_k;
             dot = fmaf chain over <= 16 bases: 16 u sum_j w_j |gw_j| + the 4 u of each gw_j -> 20 u sum_j w_j A_j; gw_k - dot and the
             product with w_k: 2 u more on both parts.  6 u w_k A_k + 22 u w_k sum_j w_j A_j <= 22 u mag_w: K_W = 24.  LOSS mode: dL/dpred
             = gmul * 2 (pc - t) / (3 M) (+ g_pred32) and g_in = gmul (w_u - w_nu) carry <= 5 roundings of their own: K_W_LOSS = 32.
  g_o_raw    one fp16 ulp + K_O u mag_o: add, 1 - t^2 (exact or one rounding, no cancellation: t is fp16), product: K_O = 4; LOSS mode:
             5 u on dL/dpred, 3 on gmul * 2 c o, one add more: K_O_LOSS = 12.
  g_palette  K_P u sum_i |w_ik gpc_ic| with K_P = the depth of the reduction: product 1, 64-lane butterfly 6, 4 waves 3,
             ceil(blocks / 64) strided adds, butterfly 6 -> 16 + ceil(blocks / 64), + 2 slack; LOSS mode + 5 (dL/dpred).
  fin terms  sums of non-negative terms, so the magnitude sum is the term itself: per row <= 5 roundings (difference, fmaf chain of
             3), then the same reduction tree, a product and a division: K_S = 24 + ceil(blocks / 64).
  regulariser value: every dists_ij carries <= 6 u, S <= 4 terms per lane + butterfly: 16 u, m: 6 u, P^2 m and the division: 2 u
             -> S / (P^2 m) to 24 u; 1 - ratio, the product with w_distinct, the valid sum (8 u) and the final add: <= 32 u (|w_v| sum
             |floor(p) p| + |w_d| (1 + ratio)).  Gradient: dS / m 15 u, S / m^2 dm 43 u, the outer operations and gmul 7 u:
             K_REG_GRAD = 64 on the magnitude sum |w_v floor(p)| + |w_d| (|dS| / m + S / m^2 |dm|) / P^2 (term-wise magnitudes).

Observed on MI355X, worst over all cases (also in DESIGN.md section 4c): g_w_logits and g_o_raw 0.50 of their bound -- half an fp16
ulp, the store's own rounding, i.e. the kernels' fp32 values round to the same fp16 number as the float64 ones almost everywhere;
g_palette 1.7 u of its magnitude sum (K_P = 19 - 25); fin terms 2.1 u (K_S = 25 - 26); regulariser value 1.3 u (32), gradient 4.1 u
(64).  expf(0) = 1, expf(-200) = 0 and half(tanhf(+-20)) = +-1 hold exactly (test_exact_cases_are_equal).
"""
import numpy as np
import pytest
import torch

import palette_util as U
from gpu_util import DEV, N
from laenerf_amd.editing import (palet_reg_numpy, palette_backward_numpy, palette_forward_numpy, palette_recompose_bits,
                                 style_loss_numpy)
from laenerf_amd.editing.palette_reference import half, half_ulp

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
W_ULPS = 28.0            # 4 x the measured worst |w - w64| / (u w64) = 4 x 6.98 (the margin only has to absorb a math-library change)
K_W, K_W_LOSS, K_O, K_O_LOSS = 24.0, 32.0, 4.0, 12.0
K_REG_VALUE, K_REG_GRAD = 32.0, 64.0
NAN16 = float("nan")


def strided_adds(M):
    """ceil(workgroups / 64): the adds each lane of a final reduction makes over the per-workgroup partials"""
    return -(-(-(-M // 256)) // 64)


def k_reduce(M, loss):
    return 18.0 + strided_adds(M) + (5.0 if loss else 0.0)


def k_sum(M):
    return 24.0 + strided_adds(M)


def dev(a, dtype=None):
    t = torch.tensor(np.asarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def B():
    from laenerf_amd.backend import style_backend
    return style_backend


def run_forward(c):
    wl, ol, pal = dev(c.w_logits), dev(c.o_raw), dev(c.palette)
    pred = torch.full((c.M, 3), NAN16, dtype=torch.half, device=DEV)
    w_hat = torch.full((c.M, c.na), NAN16, dtype=torch.float32, device=DEV)
    o_hat = torch.full((c.M, 3), NAN16, dtype=torch.half, device=DEV)
    B().palette_forward(wl, ol, pal, c.P, c.mask, c.M, pred, w_hat, o_hat)
    return wl, ol, pal, pred, w_hat, o_hat


def grad_buffers(c):
    return (torch.full((c.M, 16), NAN16, dtype=torch.half, device=DEV), torch.full((c.M, 16), NAN16, dtype=torch.half, device=DEV),
            torch.full((c.P, 3), NAN16, dtype=torch.float32, device=DEV))


def bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32)


def check_entries(name, got, ref, mag, K, ulp16=True):
    """every entry within [one fp16 ulp of the reference entry +] K u mag; prints the worst error in units of its bound"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = (half_ulp(ref) if ulp16 else 0.0) + K * U24 * mag
    err = np.abs(got - ref)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    fp32 = float((err / np.where(mag > 0, U24 * mag, np.inf)).max()) if not ulp16 else float("nan")
    print(f"  {name}: worst err / bound {worst:.3f}" + ("" if ulp16 else f" ({fp32:.2f} u of the magnitude sum, K = {K:g})"))
    assert np.isfinite(got).all() and (err <= tol).all(), (name, worst)


def check_zero_columns(c, g_wl, g_ol):
    """padded and inactive columns are +0 (bit pattern 0), not merely zero"""
    dead = [k for k in range(16) if k not in c.cols]
    assert not bits(g_wl)[:, dead].any() and not bits(g_ol)[:, 3:].any()


# ------------------------------------------------------------------------------------------------------------------------ forward

@pytest.mark.parametrize("P,mask,M", U.RANDOM_CASES)
def test_forward_against_float64_and_bit_exact_recomposition(P, mask, M):
    c = U.random_case(P, mask, M)
    _, _, _, pred, w_hat, o_hat = run_forward(c)
    w, o = N(w_hat), o_hat.detach().cpu().numpy()
    dev_w = np.abs(w.astype(np.float64) - c.fwd.w_hat) / (U24 * c.fwd.w_hat)
    print(f"  w_hat: worst |w - w64| = {dev_w.max():.2f} u w64 (bound {W_ULPS:g})")
    assert (dev_w <= W_ULPS).all()
    want_o = half(np.tanh(c.o_raw[:, :3].astype(np.float64)))
    step = np.abs(o.astype(np.float64) - want_o) / half_ulp(want_o)
    print(f"  o_hat: {int((step > 0).sum())} of {step.size} entries one fp16 step off RN_half(tanh64), worst {step.max():.0f}")
    assert (step <= 1.0).all()
    want_pred, want_pre = palette_recompose_bits(w, o, c.palette, P, mask)
    assert np.array_equal(bits(pred), want_pred.view(np.uint16))                       # every row, clamp edges included
    # and the whole forward against the restatement from the logits alone: half(acc) and half(o) may each sit one fp16 step off
    # (<= 2^-11 each: both are below 1 in magnitude ... acc up to the palette's range) and the last rounding one step of pre (< 2:
    # 2^-10), none at all on the clamp decision (no fragile rows)
    assert np.array_equal((want_pre < 0), (c.fwd.pre < 0)) and np.array_equal((want_pre > 1), (c.fwd.pre > 1))
    assert np.abs(c.fwd.pre).max() < 2 and (np.abs(N(pred).astype(np.float64) - c.fwd.pred) <= 2.0 ** -9).all()


# ------------------------------------------------------------------------------------------------------------------- plain backward

def run_plain(c, wl, ol, pal, g_pred=True, g_w=True, g_o=True):
    g_wl, g_ol, g_pal = grad_buffers(c)
    B().palette_backward(wl, ol, pal, c.P, c.mask, c.M, dev(c.g_pred) if g_pred else None, dev(c.g_w) if g_w else None,
                         dev(c.g_o) if g_o else None, g_wl, g_ol, g_pal)
    return g_wl, g_ol, g_pal


@pytest.mark.parametrize("P,mask,M", U.RANDOM_CASES)
def test_plain_backward_every_row(P, mask, M):
    c = U.random_case(P, mask, M)
    wl, ol, pal, pred, w_hat, o_hat = run_forward(c)
    g_wl, g_ol, g_pal = run_plain(c, wl, ol, pal)
    ref = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "plain", g_pred=c.g_pred, g_w=c.g_w, g_o=c.g_o,
                                 w_hat=N(w_hat), o_hat=o_hat.cpu().numpy())
    check_entries("g_w_logits", N(g_wl), ref.g_w_logits, ref.mag_w, K_W)
    check_entries("g_o_raw", N(g_ol), ref.g_o_raw, ref.mag_o, K_O)
    check_entries("g_palette", N(g_pal), ref.g_palette, ref.mag_palette, k_reduce(M, False), ulp16=False)
    check_zero_columns(c, g_wl, g_ol)
    assert not bits(g_pal)[[k for k in range(P) if k not in c.cols]].any()
    again = run_plain(c, wl, ol, pal)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((g_wl, g_ol, g_pal), again))          # same bits every run
    if M == 257:                                       # NULL upstream gradients: each of the three alone
        for kw in (dict(g_w=False, g_o=False), dict(g_pred=False, g_o=False), dict(g_pred=False, g_w=False)):
            a_wl, a_ol, a_pal = run_plain(c, wl, ol, pal, **kw)
            r = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "plain", w_hat=N(w_hat), o_hat=o_hat.cpu().numpy(),
                                       **{k: getattr(c, k) for k in ("g_pred", "g_w", "g_o") if kw.get(k, True)})
            check_entries("g_w_logits (one input)", N(a_wl), r.g_w_logits, r.mag_w, K_W)
            check_entries("g_o_raw (one input)", N(a_ol), r.g_o_raw, r.mag_o, K_O)
            check_entries("g_palette (one input)", N(a_pal), r.g_palette, r.mag_palette, k_reduce(M, False), ulp16=False)


# --------------------------------------------------------------------------------------------------- criterion forward and backward

def run_loss(c, live=None, with_pred32=False, reg=False, accumulate_on=None, lw=U.LOSS_W, target=None):
    """forward, criterion forward, criterion backward; live: device row count (the `_dev` entry points), else the exact-size ones"""
    wl, ol, pal, pred, w_hat, o_hat = run_forward(c)
    target = dev(c.target) if target is None else target
    m_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
    fin = torch.full((12,), NAN16, dtype=torch.float32, device=DEV)
    scale, upstream = dev(np.float32([U.SCALE])), dev(np.float32([U.UPSTREAM]))
    B().style_loss_forward(pred, target, w_hat, o_hat, c.M, c.na, lw, scale, fin, reg_palette=pal if reg else None,
                           reg_w=U.REG_W if reg else (0.0, 0.0), m_dev=m_dev)
    g_wl, g_ol, g_pal = grad_buffers(c)
    if accumulate_on is not None:
        g_pal = accumulate_on.clone()
    kw = dict(reg_w=U.REG_W if reg else None, accumulate=accumulate_on is not None)
    if with_pred32:
        B().style_loss_backward_image(wl, ol, pal, c.P, c.mask, c.M, target, fin, upstream, lw, dev(c.g_pred32), g_wl, g_ol, g_pal, m_dev, **kw)
    else:
        B().style_loss_backward(wl, ol, pal, c.P, c.mask, c.M, target, fin, upstream, lw, g_wl, g_ol, g_pal, m_dev=m_dev, **kw)
    return dict(pred=pred, w_hat=w_hat, o_hat=o_hat, fin=fin, g_wl=g_wl, g_ol=g_ol, g_pal=g_pal, target=target)


def check_fin(c, r, live, reg):
    """the criterion's value block against style_loss_numpy of the criterion's own inputs"""
    fin = N(r["fin"]).astype(np.float64)
    s = style_loss_numpy(N(r["pred"]), N(r["target"]), N(r["w_hat"]), N(r["o_hat"]), U.LOSS_W, U.SCALE, M_live=live,
                         reg=(c.palette,) + U.REG_W if reg else None)
    assert int(fin[6]) == s.jmax and fin[7] == U.SCALE
    ks = k_sum(c.M)
    for name, i in (("mse", 2), ("uniform", 3), ("non_uniform", 4), ("offset", 5)):
        check_entries("fin." + name, fin[i], s.fin[i], abs(s.fin[i]), ks, ulp16=False)
    if reg:
        v, _, vmag, _ = palet_reg_numpy(c.palette, *U.REG_W, with_magnitude=True)
        check_entries("fin.reg", fin[8], v, vmag, K_REG_VALUE, ulp16=False)
    else:
        assert fin[8] == 0.0
    # FIN_LOSS reproduces the three fp16 roundings of nerf/utils.py:990-995 from the kernel's own terms, in fp32, bit for bit
    f = N(r["fin"])
    h = lambda v: np.float32(np.float16(v))                                        # noqa: E731
    loss = np.float32(np.float32(f[2] + h(np.float32(f[3] + f[4]))) + h(f[5])) + h(f[8])
    assert np.float32(loss) == f[1] and np.float32(np.float32(loss) * np.float32(U.SCALE)) == f[0]
    return s


LOSS_CASES = [(8, 0xFF, 1, None, False), (8, 0xFF, 63, None, True), (8, 0xFF, 64, 64, True), (8, 0xFF, 255, None, False),
              (8, 0xFF, 256, 250, True), (8, 0xFF, 257, None, False), (8, 0xFF, 1000, 777, True), (8, 0b10110101, 257, 257, True),
              (16, 0xFFFF, 257, 1, True), (16, 0x8000, 257, None, True), (3, 0b100, 257, 256, False), (1, 1, 257, None, True),
              (8, 0b10110101, U.M_WRAP, None, False), (16, 0xFFFF, U.M_WRAP, U.M_WRAP - 200, True)]


@pytest.mark.parametrize("P,mask,M,live,with_pred32", LOSS_CASES)
def test_criterion_forward_and_backward_every_row(P, mask, M, live, with_pred32):
    """live: the device row count of the `_dev` entry points (None: the exact-size ones); with_pred32: the image terms' fp32 dL/dpred
    through style_loss_backward_image (which needs the device row count: live defaults to M there)"""
    c = U.random_case(P, mask, M)
    if with_pred32 and live is None:
        live = M
    r = run_loss(c, live, with_pred32)
    s = check_fin(c, r, live, reg=False)
    ref = palette_backward_numpy(c.w_logits, c.o_raw, c.palette, P, mask, "loss", upstream=U.UPSTREAM, scale=U.SCALE, target=c.target,
                                 lw=U.LOSS_W, jmax=s.jmax, g_pred32=c.g_pred32 if with_pred32 else None, M_live=live,
                                 w_hat=N(r["w_hat"]), o_hat=r["o_hat"].cpu().numpy())
    if live is None or live == M:
        assert s.jmax == int(np.argmax(c.fwd.w_hat.sum(0)))                          # the generator's clear winner
    check_entries("g_w_logits", N(r["g_wl"]), ref.g_w_logits, ref.mag_w, K_W_LOSS)
    check_entries("g_o_raw", N(r["g_ol"]), ref.g_o_raw, ref.mag_o, K_O_LOSS)
    check_entries("g_palette", N(r["g_pal"]), ref.g_palette, ref.mag_palette, k_reduce(M, True), ulp16=False)
    check_zero_columns(c, r["g_wl"], r["g_ol"])
    assert not bits(r["g_pal"])[[k for k in range(P) if k not in c.cols]].any()
    if live is not None and live < M:                  # rows past the device row count: +0 everywhere
        assert not bits(r["g_wl"])[live:].any() and not bits(r["g_ol"])[live:].any()
    if len(c.tie_rows) and (live is None or live > c.tie_rows[0]):
        # the tied rows alone: the non-uniform term's gradient went to the FIRST of the two equal maxima
        t = c.tie_rows[c.tie_rows < (M if live is None else live)]
        first = np.asarray(c.cols)[ref.kmax[t]]
        assert (ref.kmax[t] == np.argmax(c.w_logits[t][:, c.cols].astype(np.float64), -1)).all()
        got = N(r["g_wl"]).astype(np.float64)
        assert (np.abs(got[t, first] - ref.g_w_logits[t, first]) <= half_ulp(ref.g_w_logits[t, first]) + K_W_LOSS * U24 * ref.mag_w[t, first]).all()
    again = run_loss(c, live, with_pred32)
    assert all(np.array_equal(bits(r[k]), bits(again[k])) for k in ("fin", "g_wl", "g_ol", "g_pal"))  # same bits every run


@pytest.mark.parametrize("P,mask,M", [(8, 0b10110101, 257), (16, 0xFFFF, U.M_WRAP)])
def test_accumulate_is_one_fp32_add_per_entry(P, mask, M):
    c = U.random_case(P, mask, M)
    plain = run_loss(c, M, True, reg=True)
    base = dev(np.random.default_rng(5).standard_normal((P, 3)).astype(np.float32))
    acc = run_loss(c, M, True, reg=True, accumulate_on=base)
    assert np.array_equal(bits(acc["g_pal"]), (N(base) + N(plain["g_pal"])).view(np.uint32))
    check_fin(c, plain, M, reg=True)


# ---------------------------------------------------------------------------------------------------------------------- exact cases

@pytest.mark.parametrize("P,mask,M", U.EXACT_CASES)
def test_exact_cases_are_equal(P, mask, M):
    """expf(0) = 1, expf(-200) = 0 and half(tanhf(+-20)) = +-1 on the device (this test is what says so), so the weights are
    exactly 1/n and every output is a dyadic rational the formats hold exactly: equality on every output, the wrap size included,
    and on both clamp edges -- pre = 0 and pre = 1 pass the mask, one lattice step outside does not."""
    c = U.exact_case(P, mask, M)
    wl, ol, pal, pred, w_hat, o_hat = run_forward(c)
    assert np.array_equal(N(w_hat).astype(np.float64), c.w_hat) and np.array_equal(N(o_hat).astype(np.float64), c.o_hat)
    assert np.array_equal(N(pred).astype(np.float64), c.pred)
    g_wl, g_ol, g_pal = grad_buffers(c)
    B().palette_backward(wl, ol, pal, P, mask, M, dev(c.g_pred), dev(c.g_w), dev(c.g_o), g_wl, g_ol, g_pal)
    assert np.array_equal(N(g_wl).astype(np.float64), c.g_w_logits)
    assert np.array_equal(N(g_ol).astype(np.float64), c.g_o_raw)
    assert np.array_equal(N(g_pal).astype(np.float64), c.g_palette)
    check_zero_columns(c, g_wl, g_ol)
    # the criterion's column sums are exact too: the arg-max column is the first maximum whatever ties the draw produced
    fin = torch.full((12,), NAN16, dtype=torch.float32, device=DEV)
    B().style_loss_forward(pred, torch.zeros(M, 3, device=DEV), w_hat, o_hat, M, c.na, U.LOSS_W, None, fin)
    f = N(fin)
    assert int(f[6]) == int(np.argmax(c.column_sums)) and f[3] == np.float32(np.float32(U.LOSS_W[0]) * np.float32(c.column_sums.max()))
    assert f[7] == 1.0


@pytest.mark.parametrize("na", [2, 8, 16])
def test_tied_column_sums_take_the_first_column(na):
    """all-zero logits: every column sum is exactly M / na.  The uniform term's gradient goes to column 0 alone (torch would split
    it evenly, which the softmax backward cancels to zero: tests/test_palette_cpu.py shows both)."""
    t = U.tied_columns_case(na=na, M=12)
    c = type("C", (), dict(t, cols=list(range(na)), na=na))
    wl, ol, pal, pred, w_hat, o_hat = run_forward(c)
    assert np.array_equal(N(w_hat), np.full((12, na), 1.0 / na, np.float32))
    fin = torch.full((12,), NAN16, dtype=torch.float32, device=DEV)
    lw = (U.LOSS_W[0], 0.0, 0.0)
    target = pred.float()                              # no MSE gradient
    B().style_loss_forward(pred, target, w_hat, o_hat, 12, na, lw, None, fin)
    assert N(fin)[6] == 0.0
    g_wl, g_ol, g_pal = grad_buffers(c)
    B().style_loss_backward(wl, ol, pal, na, c.mask, 12, target, fin, dev(np.float32([1.0])), lw, g_wl, g_ol, g_pal)
    ref = palette_backward_numpy(t["w_logits"], t["o_raw"], t["palette"], na, c.mask, "loss", upstream=1.0, scale=1.0, target=N(target),
                                 lw=lw, w_hat=N(w_hat), o_hat=o_hat.cpu().numpy())
    assert (ref.g_w_logits[:, 0] > 0).all() and (ref.g_w_logits[:, 1:na] < 0).all()
    check_entries("g_w_logits", N(g_wl), ref.g_w_logits, ref.mag_w, K_W_LOSS)


# ---------------------------------------------------------------------------------------------------------------------- regulariser

@pytest.mark.parametrize("name", sorted(U.reg_palettes()))
def test_regulariser_value_and_gradient(name):
    """`palet_loss` over all P bases: value (fin[8]) and gradient (g_palette with LAE_STYLE_WITH_REG) against palet_reg_numpy.  The
    point gradients are zeroed (target = pred, no weight / offset terms), so g_palette is gmul * d(reg) alone, on active and inactive
    bases alike.  cube / dyadic6: 8 and 6 tied maxima, exact in fp32 and float64 alike; p1: the reference's 0/0 -- NaN for NaN."""
    palette, mask = U.reg_palettes()[name]
    P, M = palette.shape[0], 64
    rng = np.random.default_rng(P * 100 + mask)
    cols = [k for k in range(P) if (mask >> k) & 1]
    c = type("C", (), dict(P=P, mask=mask, M=M, cols=cols, na=len(cols), palette=palette, g_pred32=None,
                           w_logits=(2.0 * rng.standard_normal((M, 16))).astype(np.float16),
                           o_raw=(U.O_SCALE * rng.standard_normal((M, 16))).astype(np.float16)))
    pred = run_forward(c)[3]
    r = run_loss(c, reg=True, lw=(0.0, 0.0, 0.0), target=pred.float())
    v, g, vmag, gmag = palet_reg_numpy(palette, *U.REG_W, with_magnitude=True)
    fin, got = N(r["fin"]).astype(np.float64), N(r["g_pal"]).astype(np.float64)
    if name == "p1":
        assert np.isnan(v) and np.isnan(g).all() and np.isnan(fin[8]) and np.isnan(got).all()
        return
    gmul = U.UPSTREAM * U.SCALE
    check_entries("fin.reg", fin[8], v, vmag, K_REG_VALUE, ulp16=False)
    check_entries("g_palette (regulariser)", got, gmul * g, gmul * gmag, K_REG_GRAD, ulp16=False)
    assert not N(r["g_wl"]).any() and not N(r["g_ol"]).any()
