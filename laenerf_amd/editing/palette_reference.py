"""float64 numpy restatement of the palette stage (csrc/palette.hip): recomposition forward, its two backward modes, the fused
point criterion and the palette-only regulariser `palet_loss` (editing/style_encoder.py:148-158 and :183-205, nerf/utils.py:990-995).

Test infrastructure, numpy only.  Two kinds of statement live here:

  * float64 restatements that round to fp16 exactly where the kernels store or cast (`round16=True`, the default) and, with
    `round16=False`, are the plain real-valued formulation (what torch float64 autograd differentiates: tests/test_palette_cpu.py);
  * `palette_recompose_bits`, a float32 restatement of the recomposition that equals the kernel BIT for bit: half(w) * half(pal) has
    11 + 11 significand bits, so every product is exact in fp32 and the kernel's fmaf chain over the ascending active bases equals a
    multiply-then-add loop.

Tie rules (palette section): the row maximum of the non-uniform term and the column maximum of the uniform term are the
FIRST maximum (lowest index); the regulariser's d(max) is spread evenly over all tied maxima.
"""
from collections import namedtuple

import numpy as np

PAL_MAX = 16                  # FFMLP output width: the logits arrive as [M,16] rows
PAL_BLOCK = 256               # rows per workgroup of the palette kernels (reduction depth of the tolerances)

PaletteForward = namedtuple("PaletteForward", "pred w_hat o_hat pre pre_exact")
PaletteBackward = namedtuple("PaletteBackward", "g_w_logits g_o_raw g_palette mag_w mag_o mag_palette passed kmax")
StyleLoss = namedtuple("StyleLoss", "fin jmax column_sums")
FIN_LOSS_SCALED, FIN_LOSS, FIN_MSE, FIN_UNIFORM, FIN_NON_UNIFORM, FIN_OFFSET, FIN_JMAX, FIN_SCALE, FIN_REG = range(9)


def half(x):
    """round to the nearest fp16 value (ties to even), as float64"""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def half_ulp(x):
    """spacing of the fp16 grid at |x| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def active_columns(P, mask):
    cols = [k for k in range(int(P)) if (int(mask) >> k) & 1]
    if not cols or P > PAL_MAX:
        raise ValueError("palette: 1 <= P <= 16 and at least one active base")
    return cols


def _softmax64(w_logits, cols):
    z = np.asarray(w_logits, np.float64)[:, cols]
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def palette_recompose_bits(w_hat_f32, o_hat_f16, palette, P, mask):
    """-> (pred, pre) fp16, bit for bit what k_palette_fwd derives from these weights [M, n_active] fp32 and offsets [M,3] fp16:
    acc = fmaf(half(w_k), half(pal_kc), acc) over ascending active k, half(acc), half(float(acc) + float(o)), clamp"""
    cols = active_columns(P, mask)
    w = np.asarray(w_hat_f32, np.float32).astype(np.float16).astype(np.float32)
    pal = np.asarray(palette, np.float32)[cols].astype(np.float16).astype(np.float32)
    acc = np.zeros((w.shape[0], 3), np.float32)
    for j in range(len(cols)):
        acc = acc + w[:, j:j + 1] * pal[j][None, :]                     # the product is exact, so this add is the fma's one rounding
    o = np.asarray(o_hat_f16, np.float16).astype(np.float32)
    pre = (acc.astype(np.float16).astype(np.float32) + o).astype(np.float16)
    pred = np.minimum(np.maximum(pre.astype(np.float32), np.float32(0)), np.float32(1)).astype(np.float16)
    return pred, pre


def palette_forward_numpy(w_logits, o_raw, palette, P, mask, round16=True, w_hat=None):
    """w_logits, o_raw [M,16] (fp16 values), palette [P,3] fp32 -> PaletteForward(pred, w_hat [M, n_active], o_hat, pre, pre_exact),
    all float64.  Softmax over the active columns and tanh in float64; fp16 roundings where the kernel stores or casts:
    palette.half(), half(w) as matmul operand, half(acc), half(o), half(acc + o), then the clamp.  `pre_exact` is the pre-clamp
    value with none of the roundings but palette.half() (which is part of the formulation itself).  `w_hat` [M, n_active]: given
    weights in place of the float64 softmax (the exact cases: fp32 expf(-200) is 0, float64 exp(-200) is not)."""
    cols = active_columns(P, mask)
    r = half if round16 else (lambda v: np.asarray(v, np.float64))
    w_hat = _softmax64(w_logits, cols) if w_hat is None else np.asarray(w_hat, np.float64)
    t = np.tanh(np.asarray(o_raw, np.float64)[:, :3])
    pal = half(np.asarray(palette, np.float32)[cols])
    pre_exact = w_hat @ pal + t
    o_hat = r(t)
    pre = r(r(r(w_hat) @ pal) + o_hat)
    return PaletteForward(np.clip(pre, 0.0, 1.0), w_hat, o_hat, pre, pre_exact)


def palette_backward_numpy(w_logits, o_raw, palette, P, mask, mode="plain", g_pred=None, g_w=None, g_o=None, upstream=None, scale=None,
                           target=None, lw=None, jmax=None, g_pred32=None, M_live=None, w_hat=None, o_hat=None, round16=True):
    """k_palette_bwd<false|true> in float64 -> PaletteBackward.

    mode="plain": g_pred [M,3], g_w [M, n_active], g_o [M,3] (each optional) are dL/dpred, dL/dw_hat, dL/do_hat.
    mode="loss" : the gradient of  upstream * scale * (MSE(pred, target) + w_uniform * max_j sum_i w_ij
                  + w_non_uniform * sum_i (1 - max_j w_ij) + c_offset * sum o^2),  lw = (w_uniform, w_non_uniform, c_offset);
                  `jmax` is the (compact) arg-max column of the uniform term (default: the first maximum of the column sums), the row
                  arg-max is the first maximum, the MSE gradient is 2 (pc - t) / (3 M) and `g_pred32` [M,3] (the image terms' fp32
                  dL/dpred) is added where the clamp mask passes.  `M_live`: rows >= M_live get zero gradients (device row count).
    The clamp mask is inclusive (0 <= pre <= 1) and evaluated on the fp16 `pre`.

    `w_hat` [M, n_active] fp32 / `o_hat` [M,3] fp16: the forward kernel's own outputs take the place of the float64 softmax / tanh
    (the backward kernel recomputes both with the same device code); `pre` is then the bit-faithful `palette_recompose_bits`, so the
    mask is right on every row.  Without them everything derives from the logits.

    g_w_logits, g_o_raw [M,16]: float64 values BEFORE the final fp16 rounding, zeros in padded and inactive columns; g_palette [P,3]
    with zeros in inactive rows.  mag_w / mag_o / mag_palette are the sums of the magnitudes of the terms of each entry (what an fp32
    evaluation's rounding error is relative to): with A_k = |g_in_k| + sum_c |gpc_c pal_kc| (the terms of gw_k),
      mag_w[i,k] = w_k (A_k + sum_j w_j A_j),   mag_o[i,c] = (|gpc_c| + |other term|)(1 - o_c^2),   mag_palette[k,c] = sum_i |w_ik gpc_ic|."""
    cols = active_columns(P, mask)
    na = len(cols)
    M = np.asarray(w_logits).shape[0]
    live = M if M_live is None else min(int(M_live), M)
    pal = half(np.asarray(palette, np.float32)[cols])
    if w_hat is not None and o_hat is not None and round16:
        w = np.asarray(w_hat, np.float32).astype(np.float64)
        o = np.asarray(o_hat, np.float16).astype(np.float64)
        pre = palette_recompose_bits(w_hat, o_hat, palette, P, mask)[1].astype(np.float64)
    else:
        f = palette_forward_numpy(w_logits, o_raw, palette, P, mask, round16, w_hat=w_hat)
        w, o, pre = f.w_hat, f.o_hat, f.pre
    passed = (pre >= 0.0) & (pre <= 1.0)
    z3 = np.zeros((M, 3))
    kmax = np.argmax(w, -1)                                   # numpy's arg-max is the first maximum
    if mode == "plain":
        gpc = np.where(passed, z3 if g_pred is None else np.asarray(g_pred, np.float64), 0.0)
        other = z3 if g_o is None else np.asarray(g_o, np.float64)
        gin = np.zeros((M, na)) if g_w is None else np.asarray(g_w, np.float64)
        gpc_mag = np.abs(gpc)
    elif mode == "loss":
        lw = np.asarray(lw, np.float32).astype(np.float64)   # the C ABI takes the three weights as float
        gmul = float(np.float32(upstream)) * float(np.float32(scale))
        if jmax is None:
            jmax = int(np.argmax(w[:live].sum(0)))
        a = np.where(passed, gmul * 2.0 * (np.clip(pre, 0.0, 1.0) - np.asarray(target, np.float64)) / (3.0 * live), 0.0)
        b = z3 if g_pred32 is None else np.where(passed, np.asarray(g_pred32, np.float64), 0.0)
        gpc, gpc_mag = a + b, np.abs(a) + np.abs(b)
        other = gmul * 2.0 * lw[2] * o
        gin = gmul * (lw[0] * (np.arange(na)[None, :] == jmax) - lw[1] * (np.arange(na)[None, :] == kmax[:, None]))
    else:
        raise ValueError(mode)
    got = gpc + other
    gw = gin + gpc @ pal.T
    A = np.abs(gin) + gpc_mag @ np.abs(pal.T)
    g_act = w * (gw - (w * gw).sum(-1, keepdims=True))
    mag_act = w * (A + (w * A).sum(-1, keepdims=True))
    dt = 1.0 - o * o
    rows = (np.arange(M) < live)[:, None]
    g_wl, g_ol, mag_w, mag_o = (np.zeros((M, PAL_MAX)) for _ in range(4))
    g_wl[:, cols], mag_w[:, cols] = np.where(rows, g_act, 0.0), np.where(rows, mag_act, 0.0)
    g_ol[:, :3], mag_o[:, :3] = np.where(rows, got * dt, 0.0), np.where(rows, (gpc_mag + np.abs(other)) * dt, 0.0)
    g_pal, mag_pal = np.zeros((int(P), 3)), np.zeros((int(P), 3))
    g_pal[cols] = (w[:live, :, None] * gpc[:live, None, :]).sum(0)
    mag_pal[cols] = (w[:live, :, None] * gpc_mag[:live, None, :]).sum(0)
    return PaletteBackward(g_wl, g_ol, g_pal, mag_w, mag_o, mag_pal, passed, kmax)


def palet_reg_numpy(palette, w_valid, w_distinct, with_magnitude=False):
    """`palet_loss` (style_encoder.py:195-202) over ALL P bases in float64 -> (value, grad [P,3]):
        valid = sum floor(p) p,  dists_ij = |p_i - p_j|^2,  m = max dists,  distinct = mean_ij (1 - dists_ij / m)
    with d(max) spread evenly over all tied maxima (torch's full-reduction max).  P = 1 is the reference's own 0/0: NaN.
    with_magnitude: also the sums of term magnitudes (value_mag, grad_mag [P,3]) that bound an fp32 evaluation."""
    p = np.asarray(palette, np.float32).astype(np.float64)
    wv, wd = float(np.float32(w_valid)), float(np.float32(w_distinct))
    P = p.shape[0]
    diff = p[:, None, :] - p[None, :, :]
    dists = (diff ** 2).sum(-1)
    m, S = dists.max(), dists.sum()
    tied = dists == m
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = S / (P * P * m)
        value = wv * (np.floor(p) * p).sum() + wd * (1.0 - ratio)
        dS = 4.0 * diff.sum(1)                                              # d S / d p_kc = 4 sum_j (p_kc - p_jc)
        dm = 2.0 * ((tied[:, :, None] * diff).sum(1) - (tied[:, :, None] * diff).sum(0)) / tied.sum()     # pairs (k, j) and (i, k)
        grad = wv * np.floor(p) - wd * (dS / m - S / (m * m) * dm) / (P * P)
        if not with_magnitude:
            return value, grad
        dm_mag = 2.0 * ((tied[:, :, None] * np.abs(diff)).sum(1) + (tied[:, :, None] * np.abs(diff)).sum(0)) / tied.sum()
        value_mag = abs(wv) * np.abs(np.floor(p) * p).sum() + abs(wd) * (1.0 + ratio)
        grad_mag = abs(wv) * np.abs(np.floor(p)) + abs(wd) * (4.0 * np.abs(diff).sum(1) / m + S / (m * m) * dm_mag) / (P * P)
    return value, grad, value_mag, grad_mag


def style_loss_numpy(pred, target, w_hat, o_hat, lw, scale=1.0, M_live=None, reg=None):
    """k_style_loss_partial / _final in float64 from the criterion's own inputs (pred fp16, target fp32, w_hat fp32 [M, n_active],
    o_hat fp16) -> StyleLoss(fin [12], jmax, column_sums).  fin = loss * scale, loss, mse, uniform, non_uniform, offset, jmax, scale,
    reg (0 without reg = (palette, w_valid, w_distinct)), 0, 0, 0.  The three added terms each go through fp16 like
    nerf/utils.py:990-995: loss = mse + half(uniform + non_uniform) + half(offset) + half(reg).  jmax is the first maximum."""
    lw = np.asarray(lw, np.float32).astype(np.float64)
    M = np.asarray(pred).shape[0] if M_live is None else int(M_live)
    p, t = np.asarray(pred, np.float64)[:M], np.asarray(target, np.float64)[:M]
    w, o = np.asarray(w_hat, np.float64)[:M], np.asarray(o_hat, np.float64)[:M]
    sums = w.sum(0)
    jmax = int(np.argmax(sums))
    mse = ((p - t) ** 2).sum() / (3.0 * M)
    uni, non, off = lw[0] * sums[jmax], lw[1] * (1.0 - w.max(-1)).sum(), lw[2] * (o * o).sum()
    regv = 0.0 if reg is None else palet_reg_numpy(*reg)[0]
    s = float(np.float32(scale))
    loss = mse + float(half(uni + non)) + float(half(off)) + float(half(regv))
    return StyleLoss(np.array([loss * s, loss, mse, uni, non, off, float(jmax), s, regv, 0.0, 0.0, 0.0]), jmax, sums)
