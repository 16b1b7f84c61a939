"""float64 restatements and a thin C-ABI driver for the optimizer tests (csrc/optimizer.hip: k_check*, k_begin, k_apply*, k_ema_*).

`adam_step_f64` restates torch/optim/adam.py's single-tensor formulas, `scaler_begin` the GradScaler rules of torch/amp/grad_scaler.py
as k_begin applies them to the documented state words (include/laenerf.h), `ema_f64` torch_ema's update.  `exact_case` builds the
inputs whose first Adam step is exact in fp32 whatever the contraction, with the closed forms; `adam1_f32` is the kernel's statement
order in numpy float32 (no FMA).  tests/test_optim_cpu.py pins all of these without a GPU; tests/test_gpu_optim_exact.py pins the
kernels to them.  Nothing here imports the HIP library at import time."""
import ctypes
import math

import numpy as np

EINVAL, ENULL = -1, -3
U24 = 2.0 ** -24                    # half an fp32 ulp, relative
STATE_WORDS = ("scale", "growth_tracker", "found_inf", "skip", "step", "inv_bc1", "bc2_sqrt", "inv_scale", "skipped")
_FLOAT_WORDS = {"scale": 0, "inv_bc1": 5, "bc2_sqrt": 6, "inv_scale": 7}


def f32(x):
    """the value a C `float` argument receives"""
    return float(np.float32(x))


# ---------------------------------------------------------------- restatements
def effective_grad_f64(p, g, weight_decay, inv_scale):
    """the gradient Adam's moments see: unscaled, plus adam.py's grad.add(param, alpha=weight_decay)"""
    g = np.asarray(g).astype(np.float64) * f32(inv_scale)
    wd = f32(weight_decay)
    return g + wd * np.asarray(p).astype(np.float64) if wd != 0 else g


def grad_magnitude_f64(p, g, weight_decay, inv_scale):
    """|g / scale| + |weight_decay * p|: what the roundings on the way to the effective gradient are relative to (the sum itself may
    cancel; its two terms are what gets rounded)"""
    return np.abs(np.asarray(g).astype(np.float64) * f32(inv_scale)) + np.abs(f32(weight_decay) * np.asarray(p).astype(np.float64))


def adam_step_f64(p, m, v, g, lr, beta1, beta2, eps, weight_decay, step, inv_scale):
    """one torch.optim.Adam step (adam.py _single_tensor_adam, non-capturable formulas) in float64 -> (p', m', v').
    p, m, v fp32 and g fp32 / fp16 are widened; lr, betas, eps, weight_decay are rounded to the fp32 values a kernel receives;
    inv_scale is float32(1 / scale); step is the 1-based index of this step, the bias corrections are 1 - beta ** step in float64."""
    p, m, v = (np.asarray(a).astype(np.float64) for a in (p, m, v))
    lr, beta1, beta2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    g = effective_grad_f64(p, g, weight_decay, inv_scale)
    m = m + (g - m) * (1.0 - beta1)                                   # exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1.0 - beta2) * (g * g)                           # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps                         # (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    with np.errstate(invalid="ignore", divide="ignore"):              # eps = 0 and a zero gradient: 0 / 0, as in torch
        p = p - (lr / bc1) * (m / denom)                              # param.addcdiv_(exp_avg, denom, value=-step_size)
    return p, m, v


def bias_corrections_f64(beta1, beta2, step):
    """state words 5 and 6 before their rounding to fp32: 1 / (1 - beta1^step), sqrt(1 - beta2^step), betas as fp32"""
    return 1.0 / (1.0 - f32(beta1) ** step), math.sqrt(1.0 - f32(beta2) ** step)


def scaler_begin(state, found_inf, growth_interval, growth, backoff, use_scaler, betas=None):
    """k_begin over a dict of the nine documented state words -> a new dict.  `found_inf` is what the check launches (or a reporting
    backward) left in word 2.  GradScaler.step / update (grad_scaler.py): an inf skips the step, multiplies the scale by `backoff` and
    clears the tracker; `growth_interval` finite steps in a row multiply it by `growth`.  inv_scale is the one of THIS step's
    gradients (the scale before any update).  With `betas`, words 5 / 6 are the float64 formulas rounded to fp32; without, they stay."""
    s = dict(state)
    scale = np.float32(s["scale"])
    bad = bool(use_scaler) and found_inf != 0
    s["found_inf"] = 0
    s["skip"] = int(bad)
    s["inv_scale"] = float(np.float32(1.0 / float(scale))) if use_scaler else 1.0
    if bad:
        s["scale"] = float(scale * np.float32(backoff))
        s["growth_tracker"] = 0
        s["skipped"] += 1
        return s
    s["step"] += 1
    if betas is not None:
        a, b = bias_corrections_f64(betas[0], betas[1], s["step"])
        s["inv_bc1"], s["bc2_sqrt"] = f32(a), f32(b)
    if use_scaler:
        s["growth_tracker"] += 1
        if s["growth_tracker"] == growth_interval:
            s["scale"] = float(scale * np.float32(growth))
            s["growth_tracker"] = 0
    return s


def ema_f64(shadow, param, one_minus_decay):
    """torch_ema: shadow -= (1 - decay) * (shadow - param), the factor as the fp32 value the kernel receives"""
    s, p = np.asarray(shadow).astype(np.float64), np.asarray(param).astype(np.float64)
    return s - (s - p) * f32(one_minus_decay)


def adam1_f32(p, m, v, g, inv_scale, lr_over_bc1, bc2_sqrt, beta1, beta2, eps, weight_decay):
    """adam1 of csrc/optimizer.hip statement by statement in numpy float32, every operation rounded on its own (no FMA)"""
    F = np.float32
    p, m, v = (np.asarray(a, F).copy() for a in (p, m, v))
    g = np.asarray(g).astype(F) * F(inv_scale)
    if F(weight_decay) != 0:
        g = g + F(weight_decay) * p
    m = m + (g - m) * (F(1) - F(beta1))
    v = v * F(beta2) + (F(1) - F(beta2)) * (g * g)
    denom = np.sqrt(v) / F(bc2_sqrt) + F(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = p - F(lr_over_bc1) * (m / denom)
    return p, m, v


# ---------------------------------------------------------------- bounds of the general step (the counting rule)
def step_ratios(got_p, got_m, got_v, p0, m0, v0, g_mag, ref):
    """worst error / bound of p', m', v' against the float64 step `ref` = (p', m', v'); g_mag = grad_magnitude_f64(...).
    p': 2^-24 |p'| (its final rounding) + 32 * 2^-24 |u|, u = p' - p: adam1 and the two scalars feeding it go through 16 roundings,
        16 half-ulps of u, doubled for margin.
    m': 4 roundings (unscale, g - m, the product, the sum), each at most half an ulp of max(|m|, |g|), doubled: 8 * 2^-24 max(|m|, |g|).
    v': 5 roundings (unscale, g * g, the two products, the sum), v' <= max(v, g^2), doubled: 10 * 2^-24 max(v, g^2).
    |g| is g_mag: without weight decay |g / scale|; with it the decay term adds its own magnitude, because g / scale + wd p can cancel
    while the product and the sum that form it round relative to their terms.
    The p' bound counts errors RELATIVE to u.  One error is not: when m' = m + (g - m)(1 - beta1) cancels, u is small but the roundings
    of g - m and of the product are not, about 2 * 2^-24 |m| in m'.  The callers' inputs keep that below the slack the first term
    leaves (test_gpu_optim_exact.general_inputs)."""
    rp, rm, rv = ref
    p0, m0, v0 = (np.asarray(a).astype(np.float64) for a in (p0, m0, v0))
    out = []
    for got, want, bound in ((got_p, rp, U24 * np.abs(rp) + 32 * U24 * np.abs(rp - p0)),
                             (got_m, rm, 8 * U24 * np.maximum(np.abs(m0), g_mag)),
                             (got_v, rv, 10 * U24 * np.maximum(np.abs(v0), g_mag * g_mag))):
        err = np.abs(np.asarray(got).astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        out.append(float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0)
    return tuple(out)


def ema_ratio(got, shadow, param, one_minus_decay):
    """worst error / bound against ema_f64: 2^-24 |s'| (final rounding) + 4 * 2^-24 |(s - p) omd| (the difference and the product
    round, each half an ulp of the term at most; doubled for margin)"""
    want = ema_f64(shadow, param, one_minus_decay)
    term = (np.asarray(shadow).astype(np.float64) - np.asarray(param).astype(np.float64)) * f32(one_minus_decay)
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / (U24 * np.abs(want) + 4 * U24 * np.abs(term)))
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


# ---------------------------------------------------------------- exact first step
EXACT = dict(beta1=0.5, beta2=0.75, eps=0.0, lr=2.0 ** -7, scale=2.0 ** 7, weight_decay=2.0 ** -3)
P_PERIOD = 7999                    # p = j / 1024, j = -3999 .. 3999: distinct within any 7999 consecutive elements


def exact_case(n, grad_half, weight_decay=False):
    """-> dict(p fp32, g fp16 / fp32 (the stored, scaled gradient), and the closed forms p1, m1, v1 fp32, shadow1 fp16, keep bool).
    m = v = 0, state step 0, the EXACT hyper-parameters.  With u = g / scale (+ wd p): m' = u / 2, v' = u^2 / 4, sqrt(v') / sqrt(1/4) = |u|,
    m' / |u| = +-1/2, step size lr / (1/2): p' = p - lr sign(u).  Without weight decay u = +-2^(k-7) and every intermediate is a power
    of two or a multiple of 2^-10 below 4: exact with or without contraction.  With it, u = (+-2^(k+13) + j) 2^-13 is a 13-bit integer;
    u^2 rounds, but RN(sqrt(RN(u^2))) = |u| (the root of a value within 2^-24 of u^2 lies within 2^-25 |u| of |u|, less than half an
    ulp), so p' and m' are still exact and v' = RN(u^2) / 4; `keep` drops u == 0."""
    i = np.arange(n, dtype=np.int64)
    j = (i * 3001) % P_PERIOD - 3999                                  # gcd(3001, 7999) = 1
    p = (j * 2.0 ** -10).astype(np.float32)
    sign = 1.0 - 2.0 * (((i * 0x9E3779B1) >> 16) & 1)
    if weight_decay:
        k = -6 + (i * 3) % 4                                          # u = +-2^k, k in [-6, -3]: the stored gradient is u * scale
        g = (sign * 2.0 ** (k + 7)).astype(np.float32)
    elif grad_half:
        k = -24 + (i * 7) % 40                                        # [-24, 15]: down to the smallest fp16 subnormal
        g = (sign * 2.0 ** k).astype(np.float16)
    else:
        k = -40 + (i * 7) % 81                                        # [-40, 40]
        g = (sign * 2.0 ** k).astype(np.float32)
    u = g.astype(np.float64) / EXACT["scale"]
    if weight_decay:
        u = u + EXACT["weight_decay"] * p.astype(np.float64)
    keep = u != 0
    assert np.array_equal(g.astype(np.float64), sign * 2.0 ** (k + (7 if weight_decay else 0))) and np.all(np.abs(j) < 4000)
    p1 = (p.astype(np.float64) - EXACT["lr"] * np.sign(u)).astype(np.float32)
    assert np.array_equal(p1.astype(np.float64), p.astype(np.float64) - EXACT["lr"] * np.sign(u))
    m1 = (0.5 * u).astype(np.float32)
    assert np.array_equal(m1.astype(np.float64), 0.5 * u)
    v1 = (np.float32(0.25) * (u * u).astype(np.float32)).astype(np.float32)
    if not weight_decay:
        assert np.array_equal(v1.astype(np.float64), 0.25 * u * u)
    return dict(n=n, p=p, g=g, u=u, keep=keep, p1=p1, m1=m1, v1=v1, shadow1=p1.astype(np.float16), sign_g=sign)


# ---------------------------------------------------------------- the C ABI, called directly
def sweep(per_thread):
    """elements one pass of a capped launch covers (stream_blocks: at most num_cus * 16 workgroups of 256 threads)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 16 * 256 * per_thread


def _lib():
    from laenerf_amd import _lib as L
    return L


def _ptrs(tensors):
    """host array of device pointers; an entry may be a tensor, None (NULL) or a raw address"""
    L = _lib()
    vals = [t if (t is None or isinstance(t, int)) else L.ptr(t) for t in tensors]
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


def _sizes(tensors, sizes):
    vals = list(sizes) if sizes is not None else [0 if (t is None or isinstance(t, int)) else t.numel() for t in tensors]
    return (ctypes.c_uint64 * max(len(vals), 1))(*vals)


def _flags(grads, is_half):
    import torch
    vals = list(is_half) if is_half is not None else [int(g is not None and not isinstance(g, int) and g.dtype == torch.float16) for g in grads]
    return (ctypes.c_int * max(len(vals), 1))(*vals)


def new_state(scale=1.0, step=0, tracker=0, found_inf=0, device="cuda:0"):
    """the 16-word int32 state block"""
    import torch
    w = np.zeros(16, np.int32)
    w.view(np.float32)[0] = scale
    w[1], w[2], w[4] = tracker, found_inf, step
    return torch.from_numpy(w).to(device)


def read_state(st):
    """-> (dict of the nine documented words, all sixteen as an int32 array)"""
    w = st.detach().cpu().numpy().copy()
    d = {name: (float(w.view(np.float32)[i]) if name in _FLOAT_WORDS else int(w[i])) for i, name in enumerate(STATE_WORDS)}
    return d, w


def check(grad, state, n=None, is_half=None):
    import torch
    L = _lib()
    half = int(grad is not None and not isinstance(grad, int) and grad.dtype == torch.float16) if is_half is None else is_half
    n = (grad.numel() if n is None else n)
    return L.load().lae_adam_check(_ptrs([grad])[0], half, n, L.ptr(state), L.stream())


def check_multi(grads, state, sizes=None, is_half=None, n_tensors=None):
    L = _lib()
    return L.load().lae_adam_check_multi(len(grads) if n_tensors is None else n_tensors, _ptrs(grads), _flags(grads, is_half), _sizes(grads, sizes),
                                         L.ptr(state), L.stream())


def begin(state, beta1, beta2, growth_interval=2000, growth=2.0, backoff=0.5, use_scaler=1):
    L = _lib()
    return L.load().lae_adam_begin(L.ptr(state), beta1, beta2, growth_interval, growth, backoff, use_scaler, L.stream())


def apply(p, m, v, g, shadow, state, lr, beta1, beta2, eps, weight_decay, n=None, is_half=None):
    """lae_adam_apply; lr is a device fp32 tensor (its first word is read) or a raw address"""
    L = _lib()
    a = _ptrs([p, m, v, g, shadow, lr])
    return L.load().lae_adam_apply(a[0], a[1], a[2], a[3], _flags([g], None if is_half is None else [is_half])[0], a[4],
                                   p.numel() if n is None else n, L.ptr(state), a[5], beta1, beta2, eps, weight_decay, L.stream())


def apply_multi(ps, ms, vs, gs, shadows, state, lrs, beta1, beta2, eps, weight_decay, touched=None, dirty=None, sizes=None, n_tensors=None):
    """lae_adam_apply_multi; `lrs`: one device address (or one-word tensor) per tensor; touched / dirty: None or a list with None entries"""
    L = _lib()
    return L.load().lae_adam_apply_multi(len(ps) if n_tensors is None else n_tensors, _ptrs(ps), _ptrs(ms), _ptrs(vs), _ptrs(gs), _flags(gs, None),
                                         _ptrs(shadows), _sizes(ps, sizes), _ptrs(lrs), None if touched is None else _ptrs(touched),
                                         None if dirty is None else _ptrs(dirty), L.ptr(state), beta1, beta2, eps, weight_decay, L.stream())


def ema_multi(shadows, params, one_minus_decay, sizes=None, n_tensors=None):
    L = _lib()
    return L.load().lae_ema_update_multi(len(shadows) if n_tensors is None else n_tensors, _ptrs(shadows), _ptrs(params), _sizes(shadows, sizes),
                                         float(one_minus_decay), L.stream())


def ema_gated(shadows, params, step, epoch_len, count, decay, use_num_updates, sizes=None, n_tensors=None):
    L = _lib()
    return L.load().lae_ema_update_gated(len(shadows) if n_tensors is None else n_tensors, _ptrs(shadows), _ptrs(params), _sizes(shadows, sizes),
                                         L.ptr(step), int(epoch_len), L.ptr(count), float(decay), int(use_num_updates), L.stream())
