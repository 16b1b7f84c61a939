"""Per-image exposure and white balance, the host half: float64 restatements of csrc/exposure.hip, the float32 restatement of the
gained sampler's target arithmetic (csrc/batch.hip), and the perturbation helper of the tests and tools/train_loop.py.

Image i carries a log2 gain e[i][c] per colour channel.  The sampler multiplies the target colour by gains[i][c] = 2^(e[i][c] - mean_i
e[.][c]) before the background blend and also returns fg, the part of the target that scales with the gain.  Every colour criterion is a
function of pred - gt (MAPE's denominator is detached), so d loss / d gt = -d loss / d pred, and with d gt / d e = ln 2 * fg

    G[i][c] = -(ln 2 / (3 N)) * sum over the rays n of image i of  w_n^2 * dv(pred_nc - gt_nc) * fg_nc.

The mean is subtracted where the gains are published, never on the master; the gradient ignores the -1/n coupling through it (a
projection after the step).  Gains are a physical exposure only when training in linear colour (color_space='linear'); on sRGB data they
are a per-image colour compensation."""
import types

import numpy as np

__all__ = ["gained_targets_numpy", "exposure_step_numpy", "exposure_publish_numpy", "perturb_exposures", "exposure_numpy", "MODES"]

MODES = {"rgb": 0, "gray": 1}
_THREADS = 1024                                         # csrc/exposure.hip EX_THREADS: the order of the kernels' sums depends on it
_LN2 = 0.69314718055994530942


def gained_targets_numpy(colour, gains, alpha=None, bg=1.0):
    """the gained samplers' target arithmetic in float32, one rounding per operation: colour [N,3] (the texel after the optional
    srgb_to_linear), gains [N,3] (the row of each ray's image), alpha [N] or None (C = 3), bg [N,3] or a number
    -> (gt [N,3], fg [N,3]):  s = colour * gain;  with alpha: fg = s * a, gt = fg + bg * (1 - a);  without: fg = gt = s"""
    f32 = np.float32
    s = np.asarray(colour, f32) * np.asarray(gains, f32)
    if alpha is None:
        return s.copy(), s
    a = np.asarray(alpha, f32).reshape(-1, 1)
    b = np.broadcast_to(np.asarray(bg, f32), s.shape)
    fg = s * a
    return fg + b * (f32(1) - a), fg


def _block_sum(slots, terms, width):
    """the kernels' fixed-order sum: term k goes to thread slots[k] % 1024 in order, then the 1024 partial sums are added as a tree"""
    part = np.zeros((_THREADS, width))
    for s, t in zip(slots, terms):
        part[s % _THREADS] += t
    n = _THREADS // 2
    while n >= 1:
        part[:n] += part[n:2 * n]
        n //= 2
    return part[0].copy()


def exposure_step_numpy(pred, gt, fg, inds, hw, master, m, v, counts, weights=None, loss="mse", huber_delta=0.1, mode="rgb", skip=False,
                        lr=1e-3, betas=(0.9, 0.99), eps=1e-15, elem_dtype=np.float32, full=False):
    """float64 restatement of lae_exposure_step on copies -> (master [n,3], m [n,3], v [n,3], counts [n] int32); full=True: also G
    [n,3] (zeros for an image without a ray; after the 'gray' replacement).  pred, gt, fg [N,3]; inds [N] (image * hw + pixel); weights:
    the weight plane (any shape with n * hw values, float16 or float32) or None; lr: the float32 the kernel reads.  elem_dtype: the
    precision of the residual and of the criterion's derivative -- float32 as the kernel computes them (a NaN residual gives a NaN
    derivative under every criterion), float64 for a comparison with differences of a float64 loss"""
    from .raymarching.raymarching import colour_loss_numpy
    if mode not in MODES:
        raise ValueError(f"exposure_step_numpy: mode must be one of {sorted(MODES)}")
    dt = np.dtype(elem_dtype).type
    master, m, v = (np.array(a, dtype=np.float64, copy=True).reshape(-1, 3) for a in (master, m, v))
    counts = np.array(counts, dtype=np.int32, copy=True)
    inds = np.asarray(inds, dtype=np.int64)
    img = inds // int(hw)
    N = inds.shape[0]
    p, g = np.asarray(pred).astype(dt).reshape(N, 3), np.asarray(gt).astype(dt).reshape(N, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dv = colour_loss_numpy(p - g, g, loss, huber_delta, dtype=dt)[1].astype(np.float64)
        w2 = np.ones(N)
        if weights is not None:
            w = np.asarray(weights).reshape(-1)[inds].astype(np.float64)
            w2 = w * w
        terms = (w2[:, None] * dv) * np.asarray(fg, dtype=np.float64).reshape(N, 3)
    b1, b2 = float(betas[0]), float(betas[1])
    G_all = np.zeros_like(master)
    for i in range(master.shape[0]):
        sel = np.flatnonzero(img == i)
        if sel.size == 0 or skip:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            G = -(_LN2 / (3.0 * N)) * _block_sum(sel, terms[sel], 3)
            if mode == "gray":
                G = np.full(3, (G[0] + G[1]) + G[2])
        G_all[i] = G
        if not np.all(np.isfinite(G)):
            continue
        counts[i] += 1
        t = float(counts[i])
        m[i] = b1 * m[i] + (1.0 - b1) * G
        v[i] = b2 * v[i] + (1.0 - b2) * (G * G)
        d = -((np.float64(np.float32(lr)) / (1.0 - b1 ** t)) * (m[i] / (np.sqrt(v[i]) / np.sqrt(1.0 - b2 ** t) + eps)))
        for c in range(3):
            if d[c] != 0:                                  # a zero step keeps the operand's bits (-0.0 + 0.0 would not)
                master[i, c] += d[c]
    return (master, m, v, counts, G_all) if full else (master, m, v, counts)


def exposure_publish_numpy(master, center=True, full=False):
    """float64 restatement of lae_exposure_publish: gains [n,3] float32 = float32(exp2(master - mean)), mean the per-channel mean over
    the images (0 with center=False); full=True: also the float64 exponent master - mean"""
    master = np.asarray(master, dtype=np.float64).reshape(-1, 3)
    n = master.shape[0]
    mean = _block_sum(range(n), master, 3) / float(n) if center else np.zeros(3)
    ex = master - mean
    gains = np.exp2(ex).astype(np.float32)
    return (gains, ex) if full else gains


def perturb_exposures(images, stops, seed=0, wb_stops=0.0):
    """every image's colour multiplied by 2^u_i: u uniform in [-stops, stops] per image (plus, with wb_stops, a per-channel draw in
    [-wb_stops, wb_stops]), then centred so that every channel's mean over the images is 0 -> (images float32, u [n,3] float64).  uint8
    images are taken as value / 255; the result is float and is not clipped (nothing saturates); an alpha channel is left alone"""
    images = np.asarray(images)
    img = images.astype(np.float32) / np.float32(255) if images.dtype == np.uint8 else images.astype(np.float32)
    n = img.shape[0]
    rng = np.random.default_rng(seed)
    u = np.repeat(rng.uniform(-stops, stops, (n, 1)), 3, axis=1)
    if wb_stops:
        u = u + rng.uniform(-wb_stops, wb_stops, (n, 3))
    u = u - u.mean(axis=0, keepdims=True)
    img[..., :3] = img[..., :3] * np.exp2(u).astype(np.float32)[:, None, None, :]
    return img, u


exposure_numpy = types.SimpleNamespace(gained_targets=gained_targets_numpy, step=exposure_step_numpy, publish=exposure_publish_numpy)
