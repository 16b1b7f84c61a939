"""case generators for the palette-stage tests (csrc/palette.hip against laenerf_amd/editing/palette_reference.py).

Everything comes from seeded numpy generators, not from device RNG, so the conditions on the inputs (how much of the batch clamps,
no pre-clamp value at a rounding distance of the clamp edges, an unambiguous arg-max column, exact representability) are asserted
here, on the CPU, for exactly the arrays the GPU sees.  tests/test_palette_cpu.py runs every generator."""
import functools
from types import SimpleNamespace

import numpy as np

from laenerf_amd.editing.palette_reference import active_columns, half, palette_backward_numpy, palette_forward_numpy

M_SIZES = [1, 63, 64, 255, 256, 257, 1000]
M_WRAP = 16641                    # 65 workgroups of 256 rows + 1 row: the `b += 64` loops of the two final reductions wrap
MASKS = [(8, 0xFF), (8, 0b10110101), (16, 0xFFFF), (16, 0x8000), (3, 0b100), (1, 1)]
# every M with the common configuration, every (P, mask) at a size with several workgroups and an odd tail, the wrap with two masks
RANDOM_CASES = [(8, 0xFF, M) for M in M_SIZES] + [(P, mask, 257) for P, mask in MASKS[1:]] + [(8, 0b10110101, M_WRAP), (16, 0xFFFF, M_WRAP)]
EXACT_CASES = [(8, 0xFF, 1), (8, 0b10110101, 63), (16, 0xFFFF, 256), (16, 0x8000, 257), (3, 0b100, 64), (1, 1, 255), (8, 0xFF, 1000),
               (16, 0xFFFF, M_WRAP)]
FRAGILE = 2.0 ** -9               # a row is fragile if an unrounded pre-clamp entry lies this close to 0 or to 1
O_SCALE = 0.6                     # std of the offset logits: tanh(0.6 N) around a palette in [0, 1) clamps ~15 % low, ~15 % high
TIE_EVERY, TIE_PHASE = 7, 3       # rows i % 7 == 3: the two largest active logits are equal
FAVOURED_BIAS = 1.0               # added to one column's logits: the uniform term's arg-max column is unambiguous


def _seed(P, mask, M, salt=0):
    return [int(P), int(mask), int(M), int(salt)]


def _fragile_rows(pre_exact):
    return ((np.abs(pre_exact) < FRAGILE) | (np.abs(pre_exact - 1.0) < FRAGILE)).any(-1)


@functools.lru_cache(maxsize=None)
def random_case(P, mask, M):
    """-> namespace(w_logits, o_raw [M,16] fp16, palette [P,3] fp32, target [M,3] fp32, g_pred / g_o fp16, g_w / g_pred32 fp32,
    favoured (compact column), tie_rows, n_redrawn, fwd (palette_forward_numpy of the case)); arrays are read-only and shared."""
    cols = active_columns(P, mask)
    na = len(cols)
    rng = np.random.default_rng(_seed(P, mask, M))
    w_logits = (2.0 * rng.standard_normal((M, 16))).astype(np.float16)
    palette = rng.random((P, 3)).astype(np.float32)
    favoured = na // 2                                               # neither the first nor the last active column (na > 2)
    w_logits[:, cols[favoured]] += np.float16(FAVOURED_BIAS)
    tie_rows = np.arange(M)[np.arange(M) % TIE_EVERY == TIE_PHASE] if na >= 2 else np.arange(0)
    for i in tie_rows:                                               # the second largest active logit takes the value of the largest
        order = np.argsort(w_logits[i, cols].astype(np.float64), kind="stable")
        w_logits[i, cols[order[-2]]] = w_logits[i, cols[order[-1]]]
    o_raw = (O_SCALE * rng.standard_normal((M, 16))).astype(np.float16)
    n_redrawn, salt = 0, 0
    while True:
        bad = _fragile_rows(palette_forward_numpy(w_logits, o_raw, palette, P, mask).pre_exact)
        if not bad.any():
            break
        salt += 1
        assert salt < 64
        n_redrawn += int(bad.sum())
        o_raw[bad] = (O_SCALE * np.random.default_rng(_seed(P, mask, M, salt)).standard_normal((M, 16))).astype(np.float16)[bad]
    fwd = palette_forward_numpy(w_logits, o_raw, palette, P, mask)
    c = SimpleNamespace(P=P, mask=mask, M=M, cols=cols, na=na, w_logits=w_logits, o_raw=o_raw, palette=palette, favoured=favoured,
                        tie_rows=tie_rows, n_redrawn=n_redrawn, fwd=fwd,
                        target=rng.random((M, 3)).astype(np.float32),
                        g_pred=rng.standard_normal((M, 3)).astype(np.float16), g_o=rng.standard_normal((M, 3)).astype(np.float16),
                        g_w=rng.standard_normal((M, na)).astype(np.float32),
                        g_pred32=(rng.standard_normal((M, 3)) / M).astype(np.float32))
    check_random_case(c)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_random_case(c):
    """the conditions the issue of this test suite sets on the random inputs, by the float64 restatement alone"""
    pre = c.fwd.pre_exact
    assert not _fragile_rows(pre).any()
    if c.M >= 255:                                                   # fractions of the pre-clamp entries (meaningless on a handful of rows)
        assert ((pre >= 0) & (pre <= 1)).mean() >= 0.40, ((pre >= 0) & (pre <= 1)).mean()
        assert (pre < 0).mean() >= 0.05, (pre < 0).mean()
        assert (pre > 1).mean() >= 0.05, (pre > 1).mean()
    # the fp16-rounded mask input agrees with the unrounded one on every entry: no row's mask hangs on a rounding
    assert np.array_equal((c.fwd.pre >= 0) & (c.fwd.pre <= 1), (pre >= 0) & (pre <= 1))
    if c.na >= 2:
        w = c.fwd.w_hat
        top2 = np.sort(w, -1)[:, -2:]
        if c.M > TIE_PHASE:
            assert len(c.tie_rows) and np.array_equal(top2[c.tie_rows, 0], top2[c.tie_rows, 1])
        # a clear winner among the column sums: the kernels' fp32 sums of M values in [0, 1] err by at most
        # (6 + 3 + M / 16384 + 6 + 1) * 2^-24 * sum < 2e-6 * sum; the gap is asserted at 1e-2 * sum, four orders above
        s = np.sort(w.sum(0))
        assert s[-1] - s[-2] > 1e-2 * s[-1], s
        assert c.M < 255 or int(np.argmax(w.sum(0))) == c.favoured


LOSS_W = (0.3, 0.2, 0.05)         # w_uniform, w_non_uniform, c_offset: every term of dL/dlogits is far above an fp16 ulp of the entry
UPSTREAM, SCALE = 0.5, 128.0


@functools.lru_cache(maxsize=None)
def exact_case(P, mask, M):
    """every stored quantity exactly representable: active logits in {0, -200} with n in {1, 2, 4, 8, 16} columns at 0 (expf gives
    1 or 0, the weights are exactly 1/n), offset logits in {0, +-20} (tanh = 0 or +-1 after the fp16 store), palette entries multiples
    of 1/4 in [-0.5, 1.5], upstream gradients integers in [-2, 2].  Everything the kernels compute is then a multiple of 1 / (4 n^2)
    below 2048 units (fp16-exact) and every fp32 partial sum is exact, so order cannot matter and the comparison is equality.
    -> namespace(inputs, n [M], and the exact float64 outputs: w_hat, o_hat, pre, pred, g_w_logits, g_o_raw, g_palette, column_sums)"""
    cols = active_columns(P, mask)
    na = len(cols)
    rng = np.random.default_rng(_seed(P, mask, M, 1 << 20))
    n = rng.choice([v for v in (1, 2, 4, 8, 16) if v <= na], size=M)
    w_logits = np.full((M, 16), -200.0, np.float16)
    w_logits[:, [k for k in range(16) if k not in cols]] = rng.choice([0.0, -200.0, 7.0], size=(M, 16 - na)).astype(np.float16)   # never read
    for i in range(M):
        w_logits[i, rng.choice(cols, size=n[i], replace=False)] = 0.0
    o_raw = rng.choice([0.0, 20.0, -20.0], size=(M, 16)).astype(np.float16)
    palette = (rng.integers(-2, 7, size=(P, 3)) / 4.0).astype(np.float32)
    if M >= 255:                                  # rows that land on the clamp edges and one lattice step outside, whatever the draw
        k0 = cols[0]
        palette[k0] = (-0.25, 1.0, 1.25)
        w_logits[:4, cols] = -200.0
        w_logits[:4, k0] = 0.0                    # weight 1 on base k0: acc = (-0.25, 1, 1.25)
        o_raw[0, :3] = (0.0, 0.0, 0.0)            # pre = -0.25 (masked), 1 (passes), 1.25 (masked)
        o_raw[1, :3] = (20.0, -20.0, -20.0)       # pre = 0.75, 0 (passes), 0.25
        o_raw[2, :3] = (-20.0, 20.0, 0.0)         # pre = -1.25, 2, 1.25
        o_raw[3, :3] = (0.0, 0.0, -20.0)          # pre = -0.25, 1, 0.25
        n[:4] = 1
    g_pred = rng.integers(-2, 3, size=(M, 3)).astype(np.float16)
    g_o = rng.integers(-2, 3, size=(M, 3)).astype(np.float16)
    g_w = rng.integers(-2, 3, size=(M, na)).astype(np.float32)
    w_exact = np.where(w_logits[:, cols] == 0, 1.0 / n[:, None], 0.0)      # fp32 expf(-200) underflows to 0
    f = palette_forward_numpy(w_logits, o_raw, palette, P, mask, w_hat=w_exact)
    b = palette_backward_numpy(w_logits, o_raw, palette, P, mask, "plain", g_pred=g_pred, g_w=g_w, g_o=g_o, w_hat=w_exact)
    c = SimpleNamespace(P=P, mask=mask, M=M, cols=cols, na=na, n=n, w_logits=w_logits, o_raw=o_raw, palette=palette, g_pred=g_pred, g_o=g_o,
                        g_w=g_w, w_hat=f.w_hat, o_hat=f.o_hat, pre=f.pre, pred=f.pred, g_w_logits=b.g_w_logits, g_o_raw=b.g_o_raw,
                        g_palette=b.g_palette, passed=b.passed, column_sums=f.w_hat.sum(0))
    check_exact_case(c, f)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def check_exact_case(c, f):
    """representability of everything stored, and that none of the restatement's roundings rounded"""
    inv_n = 1.0 / c.n
    assert np.array_equal(np.sort(c.w_hat, -1)[:, ::-1][np.arange(c.M), c.n - 1], inv_n)       # exp(-200) / n is below 2^-149: weights 1/n and 0
    assert np.array_equal(c.w_hat.sum(-1), np.ones(c.M)) and set(np.unique(c.w_hat * c.n[:, None])) <= {0.0, 1.0}
    assert set(np.unique(c.o_hat)) <= {0.0, 1.0, -1.0}
    assert np.array_equal(c.palette * 4, np.round(c.palette * 4)) and c.palette.min() >= -0.5 and c.palette.max() <= 1.5
    assert np.array_equal(f.pre, f.pre_exact)                          # none of the five fp16 roundings of the forward rounded
    units = c.g_w_logits * (4.0 * c.n[:, None] ** 2)
    assert np.array_equal(units, np.round(units)) and np.abs(units).max() < 2048 and np.array_equal(half(c.g_w_logits), c.g_w_logits)
    assert np.array_equal(c.g_o_raw, np.round(c.g_o_raw)) and np.abs(c.g_o_raw).max() <= 4           # (g_pred + g_o) * {0, 1}
    assert np.array_equal(c.g_palette * 16, np.round(c.g_palette * 16)) and np.abs(c.g_palette).max() * 16 < 2 ** 24    # fp32-exact in any order
    assert np.array_equal(c.column_sums * 16, np.round(c.column_sums * 16))
    if c.M >= 255:
        assert (c.pre == 0.0).any() and (c.pre == 1.0).any() and c.passed[c.pre == 0.0].all() and c.passed[c.pre == 1.0].all()
        step = 0.25 / c.n[:, None]
        assert ((c.pre < 0) & (c.pre >= -step)).any() and ((c.pre > 1) & (c.pre <= 1 + step)).any()
        assert not c.passed[(c.pre < 0) | (c.pre > 1)].any()


def tied_columns_case(na=8, M=12):
    """all-zero logits: every weight is exactly 1 / na, every column sum exactly M / na -- the uniform term's arg-max is a pure tie"""
    assert na in (2, 4, 8, 16)
    return dict(w_logits=np.zeros((M, 16), np.float16), o_raw=np.zeros((M, 16), np.float16), P=na, mask=(1 << na) - 1, M=M,
                palette=(np.arange(na * 3).reshape(na, 3) % 5 / 4.0).astype(np.float32))


def reg_palettes():
    """name -> (palette [P,3] fp32, mask): the regulariser runs over all P bases, active or not"""
    cube = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)], np.float32)           # 4 space diagonals: 8 tied maxima of dists
    # an octahedron of radius 1/4 around (1/2, 1/2, 1/2) plus two interior points: 3 diameters, 6 tied maxima, every distance dyadic
    octa = np.array([[0.75, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.75, 0.5], [0.5, 0.25, 0.5], [0.5, 0.5, 0.75], [0.5, 0.5, 0.25],
                     [0.5, 0.5, 0.5], [0.625, 0.5, 0.375]], np.float32)
    rng = np.random.default_rng(808)
    rand8 = rng.random((8, 3)).astype(np.float32)
    rand8[1] = (1.3, -0.4, 0.7)
    rand8b = rng.random((8, 3)).astype(np.float32)
    rand8b[6] = (-0.2, 1.1, 2.5)
    out = {"cube": (cube, 0xFF), "dyadic6": (octa, 0xFF), "rand": (rand8, 0xFF),
           "p2": (np.array([[0.25, 1.5, -0.75], [1.0, 0.125, 0.5]], np.float32), 0b11),
           "p16": ((rng.random((16, 3)) * 1.6 - 0.3).astype(np.float32), 0xFFFF),
           "masked": (rand8b, 0b10110101),
           "p1": (np.array([[0.3, 1.2, -0.6]], np.float32), 1)}
    for name, (p, _) in out.items():
        d = ((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1)
        ties = int((d == d.max()).sum())
        assert ties == {"cube": 8, "dyadic6": 6, "p1": 1}.get(name, 2), (name, ties)
        if name not in ("cube", "dyadic6", "p1"):                   # no near-tie that fp32 and fp64 could order differently
            assert np.sort(np.unique(d))[-2] < d.max() * (1 - 1e-4)
    return out


REG_W = (1.0, 1e-2)               # palette_loss_valid, palette_loss_distinct (the shipped weights)
