"""exact-arithmetic cases for the MFMA MLP kernels (csrc/ffmlp.hip, mlpbackward.hip) and the fused NeRF head (nerfhead.hip).

Every case is built so that every quantity a kernel produces is exactly representable in the format it is stored in and every
possible fp32 partial sum is exact.  Summation order then does not matter (K = 16 or K = 32 MFMA, one or two tiles per wave,
wave-private or cooperative dW, any number of slabs) and the expected values are exact integers: one reference serves every kernel
variant, and the comparison is equality.  The reference holds int64 arrays; its matrix products run as floating-point GEMMs whose
every partial sum is an integer below the format's exact range (imatmul asserts the bound), which is exact, not rounded, arithmetic.

Weights: every matrix [out, in] is a sum of K_TERMS signed "generalised permutation" matrices -- per term one +-1 per row, the
column taken from concatenated random permutations of the `in` columns (balanced column sums) -- so entries are small integers
and every row has L1 norm <= K_TERMS.  Inputs and upstream gradients: integers in [-2, 2]; in the sparse flavour an entry is
+-1 with probability p, else 0 (the large batches: it keeps |dW| under 2048, where one unit is still one fp16 ulp or more).

Layout contract (top of ffmlp.hip): weights = W0[hidden, in] | W1.. [hidden, hidden] | Wout[16, hidden], row-major;
forward_buffer[l] = post-ReLU output of matmul l; backward_buffer[k] = dL/d(pre-activation of matmul num_layers - 1 - k).
"""
import functools

import numpy as np

K_TERMS = 4
OUT = 16
MI355X_CUS = 256
# generic-MLP batch sizes: one tile / odd tile count (one tile per wave) / 9 tiles / two tiles per wave / B % 32 != 0 with several slabs
B_SMALL = [16, 48, 144, 1152, 1168]
WRAP_SHAPES = [(32, 64, 2), (48, 64, 3), (32, 128, 2)]
HEAD_M = [16, 48, 144, 4112, 64 * 1031]
HEAD_SPARSE_FROM = 4112          # dense inputs at 4112 rows take |dW| past 2048


def fused_shape(IN, H, NL):
    """the shapes lae_ffmlp_backward serves with the recompute kernels (ffmlp.hip lae_ffmlp_backward_ex -> mlpbackward.hip)"""
    return H == 64 and NL in (2, 3) and IN in (32, 48, 64)


def wrap_sizes(IN, H, NL, cus=MI355X_CUS):
    """one batch size per kernel family at which the grid-stride loop wraps (more row groups than waves), + 48 rows = an odd
    number of tiles behind the wrap.  From the launch code of ffmlp.hip and mlpbackward.hip:
      k_mlp_fwd / k_mlp_bwd (launch_fwd, backward_w): cus * 4 blocks x 4 waves x 16 * NT rows, NT = 2 up to width 64, else 1;
      k_mlp_fwd64 (launch_fwd64): cus * 2 blocks x 4 waves x 16 rows;  k_mlp_bwd_wave (launch_bwd_fused): cus blocks x 4 waves x
      32 rows;  k_mlp_bwd_coop: cus * 2 blocks x 8 waves x 16 rows -- the largest of the three wraps all of them."""
    generic = cus * 4 * 4 * 16 * (2 if H <= 64 else 1) + 48
    sizes = [generic]
    if H <= 64:
        # sweep + 48 rows is no multiple of 32, so it takes the one-tile-per-wave kernels (two sweeps of those); sweep + 64 rows
        # wraps the two-tile instantiations k_mlp_fwd<W, 2> / k_mlp_bwd<W, 2> themselves
        sizes.append(generic + 16)
    if fused_shape(IN, H, NL):
        fused = max(cus * 2 * 4 * 16, cus * 4 * 32, cus * 2 * 8 * 16) + 48
        if fused != generic:
            sizes.append(fused)
    return sizes


def rn_f16(v):
    """RN_fp16 of exact integers (or dyadic rationals): one rounding, through float64"""
    return np.asarray(v, dtype=np.float64).astype(np.float16)


def imatmul(a, b):
    """exact integer matrix product, evaluated by a floating-point GEMM in which every partial sum is an integer below the
    format's 2**24 / 2**53 (asserted) and therefore exact in any order; back to int64."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    bound = float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) * a.shape[-1]
    assert bound < 2.0 ** 53
    ft = np.float32 if bound < 2.0 ** 24 else np.float64
    return (a.astype(ft) @ b.astype(ft)).astype(np.int64)


def gen_matrix(rng, n_out, n_in, k=K_TERMS):
    # one stream of concatenated permutations for all k terms: a matrix with fewer rows than columns (Wout) then reaches
    # k * n_out distinct columns, the most a row norm of k allows
    W = np.zeros((n_out, n_in), np.int64)
    cols = np.concatenate([rng.permutation(n_in) for _ in range(-(-k * n_out // n_in))])[:k * n_out].reshape(k, n_out)
    for t in range(k):
        W[np.arange(n_out), cols[t]] += rng.choice(np.array([-1, 1]), n_out)
    assert np.abs(W).sum(1).max() <= k
    return W


def gen_weights(rng, IN, H, NL):
    return [gen_matrix(rng, H, IN)] + [gen_matrix(rng, H, H) for _ in range(NL - 1)] + [gen_matrix(rng, OUT, H)]


def gen_ints(rng, shape, p=None, lo=-2, hi=2):
    """integers in [lo, hi]; p: the sparse flavour, +-1 with probability p, else 0"""
    if p is None:
        return rng.integers(lo, hi + 1, shape).astype(np.int64)
    return np.where(rng.random(shape) < p, rng.choice(np.array([-1, 1]), shape), 0).astype(np.int64)


def flat(mats):
    return np.concatenate([np.asarray(m).reshape(-1) for m in mats])


def forward(mats, X, drop_kstep=None):
    """-> (acts: post-ReLU activations per layer, masks, outputs).  drop_kstep = k: the first layer leaves out input columns
    16k .. 16k + 15 (a mutant for the sensitivity self-test)."""
    acts, masks = [], []
    a = np.asarray(X, np.int64)
    for l, W in enumerate(mats[:-1]):
        if l == 0 and drop_kstep is not None:
            a = a.copy(); a[:, 16 * drop_kstep:16 * drop_kstep + 16] = 0
        pre = imatmul(a, W.T)
        masks.append(pre > 0)
        a = np.where(pre > 0, pre, 0)
        acts.append(a)
    return acts, masks, imatmul(a, mats[-1].T)


def backward(mats, X, acts, masks, dY, row_weight=None):
    """-> (dH per layer in LAYER order [dH[l] = dL/d(pre-activation of matmul l)], the same before the ReLU mask, dX, dW per
    matrix).  row_weight [B]: how often a batch row counts in dW (mutants: 0 = left out, 2 = counted twice)."""
    NL = len(mats) - 1
    dH, pre = [None] * NL, [None] * NL
    d = np.asarray(dY, np.int64)
    for l in range(NL - 1, -1, -1):
        pre[l] = imatmul(d, mats[l + 1])
        d = dH[l] = np.where(masks[l], pre[l], 0)
    dX = imatmul(d, mats[0])
    rw = np.ones(len(X), np.int64) if row_weight is None else np.asarray(row_weight, np.int64)
    ins = [np.asarray(X, np.int64)] + list(acts)
    outs = dH + [np.asarray(dY, np.int64)]
    dW = [imatmul((o * rw[:, None]).T, i) for o, i in zip(outs, ins)]
    return dH, pre, dX, dW


def dw_abs_bound(mats, X, acts, dH, dY):
    """an upper bound of sum_b |dH[b, o]| * |A[b, i]| over every dW entry, max_o sum_b |dH[b, o]| * max |A|: below 2**24 every
    fp32 partial sum of every entry is exact whatever the order"""
    ins = [np.asarray(X, np.int64)] + list(acts)
    outs = list(dH) + [np.asarray(dY, np.int64)]
    return max(int(np.abs(o).sum(0).max()) * int(np.abs(i).max()) for o, i in zip(outs, ins))


class Case:
    """one network + batch with its integer reference and the values every buffer must hold (fp16, as float16 numpy)"""

    def __init__(self, IN, H, NL, mats, X, dY, denom=1, check=True):
        self.IN, self.H, self.NL, self.B = IN, H, NL, len(X)
        self.mats, self.X, self.dY, self.denom = mats, X, dY, denom
        self.acts, self.masks, self.out = forward(mats, X)
        if dY is None:                                                          # forward only
            return
        self.dH, self.pre, self.dX, self.dW = backward(mats, X, self.acts, self.masks, dY)
        if check:
            self.check_conditions()

    # dY, dH, dX and dW are numerators over `denom` (a power of two; the head's grad_h column 0 = grad_sigma * density_scale)
    def q(self, v):
        return rn_f16(np.asarray(v, np.float64) / self.denom)

    def expected(self):
        return dict(W=rn_f16(flat(self.mats)), X=rn_f16(self.X), dY=self.q(self.dY),
                    fwd_buf=rn_f16(np.stack(self.acts)), out=rn_f16(self.out),
                    bwd_buf=self.q(np.stack(self.dH[::-1])), dX=self.q(self.dX), dW=self.q(flat(self.dW)))

    def dw_accumulated(self, old):
        """RN_fp16(old + exact): the one rounding of dw_reduce_body with accumulate"""
        return rn_f16(np.asarray(old, np.float64) + flat(self.dW).astype(np.float64) / self.denom)

    def check_conditions(self, min_dx=0.20, min_dw=0.20):
        """the conditions under which the comparison is exact and carries signal -- conditions, not measurements"""
        for v in [self.X, self.out] + self.acts:
            assert np.abs(v).max() <= 2048
        # numerators over denom: fp16 holds every integer up to 2048 and every multiple of 1 / denom (denom > 1) below 1024
        for v in [self.dY, self.dX] + self.dH:
            assert np.abs(v).max() <= (2048 if self.denom == 1 else 1024) * self.denom
        for w in self.dW:
            assert np.abs(w).max() <= 2048 * self.denom, int(np.abs(w).max())
        assert dw_abs_bound(self.mats, self.X, self.acts, self.dH, self.dY) < 2 ** 24
        for l, m in enumerate(self.masks):
            on = m.mean()
            assert 0.25 <= on <= 0.75, (l, on)
        assert (self.dX != 0).mean() >= min_dx, (self.dX != 0).mean()
        for k, w in enumerate(self.dW):
            assert (w != 0).mean() >= min_dw, (k, (w != 0).mean())


# sparse flavour: the probability of a nonzero entry in the inputs and in the upstream gradient.  The largest |dW| entry grows like
# sqrt(B * p_x * p_g) while the ReLU on-fraction and the dX fill need p_x, p_g not too small; with these values every condition of
# Case.check_conditions holds at the wrap sizes (asserted there for every case handed out).
SPARSE_P = (0.25, 0.125)


def seed_of(*key):
    return int(np.random.SeedSequence([int(k) for k in key]).generate_state(1)[0])


MAX_DRAWS = 16


def draw(make, *key):
    """make(rng) with the first of MAX_DRAWS seeds whose case meets its conditions.  The conditions are properties of the
    generated inputs and of the integer reference alone (no kernel is involved), so discarding a draw biases nothing."""
    for attempt in range(MAX_DRAWS):
        try:
            return make(np.random.default_rng(seed_of(*key, attempt)))
        except AssertionError as e:
            last = e
    raise AssertionError(f"no draw of {key} meets the conditions: {last}")


@functools.lru_cache(maxsize=4)
def mlp_case(IN, H, NL, B, sparse=False):
    px, pg = SPARSE_P if sparse else (None, None)
    return draw(lambda rng: Case(IN, H, NL, gen_weights(rng, IN, H, NL), gen_ints(rng, (B, IN), px), gen_ints(rng, (B, OUT), pg)),
                IN, H, NL, B)


def generic_params(cases, cus=MI355X_CUS):
    """(IN, H, NL, B, sparse) of the generic-MLP tests"""
    ps = [(IN, H, NL, B, False) for (IN, H, NL) in cases for B in B_SMALL]
    ps += [(IN, H, NL, B, True) for (IN, H, NL) in WRAP_SHAPES for B in wrap_sizes(IN, H, NL, cus)]
    return ps


# ---------------------------------------------------------------- fused NeRF head
def ulp16(x):
    """fp16 ulp at |x| (subnormal spacing 2**-24 below 2**-14)"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -14)))
    return 2.0 ** (e - 10)


class HeadCase:
    """sigma net 32 -> 64 -> 16 (one hidden GEMM), colour net [SH(16) | geo(15) | 0] -> 64 -> 64 -> 16 with the SH columns of its
    W0 zero: the inexact SH values reach no activation, so everything but dW0[:, :16] of the colour net is an integer."""

    def __init__(self, rng, M, sparse=False, density_scale=1.0, forward_only=False):
        px, pg = SPARSE_P if sparse else (None, None)
        self.M, self.ds = M, density_scale
        self.ws = gen_weights(rng, 32, 64, 2)
        wc = gen_weights(rng, 16, 64, 3)
        wc[0] = np.concatenate([np.zeros((64, 16), np.int64), wc[0]], axis=1)     # columns 0..15 (SH) zero; 16..31 = geo | pad
        self.wc = wc
        self.enc = gen_ints(rng, (M, 32), px)
        d = rng.standard_normal((M, 3))
        self.dirs = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        # ---- forward: h = sigma net (integers); colour input = [SH | h[1:16] | 0]
        self.fwd_s = Case(32, 64, 2, self.ws, self.enc, None)
        h = self.fwd_s.out
        assert np.abs(h[:, 0]).max() <= 80                                      # fp32 exp stays finite
        cin = np.concatenate([np.zeros((M, 16), np.int64), h[:, 1:], np.zeros((M, 1), np.int64)], axis=1)
        self.fwd_c = Case(32, 64, 3, self.wc, cin, None)
        for v in [h] + self.fwd_s.acts + self.fwd_c.acts + [self.fwd_c.out]:
            assert np.abs(v).max() <= 2048
        # the forward comparison carries signal: every layer of both nets has 25 - 75 % of its units on, and the colour net, seen
        # only through rgb = fp16(sigmoid(logit)), has logits where the sigmoid is not saturated: 1 - sigmoid(8) = 3.4e-4 is the
        # last value above half an fp16 ulp below 1 (2**-12), so |logit| < 8 is where a wrong logit moves the stored half.  One
        # logit in ten there is asked (of 3 M values, M >= 16).
        for m in self.fwd_s.masks + self.fwd_c.masks:
            assert 0.25 <= m.mean() <= 0.75, m.mean()
        assert (np.abs(self.fwd_c.out[:, :3]) < 8).mean() >= 0.10
        if forward_only:
            return
        # ---- backward on exact inputs of its own: h0 = 0 (exp = 1), geo in [-2, 2], rgb = 0.5 (rgb (1 - rgb) = 1/4)
        self.h_b = np.concatenate([np.zeros((M, 1), np.int64), gen_ints(rng, (M, 15), px)], axis=1)
        self.grad_rgbs = 4 * gen_ints(rng, (M, 3), pg if pg is None else 2 * pg)     # 3 live columns of 16: a denser draw
        self.grad_sigmas = gen_ints(rng, (M,), pg)
        cin_b = np.concatenate([np.zeros((M, 16), np.int64), self.h_b[:, 1:], np.zeros((M, 1), np.int64)], axis=1)
        dYc = np.zeros((M, 16), np.int64); dYc[:, :3] = self.grad_rgbs // 4
        self.bwd_c = Case(32, 64, 3, self.wc, cin_b, dYc, check=False)
        # grad_h = [grad_sigma * density_scale | dX[16..30] of the colour net], as numerators over `den`
        den = int(round(1 / density_scale)) if density_scale < 1 else 1
        assert den * density_scale == int(den * density_scale)
        self.den = den
        gh = np.concatenate([(self.grad_sigmas * int(den * density_scale))[:, None], den * self.bwd_c.dX[:, 16:31]], axis=1)
        self.grad_h = gh
        self.bwd_s = Case(32, 64, 2, self.ws, self.enc, gh, denom=den, check=False)
        self.check_conditions()

    def check_conditions(self):
        c, s = self.bwd_c, self.bwd_s
        for v in [c.dY, c.dX] + c.acts + c.dH + c.dW:
            assert np.abs(v).max() <= 2048
        for v in [s.dY, s.dX] + s.dH:                                           # fp16-stored multiples of 1 / den: exact below 1024 if den > 1
            assert np.abs(v).max() <= (2048 if self.den == 1 else 1024) * self.den
        for v in s.dW:                                                          # one rounding of an exact fp32 sum
            assert np.abs(v).max() <= 2048 * self.den
        assert np.abs(np.concatenate([a.reshape(-1) for a in s.acts])).max() <= 2048
        assert dw_abs_bound(c.mats, c.X, c.acts, c.dH, c.dY) < 2 ** 24 and dw_abs_bound(s.mats, s.X, s.acts, s.dH, s.dY) < 2 ** 24
        for m in s.masks + c.masks:
            assert 0.25 <= m.mean() <= 0.75, m.mean()
        assert (s.dX != 0).mean() >= 0.20 and (self.grad_h[:, 1:] != 0).mean() >= 0.20
        for w in s.dW:
            assert (w != 0).mean() >= 0.20
        # colour net: only outputs 0..2 carry a gradient, so only the hidden units with a path to them can have a nonzero dW row
        # (at most 12 of the 64 units of the last hidden layer: Wout rows have 4 entries).  The 20 % is asked of the rows that
        # can be nonzero, and of the geo columns of dW0 (its SH columns are not integers, column 31 is zero).
        reach = np.zeros(16, bool); reach[:3] = True
        for k in range(len(c.dW) - 1, -1, -1):
            w = c.dW[k][reach]
            w = w[:, 16:31] if k == 0 else w
            assert (w != 0).mean() >= 0.20, (k, (w != 0).mean())
            reach = np.abs(c.mats[k][reach]).sum(0) > 0


@functools.lru_cache(maxsize=2)
def head_case(M, sparse=False, density_scale=1.0):
    return draw(lambda rng: HeadCase(rng, M, sparse, density_scale), 7, M)


def head_fwd_wrap(cus=MI355X_CUS):
    """a row count past one sweep of k_nerf_head_fwd5's grid-stride loop (launch_head_fwd5_w: cus blocks x 8 waves x 64 rows per
    wave iteration), + 48 rows: a last group with three of its four tiles.  M = 64 * 1031 wraps only the two backward kernels
    (sweeps of cus * 128 and cus * 256 rows)."""
    return cus * 8 * 64 + 48


@functools.lru_cache(maxsize=1)
def head_fwd_case(M):
    return draw(lambda rng: HeadCase(rng, M, True, 1.0, forward_only=True), 11, M)


def head_params():
    """(M, sparse, density_scale): scale 1 at every M, the other two (powers of two: exactness survives) at M = 144"""
    return [(M, M >= HEAD_SPARSE_FROM, 1.0) for M in HEAD_M] + [(144, False, 2.0), (144, False, 0.5)]


def to_level_major(a):
    """[M, 32] -> [16, M, 2] (the grid kernels' layout: feature 2 l + ch of row m at [l, m, ch])"""
    return np.ascontiguousarray(np.asarray(a).reshape(len(a), 16, 2).transpose(1, 0, 2))
