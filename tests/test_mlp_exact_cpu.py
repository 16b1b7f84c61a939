"""the exact-arithmetic MLP cases (mlp_exact_util) without a GPU: every case the GPU file uses meets the conditions that make
the comparison exact, the CPU oracle equals the integer reference bit for bit on them (which validates the reference
independently of any kernel), and the comparison notices the errors it is meant to notice (mutants of the reference)."""
import numpy as np
import pytest

import mlp_exact_util as U
from test_gpu_ffmlp import CASES

PARAMS = U.generic_params(CASES)            # CU-dependent sizes at the MI355X's 256 CUs
# the oracle takes 5 - 15 s on a wrap-size batch (65 584 / 131 120 rows).  Above ORACLE_MAX_B rows it runs on the last ORACLE_TAIL
# rows only (rows are independent in everything but dW; the dW of those cases comes from the same integer code as the others')
ORACLE_MAX_B, ORACLE_TAIL = 5000, 1168


def bits(a):
    """fp16 bit patterns with -0 folded into +0 (the comparison is on values; every expected value is an integer)"""
    a = np.ascontiguousarray(a, np.float16) + np.float16(0)
    return a.view(np.uint16)


def assert_oracle_equal(O, c):
    if c.B > ORACLE_MAX_B:
        n = ORACLE_TAIL
        sub = U.Case(c.IN, c.H, c.NL, c.mats, c.X[-n:], c.dY[-n:], denom=c.denom, check=False)
        assert np.array_equal(sub.dX, c.dX[-n:]) and all(np.array_equal(a, b[-n:]) for a, b in zip(sub.acts + sub.dH, c.acts + c.dH))
        c = sub
    e = c.expected()
    Wh, Xh, Gh = e["W"].view(np.uint16), e["X"].view(np.uint16), e["dY"].view(np.uint16)
    out, fb = O.ffmlp_forward(Xh, Wh, c.IN, 16, c.H, c.NL)
    assert np.array_equal(bits(out.view(np.float16)), bits(e["out"]))
    assert np.array_equal(bits(fb.view(np.float16)), bits(e["fwd_buf"]))
    gw, gi, bb = O.ffmlp_backward(Gh, Xh, Wh, e["fwd_buf"].view(np.uint16), c.IN, 16, c.H, c.NL, calc_grad_inputs=True)
    assert np.array_equal(bits(bb.view(np.float16)), bits(e["bwd_buf"]))
    assert np.array_equal(bits(gi.view(np.float16)), bits(e["dX"]))
    assert np.array_equal(bits(gw.view(np.float16)), bits(e["dW"]))


@pytest.mark.parametrize("IN,H,NL,B,sparse", PARAMS)
def test_case_meets_conditions_and_oracle_equals_integers(O, IN, H, NL, B, sparse):
    c = U.mlp_case(IN, H, NL, B, sparse)
    c.check_conditions()
    e = c.expected()
    for k in ("W", "X", "dY", "fwd_buf", "out", "bwd_buf", "dX"):               # fp16 holds every one of these integers exactly
        assert np.isfinite(e[k]).all()
    assert np.array_equal(e["dX"].astype(np.int64), c.dX) and np.array_equal(e["fwd_buf"].astype(np.int64), np.stack(c.acts))
    assert np.array_equal(e["dW"].astype(np.int64), U.flat(c.dW))               # |dW| <= 2048: one unit is visible in the half
    assert_oracle_equal(O, c)


def test_wrap_sizes_are_whole_tiles_and_reach_both_tile_counts():
    """every wrap size is a whole number of 16-row tiles; up to width 64 exactly one of them is a multiple of 32 (the two-tile
    instantiations), the others are not (the one-tile fallback).  That the figures exceed one sweep follows from the launch code
    quoted in wrap_sizes; it is not checked here."""
    assert U.head_fwd_wrap() % 16 == 0 and U.head_fwd_wrap() % 64 == 48
    for IN, H, NL in U.WRAP_SHAPES:
        sizes = U.wrap_sizes(IN, H, NL)
        assert all(B % 16 == 0 for B in sizes) and sum(B % 32 == 0 for B in sizes) == (1 if H <= 64 else 0)


@pytest.mark.parametrize("M,sparse,ds", U.head_params())
def test_head_case_meets_conditions_and_oracle_equals_integers(O, M, sparse, ds):
    h = U.head_case(M, sparse, ds)
    h.check_conditions()
    assert np.array_equal(h.wc[0][:, :16], np.zeros((64, 16), np.int64))        # no SH value reaches an activation
    assert np.all(h.h_b[:, 0] == 0) and np.all(h.grad_rgbs % 4 == 0)
    # both backward nets against the oracle (the colour net's SH columns are zero inputs here: the integer part)
    assert_oracle_equal(O, h.bwd_c)
    assert_oracle_equal(O, h.bwd_s)
    # forward chain: sigma net -> colour input -> colour net
    n = min(M, ORACLE_TAIL)
    for c in (h.fwd_s, h.fwd_c):
        W, X = U.rn_f16(U.flat(c.mats)).view(np.uint16), U.rn_f16(c.X[-n:]).view(np.uint16)
        out, fb = O.ffmlp_forward(X, W, 32, 16, 64, c.NL)
        assert np.array_equal(bits(out.view(np.float16)), bits(U.rn_f16(c.out[-n:])))
        assert np.array_equal(bits(fb.view(np.float16)), bits(U.rn_f16(np.stack([a[-n:] for a in c.acts]))))


def test_head_forward_wrap_case_meets_conditions_and_oracle_equals_integers(O):
    h = U.head_fwd_case(U.head_fwd_wrap())
    n = ORACLE_TAIL
    for c in (h.fwd_s, h.fwd_c):
        W, X = U.rn_f16(U.flat(c.mats)).view(np.uint16), U.rn_f16(c.X[-n:]).view(np.uint16)
        out, fb = O.ffmlp_forward(X, W, 32, 16, 64, c.NL)
        assert np.array_equal(bits(out.view(np.float16)), bits(U.rn_f16(c.out[-n:])))
        assert np.array_equal(bits(fb.view(np.float16)), bits(U.rn_f16(np.stack([a[-n:] for a in c.acts]))))


def test_accumulate_expectation_rounds_once():
    c = U.mlp_case(48, 64, 3, 1168)
    old = np.random.default_rng(0).integers(-8, 9, U.flat(c.dW).shape)
    exp = c.dw_accumulated(old)
    assert np.array_equal(exp.astype(np.float64), (old + U.flat(c.dW)).astype(np.float64).astype(np.float16).astype(np.float64))
    assert np.abs(old + U.flat(c.dW)).max() > 1024                              # some sums are past the half's integer range of step 1 / 2
    assert not np.array_equal(exp, c.expected()["dW"])


# ---------------------------------------------------------------- sensitivity of the comparison
def compared(c, acts, out, dH, dX, dW):
    return dict(fwd_buf=U.rn_f16(np.stack(acts)), out=U.rn_f16(out), bwd_buf=c.q(np.stack(dH[::-1])), dX=c.q(dX), dW=c.q(U.flat(dW)))


def differs(a, b):
    return [k for k in a if not np.array_equal(bits(a[k]), bits(b[k]))]


@pytest.mark.parametrize("IN,H,NL,B", [(48, 64, 3, 144), (32, 64, 2, 1168), (32, 128, 2, 1152)])
def test_mutants_change_a_compared_bit(IN, H, NL, B):
    """the errors the GPU test is there to catch, applied to the reference: each changes the bits of a compared array"""
    c = U.mlp_case(IN, H, NL, B)
    ref = compared(c, c.acts, c.out, c.dH, c.dX, c.dW)
    assert differs(ref, compared(c, c.acts, c.out, c.dH, c.dX, c.dW)) == []
    live = np.flatnonzero((np.abs(c.dH[0]).sum(1) > 0) & (np.abs(c.X).sum(1) > 0))   # rows that contribute to dW0 at all
    assert len(live) > B // 4
    row = int(live[len(live) // 2])
    for weight in (0, 2):                                       # one batch row left out of dW / counted twice
        rw = np.ones(B, np.int64); rw[row] = weight
        dW = U.backward(c.mats, c.X, c.acts, c.masks, c.dY, row_weight=rw)[3]
        assert differs(ref, compared(c, c.acts, c.out, c.dH, c.dX, dW)) == ["dW"]
    dX = c.dX.copy(); dX[16:32] = c.dX[32:48]                   # one 16-row tile's dX taken from the next tile
    assert differs(ref, compared(c, c.acts, c.out, c.dH, dX, c.dW)) == ["dX"]
    # one ReLU mask bit flipped, at a unit whose incoming gradient is not zero (elsewhere the flip changes nothing)
    l = c.NL - 1
    b, u = (int(v[0]) for v in np.nonzero(c.pre[l]))
    masks = [m.copy() for m in c.masks]; masks[l][b, u] ^= True
    dH, _, dX, dW = U.backward(c.mats, c.X, c.acts, masks, c.dY)
    assert "bwd_buf" in differs(ref, compared(c, c.acts, c.out, dH, dX, dW))
    # one k-step (16 input columns) left out of the first layer
    acts, masks, out = U.forward(c.mats, c.X, drop_kstep=IN // 16 - 1)
    assert "fwd_buf" in differs(ref, compared(c, acts, out, c.dH, c.dX, c.dW))
