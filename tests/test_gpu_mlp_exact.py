"""-m gpu: the MFMA MLP kernels and the fused NeRF head against exact integer arithmetic (mlp_exact_util).

Every case is built so that each value a kernel stores is an exactly representable integer and every fp32 partial sum is exact
(tests/test_mlp_exact_cpu.py asserts the conditions and that the CPU oracle equals the integer reference bit for bit).  The
expected bits therefore do not depend on the summation order -- K = 16 or K = 32 MFMA, one or two tiles per wave, wave-private or
cooperative dW, any slab count -- and every comparison is torch.equal: a dropped, duplicated or misplaced row, tile, k-step or
ReLU mask changes an integer and therefore a bit.  Outputs start NaN-filled, so an unwritten element shows.  The only
tolerances are the three bounded comparisons of the head (sigma / rgb behind expf, the SH columns of the colour dW0, the
trunc_exp clamp rows); each is derived where it is used."""
import types

import numpy as np
import pytest
import torch

import mlp_exact_util as U
from gpu_util import DEV, T
from test_gpu_ffmlp import CASES

pytestmark = pytest.mark.gpu

CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else U.MI355X_CUS
PARAMS = U.generic_params(CASES, CUS)
NAN = float("nan")


def same(got, exp, what):
    """torch.equal, with the place of the first mismatches in the message (the integer structure tells rows / tiles / columns)"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, what
    if torch.equal(got, exp):
        return
    bad = torch.nonzero(~(got == exp))
    first = [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(exp[tuple(ix)])) for ix in bad[:6]]
    pytest.fail(f"{what}: {len(bad)} of {got.numel()} elements differ; first (index, got, expected): {first}; "
                f"rows {sorted(set(int(ix[-2]) for ix in bad[:2000]))[:12] if got.dim() >= 2 else ''}")


def nan_like(shape, dtype=torch.half):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


@pytest.fixture(scope="module", params=PARAMS, ids=lambda p: "-".join(str(int(v)) for v in p[:4]) + ("-sparse" if p[4] else ""))
def case(request):
    IN, H, NL, B, sparse = request.param
    c = U.mlp_case(IN, H, NL, B, sparse)
    e = c.expected()
    return types.SimpleNamespace(c=c, IN=IN, H=H, NL=NL, B=B, nW=len(e["W"]), **{k: T(v) for k, v in e.items()})


def test_forward_and_inference(case):
    from laenerf_amd.backend import ffmlp_backend as F
    k = case
    recompute = F.fused_backward_available(k.IN, k.H, k.NL, 0)
    try:
        F.ffmlp_set_mode(1)                                  # the buffer-faithful path fills forward_buffer for every shape
        out, fb = nan_like((k.B, 16)), nan_like((k.NL, k.B, k.H))
        F.ffmlp_forward(k.X, k.W, k.B, k.IN, 16, k.H, k.NL, 0, 6, fb, out)
        same(fb, k.fwd_buf, "mode 1 forward_buffer"); same(out, k.out, "mode 1 outputs")
        out_i = nan_like((k.B, 16))
        F.ffmlp_inference(k.X, k.W, k.B, k.IN, 16, k.H, k.NL, 0, 6, None, out_i)
        same(out_i, k.out, "mode 1 inference")
    finally:
        F.ffmlp_set_mode(0)
    out, fb = nan_like((k.B, 16)), torch.full((k.NL, k.B, k.H), -7.0, dtype=torch.half, device=DEV)
    F.ffmlp_forward(k.X, k.W, k.B, k.IN, 16, k.H, k.NL, 0, 6, fb, out)
    same(out, k.out, "mode 0 outputs")
    if recompute:
        assert bool((fb == -7.0).all())                      # the recompute backward never reads it: left untouched
    else:
        same(fb, k.fwd_buf, "mode 0 forward_buffer")
    out_i = nan_like((k.B, 16))
    F.ffmlp_inference(k.X, k.W, k.B, k.IN, 16, k.H, k.NL, 0, 6, None, out_i)
    same(out_i, k.out, "mode 0 inference")


def test_backward(case):
    from laenerf_amd.backend import ffmlp_backend as F
    k = case
    try:
        for mode in (1, 0, 3):
            F.ffmlp_set_mode(mode)
            fused = mode != 1 and F.fused_backward_available(k.IN, k.H, k.NL, 0)
            fb = None if fused else k.fwd_buf                # the reference's forward buffer where a buffer is read
            bb = None if fused else nan_like((k.NL, k.B, k.H))
            gi, gw = nan_like((k.B, k.IN)), nan_like((k.nW,))
            F.ffmlp_backward(k.dY, k.X, k.W, fb, k.B, k.IN, 16, k.H, k.NL, 0, 6, True, bb, gi, gw)
            if not fused:
                same(bb, k.bwd_buf, f"mode {mode} backward_buffer")
            same(gi, k.dX, f"mode {mode} grad_inputs"); same(gw, k.dW, f"mode {mode} grad_weights")
            # calc_grad_inputs = False: the same weight gradient, grad_inputs untouched
            bb = None if fused else nan_like((k.NL, k.B, k.H))
            gi, gw = nan_like((k.B, k.IN)), nan_like((k.nW,))
            F.ffmlp_backward(k.dY, k.X, k.W, fb, k.B, k.IN, 16, k.H, k.NL, 0, 6, False, bb, gi, gw)
            same(gw, k.dW, f"mode {mode} grad_weights without grad_inputs")
            if not fused:
                same(bb, k.bwd_buf, f"mode {mode} backward_buffer without grad_inputs")
            assert bool(gi.isnan().all()), mode
    finally:
        F.ffmlp_set_mode(0)


def test_backward_accumulate(case):
    """lae_ffmlp_backward_ex, accumulate = 1: grad_weights = RN_fp16(old + exact), one rounding (dw_reduce_body); the shapes the
    fused backward does not serve answer LAE_EINVAL"""
    from laenerf_amd.backend import ffmlp_backend as F
    k = case
    old = np.random.default_rng(k.B).integers(-8, 9, k.nW)
    if not F.fused_backward_available(k.IN, k.H, k.NL, 0):
        gw = T(U.rn_f16(old))
        with pytest.raises(RuntimeError):
            F.ffmlp_backward(k.dY, k.X, k.W, k.fwd_buf, k.B, k.IN, 16, k.H, k.NL, 0, 6, True, nan_like((k.NL, k.B, k.H)),
                             nan_like((k.B, k.IN)), gw, accumulate=True)
        same(gw, T(U.rn_f16(old)), "grad_weights after the refused call")
        return
    exp = T(k.c.dw_accumulated(old))
    try:
        for mode in (0, 3):
            F.ffmlp_set_mode(mode)
            gi, gw = nan_like((k.B, k.IN)), T(U.rn_f16(old))
            F.ffmlp_backward(k.dY, k.X, k.W, None, k.B, k.IN, 16, k.H, k.NL, 0, 6, True, None, gi, gw, accumulate=True)
            same(gw, exp, f"mode {mode} accumulated grad_weights"); same(gi, k.dX, f"mode {mode} grad_inputs")
        F.ffmlp_set_mode(1)                                  # the buffer-faithful path has no accumulate either
        gw = T(U.rn_f16(old))
        with pytest.raises(RuntimeError):
            F.ffmlp_backward(k.dY, k.X, k.W, k.fwd_buf, k.B, k.IN, 16, k.H, k.NL, 0, 6, True, nan_like((k.NL, k.B, k.H)),
                             nan_like((k.B, k.IN)), gw, accumulate=True)
    finally:
        F.ffmlp_set_mode(0)


# ---------------------------------------------------------------- fused NeRF head
def ulp32(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))) - 23)


def sigma_bound(ref):
    """sigma = density_scale * expf((float)h0) (k_nerf_head_fwd5): h0 is an exact integer, expf is within 1 fp32 ulp (HIP's
    documented bound), the product with a power of two is exact, the value is stored as fp32 (the narrowest format it passes
    through: 1 ulp) -> 2 fp32 ulps of the fp64 value"""
    return 2 * ulp32(ref)


def rgb_bound(ref):
    """rgb = (float)(half)(1 / (1 + expf(-(float)(half)logit))): the logit is an exact integer also as a half; expf within 1 fp32
    ulp, the sum rounds once (0.5 ulp), the division is within HIP's documented 2.5 ulp -> at most 4 fp32 ulps = 2**-21 relative
    before the value is rounded to fp16, the narrowest format it passes through: 1 fp16 ulp.  (Past |logit| = 88 expf overflows
    to inf or underflows to 0 and rgb is exactly 0 or 1: within 2**-24, the smallest fp16 ulp, of the fp64 value.)"""
    return U.ulp16(ref) + 2.0 ** -21 * np.abs(ref)


@pytest.fixture(scope="module", params=U.head_params(), ids=lambda p: f"{p[0]}-{'sparse' if p[1] else 'dense'}-{p[2]}")
def head(request):
    M, sparse, ds = request.param
    h = U.head_case(M, sparse, ds)
    s, c = h.bwd_s, h.bwd_c
    k = types.SimpleNamespace(h=h, M=M, ds=ds, ws=T(U.rn_f16(U.flat(h.ws))), wc=T(U.rn_f16(U.flat(h.wc))), dirs=T(h.dirs))
    k.enc = {False: T(U.rn_f16(h.enc)), True: T(U.to_level_major(U.rn_f16(h.enc)))}
    k.h_fwd = T(U.rn_f16(h.fwd_s.out))
    k.h_b = T(U.rn_f16(h.h_b)); k.rgbs = torch.full((M, 3), 0.5, device=DEV)
    k.gs = T(h.grad_sigmas.astype(np.float32)); k.gr = T(h.grad_rgbs.astype(np.float32))
    k.grad_h = T(s.q(h.grad_h))
    k.grad_enc = {False: T(s.q(s.dX)), True: T(U.to_level_major(s.q(s.dX)))}
    return k


def check_head_forward(h, M, ds, enc, dirs, ws, wc, h_fwd, level_major):
    """nerf_head_forward and nerf_density_forward on the forward chain of HeadCase h: h_out exact, sigma and rgb to their bounds"""
    from laenerf_amd.backend import ffmlp_backend as F
    hq, sig, rgb = nan_like((M, 16)), nan_like((M,), torch.float32), nan_like((M, 3), torch.float32)
    F.nerf_head_forward(enc, dirs, ws, wc, M, ds, hq, sig, rgb, level_major=level_major)
    same(hq, h_fwd, "h_out")
    hq2, sig2 = nan_like((M, 16)), nan_like((M,), torch.float32)
    F.nerf_density_forward(enc, ws, M, ds, hq2, sig2, level_major=level_major)
    same(hq2, hq, "nerf_density_forward h_out"); same(sig2, sig, "nerf_density_forward sigmas")
    h0 = h.fwd_s.out[:, 0].astype(np.float64)
    logits = h.fwd_c.out[:, :3].astype(np.float64)
    assert np.abs(h0).max() <= 80                                               # fp32 exp stays finite
    ref = ds * np.exp(h0)
    assert np.all(np.abs(sig.cpu().numpy().astype(np.float64) - ref) <= sigma_bound(ref))
    ref = 1.0 / (1.0 + np.exp(-logits))
    assert np.all(np.abs(rgb.cpu().numpy().astype(np.float64) - ref) <= rgb_bound(ref))


@pytest.mark.parametrize("level_major", [False, True])
def test_head_forward(head, level_major):
    """(M = 64 * 1031 is past one sweep of both backward kernels only: test_head_forward_past_one_sweep wraps the forward kernels)"""
    k = head
    check_head_forward(k.h, k.M, k.ds, k.enc[level_major], k.dirs, k.ws, k.wc, k.h_fwd, level_major)


@pytest.mark.parametrize("level_major", [False, True])
def test_head_forward_past_one_sweep(level_major):
    """k_nerf_head_fwd5<true | false, 8> (nerf_head_forward / nerf_density_forward) with more 64-row groups than waves: the
    `grp += nwaves` loop and its prefetch of the next group's inputs run a second time; forward only, sparse flavour"""
    M = U.head_fwd_wrap(CUS)
    h = U.head_fwd_case(M)
    enc = U.rn_f16(h.enc)
    check_head_forward(h, M, 1.0, T(U.to_level_major(enc) if level_major else enc), T(h.dirs), T(U.rn_f16(U.flat(h.ws))),
                       T(U.rn_f16(U.flat(h.wc))), T(U.rn_f16(h.fwd_s.out)), level_major)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("level_major", [False, True])
def test_head_backward(O, head, level_major, mode, accumulate):
    """the kernel takes h and rgbs as inputs: h0 = 0 (expf = 1), rgb = 0.5 (rgb (1 - rgb) = 1/4), grad_rgbs multiples of 4.  It
    recomputes the colour-net input [SH(dirs) | h[1:16] | 0] itself; the SH columns of the colour W0 are zero, so the SH values
    reach only the gradient of those columns."""
    from laenerf_amd.backend import ffmlp_backend as F
    k, h = head, head.h
    M, s, c = k.M, h.bwd_s, h.bwd_c
    rng = np.random.default_rng(M)
    old_s, old_c = rng.integers(-8, 9, len(U.flat(h.ws))), rng.integers(-8, 9, len(U.flat(h.wc)))
    gh, genc = nan_like((M, 16)), nan_like(tuple(k.enc[level_major].shape))
    gws = T(U.rn_f16(old_s)) if accumulate else nan_like((len(old_s),))
    gwc = T(U.rn_f16(old_c)) if accumulate else nan_like((len(old_c),))
    try:
        F.ffmlp_set_mode(mode)
        F.nerf_head_backward(k.gs, k.gr, k.enc[level_major], k.dirs, k.h_b, k.rgbs, k.ws, k.wc, M, k.ds, gh, genc, gws, gwc,
                             accumulate=accumulate, level_major=level_major)
    finally:
        F.ffmlp_set_mode(0)
    same(gh, k.grad_h, "grad_h"); same(genc, k.grad_enc[level_major], "grad_enc")
    same(gws, T(s.dw_accumulated(old_s) if accumulate else s.q(U.flat(s.dW))), "grad_sigma_weights")
    # colour net: everything but dW0[:, :16] is an integer
    exp_c = c.dw_accumulated(old_c) if accumulate else c.q(U.flat(c.dW))
    got0, exp0 = gwc[:64 * 32].reshape(64, 32), T(exp_c[:64 * 32].reshape(64, 32))
    same(gwc[64 * 32:], T(exp_c[64 * 32:]), "grad_color_weights behind W0")
    same(got0[:, 16:], exp0[:, 16:], "grad_color_weights W0, geo columns and pad")
    if not accumulate:
        assert bool((got0[:, 31] == 0).all())                # the zero pad
    # dW0[o, i < 16] = sum_b dH0[b, o] * SH[b, i] with SH rounded to fp16 by the kernel and dH0 an exact integer: against the fp64
    # sum (the oracle's SH values) the product terms are off by one fp16 ulp of the SH operand at most, 2**-10 relative each, and
    # the stored half by one ulp, 2**-10 of the stored value (old + sum with accumulate); the fp32 accumulation is negligible
    sh = O.sh_encode_forward(h.dirs, 4)[0].astype(np.float64)
    dH0 = c.dH[0].astype(np.float64)
    ref = dH0.T @ sh + (old_c[:64 * 32].reshape(64, 32)[:, :16] if accumulate else 0.0)
    bound = 2.0 ** -10 * (np.abs(dH0).T @ np.abs(sh)) + 2.0 ** -10 * np.abs(ref)
    got = got0[:, :16].float().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= bound), float(np.nanmax(np.abs(got - ref) - bound))
    assert np.abs(ref).max() > 1.0                           # the SH columns carry a gradient


@pytest.mark.parametrize("ds", [1.0, 0.5])
def test_head_trunc_exp_clamp(ds):
    """trunc_exp: the backward clamps h0 to +-15 (expf(clampf(h0, -15, 15))), the forward does not (activation.py:9)"""
    from laenerf_amd.backend import ffmlp_backend as F
    h = U.head_case(16, False, 1.0)
    M = 16
    h0 = np.array([-20, -15, 0, 15, 20] * 4)[:M]
    # ---- backward: rows with h0 = +-20 give the bits of the rows with h0 = +-15
    hb = h.h_b.copy(); hb[:, 0] = h0
    # grad_sigmas: 2**-12 where h0 >= 0 (exp(15) * 2**-12 = 798 fits the half), 2**12 where h0 < 0, so that both exp(-15) * 2**12 =
    # 1.25e-3 and the unclamped exp(-20) * 2**12 = 8.4e-6 are nonzero and distinct halves: a clamp missing on either side shows
    gs_np = np.where(h0 < 0, 2.0 ** 12, 2.0 ** -12)
    gs = T(gs_np.astype(np.float32))
    for mode in (0, 3):
        gh, genc = nan_like((M, 16)), nan_like((M, 32))
        gws, gwc = nan_like((len(U.flat(h.ws)),)), nan_like((len(U.flat(h.wc)),))
        try:
            F.ffmlp_set_mode(mode)
            F.nerf_head_backward(gs, T(h.grad_rgbs.astype(np.float32)), T(U.rn_f16(h.enc)), T(h.dirs), T(U.rn_f16(hb)),
                                 torch.full((M, 3), 0.5, device=DEV), T(U.rn_f16(U.flat(h.ws))), T(U.rn_f16(U.flat(h.wc))), M, ds,
                                 gh, genc, gws, gwc, accumulate=False, level_major=False)
        finally:
            F.ffmlp_set_mode(0)
        g0 = gh[:, 0].cpu().numpy()
        for far, edge in ((-20, -15), (20, 15)):
            assert np.array_equal(g0[h0 == far].view(np.uint16), g0[h0 == edge][:1].view(np.uint16).repeat((h0 == far).sum()))
        # every row: fp16(grad_sigma * density_scale * exp(clamp(h0))) evaluated in fp64, to one fp16 ulp (the value is rounded to
        # fp16 once; the fp32 product and expf before it are 2**-13 of that ulp)
        ref = gs_np * ds * np.exp(np.clip(h0, -15, 15).astype(np.float64))
        assert np.all(np.abs(g0.astype(np.float64) - ref) <= U.ulp16(ref)), mode
        assert g0[h0 == 15][0] > 0 and np.all(g0[h0 == 0] == np.float16(2.0 ** -12 * ds))
        for edge, far in ((-15, -20), (15, 20)):             # the clamped value is not what the unclamped exponent would store
            with np.errstate(over="ignore"):                 # exp(20) * 2**-12 is past the half's range: inf
                unclamped = np.float64(gs_np[h0 == far][0] * ds * np.exp(float(far))).astype(np.float16)
            assert g0[h0 == edge][0] != 0 and np.isfinite(g0[h0 == edge][0]) and g0[h0 == far][0] != unclamped
        same(gh[:, 1:], T(U.rn_f16(h.bwd_c.dX[:, 16:31])), "grad_h behind column 0")   # h0 reaches nothing else
    # ---- forward, not clamped: a sigma net that copies enc[:, 0] to h0 (hidden units 0 / 1 = relu(+-x), Wout row 0 = [1, -1, 0..])
    W0, Wo = np.zeros((64, 32), np.int64), np.zeros((16, 64), np.int64)
    W0[0, 0], W0[1, 0] = 1, -1
    Wo[0, 0], Wo[0, 1] = 1, -1
    W1 = np.eye(64, dtype=np.int64)
    enc = h.enc.copy(); enc[:, 0] = h0
    ref_net = U.Case(32, 64, 2, [W0, W1, Wo], enc, None)
    assert np.array_equal(ref_net.out[:, 0], h0)
    hq, sig, rgb = nan_like((M, 16)), nan_like((M,), torch.float32), nan_like((M, 3), torch.float32)
    F.nerf_head_forward(T(U.rn_f16(enc)), T(h.dirs), T(U.rn_f16(U.flat([W0, W1, Wo]))), T(U.rn_f16(U.flat(h.wc))), M, ds, hq, sig, rgb)
    same(hq, T(U.rn_f16(ref_net.out)), "h_out")
    ref = ds * np.exp(h0.astype(np.float64))
    assert np.all(np.abs(sig.cpu().numpy().astype(np.float64) - ref) <= sigma_bound(ref))
    assert float(sig[h0 == 20][0]) > 100 * float(sig[h0 == 15][0])             # exp(20), not exp(15)
