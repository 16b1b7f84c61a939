"""-m gpu: the fused nearest-neighbour feature matcher and the NNFM loss kernels (csrc/nnfm.hip) against nnfm_numpy, the float64
restatement of the reference's argmin_cos_distance / nn_feat_replace / cos_loss (editing/semantic_encoder.py:83-164).

Bounds (none comes from the kernels' output):
  * matcher: an fp16-rounded unit vector perturbs a dot product of unit vectors by at most 2 * 2^-11 * sum |u_k v_k| <= 2^-10; fp32
    accumulation adds C * 2^-24; two cosines are compared, so the chosen column's float64 cosine is within 2^-8 of the best one for
    C <= 4096, and any row whose float64 margin exceeds 2^-8 has the exact index.  d_best is within 2^-9 of the float64 distance of
    the chosen column.
  * loss: |loss - loss64| <= (3C + 32) * 2^-24; gradient per position: max_k |dx - dx64| <= (4C + 16) * 2^-24 * 2 / ((|a_i| + 1e-8) n Na)
    (fp32 sums of C products, unit-vector components bounded by 1), both at the kernel's own match.  The gradient is linear in the
    upstream scalar g and g is a power of two here, so the bound is the unit bound times g.
"""
import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

from conftest import golden
from gpu_util import DEV, N, T
from nnfm_util import GOLDEN_CASES, golden_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1, 1), (1, 40, 70, 33), (2, 64, 150, 97), (1, 768, 256, 300), (1, 64, 130, 4100)]
COS_TOL, D_TOL = 2.0 ** -8, 2.0 ** -9


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


def _run(x, s, g=1.0, match="layer"):
    """kernels on fp32 numpy inputs [n, C, N] -> z, d_best, loss, dx (numpy)"""
    from laenerf_amd.editing import nnfm_loss, nnfm_match
    xt, stt = T(x).requires_grad_(), T(s)
    z, d = nnfm_match(xt.detach(), stt, return_distance=True)
    loss, z2 = nnfm_loss(xt, stt, match=match, return_match=True)
    (loss * g).backward()
    torch.cuda.synchronize()
    assert match != "layer" or torch.equal(z, z2)
    return N(z), N(d), float(loss.detach()), N(xt.grad)


def _check_cosine_bound(x, s, z, d):
    from laenerf_amd.editing import nnfm_numpy
    n, C, Na = x.shape
    Nb = s.shape[2]
    _, _, _, cos = nnfm_numpy(x, s)
    assert z.dtype == np.int32 and z.shape == (n, Na) and z.min() >= 0 and z.max() < Nb
    chosen = np.take_along_axis(cos, z[..., None].astype(np.int64), 2)[..., 0]
    best = cos.max(2)
    gap = float((best - chosen).max())
    derr = float(np.abs(d - (1.0 - chosen)).max())
    print(f"shape {(n, C, Na, Nb)}: worst cosine gap {gap:.3g} (bound {COS_TOL:.3g}), d_best error {derr:.3g} (bound {D_TOL:.3g}), "
          f"exact indices {int((z == cos.argmax(2)).sum())} / {n * Na}")
    assert gap <= COS_TOL
    assert derr <= D_TOL
    srt = np.sort(cos, 2)
    if Nb > 1:
        clear = (srt[..., -1] - srt[..., -2]) > COS_TOL
        assert np.array_equal(z[clear], cos.argmax(2)[clear])


def _check_loss_and_gradient(x, s, z, loss, dx, g=1.0):
    from laenerf_amd.editing import nnfm_numpy
    n, C, Na = x.shape
    _, loss64, dx64, _ = nnfm_numpy(x, s, z=z)
    lerr = abs(loss - loss64)
    na = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    bound = g * (4 * C + 16) * 2.0 ** -24 * 2.0 / ((na + 1e-8) * n * Na)
    gerr = np.abs(dx - g * dx64).max(1)
    print(f"shape {(n, C, Na, s.shape[2])} g {g}: loss error {lerr:.3g} (bound {(3 * C + 32) * 2.0 ** -24:.3g}), "
          f"worst gradient error / bound {float((gerr / bound).max()):.3g}")
    assert np.isfinite(dx).all() and np.isfinite(loss)
    assert lerr <= (3 * C + 32) * 2.0 ** -24
    assert (gerr <= bound).all()


def _planted(shape, seed):
    """content i = a positively scaled, lightly perturbed copy of style column p(i); p random, non-monotone, hits 0 and Nb - 1"""
    n, C, Na, Nb = shape
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    p = rng.integers(0, Nb, size=(n, Na))
    p[:, 0] = Nb - 1
    p[:, -1] = 0
    t = np.take_along_axis(s, np.broadcast_to(p[:, None, :], (n, C, Na)), 2)
    scale = rng.uniform(0.25, 4.0, size=(n, 1, Na))
    x = (scale * (t + 0.05 * rng.standard_normal((n, C, Na)))).astype(np.float32)
    return x, s, p


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_planted_matches_are_found_exactly(shape):
    from laenerf_amd.editing import nnfm_numpy
    x, s, p = _planted(shape, 11)
    z64, _, _, cos = nnfm_numpy(x, s)
    if shape[3] > 1:
        srt = np.sort(cos, 2)
        assert (srt[..., -1] - srt[..., -2]).min() >= 0.4          # the construction's float64 margin
    assert np.array_equal(z64, p)
    z, d, loss, dx = _run(x, s)
    assert np.array_equal(z, p)
    _check_cosine_bound(x, s, z, d)
    _check_loss_and_gradient(x, s, z, loss, dx)


@pytest.mark.parametrize("g", [1.0, 1024.0])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_random_features_meet_the_cosine_and_gradient_bounds(shape, g):
    n, C, Na, Nb = shape
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, C, Na)).astype(np.float32)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    z, d, loss, dx = _run(x, s, g=g)
    _check_cosine_bound(x, s, z, d)
    _check_loss_and_gradient(x, s, z, loss, dx, g=g)


def test_concat_arrangement_is_one_problem_over_all_layers():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, 24, 90)).astype(np.float32)
    s = rng.standard_normal((3, 24, 70)).astype(np.float32)
    z, _, loss, dx = _run(x, s, match="layer")
    from laenerf_amd.editing import nnfm_loss
    xt = T(x).requires_grad_()
    lc, zc = nnfm_loss(xt, T(s), match="concat", return_match=True)
    lc.backward()
    xc, sc = x.reshape(1, 72, 90), s.reshape(1, 72, 70)
    assert tuple(zc.shape) == (1, 90)
    _check_loss_and_gradient(xc, sc, N(zc), float(lc.detach()), N(xt.grad).reshape(1, 72, 90))
    _check_loss_and_gradient(x, s, z, loss, dx)


def test_all_cosines_negative_never_selects_a_padded_column():
    n, C, Na, Nb = 1, 40, 70, 33
    rng = np.random.default_rng(13)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    base = s[:, :, :1]                                              # every content vector opposes column 0 ...
    s = (base + 0.05 * rng.standard_normal((n, C, Nb))).astype(np.float32)   # ... and all columns are near column 0
    x = (-base + 0.05 * rng.standard_normal((n, C, Na))).astype(np.float32)
    from laenerf_amd.editing import nnfm_numpy
    assert nnfm_numpy(x, s)[3].max() < 0
    z, d, loss, dx = _run(x, s)
    assert z.max() < Nb and z.min() >= 0
    _check_cosine_bound(x, s, z, d)
    _check_loss_and_gradient(x, s, z, loss, dx)


def test_ties_go_to_the_lowest_index():
    # exact duplicate style columns in different 16-column tiles, different 64-column steps and on both sides of a 256-column chunk
    n, C, Na, Nb = 1, 64, 130, 4100
    rng = np.random.default_rng(17)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    groups = [(3, 20), (5, 70), (40, 300), (250, 260, 4099), (1000, 3000), (255, 256)]
    for grp in groups:
        for j in grp[1:]:
            s[:, :, j] = s[:, :, grp[0]]
    x = rng.standard_normal((n, C, Na)).astype(np.float32)
    for k, grp in enumerate(groups):
        for rep in range(3):
            x[:, :, 7 * k + 43 * rep] = 2.5 * s[:, :, grp[-1]]     # aimed at the LAST copy: the first must be returned
    z, d, loss, dx = _run(x, s)
    for k, grp in enumerate(groups):
        for rep in range(3):
            assert z[0, 7 * k + 43 * rep] == grp[0], (grp, z[0, 7 * k + 43 * rep])
    _check_cosine_bound(x, s, z, d)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_two_runs_give_identical_bits(shape):
    n, C, Na, Nb = shape
    rng = np.random.default_rng(23)
    x = rng.standard_normal((n, C, Na)).astype(np.float32)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    s[:, :, Nb // 2] = s[:, :, 0]
    a, b = _run(x, s), _run(x, s)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.float32(a[2]).view(np.uint32) == np.float32(b[2]).view(np.uint32)
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


def test_zero_content_position_contributes_one_and_no_gradient():
    from laenerf_amd.editing import nnfm_numpy
    n, C, Na, Nb = 2, 40, 70, 33
    rng = np.random.default_rng(29)
    x = rng.standard_normal((n, C, Na)).astype(np.float32)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    x[0, :, 5] = 0.0
    x[1, :, 69] = 0.0
    s[1, :, 4] = 0.0                                                # a zero style column is harmless too
    z, d, loss, dx = _run(x, s, g=1024.0)
    assert np.isfinite(d).all() and np.isfinite(dx).all() and np.isfinite(loss)
    assert not dx[0, :, 5].any() and not dx[1, :, 69].any()
    _check_loss_and_gradient(x, s, z, loss, dx, g=1024.0)
    # the zero positions' terms are exactly 1: removing them changes the mean accordingly
    _, loss64, _, _ = nnfm_numpy(x, s, z=z)
    keep = np.ones((n, Na), bool)
    keep[0, 5] = keep[1, 69] = False
    xn, t = x.astype(np.float64), np.take_along_axis(s.astype(np.float64), np.broadcast_to(z[:, None, :].astype(np.int64), x.shape), 2)
    cosv = (xn * t).sum(1) / ((np.sqrt((xn * xn).sum(1)) + 1e-8) * (np.sqrt((t * t).sum(1)) + 1e-8))
    assert abs(loss64 - ((1 - cosv)[keep].sum() + 2.0) / (n * Na)) <= 1e-12


def test_golden_cases_through_the_kernels():
    """The reference's own results (tests/golden/nnfm_case.npz).  The fixture's smallest float64 margin (recorded in it, about 1.1e-3) is
    below the 2^-8 that GUARANTEES the exact index, so equality with the reference's z on the rows under 2^-8 rests on the measured
    size of the fp16 error (test_random_features_* prints the worst cosine gap it sees; it is far below 1e-3), not on the bound; rows above 2^-8 are exact by the bound."""
    g = golden("nnfm_case")
    for k, shape in enumerate(GOLDEN_CASES):
        n, C, Na, _ = shape
        x, s = golden_inputs(int(g["seed"]), k, shape)
        z, d, loss, dx = _run(x, s)
        assert np.array_equal(z, g[f"z{k}"])
        _check_cosine_bound(x, s, z, d)
        _check_loss_and_gradient(x, s, z, loss, dx)
        # against the fixture itself: the kernels' bounds plus the reference's own fp32 error (1e-6 relative, as the CPU test allows it)
        assert abs(loss - float(g[f"loss{k}"])) <= (3 * C + 32) * 2.0 ** -24 + 1e-6 * abs(loss)
        ref_dx = g[f"dx{k}"].astype(np.float64)
        na = np.sqrt((x.astype(np.float64) ** 2).sum(1))
        bound = (4 * C + 16) * 2.0 ** -24 * 2.0 / ((na + 1e-8) * n * Na) + 1e-6 * np.abs(ref_dx).max()
        assert (np.abs(dx - ref_dx).max(1) <= bound).all()


def test_packed_operand_layout_and_zero_padding():
    from laenerf_amd.editing import nnfm_pack
    n, C, Nn = 2, 40, 70
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n, C, Nn)).astype(np.float32)
    garbage = torch.full((1 << 16,), float("nan"), device=DEV)     # whatever the allocator hands out next was NaN before
    del garbage
    p = N(nnfm_pack(T(x)))
    assert p.shape == (n, 128, 64)
    x64 = x.astype(np.float64)
    unit = x64 / (np.sqrt((x64 * x64).sum(1, keepdims=True) + 1e-8) + 1e-8)
    assert np.abs(p[:, :Nn, :C] - unit.transpose(0, 2, 1)).max() <= 2.0 ** -11 + 2.0 ** -20
    assert not p[:, Nn:].any() and not p[:, :, C:].any()


@settings(max_examples=50, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
@given(n=st.integers(1, 3), C=st.integers(1, 96), Na=st.integers(1, 200), Nb=st.integers(1, 200), seed=st.integers(0, 2 ** 31 - 1),
       scale=st.sampled_from([1e-3, 1.0, 50.0]))
def test_fuzz_cosine_and_gradient_bounds(n, C, Na, Nb, seed, scale):
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((n, C, Na))).astype(np.float32)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    z, d, loss, dx = _run(x, s)
    _check_cosine_bound(x, s, z, d)
    _check_loss_and_gradient(x, s, z, loss, dx)
