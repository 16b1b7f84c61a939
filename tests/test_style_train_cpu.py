"""CPU: the host-side rules of the palette-network trainer (laenerf_amd.editing.style_trainer): the view schedule, the jitter's
numpy restatement, the capacity and pad-row rule, the distillation step, and the packed edit set."""
import numpy as np
import pytest
import torch

from laenerf_amd.editing import style_trainer as ST


@pytest.mark.parametrize("V", [1, 3, 15, 16, 17, 40])
def test_schedule_groups_are_prefixes_of_fresh_permutations(V):
    sched = ST.view_schedule(V, 100, seed=5)
    assert sched.dtype == np.int32 and sched.size == 112                  # whole 16-step groups
    assert ((sched >= 0) & (sched < V)).all()
    g = torch.Generator().manual_seed(5)
    for k in range(sched.size // 16):
        want = []
        while len(want) < 16:                                              # V < 16: further fresh permutations
            want.extend(torch.randperm(V, generator=g)[:16 - len(want)].tolist())
        assert sched[16 * k:16 * (k + 1)].tolist() == want
        if V >= 16:
            assert len(set(sched[16 * k:16 * (k + 1)].tolist())) == 16      # no view twice within a group
        else:
            grp = sched[16 * k:16 * (k + 1)]
            assert sorted(grp[:V].tolist()) == list(range(V))              # the group opens with a whole permutation


def test_schedule_is_deterministic_by_seed_and_prefix_stable():
    a, b = ST.view_schedule(20, 64, seed=1), ST.view_schedule(20, 64, seed=1)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, ST.view_schedule(20, 64, seed=2))
    assert np.array_equal(ST.view_schedule(20, 160, seed=1)[:64], a)       # a longer run draws the same first groups
    with pytest.raises(ValueError):
        ST.view_schedule(0, 16)


def _jitter_f32(x_term, dirs, df, u):
    """the rule spelled out: t = fp32(fp32(u - 0.5) * df), x = fp32(x_term + fp32(t * dir)) -- each operation one float32 rounding"""
    x_term, dirs = np.asarray(x_term, np.float32), np.asarray(dirs, np.float32)
    out = np.empty_like(x_term)
    for i in range(x_term.shape[0]):
        t = np.float32(np.float32(u[i]) - np.float32(0.5))
        t = np.float32(t * np.float32(df))
        for c in range(3):
            out[i, c] = np.float32(x_term[i, c] + np.float32(t * dirs[i, c]))
    return out


def test_jitter_numpy_is_the_stated_rule():
    from laenerf_amd.data import _u32
    rng = np.random.default_rng(0)
    K = 257
    x = rng.normal(size=(K, 3)).astype(np.float32)
    d = rng.normal(size=(K, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for seed, step, df in ((0, 0, 0.01), (12345678901, 77, 3.5e-3), (2 ** 64 - 1, 2 ** 32 + 5, 1.0)):
        got = ST.jitter_numpy(x, d, df, seed, step)
        w = _u32(seed, step, np.arange(K, dtype=np.uint64), 0, 2)
        u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), _jitter_f32(x, d, df, u).view(np.uint32))
        assert (np.abs(got - x) <= 0.5 * df * 1.0001 + 1e-6).all()          # |t| <= df / 2 along a unit direction


def test_jitter_extremes_of_u():
    """u = 0 gives t = -df / 2; u -> 1 (= 1 - 2^-24) gives t = (0.5 - 2^-24) * df"""
    x = np.array([[0.25, -0.5, 1.0]], np.float32)
    d = np.array([[0.6, 0.0, -0.8]], np.float32)
    df = np.float32(0.0123)
    for u in (0.0, 1.0 - 2.0 ** -24, 0.5):
        want = _jitter_f32(x, d, df, [u])
        t = np.float32(np.float32(np.float32(u) - np.float32(0.5)) * df)
        assert np.array_equal(want[0], (x[0] + (t * d[0]).astype(np.float32)).astype(np.float32))
    assert np.array_equal(_jitter_f32(x, d, df, [0.5]), x)                  # u = 1/2: no displacement


@pytest.mark.parametrize("K", [1, 15, 16, 17, 100, 128, 129, 1000, 4097, 65535, 500001])
def test_capacity_and_pad_rows(K):
    exact, bucket = ST.capacity_for(K, "exact"), ST.capacity_for(K, "bucket")
    assert exact % 16 == 0 and exact - 16 < K <= exact
    assert bucket % 16 == 0 and bucket >= exact
    if K > 128:
        assert (bucket - K) / K <= 0.125                                    # at most 12.5 % pad rows
    else:
        assert bucket == exact
    with pytest.raises(ValueError):
        ST.capacity_for(0)
    with pytest.raises(ValueError):
        ST.capacity_for(K, "other")


def test_bucket_capacities_are_few():
    caps = {ST.capacity_for(k) for k in range(200_000, 400_000, 997)}
    assert len(caps) <= 9                                                  # ~8 per octave


@pytest.mark.parametrize("iters,dps,want", [(3000, 1500, 1504), (10000, 1500, 8512), (3000, 1504, 1504), (3000, 1505, 1504),
                                            (3000, 1496, 1520), (64, 32, 48), (64, 64, 16), (64, 100, 0), (3000, 0, None),
                                            (3000, -1, None), (3000, None, None), (16, 1, None), (17, 1, None), (50, 3, 48)])
def test_distill_step(iters, dps, want):
    assert ST.distill_step(iters, dps) == want


def _views(seed=0, counts=(5, 1, 33, 16)):
    g = torch.Generator().manual_seed(seed)
    return [dict(x_term=torch.rand(k, 3, generator=g), dirs=torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=-1),
                 targets=torch.rand(k, 3, generator=g), depth_factor=torch.tensor(0.001 * (i + 1)), w8s=torch.rand(k, generator=g))
            for i, k in enumerate(counts)]


def test_edit_set_packing_and_round_trip(tmp_path):
    from laenerf_amd.editing import EditSet
    views = _views()
    es = EditSet.from_views(views, seed=9, device="cpu")
    assert es.V == 4 and es.counts_host.tolist() == [5, 1, 33, 16] and es.offsets_host.tolist() == [0, 5, 6, 39]
    assert es.x_term.shape == (55, 3) and es.x_term.dtype == torch.float32
    for v, view in enumerate(views):
        x, d, t = es.view_arrays(v)
        assert torch.equal(x, view["x_term"]) and torch.equal(d, view["dirs"]) and torch.equal(t, view["targets"])
        assert torch.equal(es.view_points(v), view["x_term"])
        assert es.depth_factor[v].item() == np.float32(view["depth_factor"].item())
    p = tmp_path / "edit_set.npz"
    es.save(p)
    back = EditSet.load(p, device="cpu")
    assert back.seed == 9 and back.counts_host.tolist() == es.counts_host.tolist()
    for name in ("x_term", "dirs", "targets", "depth_factor", "counts", "offsets"):
        assert torch.equal(getattr(back, name), getattr(es, name)), name
    es2 = EditSet.from_arrays(es.x_term.numpy(), es.dirs.numpy(), es.targets.numpy(), [5, 1, 33, 16], es.depth_factor.numpy(), device="cpu")
    assert torch.equal(es2.x_term, es.x_term)


def test_edit_set_rejects_bad_input():
    from laenerf_amd.editing import EditSet
    x = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        EditSet(x, x, x, [4, 5], [0.1, 0.1], device="cpu")                 # counts do not add up
    with pytest.raises(ValueError):
        EditSet(x, x, x, [10, 0], [0.1, 0.1], device="cpu")                # an empty view
    es = EditSet(x, x, x, [4, 6], [0.1, 0.1], device="cpu")
    with pytest.raises(ValueError):
        es.set_schedule([0, 2])
    with pytest.raises(ValueError):
        EditSet.from_views([], device="cpu")


def test_trainer_refuses_out_of_scope_terms():
    from types import SimpleNamespace
    from laenerf_amd.editing import EditSet, StyleTrainer
    es = EditSet.from_views(_views(), device="cpu")
    for name in ("style_weight", "tv_weight", "depth_disc_weight", "smooth_trans_weight", "intensity_weight", "preserve_color"):
        params = SimpleNamespace(**{name: 1})
        with pytest.raises(NotImplementedError):
            StyleTrainer(None, es, params, 100)
