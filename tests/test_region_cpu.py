"""The region transform's rule in its numpy restatements (laenerf_amd/editing/region_transform.py; the kernels are pinned to them
bit for bit in tests/test_gpu_region.py): the composed bitfield is a conservative superset of what the warp renders, it is tight,
and rows on every boundary take the branch the rule names."""
import numpy as np
import pytest

import region_util as U
from laenerf_amd.editing import region_transform as RT
from laenerf_amd.editing.region_transform import KEPT, MOVED, VACATED, RegionTransform, region_occupancy_numpy, region_warp_numpy

F32 = np.float32
H = 32


def bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("mode", ["move", "copy", "delete"])
def test_composed_bitfield_covers_what_the_warp_renders(C, mode):
    bound = 2.0 ** (C - 1)
    n_moved = n_kept_occ = 0
    for seed in range(6):
        rng = np.random.default_rng(1000 * C + 10 * seed + len(mode))
        occ, sel = U.random_scene(rng, C, H)
        rt = U.random_transform(rng, sel, H, mode)
        assert 0.5 <= rt.scale <= 2.0 and rt.margin < 0.25 * 2.0 / H
        x = np.concatenate([rng.uniform(-bound, bound, (20000, 3)).astype(F32), U.image_points(rng, rt, 20000)])
        d = rng.standard_normal(x.shape).astype(F32)
        w = region_warp_numpy(rt, x, d, dtype=F32)
        comp = RT.unpack_bits(region_occupancy_numpy(rt, occ, dtype=F32))
        occ_b = RT.unpack_bits(occ)
        own = RT.cell_index_numpy(x, C, H, F32)[1]
        moved, kept = w["branch"] == MOVED, w["branch"] == KEPT
        assert (mode == "delete") == (not moved.any()), (seed, "the draw must exercise the moved branch")
        assert mode == "copy" or (w["branch"] == VACATED).any()
        for level in range(C):
            at = level >= own                                  # the cascades the marcher may probe x at
            idx = U.cell_at_level(x, level, H)
            assert comp[idx[moved & at]].all(), (seed, level, "a moved row's cell is not in the composed bitfield")
            had = kept & at & occ_b[idx]
            assert comp[idx[had]].all(), (seed, level, "a kept row lost its occupancy bit")
            n_kept_occ += int(had.sum())
        n_moved += int(moved.sum())
    assert n_kept_occ > 1000 and (mode == "delete" or n_moved > 1000)


def test_delete_is_occ_without_the_selection_exactly():
    for seed in range(3):
        rng = np.random.default_rng(seed)
        occ, sel = U.random_scene(rng, 1, H)
        rt = U.random_transform(rng, sel, H, "delete")
        assert np.array_equal(region_occupancy_numpy(rt, occ, dtype=F32), occ & ~sel)
        w = region_warp_numpy(rt, rng.uniform(-1, 1, (5000, 3)).astype(F32), np.ones((5000, 3), F32), dtype=F32)
        assert not (w["branch"] == MOVED).any() and set(np.unique(w["sigma_scale"])) <= {0.0, 1.0}


def test_cascade_one_keeps_the_inner_half_of_its_grid():
    """the keep part clears own-cascade cells only: a selected bit of cascade 1 inside the half cascade 0 covers stays"""
    rng = np.random.default_rng(5)
    occ, sel = U.random_scene(rng, 2, H)
    rt = U.random_transform(rng, sel, H, "delete")
    comp, own = RT.unpack_bits(region_occupancy_numpy(rt, occ, dtype=F32)), RT.own_cell_mask(2, H)
    occ_b, sel_b = RT.unpack_bits(occ), RT.unpack_bits(sel)
    assert (sel_b & ~own).any() and (sel_b & own)[H ** 3:].any()
    assert np.array_equal(comp, occ_b & ~(sel_b & own))


def dense(bits):
    g = np.zeros((H, H, H), bool)
    c = U.coords(H)
    g[c[:, 0], c[:, 1], c[:, 2]] = bits
    return g


@pytest.mark.parametrize("mode", ["move", "copy"])
def test_a_whole_cell_translation_stays_within_one_cell_of_the_shifted_selection(mode):
    """margin < 1 cell: the image of a cell shifted by whole cells touches the target cell and, through the margin, its
    neighbours -- never a cell two away.  An all-ones bitfield cannot pass."""
    for seed, k in ((0, (3, -2, 5)), (1, (-4, 0, 1)), (2, (0, 0, 0))):
        rng = np.random.default_rng(seed)
        occ, sel = U.random_scene(rng, 1, H)
        rt = RegionTransform(sel, translation=np.array(k) * (2.0 / H), mode=mode, grid_size=H)
        comp = dense(RT.unpack_bits(region_occupancy_numpy(rt, occ, dtype=F32)))
        src = dense(RT.unpack_bits(occ & sel))
        shifted = np.zeros_like(src)
        i, j, l = np.nonzero(src)
        i, j, l = i + k[0], j + k[1], l + k[2]
        ok = (i >= 0) & (i < H) & (j >= 0) & (j < H) & (l >= 0) & (l < H)
        shifted[i[ok], j[ok], l[ok]] = True
        dil = np.zeros_like(shifted)
        pad = np.pad(shifted, 1)
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    dil |= pad[a:a + H, b:b + H, c:c + H]
        keep = dense(RT.unpack_bits(occ if mode == "copy" else occ & ~sel))
        assert not (comp & ~(dil | keep)).any()
        assert (shifted & ~comp).sum() == 0 and (keep & ~comp).sum() == 0
        assert comp.sum() < 0.5 * H ** 3


def test_identity_in_copy_mode_returns_the_rows_bit_for_bit():
    rng = np.random.default_rng(3)
    for C in (1, 2):
        occ, sel = U.random_scene(rng, C, H)
        rt = RegionTransform(sel, mode="copy", grid_size=H)
        x = rng.uniform(-rt.bound, rt.bound, (30000, 3)).astype(F32)
        d = rng.standard_normal(x.shape).astype(F32)
        w = region_warp_numpy(rt, x, d, dtype=F32)
        assert (w["branch"] == MOVED).any() and (w["branch"] == KEPT).any()
        assert np.array_equal(bits32(w["xyzs"]), bits32(x)) and np.array_equal(bits32(w["dirs"]), bits32(d))
        assert (w["sigma_scale"] == 1.0).all()


@pytest.mark.parametrize("scale", [0.5, 0.7, 1.0, 1.3, 2.0])
def test_a_moved_row_carries_the_rounded_reciprocal_of_the_scale(scale):
    rng = np.random.default_rng(7)
    occ, sel = U.random_scene(rng, 1, H)
    rt = U.random_transform(rng, sel, H, "move", scale=scale, shift=0.1)
    x = U.image_points(rng, rt, 4000)
    w = region_warp_numpy(rt, x, np.ones_like(x), dtype=F32)
    moved = w["branch"] == MOVED
    assert moved.sum() > 1000
    assert (bits32(w["sigma_scale"][moved]) == bits32(F32(1.0 / scale))).all()
    assert set(np.unique(w["sigma_scale"][~moved])) <= {0.0, 1.0}


def test_the_transform_refuses_what_the_rule_does_not_cover():
    sel = np.zeros(H ** 3 // 8, np.uint8)
    for bad in (dict(scale=0.49), dict(scale=2.01), dict(scale=float("nan")), dict(mode="shear"), dict(rotation=np.diag([1.0, 1.0, -1.0])),
                dict(rotation=2 * np.eye(3)), dict(translation=[0.0, np.inf, 0.0]), dict(grid_size=48), dict(bound=2.0),
                dict(translation=[1e4, 0.0, 0.0])):
        with pytest.raises(ValueError):
            RegionTransform(sel, **{"grid_size": H, **bad})
    rt = RegionTransform(sel, grid_size=H)
    assert rt.cascade == 1 and rt.bound == 1.0 and np.array_equal(rt.M, np.eye(3, 4, dtype=F32)) and np.array_equal(rt.pivot, np.zeros(3))
    assert 0 < rt.margin < 0.01 * 2.0 / H                           # a small fraction of a cell


def test_the_inverse_is_formed_in_float64_and_rounded_once():
    rng = np.random.default_rng(11)
    occ, sel = U.random_scene(rng, 1, H)
    rt = U.random_transform(rng, sel, H, "move")
    F = np.concatenate([rt.scale * rt.rotation, (rt.pivot + rt.translation - rt.scale * rt.rotation @ rt.pivot)[:, None]], 1)
    G = np.linalg.inv(np.concatenate([F, [[0, 0, 0, 1]]]))[:3]
    assert np.abs(rt.Minv.astype(np.float64) - G).max() <= 2.0 ** -24 * np.abs(G).max() * 1.01
    assert np.array_equal(rt.M, F.astype(F32)) and np.array_equal(rt.Rt, rt.rotation.T.astype(F32))
    cells = np.flatnonzero(RT.unpack_bits(sel))
    assert np.allclose(rt.pivot, U.centres(1, H)[0][cells].mean(0))


# ---- ambiguous rows: one selected cell, points exactly on its faces, on the box and just outside it
def one_cell(C, cascade, n):
    bits = np.zeros((C, H ** 3), bool)
    bits[cascade, RT.morton_numpy(np.array([n[0]]), np.array([n[1]]), np.array([n[2]]))[0]] = True
    return U.pack(bits)


def branch_of(rt, pts):
    pts = np.asarray(pts, F32).reshape(-1, 3)
    return list(region_warp_numpy(rt, pts, np.ones_like(pts), dtype=F32)["branch"])


def test_points_on_cell_faces_belong_to_the_cell_above():
    n = (10, 11, 12)
    rt = RegionTransform(one_cell(1, 0, n), translation=[0.25, 0.0, 0.0], grid_size=H)
    lo = [F32(2.0 * k / H - 1.0) for k in n]
    hi = [F32(2.0 * (k + 1) / H - 1.0) for k in n]
    # "just under" a face is 4 ulps under it: the coordinate statement adds 1 to q / mip_bound, and that one rounding may lift a
    # point closer than that onto the face (the (c) term of the margin's derivation)
    below = [v - 4 * np.abs(np.spacing(v)) for v in lo]
    under_hi = [v - 4 * np.abs(np.spacing(v)) for v in hi]
    assert branch_of(rt, [lo, under_hi, [hi[0], lo[1], lo[2]], [lo[0], hi[1], lo[2]], [below[0], lo[1], lo[2]], [lo[0], lo[1], below[2]]]) == \
        [VACATED, VACATED, KEPT, KEPT, KEPT, KEPT]
    # the same faces seen through the inverse map: x = p + t with t = 0.25 exact
    t = F32(0.25)
    assert branch_of(rt, [[lo[0] + t, lo[1], lo[2]], [under_hi[0] + t, under_hi[1], under_hi[2]], [hi[0] + t, lo[1], lo[2]],
                          [below[0] + t, lo[1], lo[2]]]) == [MOVED, MOVED, KEPT, KEPT]
    assert branch_of(RegionTransform(one_cell(1, 0, n), translation=[0.25, 0.0, 0.0], grid_size=H, mode="copy"), [lo, [lo[0] + t, lo[1], lo[2]]]) == \
        [KEPT, MOVED]


def test_points_on_the_box_and_just_outside():
    top = one_cell(1, 0, (H - 1, 5, 5))
    y = F32(2.0 * 5.5 / H - 1.0)
    one, over = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    rt = RegionTransform(top, translation=[-0.5, 0.0, 0.0], grid_size=H)
    # sel(x) clamps like the marcher: on the bound and just beyond it the last cell answers
    assert branch_of(rt, [[one, y, y], [over, y, y], [-one, y, y]]) == [VACATED, VACATED, KEPT]
    # p = x + 0.5 as the kernel rounds it: exactly on the bound is inside the box (moved), two ulps of 1 further is outside (never
    # moved, whatever cell a clamp would hit)
    half, over_half = F32(0.5), F32(0.5) + 4 * np.spacing(F32(0.5))
    assert branch_of(rt, [[half, y, y], [over_half, y, y]]) == [MOVED, KEPT]
    bottom = RegionTransform(one_cell(1, 0, (0, 5, 5)), translation=[0.25, 0.0, 0.0], grid_size=H)
    assert branch_of(bottom, [[F32(-0.75), y, y], [F32(-0.75) - 4 * np.spacing(F32(0.75)), y, y]]) == [MOVED, KEPT]


def test_a_coordinate_of_exactly_minus_one_looks_up_cascade_one():
    """|q| = 1 has level 1 and lands on the first cell layer of cascade 1's inner half: the keep part does not clear that cell (it
    is not of its own cascade), the warp still vacates the row, and the image part takes the cell as a source"""
    q = H // 4
    sel = one_cell(2, 1, (q, q + 3, q + 3))
    y = F32((2.0 * (q + 3.5) / H - 1.0) * 2.0)
    assert RT.cell_index_numpy(np.array([[-1.0, y, y]], F32), 2, H)[0][0] == np.flatnonzero(RT.unpack_bits(sel))[0]
    rt = RegionTransform(sel, translation=[0.0, 0.5, 0.0], grid_size=H)
    assert branch_of(rt, [[-1.0, y, y], [np.nextafter(F32(-1.0), F32(0.0)), y, y], [-1.0, y + F32(0.5), y]]) == [VACATED, KEPT, MOVED]
    comp = RT.unpack_bits(region_occupancy_numpy(rt, sel, dtype=F32))
    assert comp[np.flatnonzero(RT.unpack_bits(sel))[0]]                                  # not cleared
    x = np.array([[-1.0, y + F32(0.5), y]], F32)
    assert comp[U.cell_at_level(x, 1, H)[0]]                                             # its image is covered


def test_float64_and_float32_restatements_agree_away_from_boundaries():
    rng = np.random.default_rng(13)
    occ, sel = U.random_scene(rng, 2, H)
    rt = U.random_transform(rng, sel, H, "move")
    x = np.concatenate([rng.uniform(-2, 2, (5000, 3)).astype(F32), U.image_points(rng, rt, 5000)])
    a, b = region_warp_numpy(rt, x, np.ones_like(x), dtype=F32), region_warp_numpy(rt, x, np.ones_like(x))
    same = a["branch"] == b["branch"]
    assert same.mean() > 0.995
    assert np.abs(a["xyzs"][same] - b["xyzs"][same]).max() < 1e-5
    c32, c64 = (RT.unpack_bits(region_occupancy_numpy(rt, occ, dtype=dt)) for dt in (F32, np.float64))
    assert (c32 != c64).mean() < 1e-4


def test_invalid_arguments_return_einval_before_any_launch(hip_lib):
    """no device memory is touched: every pointer here is a host address or a made-up one"""
    import ctypes
    EINVAL = -1
    one = ctypes.c_void_p(64)
    m12, r9 = (ctypes.c_float * 12)(*np.eye(3, 4).reshape(-1)), (ctypes.c_float * 9)(*np.eye(3).reshape(-1))
    nbytes = 128 ** 3 // 8
    warp = dict(xyzs=one, dirs=one, M=8, sel=one, sel_bytes=nbytes, Minv=m12, Rt=r9, inv_scale=1.0, mode=0, bound=1.0, C=1, H=128,
                xyzs_out=one, dirs_out=one, sigma_scale=one, stream=None)
    occ = dict(occ=one, sel=ctypes.c_void_p(128), bytes=nbytes, M=m12, margin=1e-5, mode=0, bound=1.0, C=1, H=128, out=ctypes.c_void_p(256),
               stream=None)
    call = lambda fn, base, **kw: fn(*{**base, **kw}.values())
    assert call(hip_lib.lae_region_warp, warp, M=0) == 0                          # nothing wrong, no rows: OK without a launch
    bad_nan = (ctypes.c_float * 12)(*([float("nan")] + [0.0] * 11))
    for kw in (dict(xyzs=None), dict(dirs=None), dict(sel=None), dict(Minv=None), dict(Rt=None), dict(xyzs_out=None), dict(dirs_out=None),
               dict(sigma_scale=None), dict(inv_scale=0.49), dict(inv_scale=2.01), dict(inv_scale=float("nan")), dict(mode=3), dict(mode=-1),
               dict(C=2), dict(C=0), dict(C=9), dict(H=64), dict(H=96), dict(sel_bytes=nbytes - 1), dict(bound=2.0), dict(bound=1.5),
               dict(Minv=bad_nan), dict(xyzs=ctypes.c_void_p(66))):
        assert call(hip_lib.lae_region_warp, warp, **kw) == EINVAL, kw
        assert call(hip_lib.lae_region_warp, warp, M=0, **kw) == EINVAL, kw       # checked before the row count is looked at
    for kw in (dict(occ=None), dict(sel=None), dict(out=None), dict(M=None), dict(mode=3), dict(C=2), dict(H=64), dict(bytes=nbytes + 8),
               dict(bound=2.0), dict(margin=-1e-6), dict(margin=0.5 / 128), dict(margin=float("nan")), dict(M=bad_nan),
               dict(out=one), dict(out=ctypes.c_void_p(128)), dict(occ=ctypes.c_void_p(66))):
        assert call(hip_lib.lae_region_occupancy, occ, **kw) == EINVAL, kw
    assert call(hip_lib.lae_region_occupancy, dict(occ, mode=3), M=None) == EINVAL
    # three cascades are refused although bound and bytes fit them: the image part's box walk is unmeasured there
    assert call(hip_lib.lae_region_warp, warp, M=0, C=3, bound=4.0, sel_bytes=3 * nbytes) == EINVAL
    assert call(hip_lib.lae_region_occupancy, occ, C=3, bound=4.0, bytes=3 * nbytes) == EINVAL
    # a grid that fits: cascade 2 needs bound 2 and twice the bytes
    assert call(hip_lib.lae_region_warp, warp, M=0, C=2, bound=2.0, sel_bytes=2 * nbytes) == 0
