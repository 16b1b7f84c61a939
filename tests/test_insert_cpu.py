"""The scene insert's rule in its numpy restatements (laenerf_amd/editing/scene_insert.py; the kernels are pinned to them bit for bit
in tests/test_gpu_insert.py): the float32 and float64 restatements agree away from the decision boundaries, the composed bitfield
is a conservative superset of what the route inserts, the margin is at least what the docstring derives, and every refusal that
needs no device."""
import numpy as np
import pytest
import torch

import insert_util as IU
import region_util as U
from laenerf_amd.editing import region_transform as RT
from laenerf_amd.editing import scene_insert as SI
from laenerf_amd.editing.scene_insert import (SceneInsert, insert_blend, insert_blend_numpy, insert_occupancy, insert_occupancy_numpy,
                                              insert_route, insert_route_numpy)

F32 = np.float32
GRIDS = [(Cs, Cd) for Cs in (1, 2) for Cd in (1, 2)]


def scenes(rng, Cs, Hs, Cd, Hd):
    src_occ, sel = U.random_scene(rng, Cs, Hs)
    dst_occ, _ = U.random_scene(rng, Cd, Hd)
    return src_occ, sel, dst_occ


@pytest.mark.parametrize("Cs,Cd", GRIDS)
def test_float32_and_float64_pick_the_same_branch(Cs, Cd):
    n_ins = 0
    for seed, (Hs, Hd), scale in ((0, (16, 32), 0.5), (1, (32, 16), 1.0), (2, (32, 32), 2.0)):
        rng = np.random.default_rng(100 * Cs + 10 * Cd + seed)
        src_occ, sel, _ = scenes(rng, Cs, Hs, Cd, Hd)
        for mode in ("replace", "add"):
            ins = IU.random_insert(rng, sel, (Cs, Hs), (Cd, Hd), mode, scale=scale)
            x, d, deltas = IU.rows(rng, ins, src_occ, 20000)
            keep = IU.clear_of_boundaries(ins, x, 1e-4)
            assert keep.mean() > 0.8
            x, d, deltas = x[keep], d[keep], deltas[keep]
            a, b = insert_route_numpy(ins, x, d, src_occ, deltas, dtype=F32), insert_route_numpy(ins, x, d, src_occ, deltas, dtype=np.float64)
            assert np.array_equal(a["slot"], b["slot"]) and a["count"] == b["count"]
            assert a["xyzs_src"].dtype == F32 and b["xyzs_src"].dtype == np.float64
            assert np.abs(a["xyzs_src"] - b["xyzs_src"]).max(initial=0) < 1e-5 and np.abs(a["dirs_src"] - b["dirs_src"]).max(initial=0) < 1e-5
            n_ins += a["count"]
            sd, rd = rng.uniform(0, 40, len(x)).astype(F32), rng.random((len(x), 3)).astype(F32)
            ss, rs = rng.uniform(0, 40, a["count"]).astype(F32), rng.random((a["count"], 3)).astype(F32)
            s32, c32 = insert_blend_numpy(ins, sd, rd, ss, rs, a["slot"], dtype=F32)
            s64, c64 = insert_blend_numpy(ins, sd, rd, ss, rs, a["slot"], dtype=np.float64)
            assert s32.dtype == F32 and np.abs(s32 - s64).max() < 1e-5 * 80 and np.abs(c32 - c64).max() < 1e-5
    assert n_ins > 3000


@pytest.mark.parametrize("Cs,Cd", GRIDS)
def test_the_composed_bitfield_covers_every_inserted_row(Cs, Cd):
    """every point the float32 route inserts finds its bit in the composed field at its own destination cascade and at every
    coarser one -- the cascades the marcher may probe it at"""
    n_ins, fill = 0, []
    for seed, (Hs, Hd), scale in ((0, (16, 32), 0.5), (1, (32, 16), 1.0), (2, (16, 32), 2.0), (3, (32, 16), 2.0), (4, (32, 16), 0.5)):
        rng = np.random.default_rng(1000 * Cs + 100 * Cd + seed)
        src_occ, sel, dst_occ = scenes(rng, Cs, Hs, Cd, Hd)
        ins = IU.random_insert(rng, sel, (Cs, Hs), (Cd, Hd), scale=scale)
        assert ins.margin < 0.25 * 2.0 / Hd
        x = np.concatenate([rng.uniform(-ins.dst_bound, ins.dst_bound, (10000, 3)).astype(F32), IU.image_points(rng, ins, src_occ, 10000)])[:20000]
        r = insert_route_numpy(ins, x, np.ones_like(x), src_occ, dtype=F32)
        comp, dst_b = RT.unpack_bits(insert_occupancy_numpy(ins, dst_occ, src_occ, dtype=F32)), RT.unpack_bits(dst_occ)
        assert not (dst_b & ~comp).any()                           # no bit is ever cleared
        own = RT.cell_index_numpy(x, Cd, Hd, F32)[1]
        for level in range(Cd):
            idx = U.cell_at_level(x, level, Hd)
            assert comp[idx[r["inserted"] & (level >= own)]].all(), (seed, level, "an inserted row's cell is not in the composed bitfield")
        n_ins += r["count"]
        fill.append(float(comp.mean()))
    assert n_ins > 5000 and min(fill) < 0.3                        # and it is no bitfield of ones


def test_the_margin_is_at_least_the_derived_bound():
    rng = np.random.default_rng(7)
    for Cs, Cd in GRIDS:
        for scale in (0.5, 1.0, 2.0):
            _, sel, _ = scenes(rng, Cs, 16, Cd, 32)
            ins = IU.random_insert(rng, sel, (Cs, 16), (Cd, 32), scale=scale, shift=0.9)
            need = SI.insert_margin_needed(ins.M, ins.Minv, ins.src_bound, ins.dst_bound)
            assert ins.margin == SI.insert_margin(ins.M, ins.Minv, ins.src_bound, ins.dst_bound) >= need > 0
            # A(Minv) is taken over the DESTINATION's bound, A(M) and the cell statement over the SOURCE's
            A = lambda K, b: float((np.abs(K[:, :3].astype(np.float64)).sum(1) * b + np.abs(K[:, 3].astype(np.float64))).max())
            u = 2.0 ** -24
            assert need == pytest.approx(u * (6.02 * A(ins.M, ins.src_bound) + 17.4 * A(ins.Minv, ins.dst_bound) + 7 * ins.src_bound), rel=1e-12)
            assert ins.margin >= u * (8 * A(ins.M, ins.src_bound) + 32 * A(ins.Minv, ins.dst_bound) + 16 * ins.src_bound)
            full = lambda K: np.vstack([K.astype(np.float64), [0, 0, 0, 1]])
            assert np.abs(full(ins.M) @ full(ins.Minv) - np.eye(4)).max() < 1e-6
            assert np.abs(ins.Rt.astype(np.float64) @ ins.rotation - np.eye(3)).max() < 1e-6
            assert ins.inv_scale == float(F32(1.0 / scale))


def test_pivot_and_position_defaults():
    rng = np.random.default_rng(3)
    _, sel, _ = scenes(rng, 2, 16, 1, 32)
    ins = SceneInsert(sel, (2, 16), (1, 32))
    ref = RT.RegionTransform(sel, grid_size=16)
    assert np.array_equal(ins.pivot, ref.selection_centroid()) and np.array_equal(ins.position, ins.pivot)
    assert np.array_equal(ins.M, np.eye(3, 4, dtype=F32)) and np.array_equal(ins.Minv, np.eye(3, 4, dtype=F32))
    moved = SceneInsert(sel, (2, 16), (1, 32), position=[0.25, -0.5, 0.125], scale=2.0, rotation=U.ROT90)
    assert np.allclose(IU.forward64(moved, moved.pivot[None])[0], [0.25, -0.5, 0.125])
    assert np.abs(moved.M.astype(np.float64) @ np.append(moved.pivot, 1.0) - [0.25, -0.5, 0.125]).max() < 1e-6


def test_scene_insert_refuses_bad_arguments():
    sel = np.zeros(16 ** 3 // 8, np.uint8)
    ok = dict(src_grid=(1, 16), dst_grid=(1, 32))
    SceneInsert(sel, **ok)
    bad = [dict(ok, mode="move"), dict(ok, scale=0.49), dict(ok, scale=2.01), dict(ok, scale=float("nan")),
           dict(ok, rotation=np.diag([1.0, 1.0, -1.0])), dict(ok, rotation=2 * np.eye(3)), dict(ok, rotation=np.full((3, 3), np.nan)),
           dict(ok, pivot=[0, np.inf, 0]), dict(ok, position=[np.nan, 0, 0]),
           dict(ok, src_grid=(2, 16)), dict(ok, src_grid=(1, 32)), dict(ok, src_grid=(3, 16)), dict(ok, dst_grid=(0, 32)),
           dict(ok, dst_grid=(1, 48)), dict(ok, dst_grid=(1, 256)), dict(ok, dst_grid=(1, 2)), dict(ok, dst_grid=32),
           dict(ok, position=[3e4, 0, 0])]                       # so far out that the margin reaches a quarter of a destination cell
    for kw in bad:
        with pytest.raises(ValueError, match="SceneInsert|region transform"):
            SceneInsert(sel, **kw)
    with pytest.raises(ValueError, match="uint8"):
        SceneInsert(sel.astype(np.int32), **ok)
    with pytest.raises(ValueError, match="uint8"):
        SceneInsert(torch.zeros(16 ** 3 // 8, dtype=torch.int8), **ok)
    far = SceneInsert(sel, (1, 16), (1, 4), position=[3e3, 0, 0])         # a coarse destination grid tolerates what a fine one does not
    with pytest.raises(ValueError, match="quarter"):
        SceneInsert(sel, (1, 16), (1, 128), position=[3e3, 0, 0])
    assert far.margin < 0.5 / 4


def test_wrappers_refuse_bad_arguments_before_touching_a_device():
    sel = np.zeros(16 ** 3 // 8, np.uint8)
    ins = SceneInsert(sel, (1, 16), (1, 32))
    x = torch.zeros(8, 3)
    occ_s, occ_d = torch.zeros(16 ** 3 // 8, dtype=torch.uint8), torch.zeros(32 ** 3 // 8, dtype=torch.uint8)
    for bad in (dict(xyzs=x.double(), dirs=x), dict(xyzs=x, dirs=x[:4]), dict(xyzs=x[:, :2], dirs=x), dict(xyzs=x.t().contiguous().t(), dirs=x),
                dict(xyzs=x, dirs=x, deltas=torch.zeros(8, 3)), dict(xyzs=x, dirs=x, deltas=torch.zeros(8, 2).half()),
                dict(xyzs=x, dirs=x, src_occ=occ_d), dict(xyzs=x, dirs=x, src_occ=occ_s.float()),
                dict(xyzs=x, dirs=x, out=(torch.zeros(8, dtype=torch.int32), x, torch.zeros(8, 3), torch.zeros(1, dtype=torch.int32))),
                dict(xyzs=x, dirs=x, out=(torch.zeros(7, dtype=torch.int32), torch.zeros(8, 3), torch.zeros(8, 3), torch.zeros(1, dtype=torch.int32))),
                dict(xyzs=x, dirs=x, out=(torch.zeros(8, dtype=torch.int32), torch.zeros(8, 3), torch.zeros(8, 3)))):
        kw = dict(dict(src_occ=occ_s), **bad)
        with pytest.raises(ValueError, match="insert_route"):
            insert_route(ins, kw.pop("xyzs"), kw.pop("dirs"), kw.pop("src_occ"), **kw)
    h16 = torch.zeros(16, dtype=torch.float16)
    slot, sd, rd, ss, rs = torch.zeros(8, dtype=torch.int32), torch.zeros(8), torch.zeros(8, 3), torch.zeros(2), torch.zeros(2, 3)
    for bad in (dict(slot=slot.long()), dict(sigma_d=sd[:4]), dict(rgb_d=rd.double()), dict(sigma_s=ss[:1]), dict(rgb_s=rs.t().contiguous().t()),
                dict(out=(sd, rd[:4])), dict(out=(sd.half(), rd)), dict(out=(torch.zeros(8), rs)), dict(sigma_d=sd.half(), rgb_d=rd.half(), inplace=True),
                dict(out=(sd, rd), inplace=True), dict(sigma_d=h16[:8], out=(h16.view(torch.float32), torch.zeros(8, 3)))):      # an fp16 input under the fp32 output
        kw = dict(dict(sigma_d=sd, rgb_d=rd, sigma_s=ss, rgb_s=rs, slot=slot), **bad)
        with pytest.raises(ValueError, match="insert_blend"):
            insert_blend(ins, kw.pop("sigma_d"), kw.pop("rgb_d"), kw.pop("sigma_s"), kw.pop("rgb_s"), kw.pop("slot"), **kw)
    for bad in (dict(dst_occ=occ_s), dict(dst_occ=occ_d.float()), dict(src_occ=occ_d), dict(out=occ_d), dict(out=occ_d[:-1].clone()),
                dict(out=torch.zeros(32 ** 3 // 8))):
        kw = dict(dict(dst_occ=occ_d, src_occ=occ_s), **bad)
        with pytest.raises(ValueError, match="insert_occupancy"):
            insert_occupancy(ins, kw.pop("dst_occ"), kw.pop("src_occ"), **kw)


def test_an_empty_selection_gives_back_the_destination():
    rng = np.random.default_rng(9)
    for Cs, Cd in GRIDS:
        src_occ, _, dst_occ = scenes(rng, Cs, 16, Cd, 32)
        ins = SceneInsert(np.zeros_like(src_occ), (Cs, 16), (Cd, 32), rotation=U.rot_z(20.0), scale=1.25, position=[0.1, -0.05, 0.2])
        assert np.array_equal(ins.pivot, np.zeros(3))
        for dt in (F32, np.float64):
            assert np.array_equal(insert_occupancy_numpy(ins, dst_occ, src_occ, dtype=dt), dst_occ)
            r = insert_route_numpy(ins, rng.uniform(-1, 1, (5000, 3)).astype(F32), np.ones((5000, 3), F32), src_occ, dtype=dt)
            assert r["count"] == 0 and (r["slot"] == -1).all() and r["xyzs_src"].shape == (0, 3)


def test_a_selected_but_unoccupied_cell_inserts_nothing():
    rng = np.random.default_rng(11)
    for Cs, Cd in GRIDS:
        src_occ, sel, dst_occ = scenes(rng, Cs, 16, Cd, 32)
        sel_only = sel & ~src_occ | np.packbits(rng.random(Cs * 16 ** 3) < 0.05, bitorder="little") & ~src_occ     # selected, never occupied
        assert sel_only.any()
        ins = IU.random_insert(rng, sel_only, (Cs, 16), (Cd, 32))
        full = np.full_like(src_occ, 0xFF)
        x = np.concatenate([IU.image_points(rng, ins, full, 5000), rng.uniform(-ins.dst_bound, ins.dst_bound, (5000, 3)).astype(F32)])
        assert insert_route_numpy(ins, x, np.ones_like(x), full, dtype=F32)["count"] > 1000          # the cells are reachable ...
        r = insert_route_numpy(ins, x, np.ones_like(x), src_occ, dtype=F32)
        assert r["count"] == 0 and (r["slot"] == -1).all()                                             # ... and insert nothing
        assert np.array_equal(insert_occupancy_numpy(ins, dst_occ, src_occ, dtype=F32), dst_occ)


def test_the_blend_rule_row_by_row():
    ins = SceneInsert(np.zeros(16 ** 3 // 8, np.uint8), (1, 16), (1, 16), scale=2.0, mode="add")
    sd, rd = np.array([3.0, 0.0, 0.0, 5.0], F32), np.array([[0.2, 0.4, 0.6]] * 4, F32)
    ss, rs = np.array([2.0, 0.0, 8.0], F32), np.array([[1.0, 0.0, 0.5]] * 3, F32)
    slot = np.array([0, 1, 2, -1], np.int32)
    sigma, rgb = insert_blend_numpy(ins, sd, rd, ss, rs, slot)
    assert np.allclose(sigma, [4.0, 0.0, 4.0, 5.0])                              # densities add, the source's divided by s
    assert np.allclose(rgb[0], 0.75 * rd[0] + 0.25 * rs[0]) and np.array_equal(rgb[1], rd[1].astype(np.float64))     # 0 + 0: the destination's colour
    assert np.allclose(rgb[2], rs[2]) and np.array_equal(rgb[3], rd[3].astype(np.float64))
    sigma, rgb = insert_blend_numpy(IU.with_mode(ins, "replace"), sd, rd, ss, rs, slot)
    assert np.allclose(sigma, [1.0, 0.0, 4.0, 5.0]) and np.allclose(rgb[:3], rs) and np.allclose(rgb[3], rd[3])


def test_the_names_are_exported_and_the_entries_declared():
    import os
    import re
    from laenerf_amd import _lib, build, editing
    for name in ("SceneInsert", "render_inserted", "insert_views", "bake_insert", "insert_route", "insert_blend", "insert_occupancy",
                 "insert_route_numpy", "insert_blend_numpy", "insert_occupancy_numpy"):
        assert hasattr(editing, name), name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "laenerf.h")).read()
    for name in ("lae_insert_route", "lae_insert_blend", "lae_insert_occupancy"):
        proto = re.search(r"LAE_API\s+int\s+" + name + r"\s*\(([^;]*)\);", hdr)
        assert proto and len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    assert "insert.hip" in build.SOURCES
