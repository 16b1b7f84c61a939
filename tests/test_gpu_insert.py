"""-m gpu: the scene insert on the device (csrc/insert.hip, laenerf_amd/editing/scene_insert.py).  The three kernels equal their
numpy restatements bit for bit and give the same bytes twice; an empty selection and the identity self-insert leave the render
untouched bit for bit; an `add` insert equals the render of the analytic scene that holds both objects within the spread of two
legitimate discretisations of that scene; baking puts the object into the destination NeRF."""
import functools
import importlib

import numpy as np
import pytest
import torch

import insert_util as IU
import region_util as U
from gpu_util import DEV, N, T
from laenerf_amd.editing import region_transform as RT
from laenerf_amd.editing.scene_insert import (SceneInsert, insert_blend, insert_blend_numpy, insert_occupancy, insert_occupancy_numpy,
                                              insert_route, insert_route_numpy)

pytestmark = pytest.mark.gpu
F32 = np.float32
SCAN_WIDTH = 1024                  # workgroup counts one pass of lae_insert_route's scan takes (insert.hip IR_SCAN_THREADS) ...
TILE = 1024                        # ... each the count of this many rows (IR_TILE): more than SCAN_WIDTH * TILE rows need a second pass


def bits32(a):
    return np.ascontiguousarray(N(a) if torch.is_tensor(a) else a, dtype=F32).view(np.uint32)


def check_route(ins, src_occ, x, d, deltas):
    """the device route on rows (x, d, deltas or None) against the float32 restatement, twice -> the restatement's dict"""
    want = insert_route_numpy(ins, x, d, src_occ, deltas, dtype=F32)
    xs, ds, occ = T(x), T(d), T(src_occ)
    dl = None if deltas is None else T(deltas)
    got = insert_route(ins, xs, ds, occ, deltas=dl)
    M = len(x)
    bufs = (torch.full((M,), 7, dtype=torch.int32, device=DEV), torch.full((M, 3), 3.0, device=DEV), torch.full((M, 3), 3.0, device=DEV),
            torch.full((1,), 9, dtype=torch.int32, device=DEV))
    again = insert_route(ins, xs, ds, occ, deltas=dl, out=bufs)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(again, bufs))
    assert torch.equal(xs, T(x)) and torch.equal(ds, T(d))                    # the inputs are untouched
    for slot, xo, do, count in (got, again):
        k = int(count.item())
        assert k == want["count"] and np.array_equal(N(slot), want["slot"]), (M, k, want["count"])
        assert np.array_equal(bits32(xo[:k]), bits32(want["xyzs_src"])) and np.array_equal(bits32(do[:k]), bits32(want["dirs_src"]))
    assert torch.equal(again[1][want["count"]:], torch.full_like(again[1][want["count"]:], 3.0))      # rows beyond count are not written
    ins_rows = np.flatnonzero(want["inserted"])
    assert np.array_equal(want["slot"][ins_rows], np.arange(want["count"]))   # 0 .. count-1 in ascending row order
    return want


def check_blend(ins, rng, slot, count):
    """both modes, fp16 and fp32 inputs, rows with sigma_d = ss = 0, out of place, into buffers and in place"""
    M = len(slot)
    sd, rd = rng.uniform(0, 40, M).astype(F32), rng.random((M, 3)).astype(F32)
    ss, rs = rng.uniform(0, 40, count).astype(F32), rng.random((count, 3)).astype(F32)
    sd[1::5] = 0.0
    ss[0::3] = 0.0
    zero_zero = 0
    for mode in ("replace", "add"):
        im = IU.with_mode(ins, mode)
        for half in (False, True):
            cast = (lambda a: a.astype(np.float16)) if half else (lambda a: a)
            arrs = [cast(a) for a in (sd, rd, ss, rs)]
            want = insert_blend_numpy(im, *arrs, slot, dtype=F32)
            dev = [T(a) for a in arrs]
            st = T(slot)
            got = insert_blend(im, *dev, st)
            buf = (torch.full((M,), 5.0, device=DEV), torch.full((M, 3), 5.0, device=DEV))
            again = insert_blend(im, *dev, st, out=buf)
            assert again[0].data_ptr() == buf[0].data_ptr() and got[0].dtype == got[1].dtype == torch.float32
            outs = [got, again]
            if not half:
                outs.append(insert_blend(im, dev[0].clone(), dev[1].clone(), dev[2], dev[3], st, inplace=True))
            else:                                                         # mixed: an fp32 destination beside an fp16 source, in place
                mixed = insert_blend(im, dev[0].float(), dev[1].float(), dev[2], dev[3], st, inplace=True)
                outs.append(mixed)
            for sg, rgb in outs:
                assert np.array_equal(bits32(sg), bits32(want[0])) and np.array_equal(bits32(rgb), bits32(want[1])), (mode, half, M)
            hit = slot >= 0
            zero_zero += int(((arrs[0].astype(F32)[hit] == 0) & (arrs[2].astype(F32)[slot[hit]] == 0)).sum())
    return zero_zero


ROTS = {"general": None, "rot90": U.ROT90}
HS = [(16, 32), (32, 16), (32, 32)]


@pytest.mark.parametrize("Cs,Cd", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_kernels_equal_the_restatements_bit_for_bit(Cs, Cd):
    n_ins = n_not = zero_zero = grew = 0
    for hi, (Hs, Hd) in enumerate(HS):
        for si, scale in enumerate((0.5, 1.0, 2.0)):
            for ri, rot in enumerate(ROTS):
                rng = np.random.default_rng(10000 * Cs + 1000 * Cd + 100 * hi + 10 * si + ri)
                src_occ, sel = U.random_scene(rng, Cs, Hs)
                dst_occ, _ = U.random_scene(rng, Cd, Hd)
                ins = IU.random_insert(rng, sel, (Cs, Hs), (Cd, Hd), scale=scale, rotation=ROTS[rot])
                x, d, deltas = IU.rows(rng, ins, src_occ, 4097)
                want = check_route(ins, src_occ, x, d, deltas)
                free = check_route(ins, src_occ, x, d, None)
                assert free["count"] > want["count"] > 0                 # rows with a zero step were skipped, and only they
                assert not want["inserted"][deltas[:, 0] == 0].any()
                n_ins += want["count"]; n_not += int((~want["inserted"]).sum())
                zero_zero += check_blend(ins, rng, want["slot"], want["count"])
                comp = insert_occupancy(ins, T(dst_occ), T(src_occ))
                comp2 = insert_occupancy(ins, T(dst_occ), T(src_occ), out=torch.full_like(comp, 0xA5))
                ref = insert_occupancy_numpy(ins, dst_occ, src_occ, dtype=F32)
                assert np.array_equal(N(comp), ref) and torch.equal(comp, comp2), (Hs, Hd, scale, rot)
                grew += not np.array_equal(ref, dst_occ)
    assert n_ins > 5000 and n_not > 5000 and zero_zero > 50 and grew >= 12       # (an image may fall on cells the destination holds already)


@pytest.mark.parametrize("M", [0, 1, 1023, 70001, SCAN_WIDTH * TILE + 4099])
def test_row_counts(M):
    """no row, one row, less than a workgroup's tile, many workgroups, and more workgroups than one pass of the scan takes"""
    rng = np.random.default_rng(M % 1000)
    src_occ, sel = U.random_scene(rng, 2, 16)
    ins = IU.random_insert(rng, sel, (2, 16), (1, 32), scale=0.5, mode="add")
    x, d, deltas = IU.rows(rng, ins, src_occ, max(M, 1))
    x, d, deltas = x[:M], d[:M], deltas[:M]
    if M == 1:
        x = IU.image_points(rng, ins, src_occ, 50)[:1]; d = np.ones((1, 3), F32); deltas = np.ones((1, 2), F32)
    want = check_route(ins, src_occ, x, d, deltas)
    assert want["count"] == (1 if M == 1 else want["count"]) and (M < 1000 or want["count"] > M // 20)
    if M > SCAN_WIDTH * TILE:                                                 # (the scan is the route's alone: nothing else at this size)
        assert want["slot"][SCAN_WIDTH * TILE:].max() > want["slot"][:SCAN_WIDTH * TILE].max() >= 0     # slots on both sides of the carry
        return
    check_route(ins, src_occ, x, d, None)
    check_blend(ins, rng, want["slot"], want["count"])


def test_rows_of_zeros_and_full_selections():
    rng = np.random.default_rng(5)
    for Cs, Cd in ((1, 2), (2, 1)):
        src_occ, _ = U.random_scene(rng, Cs, 16)
        dst_occ, _ = U.random_scene(rng, Cd, 16)
        for sel, occ in ((np.full_like(src_occ, 0xFF), src_occ), (np.full_like(src_occ, 0xFF), np.full_like(src_occ, 0xFF)),
                         (np.zeros_like(src_occ), src_occ)):
            ins = SceneInsert(sel, (Cs, 16), (Cd, 16), rotation=U.rot_z(20.0), scale=1.25, pivot=[0, 0, 0], position=[0.1, -0.05, 0.2])
            x, d, deltas = IU.rows(rng, ins, occ, 2000)
            x[:500] = 0.0; d[:500] = 0.0
            want = check_route(ins, occ, x, d, None)                       # zeros are rows like any other without deltas
            deltas[:500] = 0.0
            assert not check_route(ins, occ, x, d, deltas)["inserted"][:500].any()
            assert np.isfinite(want["xyzs_src"]).all()
            got = N(insert_occupancy(ins, T(dst_occ), T(occ)))
            assert np.array_equal(got, insert_occupancy_numpy(ins, dst_occ, occ, dtype=F32))
            if not sel.any():
                assert np.array_equal(got, dst_occ) and want["count"] == 0


@pytest.mark.parametrize("Cs,Cd", [(1, 2), (2, 1), (2, 2)])
def test_the_device_bitfield_covers_the_rows_the_device_routes(Cs, Cd):
    n_ins = 0
    for seed, (Hs, Hd), scale in ((0, (16, 32), 0.5), (1, (32, 16), 2.0), (2, (32, 32), 1.0)):
        rng = np.random.default_rng(31 + 100 * Cs + 10 * Cd + seed)
        src_occ, sel = U.random_scene(rng, Cs, Hs)
        dst_occ, _ = U.random_scene(rng, Cd, Hd)
        ins = IU.random_insert(rng, sel, (Cs, Hs), (Cd, Hd), scale=scale)
        x = np.concatenate([rng.uniform(-ins.dst_bound, ins.dst_bound, (20000, 3)).astype(F32), IU.image_points(rng, ins, src_occ, 20000)])
        slot = N(insert_route(ins, T(x), T(np.ones_like(x)), T(src_occ))[0])
        comp, dst_b = RT.unpack_bits(N(insert_occupancy(ins, T(dst_occ), T(src_occ)))), RT.unpack_bits(dst_occ)
        assert not (dst_b & ~comp).any()
        own = RT.cell_index_numpy(x, Cd, Hd, F32)[1]
        for level in range(Cd):
            idx = U.cell_at_level(x, level, Hd)
            assert comp[idx[(slot >= 0) & (level >= own)]].all(), (seed, level)
        n_ins += int((slot >= 0).sum())
    assert n_ins > 10000


def test_route_and_blend_replay_from_a_graph():
    rng = np.random.default_rng(8)
    src_occ, sel = U.random_scene(rng, 2, 32)
    ins = IU.random_insert(rng, sel, (2, 32), (1, 32), scale=0.5, mode="add")
    x, d, deltas = IU.rows(rng, ins, src_occ, 4097)
    xs, ds, dl, occ = T(x), T(d), T(deltas), T(src_occ)
    eager = insert_route(ins, xs, ds, occ, deltas=dl)
    k = int(eager[3].item())
    sd, rd = torch.rand(4097, device=DEV) * 40, torch.rand(4097, 3, device=DEV)
    ss, rs = (torch.rand(4097, device=DEV) * 40).half(), torch.rand(4097, 3, device=DEV).half()      # a source array of full capacity
    eager_b = insert_blend(ins, sd, rd, ss, rs, eager[0])
    ins.sel_on(xs.device)
    bufs = (torch.empty(4097, dtype=torch.int32, device=DEV), torch.zeros(4097, 3, device=DEV), torch.zeros(4097, 3, device=DEV),
            torch.empty(1, dtype=torch.int32, device=DEV))
    bo = (torch.empty(4097, device=DEV), torch.empty(4097, 3, device=DEV))
    insert_route(ins, xs, ds, occ, deltas=dl, out=bufs); insert_blend(ins, sd, rd, ss, rs, bufs[0], out=bo)      # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        insert_route(ins, xs, ds, occ, deltas=dl, out=bufs)
        insert_blend(ins, sd, rd, ss, rs, bufs[0], out=bo)
    bufs[0].fill_(-5); bufs[1].fill_(7.0); bufs[2].fill_(7.0); bufs[3].fill_(77); bo[0].fill_(7.0); bo[1].fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert int(bufs[3].item()) == k and torch.equal(bufs[0], eager[0])
    assert np.array_equal(bits32(bufs[1][:k]), bits32(eager[1][:k])) and np.array_equal(bits32(bufs[2][:k]), bits32(eager[2][:k]))
    assert np.array_equal(bits32(bo[0]), bits32(eager_b[0])) and np.array_equal(bits32(bo[1]), bits32(eager_b[1]))


def test_the_wrappers_refuse_bad_arguments():
    rng = np.random.default_rng(2)
    src_occ, sel = U.random_scene(rng, 1, 16)
    dst_occ, _ = U.random_scene(rng, 1, 32)
    ins = IU.random_insert(rng, sel, (1, 16), (1, 32))
    x, so, do = torch.zeros(8, 3, device=DEV), T(src_occ), T(dst_occ)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    for bad in (dict(xyzs=x.double()), dict(dirs=x[:4]), dict(xyzs=x[:, :2]), dict(xyzs=x.t().contiguous().t()), dict(deltas=torch.zeros(8, 3, device=DEV)),
                dict(src_occ=do), dict(out=(i32(8), x, torch.zeros_like(x), i32(1))), dict(out=(i32(8).long(), torch.zeros_like(x), torch.zeros_like(x), i32(1)))):
        kw = dict(dict(xyzs=x, dirs=x, src_occ=so), **bad)
        with pytest.raises(ValueError, match="insert_route"):
            insert_route(ins, kw.pop("xyzs"), kw.pop("dirs"), kw.pop("src_occ"), **kw)
    sd, rd, ss, rs, slot = torch.zeros(8, device=DEV), torch.zeros(8, 3, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, 3, device=DEV), i32(8)
    for bad in (dict(sigma_d=sd.double()), dict(rgb_d=rd[:4]), dict(rgb_s=rs.t().contiguous().t()), dict(slot=slot.long()), dict(out=(sd, rs)), dict(out=(slot.view(torch.float32), torch.zeros_like(rd))),
                dict(out=(ss, torch.zeros_like(rd))), dict(out=(torch.zeros_like(sd), rd[:4])), dict(sigma_d=sd.half(), rgb_d=rd.half(), inplace=True)):
        kw = dict(dict(sigma_d=sd, rgb_d=rd, sigma_s=ss, rgb_s=rs, slot=slot), **bad)
        with pytest.raises(ValueError, match="insert_blend"):
            insert_blend(ins, kw.pop("sigma_d"), kw.pop("rgb_d"), kw.pop("sigma_s"), kw.pop("rgb_s"), kw.pop("slot"), **kw)
    for bad in (dict(dst_occ=do[:-1]), dict(dst_occ=do.float()), dict(src_occ=do), dict(out=do), dict(out=so), dict(out=do[:-1].clone())):
        kw = dict(dict(dst_occ=do, src_occ=so), **bad)
        with pytest.raises(ValueError, match="insert_occupancy"):
            insert_occupancy(ins, kw.pop("dst_occ"), kw.pop("src_occ"), **kw)
    with pytest.raises(RuntimeError):
        insert_route(ins, x.cpu(), x.cpu(), so.cpu())
    with pytest.raises(RuntimeError):
        insert_blend(ins, sd.cpu(), rd.cpu(), ss.cpu(), rs.cpu(), slot.cpu())
    with pytest.raises(RuntimeError):
        insert_occupancy(ins, do.cpu(), so.cpu())


# ---------------------------------------------------------------- renders of the analytic blobs
G, CELL, MARGIN = IU.G, IU.CELL, IU.MARGIN
A = dict(c=IU.A_C, r=IU.A_R, phase=0.3)
B = dict(c=IU.B_C, r=IU.B_R, phase=1.7)


def renderer_of(model, bits, bound=1):
    from laenerf_amd.renderer import NeRFRenderer
    r = NeRFRenderer(model, bound=bound, min_near=0.2).to(DEV)
    r.density_bitfield = T(U.pack(bits))
    r.eval()
    return r


@functools.lru_cache(None)
def camera_rays():
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    ray = get_rays(T(S.lookat_poses(2, radius=3.2, seed=6)), (89.0, 89.0, 32.0, 32.0), 64, 64)
    return ray["rays_o"].reshape(-1, 3).contiguous(), ray["rays_d"].reshape(-1, 3).contiguous()


def stacked(res):
    return torch.cat([res["image"], res["weights_sum"][:, None]], 1).double()


def render(r, dens_grid=None):
    o, d = camera_rays()
    return stacked(r.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False, dens_grid=dens_grid))


class Raises(torch.nn.Module):
    def forward(self, x, d):
        raise AssertionError("the source model must not be called")


def test_an_empty_selection_is_the_destination_bit_for_bit():
    from laenerf_amd.editing import render_inserted
    dst = renderer_of(IU.Blobs([A, B]), IU.ball_bits(IU.A_C, IU.A_R + MARGIN) | IU.ball_bits(IU.B_C, IU.B_R + MARGIN))
    src = renderer_of(Raises(), np.ones(2 * G ** 3, bool), bound=2)
    ins = SceneInsert(np.zeros(2 * G ** 3 // 8, np.uint8), (2, G), (1, G), rotation=U.rot_z(30.0), scale=0.5, position=[0.1, 0.2, 0.0])
    o, d = camera_rays()
    got = render_inserted(dst, src, ins, o, d, bg_color=1, perturb=False, want_stats=True)
    want = dst.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False, want_stats=True)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(bits32(got[k]), bits32(want[k])), k
    assert float(want["weights_sum"].max()) > 0.9
    assert got["stats"]["source_calls"] == 0 and got["stats"]["inserted_rows"] == 0
    assert {k: got["stats"][k] for k in want["stats"]} == want["stats"]
    with pytest.raises(ValueError, match="render_inserted"):                  # a grid the insert was not made for
        render_inserted(dst, dst, ins, o, d)
    with pytest.raises(ValueError, match="render_inserted"):
        render_inserted(src, src, ins, o, d)


def fused_renderer():
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(23)
    net = NeRFNetwork(bound=1, log2_hashmap_size=14).to(DEV)
    net.encoder.embeddings.data.uniform_(-0.5, 0.5)
    r = NeRFRenderer(net, bound=1, min_near=0.2).to(DEV)
    net.eval(); r.eval()
    return r


@pytest.mark.parametrize("occupancy", ["full", "tight"])
@pytest.mark.parametrize("model", ["blobs", "fused"])
def test_the_identity_self_insert_is_the_plain_render_bit_for_bit(model, occupancy):
    """every cell selected, the identity map, mode replace, the source IS the destination: every marched sample whose cell is
    occupied is routed to the same field at the same place (the identity is exact in the written statement order) and pasted over
    its own value, and every other marched sample keeps the destination's value, which is the same field's.  So the result is the
    plain render of the bitfield that was MARCHED, bit for bit.
    full   every cell occupied: the composed bitfield is the scene's own, and the result equals the plain render_eval.
    tight  the scene's analytic occupancy: an identity image box reaches into the 26 neighbours of its cell through the rounding
           margin, so the composed bitfield is the occupancy dilated by one cell, the marcher takes samples the plain render skips,
           and the field has density there (a blob's soft edge, a random network everywhere).  The result equals render_eval over
           the composed bitfield bit for bit; against the scene's own bitfield it differs, and by no more than such a dilation
           moves any render (the D0 of the equivalence tests below)."""
    from laenerf_amd.editing import render_inserted
    tight = IU.ball_bits(IU.A_C, IU.A_R + MARGIN) | IU.ball_bits(IU.B_C, IU.B_R + MARGIN)
    r = renderer_of(IU.Blobs([A, B]), tight) if model == "blobs" else fused_renderer()
    if occupancy == "full":
        r.density_bitfield = T(np.full(G ** 3 // 8, 0xFF, np.uint8))
    elif model == "fused":
        r.density_bitfield = T(U.pack(tight))
    ins = SceneInsert(np.full(G ** 3 // 8, 0xFF, np.uint8), (1, G), (1, G), pivot=[0, 0, 0])
    assert np.array_equal(ins.Minv, np.eye(3, 4, dtype=F32)) and ins.inv_scale == 1.0
    composed = insert_occupancy(ins, r.density_bitfield, r.density_bitfield)
    assert torch.equal(composed, r.density_bitfield) == (occupancy == "full")
    if occupancy == "tight":
        assert np.array_equal(N(composed), U.pack(IU.dilate(tight)))
    o, d = camera_rays()
    with torch.autocast("cuda", dtype=torch.float16, enabled=model == "fused"):
        got = render_inserted(r, r, ins, o, d, bg_color=1, perturb=False, want_stats=True)
        want = r.render_eval(o, d, bg_color=1, perturb=False, frame_loop=False, dens_grid=None if occupancy == "full" else composed)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(bits32(got[k]), bits32(want[k])), k
    assert got["stats"]["inserted_rows"] > 10000 and float(want["weights_sum"].max()) > 0          # real work, and no blank frame


# (rotation in degrees about z through the blob's centre, translation, scale): tests/test_gpu_region.py's TRANSFORMS
TRANSFORMS = {"rotate": (30.0, (0.1, 0.35, -0.2), 1.0), "shrink": (0.0, (0.1, 0.4, -0.25), 0.5), "grow": (0.0, (0.15, 0.3, -0.2), 2.0)}
# one more placement: blob A's surface meets blob B's soft edge (centres 0.2 apart, radii 0.1 and 0.12)
OVERLAP = (30.0, tuple(IU.B_C + np.array([-0.19, 0.0, 0.06]) - IU.A_C), 1.0)


def insert_scene(rot, t, s, mode):
    """the destination holds blob B at bound 1; the source holds blob A in a two-cascade scene (bound 2), inside cascade 0, whose
    cells are the destination's size"""
    dst = renderer_of(IU.Blobs([B]), IU.ball_bits(IU.B_C, IU.B_R + MARGIN))
    src_bits = IU.ball_bits(IU.A_C, IU.A_R + MARGIN, C=2)
    src = renderer_of(IU.Blobs([A]), src_bits, bound=2)
    ins = SceneInsert(U.pack(src_bits), (2, G), (1, G), rotation=U.rot_z(rot), scale=s, pivot=IU.A_C, position=IU.A_C + np.asarray(t), mode=mode)
    return dst, src, ins


def truth_and_D0(rot, t, s):
    A_T = IU.placed(A, rot, t, s)
    tight = IU.ball_bits(A_T["c"], s * (IU.A_R + MARGIN)) | IU.ball_bits(IU.B_C, IU.B_R + MARGIN)
    r_T = renderer_of(IU.Blobs([A_T, B]), tight)
    base = render(r_T)
    return base, float((base - render(r_T, T(U.pack(IU.dilate(tight))))).abs().max())


@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_an_add_insert_equals_the_scene_that_holds_both_objects(name):
    """The yardstick is built here, from paths older than the feature, exactly as the region test builds it: D0 = max
    |render_eval(truth, its tight analytic occupancy) - render_eval(truth, that occupancy dilated by one cell)| over image and
    opacity, truth = Blobs([A_T, B]): the spread between two legitimate discretisations of one scene.  The composed bitfield is
    such a dilation; its image boxes may spill one cell beyond a one-cell dilation, hence 2 D0."""
    from laenerf_amd.editing import render_inserted
    rot, t, s = TRANSFORMS[name]
    base, D0 = truth_and_D0(rot, t, s)
    dst, src, ins = insert_scene(rot, t, s, "add")
    o, d = camera_rays()
    got = stacked(render_inserted(dst, src, ins, o, d, bg_color=1, perturb=False))
    err = float((got - base).abs().max())
    alone = float((render(dst) - base).abs().max())
    print(f"insert equivalence [{name}]: D0 {D0:.3e}  |inserted (add) - truth| {err:.3e}  |destination alone - truth| {alone:.3e}")
    assert D0 > 0
    assert err <= 2 * D0
    assert alone > 10 * D0                       # power: the destination without the object is far outside the bound


def test_add_blends_an_overlap_that_replace_pastes_over():
    """the power check for the blend: where the inserted blob meets B's soft edge, the mixture stays within the yardstick and the
    paste-over (which wipes B wherever A's selection reaches) does not"""
    from laenerf_amd.editing import render_inserted
    rot, t, s = OVERLAP
    base, D0 = truth_and_D0(rot, t, s)
    o, d = camera_rays()
    err = {}
    for mode in ("add", "replace"):
        dst, src, ins = insert_scene(rot, t, s, mode)
        err[mode] = float((stacked(render_inserted(dst, src, ins, o, d, bg_color=1, perturb=False)) - base).abs().max())
    print(f"insert overlap: D0 {D0:.3e}  |add - truth| {err['add']:.3e}  |replace - truth| {err['replace']:.3e}")
    assert D0 > 0
    assert err["add"] <= 2 * D0
    assert err["replace"] > 2 * D0


def test_the_tiled_order_gives_the_untiled_result():
    from laenerf_amd.editing import render_inserted
    rot, t, s = TRANSFORMS["rotate"]
    dst, src, ins = insert_scene(rot, t, s, "add")
    o, d = camera_rays()
    plain = render_inserted(dst, src, ins, o[:4096], d[:4096], bg_color=1, perturb=False)
    tiled = render_inserted(dst, src, ins, o[:4096], d[:4096], bg_color=1, perturb=False, image_hw=(64, 64), want_stats=True)
    for k in ("image", "depth", "weights_sum"):
        assert np.array_equal(bits32(tiled[k]), bits32(plain[k])), k
    assert tiled["stats"]["inserted_rows"] > 0 and float(plain["weights_sum"].max()) > 0.9


def test_insert_views_gives_what_the_exports_take():
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import insert_views
    rot, t, s = TRANSFORMS["rotate"]
    dst, src, ins = insert_scene(rot, t, s, "add")
    poses = T(S.lookat_poses(2, radius=3.2, seed=6))
    frames, depths, opac = insert_views(dst, src, ins, poses, (89.0, 89.0, 32.0, 32.0), 64, 64)
    assert frames.shape == (2, 64, 64, 3) and frames.dtype == torch.uint8 and depths.shape == opac.shape == (2, 64 * 64)
    assert depths.dtype == opac.dtype == torch.float32 and float(opac.max()) > 0.9 and bool(torch.isfinite(depths).all())
    m = dst.extract_mesh_tsdf(poses, (89.0, 89.0, 32.0, 32.0), 64, 64, resolution=32, frames=frames, depths=depths, opacities=opac)
    assert m["vertices"].shape[0] > 0


# ---------------------------------------------------------------- baking
# two opaque blobs large enough to cover 50 pixels of a 64 x 64 view (tests/test_gpu_region.py's), one scene each; A's place in
# its own scene is clear of B's in the other (centres 1.02 apart, radii 0.22 and 0.25), so A is inserted where it stood, turned
BAKE_A = dict(c=np.array([-0.4, 0.1, -0.1]), r=0.22, phase=0.3)
BAKE_B = dict(c=np.array([0.45, -0.3, 0.3]), r=0.25, phase=1.7)


def analytic_training_views(blob, n, Hh, Ww):
    """n views of one blob as teacher_views makes them: uint8 RGBA (straight colour, alpha = opacity), poses, intrinsics"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    r = renderer_of(IU.Blobs([blob]), IU.ball_bits(blob["c"], blob["r"] + MARGIN))
    poses = S.lookat_poses(n, radius=3.2, seed=0)
    focal = 0.5 * Ww / np.tan(0.5 * 0.69)
    intr = (focal, focal, Ww / 2, Hh / 2)
    ray = get_rays(T(poses), intr, Hh, Ww)
    res = r.render_eval(ray["rays_o"].reshape(-1, 3), ray["rays_d"].reshape(-1, 3), bg_color=0, perturb=False, frame_loop=False)
    ws = res["weights_sum"].clamp(0, 1)
    rgb = torch.where(ws[:, None] > 0, res["image"] / ws.clamp(min=1e-6)[:, None], torch.zeros_like(res["image"])).clamp(0, 1)
    rgba = torch.cat([rgb, ws[:, None]], 1).reshape(n, Hh, Ww, 4)
    return (rgba * 255 + 0.5).to(torch.uint8).cpu().numpy(), poses, intr


def test_baking_puts_the_object_into_the_destination_nerf():
    from laenerf_amd import synthetic as S
    from laenerf_amd.editing import bake_insert, render_inserted
    from laenerf_amd.rays import get_rays
    tl = importlib.import_module("tools.train_loop")
    dev = torch.device(DEV)
    Hh = Ww = 64
    students = []
    for blob, seed in ((BAKE_A, 1), (BAKE_B, 0)):
        images, poses, intr = analytic_training_views(blob, 24, Hh, Ww)
        tr = tl.make_trainer(dev, images, poses, intr, iters=512, student_seed=seed)
        tr.train(512)
        students.append(tr)
    tr_src, tr_dst = students
    src, dst, data = tr_src.r, tr_dst.r, tr_dst.data
    # the selection: what the source student holds occupied around blob A
    edit = src.density_bitfield & T(U.pack(IU.ball_bits(BAKE_A["c"], BAKE_A["r"] + 6 * CELL)))
    assert int(RT.unpack_bits(N(edit)).sum()) > 500
    ins = SceneInsert(edit, (1, G), (1, G), rotation=U.rot_z(30.0), mode="add")

    def views(pose):
        ray = get_rays(T(pose[None]), intr, Hh, Ww)
        o, d = ray["rays_o"][0], ray["rays_d"][0]
        dst.eval(); src.eval()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            plain = dst.render_eval(o, d, bg_color=1.0, perturb=False, image_hw=(Hh, Ww))
            target = render_inserted(dst, src, ins, o, d, bg_color=1.0, perturb=False, image_hw=(Hh, Ww))
        dst.train(); src.train()
        return {k: (plain[k].float(), target[k].float()) for k in ("image", "weights_sum")}

    # held-out poses (another seed than the training poses'); the one whose new region is largest beside a visible B
    best = None
    for pose in S.lookat_poses(6, radius=3.2, seed=77):
        v = views(pose)
        (po, to) = v["weights_sum"]
        new_px, b_px = (to > 0.9) & (po < 0.1), po > 0.9
        score = min(int(new_px.sum()), int(b_px.sum()))
        if best is None or score > best[0]:
            best = (score, pose, v, new_px, b_px)
    score, pose, before, new_px, b_px = best
    psnr = lambda a, b: float(-10 * torch.log10(((a - b) ** 2).mean()))
    psnr_before = psnr(*before["image"])
    assert int(new_px.sum()) >= 50 and int(b_px.sum()) >= 50, (int(new_px.sum()), int(b_px.sum()))
    src_before = [p.detach().clone() for p in src.model.parameters()]
    data_new, tr2 = bake_insert(dst, tr_dst.opt, data, src, ins, steps=384, lr=1e-2)
    assert data_new is not data and data_new.images.shape == (24, Hh, Ww, 4) and np.isfinite(tr2.losses()).all()
    assert all(torch.equal(a, b) for a, b in zip(src_before, src.model.parameters()))          # the source is only read
    dst.eval()
    ray = get_rays(T(pose[None]), intr, Hh, Ww)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        after = dst.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, image_hw=(Hh, Ww))
    dst.train()
    student_img, student_op = after["image"].float(), after["weights_sum"].float()
    psnr_after = psnr(student_img, before["image"][1])
    op_new, op_b = float(student_op[new_px].mean()), float(student_op[b_px].mean())
    print(f"insert bake: held-out PSNR vs the composed render {psnr_before:.2f} -> {psnr_after:.2f} dB; student opacity where the object "
          f"went {op_new:.3f} ({int(new_px.sum())} px), where B shows {op_b:.3f} ({int(b_px.sum())} px)")
    assert psnr_after > psnr_before
    assert op_new > 0.5                          # the condition the occupancy seeding is there for
    assert op_b > 0.5
