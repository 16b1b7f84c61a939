"""mask_lift_numpy (the restatement of lae_mask_lift_pack / lae_mask_lift) on hand-worked cases, and the figures the GPU test
(tests/test_gpu_mask_lift.py) rests on, asserted here on the CPU for the very inputs it uses.

Hand-worked cases: ONE occupied cell and ONE view each.  G = 2, one cascade, bound 1: the cell (1, 1, 1) is Morton index 7, its
centre (0.5, 0.5, 0.5), its side 1.  The camera looks along +z from (0.5, 0.5, -1.5) unless a case moves it; 4 x 4 pixels, fx = fy
= 2, principal point (2.5, 1.5): the centre projects to u = 2.5, v = 1.5, the middle of pixel (column 2, row 1), at t_cell = 2.

The shared scene (tests/mask_lift_util.py): the exclusion cap is a condition -- at most 0.5 % of the (occupied cell, view) pairs may
have a margin below eps = 1e-4 -- and the float32 flavour of the restatement may disagree with the float64 one on no pair outside
that set.  Measured here: 0.083 % of the pairs at V = 5, 0.066 % at V = 65 (0.33 % / 0.71 % at 1e-3), no disagreement at all."""
import ctypes

import numpy as np
import pytest

import mask_lift_util as U
from laenerf_amd.editing.mask_lift import (BEHIND, IN, OCCLUDED, OUT, OUTSIDE, POSE_CHUNK, mask_iou, mask_lift_numpy,
                                           mask_lift_pack_numpy)

DTYPES = [np.float64, np.float32]
BITS = np.array([0x80], np.uint8)                      # cell 7 of the 2^3 grid
INTR = (2.0, 2.0, 2.5, 1.5)


def _pose(o=(0.5, 0.5, -1.5)):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = o
    return P


def _one(dtype, depth=1.5, opacity=1.0, mask_at=True, o=(0.5, 0.5, -1.5), **kw):
    """one view whose planes are constant except for the mask, which is set at pixel (2, 1) only (or everywhere but there)"""
    d = np.full((1, 4, 4), depth, np.float32)
    a = np.full((1, 4, 4), opacity, np.float32)
    m = np.zeros((1, 4, 4), np.uint8) if mask_at else np.ones((1, 4, 4), np.uint8)
    m[0, 1, 2] = 1 if mask_at else 0
    return mask_lift_numpy(d, a, m, _pose(o)[None], INTR, 4, 4, BITS, 1, 1.0, 2, dtype=dtype, **kw)


def _check(r, outcome, margin, votes, selected):
    assert r["cells"].tolist() == [7] and r["centres"].tolist() == [[0.5, 0.5, 0.5]]
    assert r["outcome"].tolist() == [[outcome]]
    assert r["margin"][0, 0] == margin
    assert r["votes"][7].tolist() == list(votes) and not r["votes"][:7].any()
    assert r["grid"].tolist() == [0x80 if selected else 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_cell_one_view_each_outcome(dtype):
    # visible (2 <= 1.5 + 2 * 1), mask set: in.  Margins: |q.z| = 2, half a pixel from the border, |2 - 3.5| from the depth test
    r = _one(dtype)
    _check(r, IN, 0.5, (1, 0), True)
    assert r["pixel"].tolist() == [[[2, 1]]]
    # the same pixel with the mask clear (and set everywhere else): out
    _check(_one(dtype, mask_at=False), OUT, 0.5, (0, 1), False)
    # depth_margin = 0: the surface at 1.5 hides the centre at 2; the depth test is 0.5 away, as far as the pixel border
    _check(_one(dtype, depth_margin=0.0), OCCLUDED, 0.5, (0, 0), False)
    _check(_one(dtype, depth=1.75, depth_margin=0.0), OCCLUDED, 0.25, (0, 0), False)
    # exactly at the threshold: t_cell <= t_surf + margin holds with equality, margin 0
    _check(_one(dtype, depth=2.0, depth_margin=0.0), IN, 0.0, (1, 0), True)
    # the camera in the cell's own z plane: q.z = 0 exactly, behind, margin 0
    r = _one(dtype, o=(0.5, 0.5, 0.5))
    _check(r, BEHIND, 0.0, (0, 0), False)
    assert r["pixel"].tolist() == [[[-1, -1]]]
    _check(_one(dtype, o=(0.5, 0.5, 0.75)), BEHIND, 0.25, (0, 0), False)
    # the camera 3 to the right: u = 2 * -3 / 2 + 2.5 = -0.5, half a pixel outside the frame
    _check(_one(dtype, o=(3.5, 0.5, -1.5)), OUTSIDE, 0.5, (0, 0), False)
    # u = W exactly is outside: [0, W)
    _check(_one(dtype, o=(-1.0, 0.5, -1.5)), OUTSIDE, 0.0, (0, 0), False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_transparent_pixel_and_nan_depth(dtype):
    # opacity 0.2 < 0.5: nothing in front, visible whatever the depth says; the depth test has no threshold to be near to
    r = _one(dtype, depth=0.1, opacity=0.2, depth_margin=0.0)
    _check(r, IN, 0.5, (1, 0), True)
    assert np.all(np.isinf(r["packed"])) and np.signbit(r["packed"][0, 1, 2]) and not np.signbit(r["packed"][0, 0, 0])
    _check(_one(dtype, depth=0.1, opacity=0.2, mask_at=False), OUT, 0.5, (0, 1), False)
    # opacity exactly min_opacity counts as a surface
    _check(_one(dtype, depth=0.1, opacity=0.5, depth_margin=0.0), OCCLUDED, 0.5, (0, 0), False)
    # a NaN surface never votes, whichever input it comes from, and keeps the mask's sign bit
    for kw in (dict(depth=np.nan), dict(depth=0.0, opacity=np.nan, min_opacity=0.5), dict(depth=np.inf, opacity=np.inf)):
        r = _one(dtype, **kw)
        if "opacity" in kw and np.isnan(kw["opacity"]):
            _check(r, IN, 0.5, (1, 0), True)                       # NaN >= min_opacity is false: transparent, not undefined
            continue
        _check(r, OCCLUDED, 0.5, (0, 0), False)
        assert np.all(np.isnan(r["packed"])) and np.signbit(r["packed"][0, 1, 2]) and not np.signbit(r["packed"][0, 0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sign_bit_packing(dtype):
    # t = 0 with the mask set is -0: the sign bit alone carries the mask
    p = mask_lift_pack_numpy(np.zeros(2, np.float32), np.ones(2, np.float32), np.array([1, 0], np.uint8), dtype=dtype)
    assert p.dtype == dtype and p.tolist() == [0.0, 0.0] and np.signbit(p).tolist() == [True, False]
    # and the lift reads it as a surface AT the camera, inside the mask: 2 <= 0 + 2 is visible, 2 <= 0 + 1.5 is not
    _check(_one(dtype, depth=0.0), IN, 0.0, (1, 0), True)
    _check(_one(dtype, depth=0.0, depth_margin=1.5), OCCLUDED, 0.5, (0, 0), False)
    # any nonzero byte is "set"; the quotient is one division
    d, a = np.array([0.3, 0.7, 2.0], np.float32), np.array([0.9, 0.6, 0.4], np.float32)
    p = mask_lift_pack_numpy(d, a, np.array([255, 0, 3], np.uint8), dtype=np.float32)
    assert p.view(np.uint32).tolist() == [(d[0] / a[0]).view(np.uint32) | 0x80000000, (d[1] / a[1]).view(np.uint32), 0xff800000]


@pytest.mark.parametrize("dtype", DTYPES)
def test_min_share_tie_and_min_views(dtype):
    # two views of the cell from both sides along z; the first has its mask set, the second clear: in = 1, out = 1
    d = np.full((2, 4, 4), 1.5, np.float32)
    a = np.ones((2, 4, 4), np.float32)
    m = np.zeros((2, 4, 4), np.uint8)
    m[0] = 1
    back = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)       # a half turn about y: looks along -z
    back[:3, 3] = (0.5, 0.5, 2.5)
    P = np.stack([_pose(), back])
    run = lambda **kw: mask_lift_numpy(d, a, m, P, INTR, 4, 4, BITS, 1, 1.0, 2, dtype=dtype, **kw)
    r = run()
    assert r["outcome"].tolist() == [[IN, OUT]] and r["votes"][7].tolist() == [1, 1]
    assert r["pixel"].tolist() == [[[2, 1], [2, 1]]]                # u = 2 * -0 / 2 + 2.5 from behind as well
    assert r["grid"].tolist() == [0x80]                             # 1 >= 0.5 * 2: the tie is selected
    assert run(min_share=0.51)["grid"].tolist() == [0]
    assert run(min_views=2)["grid"].tolist() == [0]
    assert run(min_share=0.0, min_views=0)["grid"].tolist() == [0x80]
    # a cell that is not occupied takes no part, wherever it projects
    r = mask_lift_numpy(d, a, m, P, INTR, 4, 4, np.array([0x01], np.uint8), 1, 1.0, 2, dtype=dtype)
    assert r["cells"].tolist() == [0] and not r["votes"][1:].any()


def test_mask_iou():
    a = np.array([[1, 1, 0, 0]], np.uint8)
    b = np.array([[0, 7, 9, 0]], np.uint8)
    assert mask_iou(a, b) == 1 / 3 and mask_iou(a, a) == 1.0 and mask_iou(a * 0, a * 0) == 1.0 and mask_iou(a, a * 0) == 0.0
    import torch
    assert mask_iou(torch.from_numpy(a), torch.from_numpy(b)) == 1 / 3


# ---------------------------------------------------------------- the shared scene
@pytest.mark.parametrize("V", U.VIEWS)
def test_scene_shows_every_outcome_and_the_transparent_branch(V):
    assert U.VIEWS[1] == POSE_CHUNK + 1
    f, r = U.fixture(V), U.restated(V)
    assert r["cells"].size == f["occ"].sum() and 0.005 < f["occ"].mean() < 0.05      # 720 of 65536 cells, both cascades
    assert set(np.unique(r["cells"] // U.G ** 3)) == {0, 1}
    counts = np.bincount(r["outcome"].reshape(-1), minlength=5)
    print("V", V, "behind / outside / occluded / in / out", counts.tolist())
    assert (counts > 0).all()
    # the close camera is the one with cells behind it and outside its frame
    assert (r["outcome"][:, 0] == BEHIND).any() and (r["outcome"][:, 0] == OUTSIDE).any()
    # the transparent branch: pairs inside the frame whose pixel has no surface; they see the cell and vote out (no mask there)
    px = r["pixel"]
    inside = px[..., 0] >= 0
    view = np.broadcast_to(np.arange(V)[None], inside.shape)
    clear = f["opacities"][view[inside], px[..., 1][inside], px[..., 0][inside]] < 0.5
    print("transparent-pixel pairs", int(clear.sum()))
    assert clear.any() and (r["outcome"][inside][clear] == OUT).all()
    # the selection is a proper part of the shell, and every parameter the GPU test varies changes it
    n_sel = {k: int(np.unpackbits(U.restated(V, **dict(kw))["grid"]).sum())
             for k, kw in (("default", ()), ("margin0", (("depth_margin", 0.0),)), ("views2", (("min_views", 2),)), ("share1", (("min_share", 1.0),)))}
    print("selected", n_sel)
    assert 0 < n_sel["margin0"] < n_sel["default"] < r["cells"].size
    assert n_sel["views2"] < n_sel["default"] and n_sel["share1"] < n_sel["default"]


@pytest.mark.parametrize("V", U.VIEWS)
def test_exclusion_cap_and_float32_agreement(V):
    r64, r32 = U.restated(V), U.restated(V, "float32")
    band = r64["margin"] < U.EPS
    differ = r64["outcome"] != r32["outcome"]
    print("V", V, "pairs", band.size, "inside the band", int(band.sum()), f"= {100 * band.mean():.3f} %", "at 1e-3:",
          f"{100 * (r64['margin'] < 1e-3).mean():.3f} %", "float32 differs on", int(differ.sum()))
    assert band.mean() <= U.EPS_CAP
    assert not (differ & ~band).any()
    whole = ~band.any(1)                                            # cells none of whose views is excluded
    assert np.array_equal(r64["votes"][r64["cells"][whole]], r32["votes"][r32["cells"][whole]])
    assert np.array_equal(np.unpackbits(r64["grid"], bitorder="little")[r64["cells"][whole]],
                          np.unpackbits(r32["grid"], bitorder="little")[r64["cells"][whole]])
    # the float32 pack plane is the float64 one rounded nowhere but in the division
    assert np.array_equal(np.signbit(r64["packed"]), np.signbit(r32["packed"]))
    assert np.array_equal(np.isinf(r64["packed"]), np.isinf(r32["packed"]))


@pytest.mark.parametrize("V", U.VIEWS)
def test_geometric_property_of_the_scene(V):
    # what tests/test_gpu_mask_lift.py asserts of the kernel's grid holds for the rule itself on this scene
    for dm in (2.0, 0.0):
        r = U.restated(V, depth_margin=dm)
        sel = np.unpackbits(r["grid"], bitorder="little").astype(bool)[r["cells"]]
        off, across = U.geometric_violations(r["cells"][sel], r["centres"][sel], dm)
        assert sel.any() and off.size == 0 and across.size == 0


# ---------------------------------------------------------------- the C ABI, without a GPU
def test_arguments_are_rejected_before_any_launch(hip_lib):
    one = ctypes.c_void_p(256)
    pack = lambda d=one, a=one, m=one, n=16, mo=0.5, p=one: hip_lib.lae_mask_lift_pack(d, a, m, n, mo, p, None)
    assert pack(d=None) == -3 and pack(a=None) == -3 and pack(m=None) == -3 and pack(p=None) == -3
    assert pack(n=0) == -1 and pack(n=2 ** 31) == -1 and pack(mo=0.0) == -1 and pack(mo=-1.0) == -1 and pack(mo=float("nan")) == -1

    def lift(packed=one, poses=one, V=3, fx=50.0, fy=50.0, H=8, W=8, bits=one, C=1, G=32, bound=1.0, dm=2.0, mv=1, ms=0.5, out=one):
        return hip_lib.lae_mask_lift(packed, poses, V, fx, fy, 4.0, 4.0, H, W, bits, C, G, bound, dm, mv, ms, out, None, None)
    assert lift(packed=None) == -3 and lift(poses=None) == -3 and lift(bits=None) == -3 and lift(out=None) == -3
    for kw in (dict(G=48), dict(G=256), dict(G=1), dict(G=0), dict(V=0), dict(V=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768),
               dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")), dict(dm=-0.5), dict(dm=float("nan")), dict(ms=-0.1), dict(ms=1.5),
               dict(ms=float("nan")), dict(C=0), dict(C=17), dict(bound=0.0)):
        assert lift(**kw) == -1, kw
