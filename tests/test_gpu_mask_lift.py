"""lae_mask_lift_pack / lae_mask_lift (through editing.mask_lift_pack / lift_masks) against the restatement
editing.mask_lift_numpy on the scene of tests/mask_lift_util.py, and EditGrid.new_from_masks / selection_masks on a small
randomly initialised renderer.

What is compared, and how closely (tests/test_mask_lift_cpu.py asserts the figures on the CPU, for these very inputs):
  pack    bit for bit against the float32 flavour of the restatement: one division, one compare, one sign bit.
  votes   integers.  A (cell, view) pair is compared with the float64 restatement wherever its margin -- the distance of its nearest
          decision from the threshold -- is at least eps = 1e-4; the pairs inside that band may be at most 0.5 % of all (measured:
          0.083 % at V = 5, 0.066 % at V = 65).  eps is over ten times the float32 error of a pixel coordinate (56 * 2^-23 * a few
          operations, under 1e-5 px) or of a distance (4 * 2^-23): an exclusion band, not a tolerance.  The kernel has no per-pair
          output; a pair is read off a launch with that one view.  Per cell the (in, out) counts and the bit are compared wherever
          none of the cell's views is inside the band.
  scene   a property that needs no restatement: every selected cell lies within (depth_margin + 1) sides of the sphere and on the
          masked side of the cap's plane, within one side."""
import numpy as np
import pytest
import torch

import mask_lift_util as U
from gpu_util import DEV, N
from gpu_util import T as _T
from laenerf_amd.editing.mask_lift import IN, OUT

pytestmark = pytest.mark.gpu

N_CELLS = U.C * U.G ** 3


def T(a):
    return _T(np.array(a))                                           # the fixtures are read-only: hand torch a copy


@pytest.fixture(scope="module")
def packed():
    """V -> the packed planes [V, H, W] on the device, packed view by view"""
    from laenerf_amd.editing import mask_lift_pack
    out = {}
    for V in U.VIEWS:
        f = U.fixture(V)
        d, a, m = T(f["depths"]), T(f["opacities"]), T(f["masks"])
        p = torch.full((V, U.H, U.W), 7.0, device=DEV)
        for v in range(V):
            mask_lift_pack(d[v], a[v], m[v], out=p[v])
        out[V] = p
    return out


def _lift(packed, V, views=None, **kw):
    """-> (grid uint8 [N_CELLS / 8], votes uint16 [N_CELLS, 2]) as numpy; views: a slice of the fixture's views"""
    from laenerf_amd.editing import lift_masks
    f = U.fixture(V)
    sl = slice(None) if views is None else views
    g, c = lift_masks(packed[V][sl].contiguous(), T(f["poses"])[sl].contiguous(), U.INTRINSICS, U.H, U.W, T(f["bits"]), U.C, U.BOUND,
                      grid_size=U.G, votes=True, **kw)
    return N(g), N(c)


def _bits(grid):
    return np.unpackbits(grid, bitorder="little").astype(bool)


@pytest.mark.parametrize("V", U.VIEWS)
def test_pack_is_bit_exact(packed, V):
    want = U.restated(V, "float32")["packed"]
    got = N(packed[V])
    assert want.dtype == np.float32 and got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert np.isinf(got).any() and np.signbit(got).any() and (got > 0).any()


def test_pack_special_values():
    from laenerf_amd.editing import mask_lift_pack, mask_lift_pack_numpy
    nan, inf = np.nan, np.inf
    d = np.array([0.0, 0.0, 1.0, 1.0, nan, nan, 3.0, 3.0, 0.3, 0.3, inf, 2.0, 1e-30, 5.0, 0.1], np.float32)
    a = np.array([1.0, 1.0, 0.5, 0.49999997, 1.0, 1.0, nan, 0.0, 0.9, 0.7, inf, inf, 1e30, 0.75, 0.25], np.float32)
    m = np.array([1, 0, 1, 1, 1, 0, 1, 0, 255, 0, 1, 1, 0, 2, 0], np.uint8)
    for mo in (0.5, 0.25):
        got = N(mask_lift_pack(T(d), T(a), T(m), min_opacity=mo))
        want = mask_lift_pack_numpy(d, a, m, mo, np.float32)
        # a NaN's payload is the divider's business: its place and its sign bit are compared, every other value bit for bit
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.signbit(got), np.signbit(want))
        ok = ~np.isnan(want)
        assert got.view(np.uint32)[ok].tobytes() == want.view(np.uint32)[ok].tobytes()
    assert np.signbit(got[0]) and got[0] == 0 and not np.signbit(got[1])            # t = 0 with the mask set is -0


@pytest.mark.parametrize("V", U.VIEWS)
def test_votes_and_grid_against_float64(packed, V):
    f, r = U.fixture(V), U.restated(V)
    cells, occ = r["cells"], f["occ"]
    band = r["margin"] < U.EPS
    print("V", V, "pairs", band.size, "inside the band", int(band.sum()), f"= {100 * band.mean():.3f} %")
    assert band.mean() <= U.EPS_CAP
    grid, votes = _lift(packed, V)
    # cells that are not occupied: zero votes, bit clear, wherever they project
    assert not votes[~occ].any() and not _bits(grid)[~occ].any()
    # pair by pair: one launch per view
    total = np.zeros((N_CELLS, 2), np.int64)
    wrong = 0
    for v in range(V):
        g1, v1 = _lift(packed, V, views=slice(v, v + 1))
        assert not v1[~occ].any() and v1.sum(1).max() <= 1
        total += v1
        want = np.stack([r["outcome"][:, v] == IN, r["outcome"][:, v] == OUT], -1)
        keep = ~band[:, v]
        wrong += int((v1[cells][keep] != want[keep]).any(1).sum())
    assert wrong == 0
    assert np.array_equal(total, votes)                              # the chunked, sliced sum is the sum of its views
    whole = ~band.any(1)
    print("cells", cells.size, "without an excluded view", int(whole.sum()), "selected", int(_bits(grid).sum()),
          "restated", int(_bits(r["grid"]).sum()))
    assert np.array_equal(votes[cells[whole]], r["votes"][cells[whole]])
    assert np.array_equal(_bits(grid)[cells[whole]], _bits(r["grid"])[cells[whole]])
    assert votes.sum(1).max() <= V and _bits(grid).any()
    # the decision is the rule applied to the kernel's own votes, on every cell
    n_in, n_all = votes[:, 0].astype(np.float32), votes.sum(1).astype(np.float32)
    assert np.array_equal(_bits(grid), occ & (votes[:, 0] >= 1) & (n_in >= np.float32(0.5) * n_all))


@pytest.mark.parametrize("V", U.VIEWS)
@pytest.mark.parametrize("kw", [dict(min_views=2), dict(min_share=1.0), dict(depth_margin=0.0)], ids=lambda k: next(iter(k)))
def test_parameters_give_the_restated_grid(packed, V, kw):
    r = U.restated(V, **kw)
    band = r["margin"] < U.EPS
    assert band.mean() <= U.EPS_CAP
    whole = ~band.any(1)
    grid, votes = _lift(packed, V, **kw)
    cells = r["cells"]
    assert np.array_equal(votes[cells[whole]], r["votes"][cells[whole]])
    assert np.array_equal(_bits(grid)[cells[whole]], _bits(r["grid"])[cells[whole]])
    base = _bits(_lift(packed, V)[0])
    assert _bits(grid).any() and (_bits(grid) != base).any()
    if "depth_margin" not in kw:                                     # a stricter vote only removes cells (a thinner shell loses out votes too)
        assert not (_bits(grid) & ~base).any()


@pytest.mark.parametrize("V", U.VIEWS)
@pytest.mark.parametrize("depth_margin", [2.0, 0.0])
def test_selected_cells_lie_on_the_masked_cap(packed, V, depth_margin):
    from laenerf_amd.editing.mask_lift import _compact_bits
    grid, _ = _lift(packed, V, depth_margin=depth_margin)
    cells = np.flatnonzero(_bits(grid))
    m = (cells % U.G ** 3).astype(np.uint32)
    coord = np.stack([_compact_bits(m), _compact_bits(m >> 1), _compact_bits(m >> 2)], -1).astype(np.float64)
    centres = (((coord + 0.5) / U.G) * 2 - 1) * np.minimum(2.0 ** (cells // U.G ** 3), U.BOUND)[:, None]
    off, across = U.geometric_violations(cells, centres, depth_margin)
    print("selected", cells.size, "off the surface", off.size, "across the cap's plane", across.size)
    assert cells.size > 0 and off.size == 0 and across.size == 0


@pytest.mark.parametrize("V", U.VIEWS)
def test_two_calls_prefilled_outputs_and_a_graph_replay(packed, V):
    from laenerf_amd.editing import lift_masks
    f = U.fixture(V)
    first, again = _lift(packed, V), _lift(packed, V)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    poses, bits = T(f["poses"]), T(f["bits"])
    out = torch.full((N_CELLS // 8,), 0xFF, dtype=torch.uint8, device=DEV)
    args = (packed[V], poses, U.INTRINSICS, U.H, U.W, bits, U.C, U.BOUND)
    assert lift_masks(*args, grid_size=U.G, out=out) is out
    assert N(out).tobytes() == first[0].tobytes()                    # every byte rewritten: no zero fill needed
    # captured and replayed twice
    out.fill_(0xFF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lift_masks(*args, grid_size=U.G, out=out)                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lift_masks(*args, grid_size=U.G, out=out)
    for _ in range(2):
        out.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert N(out).tobytes() == first[0].tobytes()


def test_invalid_arguments_leave_the_outputs_untouched(packed):
    from laenerf_amd import _lib
    from laenerf_amd.editing import lift_masks, mask_lift_pack
    V = U.VIEWS[0]
    f = U.fixture(V)
    lib = _lib.load()
    poses, bits = T(f["poses"]), T(f["bits"])
    grid = torch.full((N_CELLS // 8,), 0xA5, dtype=torch.uint8, device=DEV)
    votes = torch.full((N_CELLS, 2), 0x7777, dtype=torch.uint16, device=DEV)
    plane = torch.full((U.H * U.W,), 7.0, device=DEV)
    fx, fy, cx, cy = U.INTRINSICS

    def lift(p=packed[V].data_ptr(), po=poses.data_ptr(), v=V, fx=fx, fy=fy, h=U.H, w=U.W, b=bits.data_ptr(), c=U.C, g=U.G, dm=2.0, ms=0.5,
             out=grid.data_ptr()):
        return lib.lae_mask_lift(p, po, v, fx, fy, cx, cy, h, w, b, c, g, U.BOUND, dm, 1, ms, out, votes.data_ptr(), None)
    assert lift(p=None) == -3 and lift(po=None) == -3 and lift(b=None) == -3 and lift(out=None) == -3
    for kw in (dict(g=24), dict(g=256), dict(v=0), dict(v=65536), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15), dict(fx=0.0), dict(fy=-2.0),
               dict(dm=-1.0), dict(ms=1.25), dict(ms=-0.25)):
        assert lift(**kw) == -1, kw
    d, a, m = T(f["depths"][0]), T(f["opacities"][0]), T(f["masks"][0])
    pack = lambda dp=d.data_ptr(), n=U.H * U.W, mo=0.5, pp=plane.data_ptr(): lib.lae_mask_lift_pack(dp, a.data_ptr(), m.data_ptr(), n, mo, pp, None)
    assert pack(dp=None) == -3 and pack(pp=None) == -3 and pack(n=0) == -1 and pack(mo=0.0) == -1 and pack(mo=-0.5) == -1
    torch.cuda.synchronize()
    assert (N(grid) == 0xA5).all() and (N(votes) == 0x7777).all() and (N(plane) == 7.0).all()
    # and the Python operators refuse what the entry points would misread
    with pytest.raises(ValueError):
        lift_masks(packed[V].double(), poses, U.INTRINSICS, U.H, U.W, bits, U.C, U.BOUND, grid_size=U.G)
    with pytest.raises(ValueError):
        lift_masks(packed[V], poses[:-1].contiguous(), U.INTRINSICS, U.H, U.W, bits, U.C, U.BOUND, grid_size=U.G)
    with pytest.raises(ValueError):
        lift_masks(packed[V], poses, U.INTRINSICS, U.H, U.W, bits[:-1].contiguous(), U.C, U.BOUND, grid_size=U.G)
    with pytest.raises(ValueError):
        lift_masks(packed[V], poses, U.INTRINSICS, U.H, U.W, bits, U.C, U.BOUND, grid_size=48)
    with pytest.raises(ValueError):
        mask_lift_pack(d, a, m.float())
    with pytest.raises(RuntimeError):
        lift_masks(packed[V].cpu(), poses, U.INTRINSICS, U.H, U.W, bits, U.C, U.BOUND, grid_size=U.G)
    assert lift() == 0                                               # the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert not (N(grid) == 0xA5).all()


# ---------------------------------------------------------------- EditGrid.new_from_masks / selection_masks on a renderer
HW_R = 32
INTR_R = (44.0, 44.0, 15.5, 16.25)


@pytest.fixture(scope="module")
def rendered():
    """a small randomly initialised renderer with the sphere preset as its occupancy, three views of it rendered as
    new_from_masks renders them, and masks painted from a 3D region: the x > 0 half of what the views see"""
    from laenerf_amd import synthetic as S
    from laenerf_amd.rays import get_rays
    from test_gpu_frame import make
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0                                           # opaque surfaces
    poses = T(S.lookat_poses(3, radius=3.2, seed=4))
    views = []
    with torch.no_grad():
        for i in range(3):
            ray = get_rays(poses[i:i + 1], INTR_R, HW_R, HW_R)
            with torch.autocast("cuda", dtype=torch.float16):
                res = r.render_eval(ray["rays_o"][0], ray["rays_d"][0], bg_color=1.0, perturb=False, scale_depth=False, image_hw=(HW_R, HW_R))
            depth, opacity = res["depth"].float().contiguous(), res["weights_sum"].float().contiguous()
            x = ray["rays_o"][0].reshape(-1, 3)[:, 0] + depth / opacity.clamp_min(1e-6) * ray["rays_d"][0].reshape(-1, 3)[:, 0]
            mask = ((opacity >= 0.5) & (x > 0)).to(torch.uint8).reshape(HW_R, HW_R)
            views.append((depth, opacity, mask))
    return r, poses, views


def _by_hand(r, poses, views, use, **kw):
    from laenerf_amd.editing import lift_masks, mask_lift_pack
    packed = torch.stack([mask_lift_pack(views[i][0], views[i][1], views[i][2].reshape(-1)) for i in use]).reshape(len(use), HW_R, HW_R)
    return lift_masks(packed, poses[use].contiguous(), INTR_R, HW_R, HW_R, r.density_bitfield, r.cascade, r.bound, grid_size=r.grid_size, **kw)


def test_new_from_masks_equals_the_hand_written_chain(rendered):
    from laenerf_amd.editing import EditGrid
    r, poses, views = rendered
    masks = [v[2] for v in views]
    assert all(0 < int(m.sum()) < m.numel() for m in masks)
    eg = EditGrid()
    eg.pts, eg._queue = np.zeros((1, 3)), torch.zeros(4, dtype=torch.int32, device=DEV)
    n = eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks)
    want = _by_hand(r, poses, views, [0, 1, 2])
    assert torch.equal(eg.grid, want) and eg.pts is None and eg._queue is None and eg.queue_length() == 0
    pop = int(np.unpackbits(N(eg.grid)).sum())
    print("selected cells", n, "of", int(np.unpackbits(N(r.density_bitfield)).sum()), "occupied")
    assert n == pop and 0 < n < int(np.unpackbits(N(r.density_bitfield)).sum())
    assert not (eg.grid & ~r.density_bitfield).any()                 # only occupied cells
    assert r.model.training is False
    # masks on the host and parameters go through
    n2 = eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, [m.cpu() for m in masks], depth_margin=0.5, min_views=2, min_share=0.75)
    assert torch.equal(eg.grid, _by_hand(r, poses, views, [0, 1, 2], depth_margin=0.5, min_views=2, min_share=0.75)) and 0 < n2 < n


def test_a_none_mask_skips_its_view_and_given_depths_bypass_the_render(rendered, monkeypatch):
    from laenerf_amd.editing import EditGrid
    r, poses, views = rendered
    masks = [v[2] for v in views]
    eg = EditGrid()
    n = eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, [masks[0], None, masks[2]])
    assert torch.equal(eg.grid, _by_hand(r, poses, views, [0, 2])) and n == int(np.unpackbits(N(eg.grid)).sum()) > 0
    assert not torch.equal(eg.grid, _by_hand(r, poses, views, [0, 1, 2]))
    with pytest.raises(ValueError):
        eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, [None, None, None])
    with pytest.raises(ValueError):
        eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks[:2])
    with pytest.raises(ValueError):
        eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks, depths=[v[0] for v in views])
    # depths / opacities of the caller's: nothing is rendered, and other planes give another grid
    def no_render(*a, **k):
        raise AssertionError("render_eval called although depths were given")
    monkeypatch.setattr(r, "render_eval", no_render)
    far = [(v[0] * 0 + 1.5 * 0.9, v[1] * 0 + 0.9, v[2]) for v in views]       # a surface at t = 1.5 everywhere, in front of every cell
    n = eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks, depths=[v[0] for v in far], opacities=torch.stack([v[1] for v in far]))
    assert torch.equal(eg.grid, _by_hand(r, poses, far, [0, 1, 2])) and n == int(np.unpackbits(N(eg.grid)).sum())
    assert n == 0                                                    # the cameras stand 3.2 from the origin, every cell within 1 of it
    n = eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks, depths=[v[0] for v in views], opacities=[v[1] for v in views])
    assert torch.equal(eg.grid, _by_hand(r, poses, views, [0, 1, 2])) and n > 0


def test_selection_masks_of_every_occupied_cell_and_mask_iou(rendered):
    from laenerf_amd.editing import EditGrid, mask_iou, selection_masks
    from laenerf_amd.rays import get_rays
    r, poses, views = rendered
    eg = EditGrid()
    eg.grid = r.density_bitfield.clone()
    for mo in (0.5, 0.9):
        got = selection_masks(r, eg, poses, INTR_R, HW_R, HW_R, min_opacity=mo)
        assert got.shape == (3, HW_R, HW_R) and got.dtype == torch.uint8 and set(np.unique(N(got))) == {0, 1}
        for i in range(3):
            ray = get_rays(poses[i:i + 1], INTR_R, HW_R, HW_R)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                res = r.render_distill(ray["rays_o"][0], ray["rays_d"][0], eg.grid, perturb=False)
            assert torch.equal(got[i].reshape(-1).bool(), res["weights"].float() >= mo)
    # the bitfield itself is accepted too; an empty selection marks nothing
    assert torch.equal(selection_masks(r, eg.grid, poses, INTR_R, HW_R, HW_R, min_opacity=0.9), got)
    assert not selection_masks(r, torch.zeros_like(eg.grid), poses, INTR_R, HW_R, HW_R).any()
    # the round trip of a lifted selection comes back near its masks (printed, not asserted: no bound is derived for it)
    masks = [v[2] for v in views]
    eg.new_from_masks(r, poses, INTR_R, HW_R, HW_R, masks)
    back = selection_masks(r, eg, poses, INTR_R, HW_R, HW_R)
    print("IoU of the round trip", [round(mask_iou(back[i], masks[i]), 3) for i in range(3)])
    assert mask_iou(masks[0], masks[0]) == 1.0 and mask_iou(masks[0], 1 - masks[0]) == 0.0
