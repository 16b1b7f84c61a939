"""Connected components on the MI355X (csrc/components.hip) against the numpy restatement of their specification, bit for bit:
labels, sizes and statistics on shapes that put full and partial tiles on every axis, the filter under every rule, marching cubes
of a filtered field, and the two users: mesh export without floaters and NeRFRenderer.prune_floaters."""
import numpy as np
import pytest
import torch

from components_util import FIELDS, SHAPES, THR, case, sphere_and_blobs
from gpu_util import DEV, T

pytestmark = pytest.mark.gpu


def D(a):
    """a device copy of a shared (read-only) reference array"""
    return T(np.array(a))


def _device_result(u, thr=THR):
    from laenerf_amd.components import component_sizes, label_components
    labels = label_components(u, thr)
    sizes, stats = component_sizes(labels)
    assert labels.dtype == sizes.dtype == stats.dtype == torch.int32 and labels.is_cuda and labels.shape == u.shape
    return labels, sizes, stats


def _equal(dev, ref):
    return all(np.array_equal(d.cpu().numpy(), r) for d, r in zip(dev, ref))


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_sizes_and_stats_equal_numpy(shape, name):
    u, labels, sizes, stats = case(shape, name)
    dev = _device_result(D(u))
    assert np.array_equal(dev[2].cpu().numpy(), stats), (dev[2].tolist(), stats.tolist())
    assert np.array_equal(dev[0].cpu().numpy(), labels)
    assert np.array_equal(dev[1].cpu().numpy(), sizes)
    if min(shape) >= 6:                                               # the boxes are not clipped: the fields are what their names say
        if "contact" in name:
            assert stats[0] == 2
        if "face_link" in name or name.startswith(("serpentine", "comb")):
            assert stats[0] == 1


RULES = [dict(largest=True), dict(min_size=1), dict(min_size=3), dict(min_fraction=0.25), dict(min_fraction=1.0),
         dict(largest=True, min_size=10 ** 9), dict(min_size=2, min_fraction=0.05)]


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(f"{k}={v}" for k, v in r.items()))
@pytest.mark.parametrize("shape, name", [((9, 17, 33), "iid_0.3116"), ((40, 24, 72), "iid_0.2"), ((5, 6, 130), "special_values"),
                                         ((3, 5, 7), "iid_0.5"), ((9, 17, 33), "all_outside")])
def test_filter_equals_numpy_in_place_and_unaligned(shape, name, rule):
    from laenerf_amd.components import filter_components, filter_components_numpy
    u = case(shape, name)[0]
    ref, ref_info = filter_components_numpy(u, THR, **rule)
    ud = D(u)
    out, info = filter_components(ud, THR, **rule)
    assert info == ref_info and out is not ud
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(ud.cpu().numpy().view(np.uint32), u.view(np.uint32))          # the input is left alone
    same, _ = filter_components(ud, THR, out=ud, **rule)                                 # in place
    assert same is ud and torch.equal(ud.view(torch.int32), out.view(torch.int32))
    base = torch.zeros(1 + u.size, device=DEV)
    shifted = base[1:].view(u.shape)                                                     # contiguous, 4 bytes past a 16-byte boundary
    shifted.copy_(D(u))
    assert shifted.data_ptr() % 16 == 4
    out2, info2 = filter_components(shifted, THR, out=torch.zeros(2 + u.size, device=DEV)[2:].view(u.shape), **rule)
    assert info2 == ref_info and out2.data_ptr() % 16 == 8 and torch.equal(out2.view(torch.int32), out.view(torch.int32))


def test_info_counts_and_argument_errors():
    from laenerf_amd.components import component_sizes, filter_components, label_components
    u, labels, sizes, stats = case((9, 17, 33), "iid_0.3116")
    out, info = filter_components(D(u), THR, min_size=3, info=True)
    kept = sizes >= 3
    assert info["n_kept"] == int(kept.sum()) and info["n_removed"] == int(stats[0]) - int(kept.sum())
    assert info["n_removed_points"] == int(sizes[(sizes > 0) & ~kept].sum())
    with pytest.raises(ValueError):
        filter_components(D(u), THR)
    with pytest.raises(RuntimeError):
        label_components(D(u).double(), THR)
    with pytest.raises(RuntimeError):
        label_components(D(u)[:, :, ::2], THR)
    with pytest.raises(RuntimeError):
        label_components(torch.zeros(4, 4, 1, device=DEV), THR)
    with pytest.raises(RuntimeError):
        component_sizes(D(labels).long())
    u = np.array(u)
    lab = label_components(u, THR)                                    # numpy in, numpy out
    assert isinstance(lab, np.ndarray) and lab.dtype == np.int32 and np.array_equal(lab, labels)
    f, _ = filter_components(u, THR, largest=True)
    assert isinstance(f, np.ndarray) and f.dtype == np.float32


def test_unaligned_field_and_two_runs_are_identical():
    u, labels, sizes, stats = case((40, 24, 72), "iid_0.3116")
    base = torch.zeros(3 + u.size, device=DEV)
    for off in (1, 3):
        shifted = base[off:off + u.size].view(u.shape)
        shifted.copy_(D(u))
        assert _equal(_device_result(shifted), (labels, sizes, stats))
    a, b = _device_result(D(u)), _device_result(D(u))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_captured_run_replayed_on_changed_input_equals_eager():
    from laenerf_amd import _lib
    from laenerf_amd.components import component_sizes, label_components
    shape = (33, 9, 17)
    lib = _lib.load()

    def run(u, out):
        labels = label_components(u, THR)
        sizes, stats = component_sizes(labels)
        rc = lib.lae_components_filter(u.data_ptr(), labels.data_ptr(), sizes.data_ptr(), u.numel(), THR, 3, -1, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return labels, sizes, stats

    u = D(case(shape, "iid_0.5")[0]).clone()
    out = torch.empty_like(u)
    run(u, out)                                                       # eager first (the library's workspace rule)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run(u, out)
    from laenerf_amd.components import filter_components_numpy
    for name in ("iid_0.3116", "comb_thin"):
        field, labels, sizes, stats = case(shape, name)
        u.copy_(D(field))
        g.replay()
        torch.cuda.synchronize()
        assert _equal(captured, (labels, sizes, stats))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), filter_components_numpy(field, THR, min_size=3)[0].view(np.uint32))


def test_marching_cubes_of_the_filtered_field_is_the_mesh_of_the_sphere_alone():
    from laenerf_amd.components import filter_components
    from laenerf_amd.mesh import marching_cubes
    both, sphere = sphere_and_blobs(48)
    f, info = filter_components(T(both), 0.0, largest=True)
    assert info["n_components"] == 4 and info["keep_root"] == info["largest_root"]
    v, t = marching_cubes(f, 0.0)
    v0, t0 = marching_cubes(T(sphere), 0.0)
    v1, t1 = marching_cubes(T(both), 0.0)
    assert torch.equal(t, t0) and torch.equal(v.view(torch.int32), v0.view(torch.int32))
    assert 0 < t.shape[0] < t1.shape[0]


# ---- renderer level: the tiny seeded renderer of tests/test_gpu_mesh.py
def _network(seed=11, **kwargs):
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=1).to(DEV).eval()
    net.encoder.embeddings.data.uniform_(-1.0, 1.0)
    net.sigma_net.weights.data.mul_(1.5)
    return NeRFRenderer(net, bound=1, density_thresh=10, **kwargs).to(DEV).eval()


def _rows(ply):
    rec = np.concatenate([ply["vertices"].view(np.uint8).reshape(len(ply["vertices"]), -1),
                          ply["normals"].view(np.uint8).reshape(len(ply["vertices"]), -1), ply["colors"]], 1)
    return {bytes(r) for r in rec}


def test_save_mesh_without_floaters_and_the_default_path(tmp_path, monkeypatch):
    from laenerf_amd import components, mesh
    r = _network()
    R = 64
    bmin, bmax = r.aabb_infer[:3].cpu(), r.aabb_infer[3:].cpu()

    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return r.model.density(pts)["sigma"]

    with torch.no_grad():
        u = mesh.extract_fields(bmin, bmax, R, query, device=DEV)
    thr = float(np.quantile(u.cpu().numpy(), 0.7))
    n_components = components.filter_components(u, thr, largest=True)[1]["n_components"]
    assert n_components > 1                                           # there is something to drop
    plain, kept = str(tmp_path / "plain.ply"), str(tmp_path / "kept.ply")
    v_all, t_all = r.save_mesh(plain, resolution=R, threshold=thr, normals=True, colors=True)
    v, t = r.save_mesh(kept, resolution=R, threshold=thr, normals=True, colors=True, keep_largest=True)
    a, b = mesh.read_ply(plain), mesh.read_ply(kept)
    assert np.array_equal(b["triangles"], t) and 0 < len(t) < len(t_all) and len(b["vertices"]) < len(a["vertices"])
    assert _rows(b) <= _rows(a)                                       # every kept vertex: the same position, normal and colour bits
    # the kept surface is the mesh of the filtered field
    f = components.filter_components(u, thr, largest=True)[0]
    vi, ti = mesh.marching_cubes(f, thr)
    assert np.array_equal(ti.cpu().numpy(), t) and np.array_equal(mesh.scale_vertices(vi.cpu().numpy(), bmin, bmax, R), v)
    # extract_mesh / extract_mesh_attributes agree with the file; min_component and min_component_fraction go through too
    v2, t2 = r.extract_mesh(resolution=R, threshold=thr, keep_largest=True)
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    m = r.extract_mesh_attributes(resolution=R, threshold=thr, keep_largest=True)
    assert np.array_equal(m["vertices"].cpu().numpy(), b["vertices"]) and np.array_equal(m["normals"].cpu().numpy(), b["normals"])
    ref = components.filter_components(u, thr, min_size=20, min_fraction=0.01)[0]
    v3, t3 = r.extract_mesh(resolution=R, threshold=thr, min_component=20, min_component_fraction=0.01)
    assert np.array_equal(t3, mesh.marching_cubes(ref, thr)[1].cpu().numpy())
    # the defaults: nothing is labelled, and the file is today's statements' file byte for byte
    def boom(*a, **k):
        raise AssertionError("the default path must not label")
    monkeypatch.setattr(components, "label_components", boom)
    default = str(tmp_path / "default.ply")
    r.save_mesh(default, resolution=R, threshold=thr, normals=True, colors=True)
    with torch.no_grad():
        vv, tt = mesh.marching_cubes(u, thr)
        attrs = mesh.vertex_attributes(u, vv, bmin, bmax)
        with torch.autocast("cuda", dtype=torch.float16):
            rgb = r.model(attrs["pos"], attrs["dirs"])[1].float()
    head, vb, fb = mesh.pack_ply(attrs["pos"], tt, normals=attrs["normals"], colors=rgb)
    today = str(tmp_path / "today.ply")
    mesh.write_ply_packed(today, head, vb, fb)
    assert open(default, "rb").read() == open(today, "rb").read() == open(plain, "rb").read()
    bare = str(tmp_path / "bare.ply")
    vb2, tb2 = r.save_mesh(bare, resolution=R, threshold=thr)
    assert np.array_equal(tb2, t_all) and np.array_equal(vb2, v_all)


def _hand_grid(H=32):
    g = np.zeros((H, H, H), np.float32)
    g[4:20, 4:20, 4:20] = 50.0
    g[26:29, 26:29, 26:29] = 60.0
    g[24:26, 2:4, 2:4] = 70.0
    g[2:4, 26:28, 10:12] = 80.0
    g[30, 30, 1] = -1.0                                               # a cell mark_untrained_grid took out earlier
    return g


def _with_grid(r, g):
    from laenerf_amd import raymarching
    H = r.grid_size
    ax = torch.arange(H, device=DEV, dtype=torch.int32)
    coords = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()
    order = raymarching.morton3D(coords).long()                       # cell (x, y, z) in C order -> its place in density_grid
    r.density_grid.zero_()
    r.density_grid[0][order] = T(g).reshape(-1)
    r.mean_density = float(r.density_grid.clamp(min=0).mean().item())
    thr = min(r.mean_density, r.density_thresh)
    r.density_bitfield = raymarching.packbits(r.density_grid, thr, r.density_bitfield)
    return order.cpu().numpy(), thr


@pytest.mark.parametrize("persist", [True, False])
def test_prune_floaters(persist):
    from laenerf_amd.components import filter_components_numpy
    r = _network(grid_size=32)
    g = _hand_grid()
    order, thr = _with_grid(r, g)
    assert 0 < thr < 10
    # rays along +z through the removed box at cells [26:29]^3 only (x and y beyond every other box)
    xy = (torch.tensor([26.5, 27.5, 28.5], device=DEV) / 32) * 2 - 1
    o = torch.stack([xy.repeat_interleave(3), xy.repeat(3), torch.full((9,), -3.0, device=DEV)], -1)
    d = torch.tensor([[0.0, 0.0, 1.0]], device=DEV).repeat(9, 1)
    with torch.autocast("cuda", dtype=torch.float16):
        before = r.render_eval(o, d, bg_color=1)
    assert (before["weights_sum"] > 0).any() and (before["image"] != 1).any()
    mean_density, mean_count, iter_density = r.mean_density, r.mean_count, r.iter_density
    info = r.prune_floaters(persist=persist)
    ref, ref_info = filter_components_numpy(g, thr, largest=True)
    assert info == ref_info and info["n_components"] == 4 and info["largest_size"] == 16 ** 3
    removed = (g > np.float32(thr)) & ~(ref > np.float32(thr))
    assert removed.sum() == 27 + 8 + 8
    want = np.where(removed, np.float32(-1.0 if persist else 0.0), g)
    grid = np.empty(32 ** 3, np.float32)
    grid[order] = want.reshape(-1)
    assert np.array_equal(r.density_grid[0].cpu().numpy().view(np.uint32), grid.view(np.uint32))
    assert np.array_equal(r.density_bitfield.cpu().numpy(), np.packbits(grid > np.float32(thr), bitorder="little"))
    assert (r.mean_density, r.mean_count, r.iter_density) == (mean_density, mean_count, iter_density)
    with torch.autocast("cuda", dtype=torch.float16):
        after = r.render_eval(o, d, bg_color=1)
    assert (after["weights_sum"] == 0).all() and (after["image"] == 1).all()
    if persist:
        r.update_extra_state()
        now = np.empty(32 ** 3, np.float32)
        now[:] = r.density_grid[0].cpu().numpy()
        assert (now[order].reshape(g.shape)[removed] == -1).all() and now[order].reshape(g.shape)[30, 30, 1] == -1


def test_prune_floaters_rules_and_cascades():
    from laenerf_amd.components import filter_components_numpy
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    r = _network(grid_size=32)
    g = _hand_grid()
    order, thr = _with_grid(r, g)
    info = r.prune_floaters(keep_largest=False, min_cells=9, persist=False)          # the 27-cell box passes, the two of 8 do not
    ref, ref_info = filter_components_numpy(g, thr, min_size=9)
    assert info == ref_info
    want = np.where((g > np.float32(thr)) & ~(ref > np.float32(thr)), np.float32(0), g)
    assert np.array_equal(r.density_grid[0].cpu().numpy()[order].reshape(g.shape), want)
    with pytest.raises(ValueError):
        r.prune_floaters(keep_largest=False)
    two = NeRFRenderer(NeRFNetwork(bound=2).to(DEV).eval(), bound=2, grid_size=32).to(DEV)
    assert two.cascade == 2
    with pytest.raises(ValueError):
        two.prune_floaters()
