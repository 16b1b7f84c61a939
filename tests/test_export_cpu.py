"""laenerf_amd/export.py without a device: every refusal of the renderer's export methods comes before any work on the model
or the device, the host pair's rule, and the import rule of the `simplify` option."""
import sys

import numpy as np
import pytest
import torch

from laenerf_amd import export, mesh
from laenerf_amd.renderer import NeRFRenderer


class _Stub:
    """stands in for the renderer: a CPU box, and a model that must not be touched"""
    aabb_infer = torch.tensor([-1.0, -1.0, -0.5, 1.0, 1.5, 1.0])

    @property
    def model(self):
        raise AssertionError("a refused call must not reach the model")


POSES = torch.eye(4).repeat(2, 1, 1)
VIEWS = dict(poses=POSES, intrinsics=(50.0, 50.0, 8.0, 8.0), H=16, W=16)


def test_importing_export_does_not_import_simplify(monkeypatch):
    """in this process: both modules are taken out of sys.modules (other test modules import simplify), export is imported
    afresh, and monkeypatch puts the process's own modules back"""
    import importlib

    import laenerf_amd
    monkeypatch.setattr(laenerf_amd, "export", export)               # restored to the module this file uses
    monkeypatch.delitem(sys.modules, "laenerf_amd.export")
    monkeypatch.delitem(sys.modules, "laenerf_amd.simplify", raising=False)
    fresh = importlib.import_module("laenerf_amd.export")
    assert fresh is not export and callable(fresh.simplified)
    assert "laenerf_amd.simplify" not in sys.modules


@pytest.mark.parametrize("simplify", [0, -1])
def test_simplify_is_refused_on_every_density_entry_point(simplify, tmp_path):
    r = _Stub()
    with pytest.raises(ValueError, match="simplify must be a positive cell size"):
        NeRFRenderer.extract_mesh(r, resolution=8, simplify=simplify)
    with pytest.raises(ValueError, match="simplify must be a positive cell size"):
        NeRFRenderer.extract_mesh_attributes(r, resolution=8, simplify=simplify)
    for flags in ({}, dict(normals=True, colors=True)):
        path = tmp_path / "m.ply"
        with pytest.raises(ValueError, match="simplify must be a positive cell size"):
            NeRFRenderer.save_mesh(r, str(path), resolution=8, simplify=simplify, **flags)
        assert not path.exists()
    with pytest.raises(ValueError, match="simplify must be a positive cell size"):
        NeRFRenderer.extract_mesh_textured(r, resolution=8, simplify=simplify)
    with pytest.raises(ValueError, match="simplify must be a positive cell size"):
        NeRFRenderer.simplify_grid(r, 8, simplify)


def test_trunc_voxels_is_refused_before_the_views_are_rendered(tmp_path):
    r = _Stub()
    with pytest.raises(ValueError, match="extract_mesh_tsdf: trunc_voxels must be positive"):
        NeRFRenderer.extract_mesh_tsdf(r, POSES, VIEWS["intrinsics"], 16, 16, resolution=8, trunc_voxels=0)
    with pytest.raises(ValueError, match="extract_mesh_tsdf: trunc_voxels must be positive"):
        NeRFRenderer.save_mesh_tsdf(r, str(tmp_path / "t.ply"), POSES, VIEWS["intrinsics"], 16, 16, resolution=8, trunc_voxels=0)
    with pytest.raises(ValueError, match="extract_mesh_textured: trunc_voxels must be positive"):
        NeRFRenderer.extract_mesh_textured(r, resolution=8, source="views", trunc_voxels=0, **VIEWS)
    with pytest.raises(ValueError, match="extract_mesh_tsdf: trunc_voxels must be positive"):
        NeRFRenderer.extract_mesh_textured(r, resolution=8, source="views", geometry="tsdf", trunc_voxels=0, **VIEWS)


@pytest.mark.parametrize("bad", [dict(source="renders"), dict(geometry="sdf"), dict(fallback="black")])
def test_unknown_names_are_refused(bad):
    with pytest.raises(ValueError, match="source is 'field' or 'views', geometry 'density' or 'tsdf', fallback 'grey' or 'field'"):
        NeRFRenderer.extract_mesh_textured(_Stub(), resolution=8, **bad)


@pytest.mark.parametrize("kw", [dict(source="views"), dict(geometry="tsdf"), dict(source="views", intrinsics=VIEWS["intrinsics"], H=16, W=16)])
def test_views_that_are_needed_but_not_given_are_refused(kw):
    with pytest.raises(ValueError, match="need poses, intrinsics, H and W"):
        NeRFRenderer.extract_mesh_textured(_Stub(), resolution=8, **kw)


def test_simplify_grid_is_the_lattice_the_renderer_method_returns():
    r = _Stub()
    assert export.grid_of(r, 8, None) is None
    with pytest.raises(TypeError):                                    # the public method takes a number, as it always has
        NeRFRenderer.simplify_grid(r, 8, None)
    assert export.grid_of(r, 9, 2.5)[0] == NeRFRenderer.simplify_grid(r, 9, 2.5)[0]
    cell, origin, dims = NeRFRenderer.simplify_grid(r, 9, 2.5)
    assert cell == float(np.float32(2.5 * 0.3125)) and origin.dtype == np.float32 and origin.tolist() == [-1.0, -1.0, -0.5]
    assert dims == (4, 5, 3)                                          # floor(extent / cell) + 2 per axis: extents 2, 2.5, 1.5


def test_host_pair():
    rng = np.random.default_rng(5)
    index = rng.uniform(0, 8, (11, 3)).astype(np.float32)
    m = {"vertices": torch.from_numpy(rng.standard_normal((11, 3)).astype(np.float32)),
         "triangles": torch.from_numpy(rng.integers(0, 11, (6, 3)).astype(np.int32))}
    r = _Stub()
    v, t = export.host_pair(m, torch.from_numpy(index), r, 9)
    assert v.dtype == np.float64 and t.dtype == np.int32 and np.array_equal(t, m["triangles"].numpy())
    assert np.array_equal(v, mesh.scale_vertices(index, r.aabb_infer[:3], r.aabb_infer[3:], 9))
    assert not np.array_equal(v, v.astype(np.float32).astype(np.float64))              # float64 arithmetic, not widened fp32
    v, t = export.host_pair(m)
    assert v.dtype == np.float64 and t.dtype == np.int32 and np.array_equal(t, m["triangles"].numpy())
    assert np.array_equal(v, m["vertices"].numpy().astype(np.float64))
    only_triangles = {"triangles": m["triangles"]}                    # the plain extract_mesh: no device positions at all
    assert np.array_equal(export.host_pair(only_triangles, torch.from_numpy(index), r, 9)[0], export.host_pair(m, torch.from_numpy(index), r, 9)[0])
