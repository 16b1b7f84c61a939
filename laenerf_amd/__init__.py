"""laenerf_amd: the package's modules are imported by name (laenerf_amd.trainer, laenerf_amd.mesh, ...); the TSDF mesh export's,
the texture atlas's, the mesh simplification's and the undistortion's operators are also reachable from here, resolved on first use so that
`import laenerf_amd` stays free of torch."""
_TSDF = ("tsdf_fuse", "tsdf_vertex_colors", "render_packed_views", "tsdf_numpy", "tsdf_vertex_colors_numpy")
_UNDISTORT = ("CameraModel", "Undistorter", "undistort_map", "distort_map", "remap", "target_intrinsics", "undistort_numpy",
              "undistort_map_numpy", "distort_map_numpy", "remap_numpy")
_ATLAS = ("atlas_layout", "atlas_uv", "atlas_owner_numpy", "atlas_texels", "atlas_fuse_views", "atlas_pack", "atlas_texels_numpy",
          "atlas_fuse_views_numpy", "atlas_pack_numpy", "sample_texture_numpy", "write_obj", "read_obj")
_SIMPLIFY = ("simplify_mesh", "simplify_numpy")
__all__ = list(_TSDF + _ATLAS + _SIMPLIFY + _UNDISTORT)


def __getattr__(name):
    if name in _TSDF:
        from . import tsdf
        return getattr(tsdf, name)
    if name in _ATLAS:
        import importlib
        return getattr(importlib.import_module(".atlas", __name__), name)
    if name in _SIMPLIFY:
        import importlib
        return getattr(importlib.import_module(".simplify", __name__), name)
    if name in _UNDISTORT:
        import importlib
        return getattr(importlib.import_module(".undistort", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
