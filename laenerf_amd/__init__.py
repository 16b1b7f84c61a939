"""laenerf_amd: the package's modules are imported by name (laenerf_amd.trainer, laenerf_amd.mesh, ...); the TSDF mesh export's
operators are also reachable from here, resolved on first use so that `import laenerf_amd` stays free of torch."""
_TSDF = ("tsdf_fuse", "tsdf_vertex_colors", "render_packed_views", "tsdf_numpy", "tsdf_vertex_colors_numpy")
__all__ = list(_TSDF)


def __getattr__(name):
    if name in _TSDF:
        from . import tsdf
        return getattr(tsdf, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
