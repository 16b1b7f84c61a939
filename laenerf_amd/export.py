"""Mesh export as one staged pipeline: every step the eight export methods of NeRFRenderer (extract_mesh, extract_mesh_attributes,
save_mesh, extract_mesh_tsdf, save_mesh_tsdf, extract_mesh_textured, save_mesh_textured, simplify_grid) chain, written once, as
free functions that take the renderer (like tsdf.render_packed_views).  The operators are mesh.py, components.py, tsdf.py,
atlas.py and simplify.py; DESIGN.md section 4h.

    1  density_field            sigma of the model on a resolution^3 lattice over aabb_infer (mesh.extract_fields)
    2  truncation, packed_views, tsdf_field
                                trunc_voxels in world units; the views rendered or taken from the caller; fused (tsdf.tsdf_fuse)
    3  surface                  mesh.drop_components -> mesh.marching_cubes -> mesh.vertex_attributes at a level of a field
    4  simplified               simplify.simplify_mesh on the lattice of simplify_grid
    5  field_colors             the model's radiance at points along directions, a chunk at a time
    6  host_pair                the (vertices, triangles) pair the extract_mesh / save_* methods return
    7  write_ply                mesh.pack_ply + mesh.write_ply_packed

density_mesh (1, 3, 4, 5), tsdf_mesh (2, 3, 4) and textured_mesh (either, then the atlas) run them in that order: a field, its
surface under the component rule, the simplification, then the colours (the TSDF's fused vertex colours go INTO the simplification).
All argument checks run before any work on the device.  Everything runs under torch.no_grad(); model.training is left alone
(tsdf.render_packed_views restores it).

The options every entry point shares:

  keep_largest / min_component / min_component_fraction -- here one value, `rule`, the three in that order (the arguments of
    mesh.drop_components after the level): floaters are dropped from the field before marching cubes.  keep_largest keeps the
    largest connected component of {field > level}, min_component those of at least that many lattice points,
    min_component_fraction those of at least that fraction of the largest.  The kept surfaces are the unfiltered mesh's, bit for
    bit, normals included: normals are taken from the unfiltered field.  With no rule nothing is labelled.
  simplify -- a cluster cell in multiples of the largest lattice spacing (simplify_grid), None: nothing changes and
    laenerf_amd.simplify is not imported.  The mesh goes through quadric vertex clustering on the device: `vertices`, `triangles`
    and `normals` are simplify_mesh's outputs (the normals the area-weighted face normals of each cluster).

What comes back: the extract_*_attributes / _tsdf / _textured methods return a dict of device tensors, `vertices` [V,3] fp32 in
the box (extract_mesh's float64 scaling rounded once to fp32), `triangles` [T,3] int32, and `normals` / `colors` [V,3] fp32 only
on request.  extract_mesh and the save_* methods return (vertices [V,3] float64, triangles [T,3] int32) on the host: the
marching-cubes vertices scaled in float64 (mesh.scale_vertices), or with simplify the simplified fp32 positions as float64."""
from typing import NamedTuple

import numpy as np
import torch

from . import mesh


def box(renderer):
    """aabb_infer on the host -> (minimum [3], maximum [3])"""
    aabb = renderer.aabb_infer.cpu()
    return aabb[:3], aabb[3:]


def simplify_grid(renderer, resolution, simplify):
    """the cluster lattice of `simplify` -> (cell, origin fp32 [3], dims): the cell is `simplify` times the largest spacing of the
    resolution^3 lattice over aabb_infer, the origin the box minimum, dims cover the box"""
    if not float(simplify) > 0.0:
        raise ValueError("simplify must be a positive cell size in lattice spacings (or None)")
    bmin, bmax = (mesh._bounds32(b) for b in box(renderer))
    cell = np.float32(float(simplify) * max(float(a[1] - a[0]) for a in mesh.lattice(bmin, bmax, int(resolution))))
    dims = tuple(int(n) for n in np.floor((bmax.astype(np.float64) - bmin.astype(np.float64)) / np.float64(cell)) + 2)
    return float(cell), bmin, dims


def grid_of(renderer, resolution, simplify):
    """simplify_grid for the pipelines below, which take it as `grid`: None where nothing is to be simplified"""
    return None if simplify is None else simplify_grid(renderer, resolution, simplify)


# ---- 1 density field
def density_field(renderer, bounds, resolution, chunk):
    """the reference's extract_fields over `bounds` (box(renderer), which every pipeline reads once): sigma of model.density under
    fp16 autocast (not multiplied by density_scale), chunk^3 points at a time -> u [R,R,R] fp32 on the device"""
    sigma = getattr(renderer.model, "density_sigma", None) or (lambda x: renderer.model.density(x)["sigma"])

    def query(pts):
        with torch.autocast("cuda", dtype=torch.float16):
            return sigma(pts)

    return mesh.extract_fields(*bounds, resolution, query, S=chunk, device=renderer.aabb_infer.device)


# ---- 2 TSDF field
class Views(NamedTuple):
    """the first six arguments of tsdf.tsdf_fuse and atlas.atlas_fuse_views; frames None: no colours are wanted"""
    packed: torch.Tensor
    poses: torch.Tensor
    intrinsics: tuple
    H: int
    W: int
    frames: torch.Tensor


def truncation(bounds, resolution, trunc_voxels, who="extract_mesh_tsdf"):
    """-> (the lattice's axes, trunc = trunc_voxels x the largest axis spacing, in world units)"""
    if not float(trunc_voxels) > 0.0:
        raise ValueError(f"{who}: trunc_voxels must be positive")
    axes = mesh.lattice(*bounds, int(resolution))
    return axes, float(trunc_voxels) * max(float(a[1] - a[0]) for a in axes)


def packed_views(renderer, poses, intrinsics, H, W, frames, depths, opacities, min_opacity, colors):
    """the views of `poses` as surface distance planes (tsdf.render_packed_views; depths / opacities replace the renders) with the
    frames that colour them: the caller's, else (colors only) the model's own renders of the same views"""
    from . import tsdf
    poses = poses.reshape(-1, 4, 4).to(renderer.aabb_infer.device).float().contiguous()
    own = bool(colors) and frames is None
    packed = tsdf.render_packed_views(renderer, poses, intrinsics, H, W, depths, opacities, min_opacity, return_frames=own)
    if own:
        packed, frames = packed
    return Views(packed, poses, intrinsics, H, W, frames if colors else None)


def tsdf_field(views, axes, trunc, min_views, colors):
    """-> tsdf.tsdf_fuse's dict: `u` to run marching cubes on at zero, with colors `rgb` and `counts` of the views' frames"""
    from . import tsdf
    return tsdf.tsdf_fuse(*views[:5], axes, trunc, frames=views.frames if colors else None, min_views=min_views)


# ---- 3 surface
def surface(bounds, u, level, rule, want):
    """the level set of the field u without the components `rule` rejects.  want: the entries of mesh.ATTRS to compute ("pos" ->
    `vertices`, "normals" -> `normals`, from the unfiltered field; none: lae_mesh_vertex_attrs is not launched)
    -> (the mesh, a dict; the marching-cubes vertices in index space; the "dirs" attribute or None)"""
    v, t = mesh.marching_cubes(mesh.drop_components(u, level, *rule), level)
    attrs = mesh.vertex_attributes(u, v, *bounds, want=want) if want else {}
    m = {"vertices": attrs["pos"], "triangles": t} if "pos" in attrs else {"triangles": t}
    if "normals" in attrs:
        m["normals"] = attrs["normals"]
    return m, v, attrs.get("dirs")


# ---- 4 simplify
def simplified(m, grid, normals):
    """m through simplify.simplify_mesh on `grid` (simplify_grid) -> (the simplified mesh: `vertices`, `triangles`, `normals` when
    asked for, `colors` where m carries them; the clusters' normals).  Colours, source by source: the TSDF's fused vertex colours
    arrive in m and leave as the means over each cluster's members; the density's are queried afterwards, at the new vertices
    along minus the new normals (density_mesh); a textured mesh carries none."""
    from . import simplify
    cell, origin, dims = grid
    s = simplify.simplify_mesh(m["vertices"], m["triangles"], cell, origin=origin, dims=dims, colors=m.get("colors"))
    keys = ("vertices", "triangles") + (("normals",) if normals else ()) + (("colors",) if "colors" in m else ())
    return {k: s[k] for k in keys}, s["normals"]


# ---- 5 field colours
def field_colors(renderer, pos, dirs, color_chunk):
    """the radiance model(pos, dirs) under the sweep's fp16 autocast, color_chunk points at a time -> [N,3] fp32"""
    rgb = torch.empty_like(pos)
    for i in range(0, pos.shape[0], color_chunk):
        with torch.autocast("cuda", dtype=torch.float16):
            rgb[i:i + color_chunk] = renderer.model(pos[i:i + color_chunk], dirs[i:i + color_chunk])[1].float()
    return rgb


# ---- 6 host pair
def host_pair(m, index_vertices=None, renderer=None, resolution=None):
    """-> (vertices [V,3] float64, triangles [T,3] int32) on the host: index_vertices scaled into the box in float64 where they
    exist (the reference's rule), else m's fp32 positions widened"""
    if index_vertices is None:
        return m["vertices"].double().cpu().numpy(), m["triangles"].cpu().numpy()
    v = mesh.scale_vertices(index_vertices.cpu().numpy(), renderer.aabb_infer[:3], renderer.aabb_infer[3:], int(resolution))
    return v, m["triangles"].cpu().numpy()


# ---- 7 PLY out
def write_ply(path, m):
    """m with its normals and colours as a binary PLY, the file's bodies packed on the device"""
    mesh.write_ply_packed(path, *mesh.pack_ply(m["vertices"], m["triangles"], normals=m.get("normals"), colors=m.get("colors")))


# ---- the three pipelines
@torch.no_grad()
def density_mesh(renderer, *, resolution, threshold, chunk, rule, grid, normals=False, colors=False, color_chunk=1 << 20,
                 host_only=False):
    """the level set of the density at `threshold`; grid: grid_of(...), which the caller evaluates (and which refuses) before
    anything runs -> (the mesh, its index-space vertices or None with a grid).  colors: the radiance at each vertex seen along
    minus its normal ((0, 0, 1) where the normal is zero).  host_only: the caller wants host_pair alone"""
    bounds = box(renderer)
    u = density_field(renderer, bounds, resolution, chunk)
    if grid is not None:
        want = ("pos",)                                                        # the simplification makes the normals
    elif host_only and not normals and not colors:
        want = ()                                                              # triangles alone: host_pair scales the index-space vertices
    else:
        want = ("pos",) + (("normals",) if normals else ()) + (("dirs",) if colors else ())
    m, v, dirs = surface(bounds, u, threshold, rule, want)
    if grid is not None:
        m, n = simplified(m, grid, normals)
        v = None
        if colors:
            flat = (n == 0).all(1, keepdim=True)                               # vertex_attributes' fallback direction
            dirs = torch.where(flat, torch.tensor([0.0, 0.0, 1.0], device=flat.device), -n).contiguous()
    if colors:
        m["colors"] = field_colors(renderer, m["vertices"], dirs, color_chunk)
    return m, v


def fused_mesh(bounds, views, axes, trunc, min_views, rule, grid, normals, colors):
    """tsdf_mesh from the views on"""
    from . import tsdf
    f = tsdf_field(views, axes, trunc, min_views, colors)
    m, v, _ = surface(bounds, f["u"], 0.0, rule, ("pos", "normals") if normals and grid is None else ("pos",))
    if colors:
        m["colors"], n_grey = tsdf.tsdf_vertex_colors(f["rgb"], f["counts"], v)
    if grid is not None:
        m, _ = simplified(m, grid, normals)
        v = None
    if colors:
        m["n_grey"] = n_grey
    return m, v


@torch.no_grad()
def tsdf_mesh(renderer, poses, intrinsics, H, W, *, resolution, trunc_voxels, frames, depths, opacities, min_opacity, min_views,
              normals, colors, rule, simplify):
    """the zero set of the views' truncated signed distance field -> (the mesh, its index-space vertices or None with simplify).
    colors: fused from the frames per vertex, plus `n_grey`, the vertices no view coloured -- counted before the simplification"""
    bounds = box(renderer)
    axes, trunc = truncation(bounds, resolution, trunc_voxels)
    grid = grid_of(renderer, resolution, simplify)
    views = packed_views(renderer, poses, intrinsics, H, W, frames, depths, opacities, min_opacity, colors)
    return fused_mesh(bounds, views, axes, trunc, min_views, rule, grid, normals, colors)


@torch.no_grad()
def textured_mesh(renderer, *, resolution, threshold, cell, texture_size, source, geometry, poses, intrinsics, H, W, frames,
                  trunc_voxels, min_cos, fallback, rule, chunk, color_chunk, depths, opacities, min_opacity, min_views, simplify):
    """NeRFRenderer.extract_mesh_textured: either geometry with normals and no vertex colours, simplified, then its atlas"""
    from . import atlas
    if source not in ("field", "views") or geometry not in ("density", "tsdf") or fallback not in ("grey", "field"):
        raise ValueError("extract_mesh_textured: source is 'field' or 'views', geometry 'density' or 'tsdf', fallback 'grey' or 'field'")
    need_views = source == "views" or geometry == "tsdf"
    if need_views and (poses is None or intrinsics is None or H is None or W is None):
        raise ValueError("extract_mesh_textured: source='views' and geometry='tsdf' need poses, intrinsics, H and W")
    if need_views:
        bounds = box(renderer)
        axes, trunc = truncation(bounds, resolution, trunc_voxels, "extract_mesh_tsdf" if geometry == "tsdf" else "extract_mesh_textured")
    grid = grid_of(renderer, resolution, simplify)
    dev = renderer.aabb_infer.device
    if need_views:
        views = packed_views(renderer, poses, intrinsics, H, W, frames, depths, opacities, min_opacity, source == "views")
    if geometry == "tsdf":
        m, _ = fused_mesh(bounds, views, axes, trunc, min_views, rule, grid, True, False)
    else:
        m, _ = density_mesh(renderer, resolution=resolution, threshold=threshold, chunk=chunk, rule=rule, grid=grid, normals=True)
    verts, tris, normals = m["vertices"], m["triangles"], m["normals"]
    T = tris.shape[0]
    lay = atlas.atlas_layout(T, cell, texture_size)
    out = {"vertices": verts, "triangles": tris, "normals": normals, "layout": lay,
           "uv": torch.from_numpy(atlas.atlas_uv(lay)).to(dev), "n_grey": torch.zeros(1, dtype=torch.int32, device=dev)}
    if T == 0:
        out["texture"] = torch.zeros(lay.S, lay.S, 3, dtype=torch.uint8, device=dev)
        out["texels"] = None
        return out
    tx = atlas.atlas_texels(verts, tris, normals, lay.cell)
    if source == "field":
        rgb = field_colors(renderer, tx["pos"], tx["dirs"], color_chunk)
    else:
        f = atlas.atlas_fuse_views(*views, tx["pos"], tx["nrm"], tx["owner"], trunc, min_cos, counts=fallback == "field")
        rgb, out["n_grey"] = f["rgb"], f["n_grey"]
        if fallback == "field":
            unseen = ((f["counts"].to(torch.int32) == 0) & (tx["owner"] >= 0)).nonzero().reshape(-1)
            if unseen.numel():
                rgb[unseen] = field_colors(renderer, tx["pos"][unseen].contiguous(), tx["dirs"][unseen].contiguous(), color_chunk)
    out["texture"] = atlas.atlas_pack(rgb, tx["owner"], lay)
    out["texels"] = {"pos": tx["pos"], "dirs": tx["dirs"], "owner": tx["owner"], "rgb": rgb}
    return out
