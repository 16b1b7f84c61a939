"""Connected components of a lattice's inside set on the device (csrc/components.hip): the pass that drops floaters between
the density sweep and marching cubes (mesh.extract_geometry, NeRFRenderer.extract_mesh / save_mesh) and from the occupancy
grid (NeRFRenderer.prune_floaters).  The reference has nothing here: it exports through trimesh and stops.

    label_components(u, threshold)          labels [nx,ny,nz] int32: the smallest linear index of the point's component, -1 outside
    component_sizes(labels)                 (sizes [N] int32: the component's size at its root, 0 elsewhere; stats int32[4])
    filter_components(u, threshold, ...)    u with the components a rule rejects pushed down to the threshold
    components_numpy / filter_components_numpy   the same specification restated with a Python union-find (what the tests compare against)

The specification (include/laenerf.h, lae_components_*): a point is inside iff u > threshold in fp32 (marching cubes' rule: NaN
outside, +inf inside); inside points that differ by 1 in exactly one coordinate are connected (6-connectivity; edge and corner
contact does not connect); stats = (n_components, largest_root, largest_size, n_inside), ties for the largest to the lowest root,
(0, -1, 0, 0) with no inside point.  A component is kept iff its size >= min_size and (keep_root < 0 or its root == keep_root); the
inside points of the others become float32(threshold), which is outside.  Everything is integer work: the same bits on every run.

With 6-connectivity an inside point next to a kept inside point is kept too, so no crossed lattice edge of a kept component
changes either of its end values: marching cubes of the filtered field gives the kept surfaces of the unfiltered mesh bit for bit.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, need_contig, need_cuda, ptr, stream
from .mesh import _check_shape

STATS = ("n_components", "largest_root", "largest_size", "n_inside")


def _need_field(u, what):
    need_cuda(u)
    if u.dtype != torch.float32:
        raise RuntimeError(f"laenerf_amd.{what}: field must be float32")
    need_contig(u)
    _check_shape(u.shape)


def label_components(u, threshold):
    """u: a CUDA fp32 contiguous tensor [nx,ny,nz] -> labels [nx,ny,nz] int32 on the same device; a numpy array -> uploaded, run on
    the device, a numpy int32 array.  A CPU tensor is an error (there is no CPU fallback).  No host read, capturable."""
    if isinstance(u, np.ndarray):
        return label_components(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda(), threshold).cpu().numpy()
    if not isinstance(u, torch.Tensor):
        raise TypeError("laenerf_amd.label_components: u must be a torch tensor or a numpy array")
    _need_field(u, "label_components")
    nx, ny, nz = u.shape
    labels = torch.empty(nx, ny, nz, dtype=torch.int32, device=u.device)
    check(_lib.load().lae_components_label(ptr(u), nx, ny, nz, float(threshold), ptr(labels), stream()), "components_label")
    return labels


def component_sizes(labels):
    """labels (label_components' output, a CUDA int32 tensor) -> (sizes [N] int32, stats [4] int32), both on the device"""
    need_cuda(labels)
    if labels.dtype != torch.int32:
        raise RuntimeError("laenerf_amd.component_sizes: labels must be int32")
    need_contig(labels)
    N = labels.numel()
    sizes = torch.empty(N, dtype=torch.int32, device=labels.device)
    stats = torch.empty(4, dtype=torch.int32, device=labels.device)
    check(_lib.load().lae_components_sizes(ptr(labels), N, ptr(sizes), ptr(stats), stream()), "components_sizes")
    return sizes, stats


def keep_rule(stats, largest=False, min_size=None, min_fraction=None):
    """the rule as the kernel's (min_size, keep_root), from stats (4 ints on the host), in Python integers: `largest` keeps the
    largest component alone; min_size keeps components of at least that many points; min_fraction=f those of at least
    ceil(f * largest_size) points.  Rules combine (a component must pass every one given); none given is a ValueError."""
    if not largest and min_size is None and min_fraction is None:
        raise ValueError("laenerf_amd.filter_components: give a rule (largest=True, min_size=n or min_fraction=f)")
    n_comp, largest_root, largest_size, _ = (int(x) for x in stats)
    ms = 0 if min_size is None else int(min_size)
    if min_fraction is not None:
        f = float(min_fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError("laenerf_amd.filter_components: min_fraction must be in [0, 1]")
        ms = max(ms, math.ceil(f * largest_size))
    ms = max(0, min(ms, 2 ** 31 - 1))
    return ms, (largest_root if largest and n_comp > 0 else -1)


def filter_components(u, threshold, largest=False, min_size=None, min_fraction=None, out=None, info=False):
    """-> (u_filtered, info dict).  Labels, counts, reads stats back (4 ints: the one host read), turns the rule into
    (min_size, keep_root) (keep_rule) and launches the filter.  out: a tensor like u to write into (u itself: in place).
    info dict: n_components, n_inside, largest_size, largest_root, min_size, keep_root; with info=True also n_kept, n_removed
    (components) and n_removed_points, which cost a second host read.  numpy in -> numpy out, like marching_cubes."""
    if isinstance(u, np.ndarray):
        if out is not None:
            raise ValueError("laenerf_amd.filter_components: out= goes with a device tensor")
        f, inf = filter_components(torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda(), threshold, largest, min_size,
                                   min_fraction, info=info)
        return f.cpu().numpy(), inf
    if not isinstance(u, torch.Tensor):
        raise TypeError("laenerf_amd.filter_components: u must be a torch tensor or a numpy array")
    _need_field(u, "filter_components")
    if not largest and min_size is None and min_fraction is None:
        raise ValueError("laenerf_amd.filter_components: give a rule (largest=True, min_size=n or min_fraction=f)")
    if out is None:
        out = torch.empty_like(u)
    else:
        need_cuda(out)
        need_contig(out)
        if out.dtype != torch.float32 or out.shape != u.shape:
            raise RuntimeError("laenerf_amd.filter_components: out must be a float32 tensor of u's shape")
    thr = float(threshold)
    labels = label_components(u, thr)
    sizes, stats = component_sizes(labels)
    st = stats.tolist()                                                     # the one host read
    ms, keep_root = keep_rule(st, largest, min_size, min_fraction)
    check(_lib.load().lae_components_filter(ptr(u), ptr(labels), ptr(sizes), u.numel(), thr, ms, keep_root, ptr(out), stream()),
          "components_filter")
    res = dict(zip(STATS, st), min_size=ms, keep_root=keep_root)
    if info:
        kept = (sizes >= max(ms, 1)) if keep_root < 0 else ((sizes >= max(ms, 1)) & (torch.arange(sizes.numel(), device=sizes.device) == keep_root))
        n_kept, pts = torch.stack([kept.sum(), sizes[kept].sum()]).tolist()
        res.update(n_kept=n_kept, n_removed=st[0] - n_kept, n_removed_points=st[3] - pts)
    return out, res


# ---------------------------------------------------------------------------------------------------------------------------
# the specification restated on the host: numpy for the inside test and the neighbour pairs, a Python union-find over the pairs

def components_numpy(u, threshold):
    """-> (labels [nx,ny,nz] int32, sizes [N] int32, stats [4] int32) as lae_components_label / lae_components_sizes define them"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    _check_shape(u.shape)
    inside = u > np.float32(threshold)
    N = u.size
    idx = np.arange(N, dtype=np.int64).reshape(u.shape)
    pairs = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        both = inside[tuple(lo)] & inside[tuple(hi)]
        pairs.append(np.stack([idx[tuple(lo)][both], idx[tuple(hi)][both]], 1))
    parent = list(range(N))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in np.concatenate(pairs).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:                                                        # the smaller index stays the root
            parent[max(ra, rb)] = min(ra, rb)
    flat = inside.reshape(-1)
    labels = np.full(N, -1, np.int32)
    for p in np.nonzero(flat)[0].tolist():
        labels[p] = find(p)
    sizes = np.bincount(labels[flat], minlength=N).astype(np.int32)
    roots = np.nonzero(sizes)[0]
    if len(roots):
        largest_size = int(sizes.max())
        stats = [len(roots), int(roots[sizes[roots] == largest_size][0]), largest_size, int(flat.sum())]
    else:
        stats = [0, -1, 0, 0]
    return labels.reshape(u.shape), sizes, np.array(stats, np.int32)


def filter_components_numpy(u, threshold, largest=False, min_size=None, min_fraction=None):
    """-> (u_filtered fp32, info dict) as filter_components defines them"""
    u = np.ascontiguousarray(u, dtype=np.float32)
    labels, sizes, stats = components_numpy(u, threshold)
    ms, keep_root = keep_rule(stats, largest, min_size, min_fraction)
    flat = labels.reshape(-1)
    inside = flat >= 0
    kept = np.zeros(flat.shape, bool)
    kept[inside] = sizes[flat[inside]] >= ms
    if keep_root >= 0:
        kept &= flat == keep_root
    out = u.copy().reshape(-1)
    out[inside & ~kept] = np.float32(threshold)
    return out.reshape(u.shape), dict(zip(STATS, (int(x) for x in stats)), min_size=ms, keep_root=keep_root)
