#!/usr/bin/env python3
"""Generate tests/golden/rayreg_case.npz: the reference's own get_ref_supervision (editing/single_view_edit_dataset.py, unmodified,
on the CPU in fp32) on a small surface cloud.

Needs the reference checkout (LAE_REFERENCE, default /root/reference); the tests read only the emitted file.  The module imports
packages that are not installed (icecream, cv2, torchvision, the dataset classes), so the one function is cut out of the file's
syntax tree and executed with `th` = torch; it does not use `self`.  `.cuda()` is made the identity for the call.  The inputs are
drawn by tests/rayreg_util.surface_case from the recorded seed; the file stores the seed, the shape, the scalars, and the
reference's unclamped min_dist, mask_dist, target and target_weights.

The seed is the first of rayreg_util.GOLDEN_SEEDS for which, in float64, no row's nearest distance lies within relative 2e-6 of
reg_dist or radius and every best / second-best gap exceeds relative 4e-6: the tests ask for the reference's mask and indices
exactly from fp32 kernels, so the fixture must not hinge on a rounding.  The choice reads the inputs only; the smaller of the two
margins is stored.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LAE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, ".."))


def reference_function():
    path = os.path.join(REF, "editing", "single_view_edit_dataset.py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SingleViewEditDataset")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "get_ref_supervision")
    scope = {"th": torch, "torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), scope)
    return scope["get_ref_supervision"]


def main():
    if not os.path.isdir(REF):
        sys.exit(f"make_golden_rayreg: no reference checkout at {REF}")
    from rayreg_util import GAP_MARGIN, GOLDEN_SEEDS, GOLDEN_SHAPE, MIN_TV, RADIUS, REG_DIST, THRESHOLD_MARGIN, brute_force, separation, surface_case
    M, n = GOLDEN_SHAPE
    for seed in GOLDEN_SEEDS:
        ref_x, ref_rgb, ref_dirs, x, dirs = surface_case(M, n, seed)
        best, second, _ = brute_force(ref_x, x)
        thr, gap = separation(best, second)
        if thr > THRESHOLD_MARGIN and gap > GAP_MARGIN:
            break
    else:
        sys.exit("make_golden_rayreg: no seed is clear of the thresholds")
    print("seed", seed, "threshold margin", thr, "gap margin", gap)
    fn = reference_function()
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        t = torch.from_numpy
        min_dist, mask_dist, target, target_weights = fn(None, t(x), t(ref_x), t(ref_rgb), REG_DIST, ref_dirs=t(ref_dirs), dirs=t(dirs))
    finally:
        torch.Tensor.cuda = cuda
    target_weights = torch.clamp_min(target_weights, 0)                      # the caller's line :226
    print("registered", mask_dist[0].numel(), "of", n, "weights in", float(target_weights.min()), float(target_weights.max()))
    out = {"seed": np.int64(seed), "shape": np.array(GOLDEN_SHAPE, np.int64), "margin": np.float64(min(thr, gap)),
           "reg_dist": np.float64(REG_DIST), "radius": np.float64(RADIUS), "min_tv_factor": np.float64(MIN_TV),
           "min_dist": min_dist.numpy().astype(np.float32), "mask_dist": mask_dist[0].numpy().astype(np.int64),
           "target": target.numpy().astype(np.float32), "target_weights": target_weights.numpy().astype(np.float32)}
    path = os.path.join(HERE, "rayreg_case.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
