#!/usr/bin/env python3
"""Generate tests/golden/distort_case.npz: the reference's own eff_distloss (loss.py:29-76, unmodified, on the CPU in float64) on the
weights of every ray of the depth_sup_util compositing case.

Needs the reference checkout (LAE_REFERENCE, default /root/reference); the tests read only the emitted file.  Per ray of the case
that has samples, the float64 w, t, delta of the samples the forward uses (composite_depth_numpy(samples=True)) go to
eff_distloss(w[None], t[None], delta[None]) -- m = t, interval = deltas[:,0], the call the distortion term restates -- and the value
(one ray: its mean over rays is the ray's value) and its gradient with respect to w are recorded, concatenated in row order.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LAE_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))


def main():
    if not os.path.isdir(REF):
        sys.exit(f"make_golden_distort: no reference checkout at {REF}")
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(REF, "loss.py"))
    ref_loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_loss)
    from depth_sup_util import T_THRESH, build_case
    from laenerf_amd.raymarching.raymarching import composite_depth_numpy
    c = build_case()
    f = composite_depth_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], T_THRESH, samples=True)
    rows, values, counts, grads = [], [], [], []
    for n, (w, t, _) in sorted(f["samples"].items()):
        off = int(c["rays"][n, 1])
        delta = c["deltas"][off:off + len(w), 0].astype(np.float64)
        wt = torch.from_numpy(w[None].copy()).requires_grad_()
        loss = ref_loss.eff_distloss(wt, torch.from_numpy(t[None].copy()), torch.from_numpy(delta[None].copy()))
        loss.backward()
        rows.append(n); values.append(float(loss.detach())); counts.append(len(w)); grads.append(wt.grad[0].numpy())
    out = os.path.join(HERE, "distort_case.npz")
    np.savez(out, rows=np.array(rows, np.int64), value=np.array(values, np.float64), count=np.array(counts, np.int64),
             grad_w=np.concatenate(grads).astype(np.float64))
    print(out, len(rows), "rays", int(sum(counts)), "samples")


if __name__ == "__main__":
    main()
