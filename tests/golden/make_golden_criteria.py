#!/usr/bin/env python3
"""Generate tests/golden/criteria.npz: the reference's own huber_loss(delta=0.1, reduction='none') and mape_loss(reduction='none')
(loss.py:7-26, unmodified, on CPU float32 tensors) on a few hundred elements in [0, 1].

Needs the reference checkout (LAE_REFERENCE, default /root/reference); the tests read only the emitted file.  The elements hold, beside
random pairs, the cases the criteria branch on: pred == target, |pred - target| equal to the float32 value of delta on either side
(pairs for which the float32 subtraction is exact), and target == 0.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("LAE_REFERENCE", "/root/reference")
DELTA = 0.1


def main():
    if not os.path.isdir(REF):
        sys.exit(f"make_golden_criteria: no reference checkout at {REF}")
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(REF, "loss.py"))
    ref_loss = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_loss)
    rng = np.random.default_rng(41)
    f32 = np.float32
    d = f32(DELTA)
    pred, target = rng.uniform(0, 1, 256).astype(f32), rng.uniform(0, 1, 256).astype(f32)
    close = rng.uniform(0, 1, 64).astype(f32)                                  # both Huber branches near the knee
    pred = np.concatenate([pred, (close + rng.uniform(-0.2, 0.2, 64).astype(f32)).clip(0, 1).astype(f32)])
    target = np.concatenate([target, close])
    same = rng.uniform(0, 1, 16).astype(f32)                                   # pred == target
    pred, target = np.concatenate([pred, same]), np.concatenate([target, same])
    t = rng.uniform(0, 0.85, 4096).astype(f32)                                 # |e| == float32(delta), exactly, on either side
    up = (t + d).astype(f32)
    keep = (up - t).astype(f32) == d
    knee_t, knee_p = t[keep][:16], up[keep][:16]
    assert knee_t.size == 16
    pred, target = np.concatenate([pred, knee_p, knee_t]), np.concatenate([target, knee_t, knee_p])
    zero_p = rng.uniform(0, 1, 16).astype(f32)                                 # target == 0 (the MAPE floor), one of them with pred == 0
    zero_p[0] = 0
    pred, target = np.concatenate([pred, zero_p]), np.concatenate([target, np.zeros(16, f32)])
    p, g = torch.from_numpy(pred), torch.from_numpy(target)
    huber = ref_loss.huber_loss(p, g, delta=DELTA, reduction="none").numpy()
    mape = ref_loss.mape_loss(p, g, reduction="none").numpy()
    assert huber.dtype == np.float32 and mape.dtype == np.float32
    out = os.path.join(HERE, "criteria.npz")
    np.savez(out, pred=pred, target=target, huber=huber, mape=mape, delta=np.float64(DELTA))
    print(out, pred.size, "elements,", int((pred == target).sum()), "equal,", int((np.abs(pred - target) == d).sum()), "at the knee,",
          int((target == 0).sum()), "with target 0")


if __name__ == "__main__":
    main()
