"""Recipe for tests/golden/error_map_rays.npz: the reference's own `get_rays(..., error_map=...)` (nerf/utils.py:112-124) on
the CPU with fixed torch seeds.  Runs only where the reference tree exists (LAE_REFERENCE, as make_golden.py); the tests read
only the .npz.

    python tests/golden/make_golden_error_map.py

Recorded per case: poses [B,4,4], cfg (H, W, N), intrinsics, the map [B,16384], inds [B,N] and inds_coarse [B,N].  The maps
hold zeros, a hot region and random weights on a coarse grid (it compresses), so the drawn cells cover both rare and common cells; H x W is below and above
128 x 128 in each direction."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import look_at_poses, reference_get_rays, save  # noqa: E402


def main():
    get_rays = reference_get_rays()
    out = {}
    poses = torch.from_numpy(look_at_poses(3, 3.2, seed=9))
    for tag, (B, H, W, N) in (("small", (2, 37, 53, 256)), ("wide", (1, 300, 200, 1024)), ("square", (3, 128, 128, 512)),
                              ("odd", (1, 801, 97, 2048))):
        torch.manual_seed(31)
        emap = torch.randint(0, 8, (B, 128 * 128)).float() / 4   # weights 0 .. 1.75 (an eighth of them 0: never drawn)
        emap[:, 4000:4100] = 50.0                               # a hot region
        intr = (0.9 * W, 0.9 * W, W / 2, H / 2)
        torch.manual_seed(47)
        res = get_rays(poses[:B], np.array(intr, np.float32), H, W, N, error_map=emap)
        out[f"{tag}_poses"] = poses[:B].numpy()
        out[f"{tag}_cfg"] = np.array([H, W, N], np.int64)
        out[f"{tag}_intr"] = np.array(intr, np.float32)
        out[f"{tag}_map"] = emap.numpy()
        out[f"{tag}_inds"] = res["inds"].contiguous().numpy()
        out[f"{tag}_inds_coarse"] = res["inds_coarse"].numpy()
    save("error_map_rays", **out)


if __name__ == "__main__":
    main()
