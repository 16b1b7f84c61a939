"""The hand-built compositing case of the depth-supervision tests (test_depth_sup_cpu.py, test_gpu_depth_sup.py): a `rays` table in
the contiguous ray-id-order layout of march_rays_train with a rows_end, chosen so that every path of the one-wave-per-ray kernels
is taken."""
import numpy as np

T_THRESH = 1e-4
SEED = 20
#        num_steps, kind
RAYS = [(0, "plain"), (1, "plain"), (63, "plain"), (64, "plain"), (65, "plain"), (128, "plain"), (129, "plain"), (200, "plain"),
        (100, "stop_first"),      # dense from the start: the early stop falls into the first pass of 64 samples
        (150, "stop_second"),     # thin for 70 samples, then dense: the stop falls into the second pass
        (90, "stop_lane63"),      # empty up to sample 62, opaque at sample 63: the stop is lane 63 of the first pass
        (5, "plain"),
        (50, "dropped")]          # offset + num_steps > M: the ray is dropped (march_rays_train's truncated last ray)
TAIL_ROWS = 37                    # rows [rows_end, M) no ray owns


def build_case(seed=SEED):
    """-> dict of float32 / int32 numpy arrays: sigmas [M], rgbs [M,3], deltas [M,2], rays [N,3] (index, offset, num_steps; the
    indices a permutation of the ray ids), rows_end, M, N, nears, fars [N], bg_rays [N,3], kinds"""
    rng = np.random.default_rng(seed)
    N = len(RAYS)
    assert N % 4 != 0
    owned = sum(s for s, k in RAYS if k != "dropped")
    M = owned + TAIL_ROWS
    sig = np.zeros(M, np.float32)
    index = rng.permutation(N).astype(np.int32)
    rays = np.zeros((N, 3), np.int32)
    off = 0
    for n, (steps, kind) in enumerate(RAYS):
        rays[n] = (index[n], off, steps)
        if kind == "dropped":
            assert off == owned and off + steps > M
            continue
        k = np.arange(steps)
        if kind == "plain":
            s = rng.uniform(0, 2.0, steps)
        elif kind == "stop_first":
            s = rng.uniform(0, 60.0, steps)
        elif kind == "stop_second":
            s = np.where(k < 70, rng.uniform(0, 2.0, steps), rng.uniform(0, 100.0, steps))
        else:
            s = np.where(k < 63, 0.5, np.where(k == 63, 2000.0, rng.uniform(0, 2.0, steps)))
        sig[off:off + steps] = s
        off += steps
    sig[owned:] = rng.uniform(0, 2.0, TAIL_ROWS)                      # whatever lies in the tail must not matter
    deltas = np.stack([rng.uniform(0.005, 0.02, M), rng.uniform(0.005, 0.03, M)], -1).astype(np.float32)
    nears = rng.uniform(0.2, 1.0, N).astype(np.float32)
    return dict(sigmas=sig, rgbs=rng.uniform(0, 1, (M, 3)).astype(np.float32), deltas=deltas, rays=rays, rows_end=owned, M=M, N=N,
                nears=nears, fars=(nears + rng.uniform(1.0, 3.0, N)).astype(np.float32),
                bg_rays=rng.uniform(0, 1, (N, 3)).astype(np.float32), kinds=[k for _, k in RAYS])


def build_grads(N, seed=SEED + 1):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(N).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32),
            rng.standard_normal(N).astype(np.float32))
