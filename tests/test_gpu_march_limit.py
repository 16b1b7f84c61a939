"""lae_march_rays_train_limit (march_rays_train(..., m_limit=, capacity=)): a device truncation threshold gives exactly
what lae_march_rays_train gives with the same threshold on the host, in a buffer of any larger capacity."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, T, scene

pytestmark = pytest.mark.gpu


def _host_march(sc, o, d, nears, fars, bits, M, noises):
    from laenerf_amd.backend import raymarching_backend as B
    n = o.shape[0]
    xyzs, dirs, deltas = (torch.full((M, k), float("nan"), device=DEV) for k in (3, 3, 2))
    rays = torch.empty(n, 3, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    rows_end = torch.empty(1, dtype=torch.int32, device=DEV)
    B.march_rays_train(o, d, bits, sc["bound"], 0.0, 1024, n, sc["C"], 128, M, nears, fars, xyzs, dirs, deltas, rays, counter, noises,
                       rows_end)
    return xyzs, dirs, deltas, rays, counter, rows_end


@pytest.mark.parametrize("C,seed", [(1, 0), (2, 1)])
def test_device_threshold_equals_host_threshold(C, seed):
    from laenerf_amd.backend import raymarching_backend as B
    from laenerf_amd.raymarching import raymarching as rm
    sc = scene(C=C, bound=float(2 ** (C - 1)), n_rays=3000, seed=seed)
    rng = np.random.default_rng(seed)
    bits_np = sc["bits"].copy()
    bits_np &= rng.integers(0, 256, bits_np.shape, dtype=np.uint8) | rng.integers(0, 256, bits_np.shape, dtype=np.uint8)  # random holes
    o, d, nears, fars, bits = T(sc["o"]), T(sc["d"]), T(sc["nears"]), T(sc["fars"]), T(bits_np)
    noises = torch.rand(o.shape[0], device=DEV)
    n = o.shape[0]
    total = int(_host_march(sc, o, d, nears, fars, bits, n * 1024, noises)[4][0].item())
    assert total > 1000
    for M in (total // 3, total // 2 + 7, total, total + 513):
        h = _host_march(sc, o, d, nears, fars, bits, M, noises)
        for M_cap in (M, M + 1000):
            xyzs, dirs, deltas = (torch.full((M_cap, k), float("nan"), device=DEV) for k in (3, 3, 2))
            rays = torch.empty(n, 3, dtype=torch.int32, device=DEV)
            counter = torch.zeros(2, dtype=torch.int32, device=DEV)
            rows_end = torch.empty(1, dtype=torch.int32, device=DEV)
            m_limit = torch.tensor([M], dtype=torch.int32, device=DEV)
            B.march_rays_train_limit(o, d, bits, sc["bound"], 0.0, 1024, n, sc["C"], 128, M_cap, m_limit, nears, fars, xyzs, dirs, deltas,
                                     rays, counter, noises, rows_end)
            assert torch.equal(rays, h[3]) and torch.equal(counter, h[4]) and torch.equal(rows_end, h[5]), (M, M_cap)
            for a, b in ((xyzs, h[0]), (dirs, h[1]), (deltas, h[2])):
                assert torch.equal(a[:M], b), (M, M_cap)                 # rows [0, M), the tail [rows_end, M) zero in both
                assert (a[M:] == 0).all(), (M, M_cap)                     # rows [M, M_cap): zero-filled
    # the Python keyword path: same buffers as the Function with mean_count, without a host read
    counter_a = torch.zeros(2, dtype=torch.int32, device=DEV)
    counter_b = torch.zeros(2, dtype=torch.int32, device=DEV)
    M = (total // 2) // 128 * 128
    a = rm.march_rays_train(o, d, sc["bound"], bits, sc["C"], 128, nears, fars, counter_a, M - 128, False, 128, False, 0, 1024)
    b = rm.march_rays_train(o, d, sc["bound"], bits, sc["C"], 128, nears, fars, counter_b, perturb=False, dt_gamma=0, max_steps=1024,
                            m_limit=torch.tensor([M], dtype=torch.int32, device=DEV), capacity=M + 256)
    assert torch.equal(counter_a, counter_b) and torch.equal(a[3], b[3]) and torch.equal(a[3].rows_end, b[3].rows_end)
    for x, y in zip(a[:3], b[:3]):
        assert x.shape[0] == M and y.shape[0] == M + 256
        assert torch.equal(x, y[:M]) and (y[M:] == 0).all()


def test_threshold_change_in_one_captured_graph():
    from laenerf_amd.raymarching import raymarching as rm
    sc = scene(C=1, n_rays=2048, seed=5)
    o, d, nears, fars, bits = T(sc["o"]), T(sc["d"]), T(sc["nears"]), T(sc["fars"]), T(sc["bits"])
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    m_limit = torch.tensor([4096], dtype=torch.int32, device=DEV)
    rm.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, counter, perturb=False, m_limit=m_limit, capacity=1 << 16)   # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        counter.zero_()
        out = rm.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, counter, perturb=False, m_limit=m_limit, capacity=1 << 16)
    for M in (2048, 29952, 1 << 16):
        m_limit.fill_(M)
        g.replay()
        c2 = torch.zeros(2, dtype=torch.int32, device=DEV)
        ref = rm.march_rays_train(o, d, 1.0, bits, 1, 128, nears, fars, c2, M - 128, False, 128, False, 0, 1024)
        assert torch.equal(out[3], ref[3]) and torch.equal(counter, c2)
        assert torch.equal(out[0][:M], ref[0]) and (out[0][M:] == 0).all()
