"""lae_sample_train_batch (ResidentImages.sample) against its numpy restatement, lae_get_rays and torch's blend."""
import numpy as np
import pytest
import torch

from gpu_util import DEV

pytestmark = pytest.mark.gpu

N_IMG, H, W = 5, 37, 29             # H * W = 1073: not a power of two


def _scene(C, dtype, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, size=(N_IMG, H, W, C), dtype=np.uint8)
    if dtype == torch.uint8:
        img = torch.from_numpy(u8)
    else:
        img = torch.from_numpy(rng.random((N_IMG, H, W, C), dtype=np.float32)).to(dtype)
    return img, S.lookat_poses(N_IMG, seed=seed), (31.5, 33.0, W / 2 + 0.3, H / 2 - 0.7)


def _as_f32(img):
    return img.float() / 255 if img.dtype == torch.uint8 else img.float()     # numpy's astype(float32) / 255


@pytest.mark.parametrize("mode", ["image", "all"])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
def test_batch_matches_restatement_get_rays_and_blend(mode, C, dtype):
    from laenerf_amd.data import ResidentImages, draw_background, draw_indices
    img, poses, intr = _scene(C, dtype)
    seed, step, n = 0x1234_5678_9ABC, 41, 3000
    d = ResidentImages.from_arrays(img, poses, intr, mode=mode, bg="random" if C == 4 else "white", seed=seed, device=DEV)
    b = d.sample(n, step=step)
    assert int(d.step.item()) == step + 1
    im, px = draw_indices(seed, step, n, N_IMG, H, W, mode)
    assert np.array_equal(b["inds"].cpu().numpy(), im * H * W + px)
    if mode == "image":
        assert len(set(im.tolist())) == 1
    # rays, nears, fars: lae_get_rays on the drawn pixels, one pose per ray
    P = d.poses[torch.from_numpy(im).to(DEV)].contiguous()
    from laenerf_amd import _lib
    ro = torch.empty(n, 1, 3, device=DEV); rd = torch.empty_like(ro)
    ne = torch.empty(n, 1, device=DEV); fa = torch.empty_like(ne)
    inds = torch.from_numpy(px).to(DEV).contiguous()
    _lib.check(_lib.load().lae_get_rays(_lib.ptr(P), n, *intr, H, W, _lib.ptr(inds), 1, 1, 0, 0.0, 0.0, _lib.ptr(ro), _lib.ptr(rd),
                                        _lib.ptr(d.aabb), d.min_near, _lib.ptr(ne), _lib.ptr(fa), _lib.stream()), "get_rays")
    for got, want in ((b["rays_o"], ro.view(n, 3)), (b["rays_d"], rd.view(n, 3)), (b["nears"], ne.view(n)), (b["fars"], fa.view(n))):
        assert torch.equal(got, want)
    # gt: torch's CPU expression on the same background
    pix = _as_f32(img).reshape(-1, C)[torch.from_numpy(im * H * W + px)]
    if C == 4:
        bg = torch.from_numpy(draw_background(seed, step, n))
        assert torch.equal(b["bg"].cpu(), bg)
        want = pix[:, :3] * pix[:, 3:] + bg * (1 - pix[:, 3:])
    else:
        assert b["bg"] == 1
        want = pix
    assert torch.equal(b["gt"].cpu(), want)


def test_white_background_with_alpha_and_linear():
    from laenerf_amd.data import ResidentImages, draw_indices
    img, poses, intr = _scene(4, torch.float32, seed=3)
    d = ResidentImages.from_arrays(img, poses, intr, bg="white", color_space="linear", seed=5, device=DEV)
    b = d.sample(2048, step=9)
    im, px = draw_indices(5, 9, 2048, N_IMG, H, W)
    pix = img.reshape(-1, 4)[torch.from_numpy(im * H * W + px)].double()
    rgb = torch.where(pix[:, :3] < 0.04045, pix[:, :3] / 12.92, ((pix[:, :3] + 0.055) / 1.055) ** 2.4)
    want = rgb * pix[:, 3:] + (1 - pix[:, 3:])
    assert torch.allclose(b["gt"].cpu().double(), want, rtol=1e-6, atol=1e-7)


def test_graph_replays_draw_fresh_batches():
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(4, torch.uint8)
    d = ResidentImages.from_arrays(img, poses, intr, seed=77, device=DEV)
    s, n = 1000, 4096
    eager = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.sample(n, step=s + i).items()} for i in range(3)]
    d.sample(n, step=0)                                      # buffers exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = d.sample(n)
    d.step.fill_(s)
    for i in range(3):
        g.replay()
        for k in ("rays_o", "rays_d", "nears", "fars", "gt", "bg", "inds"):
            assert torch.equal(out[k], eager[i][k]), (i, k)
    assert int(d.step.item()) == s + 3


def test_chi_square_of_2_20_draws():
    from laenerf_amd.data import ResidentImages
    img, poses, intr = _scene(4, torch.uint8)
    d = ResidentImages.from_arrays(img, poses, intr, mode="all", seed=2024, device=DEV)
    n = 1 << 20
    b = d.sample(n, step=3)
    inds = b["inds"].cpu().numpy()

    def chi2(counts):
        e = counts.sum() / counts.size
        return float(((counts - e) ** 2 / e).sum()), counts.size - 1

    for counts in (np.bincount(inds % (H * W), minlength=H * W), np.bincount(inds // (H * W), minlength=N_IMG),
                   np.bincount((b["bg"].cpu().numpy() * 64).astype(np.int64).ravel(), minlength=64)):
        x, dof = chi2(counts.astype(np.float64))
        assert x < dof + 6 * np.sqrt(2 * dof), (x, dof)           # 6 sigma of the chi-square distribution
