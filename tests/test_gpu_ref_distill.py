"""The Ref-NPR distillation stage (laenerf_amd/editing/ref_distill.py) on the synthetic sphere scene of test_gpu_rayreg.py's end-to-end
case: three 96 x 96 RGBA views, the template painted on view 0 (which registers onto itself), views 1 and 2 registered to its cloud.
`build_ref_distill_data` against `ref_distill_numpy` (pinned to the reference's loop by test_ref_distill_cpu.py), the background rule
of a skipped view, and `distill_ref_npr` through the captured Trainer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import DEV, N, T
from rayreg_util import MIN_TV, REG_DIST
from test_gpu_distill import REF_HALF_TOL          # the distill tests' bound on the palette network's colours (fp16 roundings in [0, 1])

pytestmark = pytest.mark.gpu

H = W = 96


@pytest.fixture(scope="module")
def scene():
    from test_gpu_frame import make
    from test_gpu_rayreg import poses_looking_at_origin
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.editing import LAENeRF, extract_ref_cloud, register_views
    net, r = make(bound=1, seed=2)
    intr = np.array([133.3, 133.3, 48.0, 48.0], np.float32)
    P = poses_looking_at_origin(3, 3.2, seed=1)
    P[1, :3, 3] = P[0, :3, 3] + 0.3 * P[0, :3, 0]
    P[1, :3, :3] = P[0, :3, :3]
    poses = T(P)
    r.density_scale = 30.0
    g = torch.Generator().manual_seed(3)
    images = torch.rand(3, H, W, 4, generator=g).to(DEV)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    inside = (((yy - 48) ** 2 + (xx - 48) ** 2) < 30 ** 2).to(DEV)
    images[..., 3] = torch.where(inside, images[..., 3] * 0.5 + 0.5, torch.zeros_like(images[..., 3]))
    painted = torch.rand(H, W, 4, generator=g).to(DEV)
    torch.manual_seed(11)
    cloud = extract_ref_cloud(r, poses[0], intr, H, W, painted, images[0, ..., 3], n_jitter=2)
    torch.manual_seed(11)
    views, skipped = register_views(r, poses, intr, H, W, images, cloud, REG_DIST, MIN_TV, batch_views=2)
    assert skipped == [] and len(views) == 3
    params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(0)
    enc = LAENeRF(params, dir_encoding="sphere_harmonics").to(DEV)
    data = ResidentImages(images, poses, tuple(float(v) for v in intr), device=DEV)
    return SimpleNamespace(net=net, r=r, poses=poses, intr=intr, images=images, cloud=cloud, views=views, enc=enc, data=data, inside=inside)


def _restated(s, views, dtype):
    """ref_distill_numpy on rows packed here, the colours from one un-chunked call of the network"""
    from laenerf_amd.editing import DistillSet, pack_ref_rows, ref_distill_numpy
    rows = {k: t.numpy() for k, t in pack_ref_rows(views, 3, H * W).items()}
    ds = DistillSet.from_views(views, [], 3, device=DEV)
    s.enc.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        colours = s.enc(ds.x_term, d=ds.dirs).float()
    s.enc.train()
    assert colours.min() >= 0 and colours.max() <= 1
    return ref_distill_numpy(N(s.images), rows["reg_img"], rows["reg_pix"], rows["reg_rgb"], rows["reg_w"], N(ds.img_idx), N(ds.pix),
                             N(colours), N(ds.depth), dtype=dtype), rows, ds


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_build_against_the_restatement(scene, dtype):
    from laenerf_amd.editing import build_ref_distill_data
    s = scene
    before = s.data.images.clone()
    out = build_ref_distill_data(s.data, s.views, s.enc, dtype=dtype)
    assert out is not s.data and torch.equal(s.data.images, before) and s.data.pixel_weights is None       # `data` is left untouched
    assert torch.equal(out.poses, s.data.poses) and out.intrinsics == s.data.intrinsics and out.bg == s.data.bg and out.mode == s.data.mode
    assert (out.seed, out.bound, out.C) == (s.data.seed, s.data.bound, 4)
    np_dt = np.float16 if dtype == torch.float16 else np.float32
    (im, w, s2, d), rows, ds = _restated(s, s.views, np_dt)
    bits = np.uint16 if dtype == torch.float16 else np.uint32
    got = {k: getattr(out, k).cpu().numpy() for k in ("images", "pixel_weights", "second_target", "depths")}
    assert got["images"].dtype == got["pixel_weights"].dtype == got["second_target"].dtype == np_dt and got["depths"].dtype == np.float32
    assert np.array_equal(got["images"].view(bits), im.view(bits))                                         # copies and single roundings
    assert np.array_equal(got["pixel_weights"].view(bits), w.view(bits))
    assert np.array_equal(got["depths"].view(np.uint32), d.view(np.uint32))
    err = np.abs(got["second_target"].astype(np.float32) - s2.astype(np.float32)).max()
    print(f"second target against the restatement ({np_dt.__name__}): max |diff| {err:.3e} (bound {REF_HALF_TOL})")
    assert err <= REF_HALF_TOL
    assert np.array_equal(got["second_target"][..., 3].view(bits), s2[..., 3].view(bits))                  # its alpha is a copy
    # what the scene holds: registered rows on every view, weights above 1 nowhere but at registered pixels, depth at the K pixels
    K = int(s.inside.sum())
    assert ds.R == 3 * K and rows["reg_img"].size > K and (got["depths"] > 0).sum() == (N(ds.depth) > 0).sum()
    a = N(s.images)[..., 3]
    off = np.ones((3, H * W), bool)
    off[rows["reg_img"], rows["reg_pix"]] = False
    assert np.array_equal(got["pixel_weights"].reshape(3, -1)[off], (np.float32(1) - a).astype(np_dt).reshape(3, -1)[off])
    assert not got["images"][..., :3].reshape(3, -1, 3)[off].any() and not got["second_target"][~N(s.inside)[None].repeat(3, 0)].any()


def test_a_skipped_view_keeps_the_background_rule(scene):
    from laenerf_amd.editing import build_ref_distill_data, register_views
    from laenerf_amd.data import ResidentImages
    s = scene
    blank = s.images.clone()
    blank[1, ..., 3] = 0
    torch.manual_seed(11)
    views, skipped = register_views(s.r, s.poses, s.intr, H, W, blank, s.cloud, REG_DIST, MIN_TV, batch_views=2)
    assert skipped == [1] and [v["pose_idx"] for v in views] == [0, 2]
    data = ResidentImages(blank, s.poses, tuple(float(v) for v in s.intr), device=DEV)
    out = build_ref_distill_data(data, views, s.enc)
    assert not out.images[1].any() and (out.pixel_weights[1] == 1).all() and not out.second_target[1].any() and not out.depths[1].any()
    assert out.images[0, ..., :3].any() and out.second_target[2].any() and out.depths[0].any()
    # three-channel data: a = 1 everywhere
    rgb = ResidentImages(s.images[..., :3].contiguous(), s.poses, tuple(float(v) for v in s.intr), device=DEV)
    o3 = build_ref_distill_data(rgb, s.views, s.enc)
    assert (o3.images[..., 3] == 1).all() and o3.bg == "white" and (o3.pixel_weights >= 0).all()
    assert (o3.second_target[..., 3][s.inside[None].expand(3, -1, -1)] == 1).all()


def _optimizer(net):
    from laenerf_amd.optim import FusedAdam
    return FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, device_lr=True)


def test_distill_ref_npr_runs_captured_and_lowers_the_loss(scene):
    """208 steps (distill_steps(200)): every history finite, at least one captured group, the total loss of the last group below the
    first group's mean"""
    from laenerf_amd.editing import distill_ref_npr
    s = scene
    torch.manual_seed(7)
    distilled, tr = distill_ref_npr(s.r, _optimizer(s.net), s.data, s.enc, s.views, steps=200, trainer_kw=dict(num_rays=2048, seed=1))
    s.r.eval(); s.net.eval()
    assert tr.global_step == 208 and tr.captures >= 1
    assert tr.pixel_weights and tr.second_weight == 0.5 and tr.depth_weight == 1e-3 and tr.data is distilled
    hist = {name: getattr(tr, name)() for name in ("losses", "second_losses", "depth_losses")}
    for name, h in hist.items():
        assert h.shape == (208,) and np.isfinite(h).all(), name
    first, last = hist["losses"][:16].mean(), hist["losses"][-16:].mean()
    print(f"distill_ref_npr: total loss first group {first:.5f}, last group {last:.5f}; second term {hist['second_losses'][:16].mean():.5f} -> "
          f"{hist['second_losses'][-16:].mean():.5f}; depth term {hist['depth_losses'][:16].mean():.4f} -> {hist['depth_losses'][-16:].mean():.4f}; "
          f"captures {tr.captures}")
    assert last < first
