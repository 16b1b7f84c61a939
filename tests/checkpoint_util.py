"""Shared by test_gpu_checkpoint.py: the scene of test_gpu_trainer.py (6 RGBA images of 48 x 40, log2_hashmap_size=16, 2048 rays),
trainers on it in the configurations the checkpoint tests use, and the comparison of two trainers' complete state."""
import numpy as np
import torch

from gpu_util import DEV

ITERS, LR, RAYS = 400, 1e-2, 2048

# the Trainer arguments of each configuration (graph=True, capacity='bucket' unless the test says otherwise)
CONFIGS = {
    "plain": {},
    "ema": {"error_map": "ema", "ema_decay": 0.95, "epoch_len": 5},      # several gated EMA updates on either side of a save
    "depth": {"depth_weight": 0.1, "distort_weight": 0.01},
}


def images(n=6, H=48, W=40, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((n, H, W)) < 0.5, 255, img[..., 3])
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    return img, S.lookat_poses(n, seed=seed), (focal, focal, W / 2, H / 2)


def depth_plane(n, H, W):
    """a random depth plane with 30 % unsupervised pixels (test_gpu_depth_sup.py's)"""
    rng = np.random.default_rng(12)
    plane = rng.uniform(2.0, 4.0, (n, H, W)).astype(np.float16)
    plane[rng.random(plane.shape) < 0.3] = 0
    return plane


def setup(net_seed=0, log2_hashmap_size=16, depth=False):
    """fresh network (drawn from net_seed), renderer, optimizer and images"""
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(net_seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=log2_hashmap_size).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=True)
    img, poses, intr = images()
    data = ResidentImages.from_arrays(img, poses, intr, device=DEV)
    if depth:
        data.set_depths(depth_plane(data.n_img, data.H, data.W))
    return r, opt, data


def make_trainer(config="plain", net_seed=0, torch_seed=7, seed=1, graph=True, num_rays=RAYS, log2_hashmap_size=16):
    """torch.manual_seed(torch_seed) (after the network was drawn), then a Trainer built with `seed`"""
    from laenerf_amd.trainer import Trainer
    kw = CONFIGS[config]
    r, opt, data = setup(net_seed, log2_hashmap_size, depth="depth_weight" in kw)
    torch.manual_seed(torch_seed)
    return Trainer(r, opt, data, ITERS, LR, num_rays=num_rays, seed=seed, graph=graph, capacity="bucket", **kw)


def fresh_for_resume(config="plain", graph=True, **kw):
    """a trainer that shares nothing with the saved run by accident: another network seed, another torch seed, another sampler seed"""
    return make_trainer(config, net_seed=1234, torch_seed=4321, seed=99, graph=graph, **kw)


def tensors(tr):
    """every tensor of a trainer's state, named, cloned"""
    r, opt = tr.r, tr.opt
    out = {}
    for i, (p, m, v, *_) in enumerate(opt.items):
        out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach().clone(), m.clone(), v.clone()
    out["density_grid"], out["density_bitfield"] = r.density_grid.clone(), r.density_bitfield.clone()
    out["step_counter"], out["words"], out["data_step"] = r.step_counter.clone(), opt.dev_state.clone(), tr.data.step.clone()
    if tr.data.error_map is not None:
        out["error_map"] = tr.data.error_map.clone()
    if tr.ema is not None:
        for i, t in enumerate(tr.ema.shadow_params):
            out[f"ema{i}"] = t.clone()
        out["ema_count"] = tr.ema.device_count().clone()
    return out


def scalars(tr):
    r = tr.r
    return {"mean_count": r.mean_count, "mean_density": r.mean_density, "iter_density": r.iter_density, "local_step": r.local_step,
            "global_step": tr.global_step, "seed": tr.data.seed, "steps_skipped": tr.steps_skipped}


def snapshot(tr):
    return tensors(tr), scalars(tr), torch.cuda.get_rng_state(DEV).clone()


def assert_same_state(a, b):
    """a, b: trainers or snapshot()s; torch.equal on every tensor, == on every scalar"""
    ta, sa = (tensors(a), scalars(a)) if not isinstance(a, tuple) else a[:2]
    tb, sb = (tensors(b), scalars(b)) if not isinstance(b, tuple) else b[:2]
    assert ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert sa == sb


def assert_same_tail(full, resumed, m):
    """the resumed trainer's per-step records against the last m of the uninterrupted run's"""
    for name in type(full).RECORDS:                       # every per-step record the Trainer keeps
        a, c = getattr(full, name)(), getattr(resumed, name)()
        if a.size == 0:
            assert c.size == 0, name
            continue
        assert c.shape == (m,) and np.isfinite(c).all(), name
        assert np.array_equal(c, a[-m:]), name
