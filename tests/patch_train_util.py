"""Shared by test_gpu_patch_train.py: the LPIPS chain written with torch operators, the head-gradient kernel called through the C ABI
on arbitrary layer shapes, and patch trainers on the scene of test_gpu_trainer.py at 64 x 64."""
import ctypes

import numpy as np
import torch

from gpu_util import DEV

ITERS, LR, RAYS, P = 400, 1e-2, 2048, 32


# ---------------------------------------------------------------------------------------------------------------- torch chains
def torch_pack(pred, gt, P, normalize):
    """lae_patch_pack with torch operators (shift and scale as tensors: a true division, as the kernel's)"""
    from laenerf_amd.metrics import LPIPS_SCALE, LPIPS_SHIFT
    shift = torch.tensor(LPIPS_SHIFT, dtype=pred.dtype, device=pred.device).view(1, 1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=pred.dtype, device=pred.device).view(1, 1, 3, 1, 1)
    v = torch.stack([gt.reshape(-1, P, P, 3), pred.reshape(-1, P, P, 3)], 1).permute(0, 1, 4, 2, 3)
    u = 2 * v - 1 if normalize else v
    return ((u - shift) / scale).reshape(-1, 3, P, P)


def torch_head(feats, lins):
    """lpips' normalize_tensor, NetLinLayer, spatial_average and the sum over the layers in the features' dtype -> [B]"""
    total = 0
    for f, w in zip(feats, lins):
        f0, f1 = f[0::2], f[1::2]
        n0 = torch.sqrt((f0 * f0).sum(1, keepdim=True))
        n1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
        d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
        total = total + (d * w.to(f.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def torch_chain(lp, pred, gt, P, normalize, dtype, device):
    """mean LPIPS over the patches with torch operators only (torch pack, trunk, torch head) in `dtype` on `device` -> (value,
    gradient on pred)"""
    import copy
    trunk = copy.deepcopy(lp.trunk).to(device=device, dtype=dtype)
    lins = [w.detach().to(device=device, dtype=dtype) for w in lp.lins]
    pred = pred.detach().to(device=device, dtype=dtype).requires_grad_(True)
    h = torch_pack(pred, gt.detach().to(device=device, dtype=dtype), P, normalize)
    feats = []
    with torch.autocast("cuda", enabled=False):
        for i, layer in enumerate(trunk):
            h = layer(h)
            if i in (1, 4, 7, 9, 11):
                feats.append(h)
    val = torch_head(feats, lins).mean()
    val.backward()
    return val.detach(), pred.grad.detach()


# ---------------------------------------------------------------------------------------------------------------- the head's gradient
def head_grad_abi(feats, weights, gout, both):
    """lae_lpips_head_grad on any n_layers <= 5 layers: feats fp32 [2B, C, hw] device tensors -> fp32 gradients (buffers prefilled
    with NaN: every element must be written)"""
    from laenerf_amd import _lib
    n = len(feats)
    grads = [torch.full_like(f, float("nan")) for f in feats]
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    _lib.check(_lib.load().lae_lpips_head_grad(n, arr(feats), arr(weights), (ctypes.c_uint32 * n)(*[f.shape[1] for f in feats]),
                                               (ctypes.c_uint32 * n)(*[f.shape[2] for f in feats]), feats[0].shape[0] // 2,
                                               _lib.ptr(gout), arr(grads), int(both), _lib.stream()), "lpips_head_grad")
    return grads


# ---------------------------------------------------------------------------------------------------------------- trainers
def images(n=6, H=64, W=64, seed=0):
    from laenerf_amd import synthetic as S
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((n, H, W)) < 0.5, 255, img[..., 3])
    focal = 0.5 * W / np.tan(0.5 * 0.69)
    return img, S.lookat_poses(n, seed=seed), (focal, focal, W / 2, H / 2)


def setup(net_seed=0, device_lr=True):
    from laenerf_amd.data import ResidentImages
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(net_seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    r = NeRFRenderer(net, bound=1).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(LR), betas=(0.9, 0.99), eps=1e-15, device_lr=device_lr)
    img, poses, intr = images()
    return r, opt, ResidentImages.from_arrays(img, poses, intr, device=DEV)


_LPIPS = []


def lpips():
    """LPIPS.random(0) on the device, built once"""
    if not _LPIPS:
        from laenerf_amd.metrics import LPIPS
        _LPIPS.append(LPIPS.random(0, device=DEV))
    return _LPIPS[0]


def make_trainer(net_seed=0, torch_seed=7, seed=1, graph=True, **kw):
    from laenerf_amd.trainer import Trainer
    r, opt, data = setup(net_seed)
    torch.manual_seed(torch_seed)
    kw.setdefault("patch_size", P)
    if kw["patch_size"] != 1:
        kw.setdefault("lpips", lpips())
    return Trainer(r, opt, data, ITERS, LR, num_rays=RAYS, seed=seed, graph=graph, capacity="bucket", **kw)


def state(tr):
    r, opt = tr.r, tr.opt
    out = [p.detach().clone() for p, *_ in opt.items]
    out += [m.clone() for _, m, *_ in opt.items] + [v.clone() for _, _, v, *_ in opt.items]
    out += [r.density_grid.clone(), r.density_bitfield.clone(), opt.dev_state.clone(), r.step_counter.clone(), tr.data.step.clone()]
    if tr.ema is not None:
        out += [t.clone() for t in tr.ema.shadow_params]
    return out


def assert_same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i
