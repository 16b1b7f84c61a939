"""Scoring a trained NeRF on held-out views: PSNR, LPIPS (alex, v0.1), LAENeRF's masked MSE, uint8 test images.

The reference ends training with `trainer.evaluate(test_loader)` and `trainer.test(test_loader)` (main_nerf.py:201-219,
258-264): every view is rendered with the EMA weights, scored by PSNRMeter and LPIPSMeter(net='alex') (nerf/utils.py:240-247,
main_nerf.py:203, 242) and written as uint8 PNGs; LAENeRF's GUI adds `eval_masked` (nerf/gui.py:853-947), the MSE outside an
edit mask.  Here each rendered view goes through ONE kernel (`lae_eval_view`, csrc/evaluate.hip) that reads the render and
the ground truth in its storage dtype once and writes what is asked: the squared error into a per-view device slot (fp64, fixed
order: the whole split needs one host read), the masked squared error, uint8 rgb / depth and the LPIPS input.  LPIPS's AlexNet
trunk is torch modules on MIOpen (plumbing, like the VGG of editing/style_network.py); its distance head over all five layers
and a batch of view pairs is ONE launch (`lae_lpips_head`).

    lp = load_lpips_alex("alexnet-owt-7be5be79.pth", "alex.pth")     # torchvision trunk + the lpips package's v0.1 heads
    res = trainer.evaluate_one_epoch(test_data, lpips=lp, masks=load_masks("scene", "test"))

A result without ground truth -- a recolored, stylized or distilled NeRF -- is scored by its view consistency instead (the
reference's scripts/eval/consistency_metrics.py): `trainer.evaluate_consistency(test_data, step=1 | 7, frames=...)` warps frame i
onto frame i + step through the model's own depth, ONE gather kernel per pair (`lae_consistency_pair`), and reports the masked
squared error and the LPIPS of the warped frame against the target; `consistency_numpy` restates the kernel in float64.

Nothing is downloaded: the weights come from files (or dicts) the user already has.  `LPIPS.random(seed)` builds seeded
weights for tests and benchmarks.  Parity with the lpips package itself is pinned only by a restatement (tests/lpips_util.py):
neither the package nor its pretrained weights were available to test against.
"""
import contextlib
import ctypes
import json
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr, stream

__all__ = ["LPIPS", "alexnet_trunk", "load_lpips_alex", "load_masks", "eval_view", "eval_view_numpy", "psnr_from_sse",
           "consistency_pair", "consistency_numpy", "lpips_head", "lpips_head_numpy", "lpips_head_grad_numpy", "patch_pack_numpy", "ALEX_CHANNELS", "ALEX_TAPS", "LPIPS_SHIFT", "LPIPS_SCALE", "EVAL_SCRATCH_DOUBLES", "CONSISTENCY_SCRATCH_DOUBLES",
           "ssim", "ssim_numpy", "ssim_grad_numpy", "ssim_scratch_doubles", "SSIM_TILE_H", "SSIM_TILE_W", "SSIM_MINMAX_BLOCKS"]

ALEX_CHANNELS = (64, 192, 384, 256, 256)
ALEX_TAPS = (1, 4, 7, 9, 11)                  # relu1..relu5 of torchvision's alexnet().features (lpips' pretrained alexnet slices)
ALEX_CONVS = {0: (64, 3, 11), 3: (192, 64, 5), 6: (384, 192, 3), 8: (256, 384, 3), 10: (256, 256, 3)}
LPIPS_SHIFT = (-0.030, -0.088, -0.188)        # lpips ScalingLayer
LPIPS_SCALE = (0.458, 0.448, 0.450)
EVAL_SCRATCH_DOUBLES = 2048                   # include/laenerf.h LAE_EVAL_VIEW_SCRATCH_DOUBLES
CONSISTENCY_SCRATCH_DOUBLES = 16384           # include/laenerf.h LAE_CONSISTENCY_SCRATCH_DOUBLES
SSIM_TILE_H, SSIM_TILE_W = 16, 32             # include/laenerf.h LAE_SSIM_TILE_H / _W: window positions per workgroup of lae_ssim
SSIM_MINMAX_BLOCKS = 256                      # include/laenerf.h LAE_SSIM_MINMAX_BLOCKS
_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.float32: 2}


def alexnet_trunk():
    """torchvision's alexnet().features[0:12] (ReLU not in place), randomly initialised"""
    return nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU())


class LPIPS(nn.Module):
    """LPIPS(net='alex', version='0.1') with frozen weights: `trunk` = alexnet_trunk(), `lins` = five [C_k] head vectors.
    `self(x)` takes the scaled input lae_eval_view writes ([2B,3,H,W] or [B,2,3,H,W]: pair p = x0 (the ground truth), then
    x1) and returns the B distances as float64 on the device."""

    def __init__(self, trunk, lins):
        super().__init__()
        if len(trunk) != 12:
            raise ValueError("LPIPS: the trunk must be alexnet().features[0:12]")
        if len(lins) != 5 or any(tuple(w.shape) != (c,) for w, c in zip(lins, ALEX_CHANNELS)):
            raise ValueError(f"LPIPS: the heads must be five vectors of {ALEX_CHANNELS} weights")
        self.trunk = trunk
        for k, w in enumerate(lins):
            self.register_buffer(f"lin{k}", w.detach().float().contiguous().clone())
        for p in self.trunk.parameters():
            p.requires_grad_(False)
        self.eval()
        self._scratch = {}

    @property
    def lins(self):
        return [getattr(self, f"lin{k}") for k in range(5)]

    @classmethod
    def random(cls, seed=0, device=None):
        """seeded stand-in weights (uniform within torch's default conv bounds, heads uniform in [0, 1)): tests and benchmarks"""
        g = torch.Generator().manual_seed(int(seed))
        trunk = alexnet_trunk()
        with torch.no_grad():
            for i, (_, c_in, k) in ALEX_CONVS.items():
                bound = 1.0 / math.sqrt(c_in * k * k)
                trunk[i].weight.copy_(torch.rand(trunk[i].weight.shape, generator=g) * 2 * bound - bound)
                trunk[i].bias.copy_(torch.rand(trunk[i].bias.shape, generator=g) * 2 * bound - bound)
        m = cls(trunk, [torch.rand(c, generator=g) for c in ALEX_CHANNELS])
        return m.to(device) if device is not None else m

    @torch.no_grad()
    def features(self, x):
        """the five relu taps of the trunk for x [N,3,H,W] (fp32, autocast off) -> list of contiguous [N,C_k,h_k,w_k]"""
        out = []
        with torch.autocast("cuda", enabled=False):
            h = x.float()
            for i, layer in enumerate(self.trunk):
                h = layer(h)
                if i in ALEX_TAPS:
                    out.append(h.contiguous())
        return out

    @torch.no_grad()
    def head(self, feats, out=None):
        """lpips' distance head on the taps of 2B images (pairs = consecutive rows) -> [B] float64: one launch over the five
        layers (lae_lpips_head) + one fixed-order sum"""
        if len(feats) != 5:
            raise ValueError("LPIPS.head: five feature maps expected")
        n2 = int(feats[0].shape[0])
        if n2 % 2:
            raise ValueError("LPIPS.head: feature maps of 2B images expected")
        B = n2 // 2
        for f, c in zip(feats, ALEX_CHANNELS):
            if f.dim() != 4 or f.shape[0] != n2 or f.shape[1] != c or f.dtype != torch.float32 or not f.is_contiguous():
                raise ValueError("LPIPS.head: contiguous fp32 [2B, C, h, w] feature maps expected")
        _lib.need_cuda(*feats, *self.lins)
        hw = [int(f.shape[2] * f.shape[3]) for f in feats]
        n_part = B * sum(-(-h // 256) for h in hw)
        dev = feats[0].device
        scratch = self._scratch.get((dev, n_part))
        if scratch is None:
            scratch = self._scratch[(dev, n_part)] = torch.empty(n_part, dtype=torch.float64, device=dev)
        if out is None:
            out = torch.empty(B, dtype=torch.float64, device=dev)
        if out.dtype != torch.float64 or out.numel() != B or not out.is_contiguous():
            raise ValueError("LPIPS.head: out must be a contiguous float64 tensor of B values")
        arr = lambda ts: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])
        check(_lib.load().lae_lpips_head(5, arr(feats), arr(self.lins), (ctypes.c_uint32 * 5)(*ALEX_CHANNELS),
                                         (ctypes.c_uint32 * 5)(*hw), B, ptr(scratch), ptr(out), stream()), "lpips_head")
        return out

    def forward(self, x, out=None):
        return self.head(self.features(x.reshape(-1, *x.shape[-3:])), out=out)

    def features_grad(self, x):
        """features() without no_grad: the five taps as part of x's autograd graph (fp32, autocast off; the trunk's weights stay
        frozen, so its backward computes input gradients only) -- LPIPS as a training term, losses.lpips_patch_loss"""
        out = []
        with _deterministic_convs(), torch.autocast("cuda", enabled=False):
            h = x.float()
            for i, layer in enumerate(self.trunk):
                h = layer(h)
                if i in ALEX_TAPS:
                    out.append(h.contiguous())
        return out

    def head_grad(self, feats, gout, both=False):
        """the gradient of head() with respect to the taps (lae_lpips_head_grad, one launch): gout float64 [B] on the device ->
        five fp32 tensors shaped like feats; both=False writes zeros into the x0 (ground-truth) rows.  A pixel whose feature
        norm is exactly 0 gets a zero gradient on that side (include/laenerf.h; `lpips_head_grad_numpy` restates it)"""
        n2 = int(feats[0].shape[0])
        B = n2 // 2
        if len(feats) != 5 or n2 % 2:
            raise ValueError("LPIPS.head_grad: five feature maps of 2B images expected")
        for f, c in zip(feats, ALEX_CHANNELS):
            if f.dim() != 4 or f.shape[0] != n2 or f.shape[1] != c or f.dtype != torch.float32 or not f.is_contiguous():
                raise ValueError("LPIPS.head_grad: contiguous fp32 [2B, C, h, w] feature maps expected")
        if gout.dtype != torch.float64 or gout.numel() != B or not gout.is_contiguous():
            raise ValueError("LPIPS.head_grad: gout must be a contiguous float64 tensor of B values")
        _lib.need_cuda(*feats, *self.lins, gout)
        hw = [int(f.shape[2] * f.shape[3]) for f in feats]
        grads = [torch.empty_like(f) for f in feats]
        arr = lambda ts: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])
        check(_lib.load().lae_lpips_head_grad(5, arr(feats), arr(self.lins), (ctypes.c_uint32 * 5)(*ALEX_CHANNELS),
                                              (ctypes.c_uint32 * 5)(*hw), B, ptr(gout), arr(grads), int(bool(both)), stream()),
              "lpips_head_grad")
        return grads


@contextlib.contextmanager
def _deterministic_convs():
    """torch's request for deterministic convolution algorithms, for the block's duration.  On maps as small as a patch's, the
    trunk's convolutions were seen to differ in their last bits from call to call on the same input (measured: features of the
    last two taps, about 4e-9), and a training run is to repeat bit for bit -- graph replay against eager steps, a
    resumed run against the uninterrupted one.  The flag is read when a convolution runs, forward or backward."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


class _LpipsTrunk(torch.autograd.Function):
    """LPIPS.features_grad as one autograd node, so that the trunk's backward runs under _deterministic_convs like its forward"""

    @staticmethod
    def forward(ctx, lp, x):
        with torch.enable_grad():
            xd = x.detach().requires_grad_(True)
            feats = lp.features_grad(xd)
        ctx.xd, ctx.feats = xd, feats
        return tuple(f.detach() for f in feats)

    @staticmethod
    def backward(ctx, *grads):
        with _deterministic_convs():
            (gx,) = torch.autograd.grad(ctx.feats, ctx.xd, grads)
        return None, gx


def lpips_features(lp, x):
    """lp.features_grad(x) with the trunk's backward as deterministic as its forward -> the five taps, part of x's autograd graph"""
    return list(_LpipsTrunk.apply(lp, x))


class _LpipsHead(torch.autograd.Function):
    """LPIPS.head with a gradient: lae_lpips_head forward, lae_lpips_head_grad backward (one launch each over the five layers)"""

    @staticmethod
    def forward(ctx, lp, both, *feats):
        feats = [f.detach() for f in feats]
        ctx.lp, ctx.both = lp, both
        ctx.save_for_backward(*feats)
        return lp.head(feats)

    @staticmethod
    def backward(ctx, gout):
        return (None, None, *ctx.lp.head_grad(list(ctx.saved_tensors), gout.to(torch.float64).contiguous(), ctx.both))


def lpips_head(lp, feats, both=True):
    """lp.head(feats) -> [B] float64 with autograd onto the taps (both=False: onto the x1 rows only, zeros for the x0 rows)"""
    return _LpipsHead.apply(lp, bool(both), *feats)


def _pairs(f):
    f = np.asarray(f, dtype=np.float64)
    f = f.reshape(f.shape[0], f.shape[1], -1)
    return f, f[0::2], f[1::2]


def lpips_head_numpy(feats, weights):
    """float64 restatement of lae_lpips_head: feats a list of [2B, C, ...] arrays (pairs = consecutive rows), weights a list of
    [C] -> [B] float64, sum_l mean_px sum_c w_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2"""
    total = 0.0
    for f, w in zip(feats, weights):
        _, f0, f1 = _pairs(f)
        w = np.asarray(w, dtype=np.float64).reshape(1, -1, 1)
        n0, n1 = np.sqrt((f0 * f0).sum(1, keepdims=True)), np.sqrt((f1 * f1).sum(1, keepdims=True))
        d = f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)
        total = total + (w * d * d).sum(1).mean(-1)
    return total


def lpips_head_grad_numpy(feats, weights, gout, both=True):
    """float64 restatement of lae_lpips_head_grad -> a list of arrays shaped like feats: the gradient of
    sum_p gout[p] * lpips_head_numpy(...)[p] with respect to the features, the zero-norm rule included (a pixel whose norm is
    exactly 0 gets a zero gradient on that side); both=False: zeros in the x0 rows"""
    gout = np.asarray(gout, dtype=np.float64).reshape(-1, 1, 1)
    out = []
    for f, w in zip(feats, weights):
        shape = np.asarray(f).shape
        f, f0, f1 = _pairs(f)
        hw = f.shape[2]
        w = np.asarray(w, dtype=np.float64).reshape(1, -1, 1)
        n0, n1 = np.sqrt((f0 * f0).sum(1, keepdims=True)), np.sqrt((f1 * f1).sum(1, keepdims=True))
        e0, e1 = n0 + 1e-10, n1 + 1e-10
        wd = w * (f0 / e0 - f1 / e1)
        a0, a1 = (wd * f0).sum(1, keepdims=True), (wd * f1).sum(1, keepdims=True)
        k = 2.0 * gout / hw
        g = np.zeros_like(f)
        with np.errstate(divide="ignore", invalid="ignore"):
            if both:
                g[0::2] = np.where(n0 != 0, k * (wd / e0 - f0 * (a0 / (n0 * e0 * e0))), 0.0)
            g[1::2] = np.where(n1 != 0, -k * (wd / e1 - f1 * (a1 / (n1 * e1 * e1))), 0.0)
        out.append(g.reshape(shape))
    return out


def patch_pack_numpy(pred, gt, patch_size, normalize=False):
    """float32 restatement of lae_patch_pack: pred / gt [n_patch * P^2, 3] -> [2 * n_patch, 3, P, P], image 2p the ground truth of patch
    p, 2p + 1 its prediction, ((2v - 1 if normalize else v) - shift) / scale with eval_view_numpy's statements"""
    f32 = np.float32
    P = int(patch_size)
    shift, scale = np.array(LPIPS_SHIFT, f32)[:, None], np.array(LPIPS_SCALE, f32)[:, None]
    planes = []
    for v in (gt, pred):
        v = np.asarray(v, dtype=f32).reshape(-1, P * P, 3)
        u = f32(2) * v - f32(1) if normalize else v
        planes.append(((u.transpose(0, 2, 1) - shift) / scale).astype(f32))
    return np.stack(planes, 1).reshape(-1, 3, P, P)


def _state_dict(src):
    sd = src if isinstance(src, dict) else torch.load(src, map_location="cpu", weights_only=True)
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return sd


def load_lpips_alex(alexnet_weights, lin_weights, device=None):
    """LPIPS from weights the user already has: `alexnet_weights` a torchvision `alexnet` state dict (path or dict;
    `features.{0,3,6,8,10}.weight / .bias`, other keys ignored), `lin_weights` the lpips package's weights/v0.1/alex.pth
    (`lin{k}.model.1.weight`, [1, C_k, 1, 1]).  Missing keys, keys of layers without weights and wrong shapes raise ValueError."""
    sd = _state_dict(alexnet_weights)
    trunk = alexnet_trunk()
    for k in sd:
        parts = k.split(".")
        if len(parts) == 3 and parts[0] == "features" and parts[1].isdigit() and int(parts[1]) < 12:
            if int(parts[1]) not in ALEX_CONVS or parts[2] not in ("weight", "bias"):
                raise ValueError(f"load_lpips_alex: unexpected key {k!r} (layer {parts[1]} is {type(trunk[int(parts[1])]).__name__})")
    for i in ALEX_CONVS:
        for name in ("weight", "bias"):
            key = f"features.{i}.{name}"
            if key not in sd:
                raise ValueError(f"load_lpips_alex: missing {key!r}")
            t = torch.as_tensor(sd[key])
            p = getattr(trunk[i], name)
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"load_lpips_alex: {key} has shape {tuple(t.shape)}, AlexNet needs {tuple(p.shape)}")
            with torch.no_grad():
                p.copy_(t.float())
    ld = _state_dict(lin_weights)
    lins = []
    for k, c in enumerate(ALEX_CHANNELS):
        key = f"lin{k}.model.1.weight"
        if key not in ld:
            raise ValueError(f"load_lpips_alex: missing {key!r}")
        t = torch.as_tensor(ld[key])
        if tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"load_lpips_alex: {key} has shape {tuple(t.shape)}, the v0.1 alex head needs {(1, c, 1, 1)}")
        lins.append(t.float().reshape(c))
    m = LPIPS(trunk, lins)
    return m.to(device) if device is not None else m


def _mask_plane(im):
    """the reference's `mask[..., -1]` of a cv2.IMREAD_UNCHANGED read (BGR / BGRA order: alpha, else red) as one uint8 plane;
    a one-channel mask is taken as it is"""
    if im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info):
        return im.convert("RGBA").getchannel("A")
    if im.mode in ("RGB", "P", "CMYK", "YCbCr"):
        return im.convert("RGB").getchannel("R")
    return im.convert("L")


def load_masks(transforms_path, split=None, H=None, W=None, device=None, undistorter=None):
    """the `<image>_mask.png` beside each frame of a blender-style scene (provider.py:216-223) -> a list with one uint8 [H, W]
    tensor per frame (None where the frame has no mask), in the frame order of ResidentImages.from_transforms (frames whose
    image is missing are skipped there and here).  A mask of another size is resized to H x W (default: its image's size) with
    PIL's bilinear filter (the reference: cv2.resize, also bilinear; the two can differ at the mask's edge).
    undistorter (the .undistorter of ResidentImages.from_transforms(undistort=True)): every mask is resampled into the pinhole
    camera with lae_remap's nearest mode, on the undistorter's device; H, W default to the captures' size there."""
    from PIL import Image
    path = transforms_path
    if os.path.isdir(path):
        path = os.path.join(path, f"transforms_{split}.json" if split else "transforms.json")
    root = os.path.dirname(os.path.abspath(path))
    with open(path) as f:
        frames = json.load(f)["frames"]
    out = []
    for fr in frames:
        f_path = os.path.join(root, fr["file_path"])
        if "." not in os.path.basename(f_path):
            f_path += ".png"
        if not os.path.exists(f_path):
            continue
        m_path = os.path.splitext(f_path)[0] + "_mask.png"
        if not os.path.exists(m_path):
            out.append(None)
            continue
        if undistorter is not None and (H is None or W is None):
            h, w = undistorter.Hs, undistorter.Ws
        elif H is None or W is None:
            with Image.open(f_path) as im:
                h, w = im.height, im.width
        else:
            h, w = int(H), int(W)
        with Image.open(m_path) as im:
            m = _mask_plane(im)
            if (m.height, m.width) != (h, w):
                m = m.resize((w, h), Image.BILINEAR)
            t = torch.from_numpy(np.asarray(m, dtype=np.uint8).copy())
        out.append(t.to(device) if device is not None else t)
    if undistorter is not None:
        from .undistort import remap
        idx = undistorter.cam_index
        for k, t in enumerate(out):
            if t is not None:
                ci = None if idx is None else idx[k:k + 1].contiguous()
                m = remap(t.to(undistorter.device).reshape(1, *t.shape, 1).contiguous(), undistorter.maps, ci, "nearest")
                out[k] = m.reshape(undistorter.H, undistorter.W)
    return out


def psnr_from_sse(sse, n_values):
    """PSNRMeter (nerf/utils.py:240-247): -10 log10(sse / n_values), elementwise"""
    return -10.0 * np.log10(np.maximum(np.asarray(sse, dtype=np.float64) / float(n_values), 1e-20))


def eval_view(pred, gt, depth=None, bg=1.0, sse=None, mask=None, masked_sse=None, gt_out=None, rgb_u8=None, depth_u8=None,
              lpips_in=None, scratch=None):
    """one rendered view against its ground truth in one pass (lae_eval_view).  pred fp32 with HW*3 values, gt the view's
    stored image (uint8 / fp16 / fp32, HW*C values, C = 3 or 4; read as stored, no fp32 copy) or None, depth fp32 [HW].
    Outputs, each optional and written in place:
      sse        float64 slot: the sum over HW*3 of (pred - gt)^2, gt blended over `bg` when C = 4
      masked_sse float64 slot (with `mask`, uint8 [HW]): the same sum against the UNblended gt[:3], over the pixels whose mask
                 byte is 0 -- eval_masked's m = 1 - clip(mask[..., -1], 0, 1), its mean times 3HW
      gt_out     fp32 [HW,3], the blended ground truth
      rgb_u8 / depth_u8  clip(x, 0, 1) * 255 truncated (the reference's unclipped astype(np.uint8) is undefined outside [0,1])
      lpips_in   fp32 [2,3,H,W]: index 0 the blended gt, 1 pred, each ((2x - 1) - shift) / scale (lpips' ScalingLayer)"""
    lib = _lib.load()
    HW = pred.numel() // 3
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() != 3 * HW:
        raise ValueError("eval_view: pred must be a contiguous fp32 tensor of HW x 3 values")
    C = 3
    if gt is not None:
        C = int(gt.shape[-1])
        if gt.dtype not in _DTYPES or C not in (3, 4) or gt.numel() != HW * C or not gt.is_contiguous():
            raise ValueError("eval_view: gt must be a contiguous uint8 / fp16 / fp32 image of HW x 3 or 4 values")
    for name, t, dt, n in (("depth", depth, torch.float32, HW), ("mask", mask, torch.uint8, HW), ("gt_out", gt_out, torch.float32, 3 * HW),
                           ("rgb_u8", rgb_u8, torch.uint8, 3 * HW), ("depth_u8", depth_u8, torch.uint8, HW),
                           ("lpips_in", lpips_in, torch.float32, 6 * HW), ("sse", sse, torch.float64, 1),
                           ("masked_sse", masked_sse, torch.float64, 1)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"eval_view: {name} must be a contiguous {dt} tensor of {n} values")
    if scratch is None:
        scratch = torch.empty(EVAL_SCRATCH_DOUBLES, dtype=torch.float64, device=pred.device)
    _lib.need_cuda(pred, gt, depth, mask, gt_out, rgb_u8, depth_u8, lpips_in, sse, masked_sse, scratch)
    check(lib.lae_eval_view(ptr(pred), ptr(depth), ptr(gt), _DTYPES[gt.dtype] if gt is not None else 0, C, HW, float(bg),
                            ptr(mask), ptr(scratch), ptr(sse), ptr(masked_sse), ptr(gt_out), ptr(rgb_u8), ptr(depth_u8), ptr(lpips_in),
                            stream()), "eval_view")


def eval_view_numpy(pred, gt, depth=None, bg=1.0, mask=None):
    """numpy restatement of lae_eval_view -> dict gt (blended, fp32 [HW,3]), sse, masked_sse (fp64 sums; None without a
    mask), rgb_u8 [HW,3], depth_u8 [HW] (None without depth), lpips_in [2,3,HW] fp32"""
    f32 = np.float32
    pred = np.asarray(pred, dtype=f32).reshape(-1, 3)
    HW = pred.shape[0]
    g = np.asarray(gt)
    g = g.reshape(HW, g.shape[-1])
    x = g.astype(f32) * (f32(1.0) / f32(255.0)) if g.dtype == np.uint8 else g.astype(f32)
    raw = x[:, :3]
    blend = raw * x[:, 3:] + f32(bg) * (f32(1.0) - x[:, 3:]) if g.shape[1] == 4 else raw.copy()
    p64 = pred.astype(np.float64)
    out = {"gt": blend, "sse": float(((p64 - blend.astype(np.float64)) ** 2).sum()), "masked_sse": None, "depth_u8": None}
    if mask is not None:
        m = (np.asarray(mask, dtype=np.uint8).reshape(HW) == 0)[:, None]
        out["masked_sse"] = float((((p64 - raw.astype(np.float64)) ** 2) * m).sum())
    out["rgb_u8"] = (np.clip(pred, f32(0), f32(1)) * f32(255)).astype(np.uint8)
    if depth is not None:
        out["depth_u8"] = (np.clip(np.asarray(depth, dtype=f32).reshape(HW), f32(0), f32(1)) * f32(255)).astype(np.uint8)
    shift, scale = np.array(LPIPS_SHIFT, f32)[:, None], np.array(LPIPS_SCALE, f32)[:, None]
    out["lpips_in"] = np.stack([((f32(2) * v.T - f32(1)) - shift) / scale for v in (blend, pred)]).astype(f32)
    return out


def consistency_pair(frame_a, frame_b, depth_a, opacity_a, depth_b, opacity_b, pose_a, pose_b, intrinsics, H, W, min_opacity=0.5,
                     sse=None, count=None, valid=None, warped=None, lpips_in=None, scratch=None):
    """multi-view consistency of two rendered views in one pass (lae_consistency_pair): the source frame `a` is warped onto the
    target frame `b` by the reprojection through the views' own depth, occlusions and motion boundaries are masked, and the
    squared error of the warped frame against the target is summed over the pixels that are left.  The metric follows the
    reference's scripts/eval/consistency_metrics.py (short- and long-range consistency as LAENeRF, ARF and Ref-NPR report it)
    with RAFT's optical flow replaced by the exact flow of the model's geometry; it is written down in full above
    k_consistency_pair (csrc/evaluate.hip) and in DESIGN.md section 4i, and restated by `consistency_numpy`.

    frame_a / frame_b uint8 or fp32 with HW x 3 values (read as stored; uint8 = value / 255); depth_* the raw `sum w t` and
    opacity_* the `weights_sum` of render_eval(scale_depth=False), fp32 [HW]; pose_* fp32 [4,4] cam2world on the device;
    intrinsics (fx, fy, cx, cy).  A pixel has geometry iff its opacity >= min_opacity (default 0.5: a choice, below one half the
    expected termination is not a surface).  Outputs, written in place:
      sse, count  float64 slots (allocated when None): the sum of err over the valid pixels and their number; warp_mse =
                  sse / count -- the number the script prints as "RSME", although it takes no root.  count == 0 gives sse == 0.
      valid       uint8 [HW];  warped  fp32 [HW,3], 0 where invalid
      lpips_in    fp32 [2,3,H,W] for LPIPS: index 0 the warped frame with invalid pixels filled from b, index 1 frame b
    Two deliberate departures from the script: (1) it multiplies the error by the occlusion mask itself, whereas the metric it
    follows (Lai et al.) uses the complement, and so does this; (2) it feeds LPIPS the warped frame with remap's zero border,
    whereas invalid pixels are filled from the target here, so that they contribute nothing.
    -> (sse, count)"""
    lib = _lib.load()
    H, W = int(H), int(W)
    HW = H * W
    if H < 2 or W < 2:
        raise ValueError("consistency_pair: H and W must be at least 2")
    if len(intrinsics) != 4:
        raise ValueError("consistency_pair: intrinsics = (fx, fy, cx, cy)")
    for name, t in (("frame_a", frame_a), ("frame_b", frame_b)):
        if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.float32) or t.numel() != 3 * HW or not t.is_contiguous():
            raise ValueError(f"consistency_pair: {name} must be a contiguous uint8 or fp32 tensor of H x W x 3 values")
    if frame_a.dtype != frame_b.dtype:
        raise ValueError("consistency_pair: both frames must have one dtype")
    dev = frame_a.device
    if sse is None:
        sse = torch.zeros(1, dtype=torch.float64, device=dev)
    if count is None:
        count = torch.zeros(1, dtype=torch.float64, device=dev)
    for name, t, dt, n, opt in (("depth_a", depth_a, torch.float32, HW, False), ("opacity_a", opacity_a, torch.float32, HW, False),
                                ("depth_b", depth_b, torch.float32, HW, False), ("opacity_b", opacity_b, torch.float32, HW, False),
                                ("pose_a", pose_a, torch.float32, 16, False), ("pose_b", pose_b, torch.float32, 16, False),
                                ("sse", sse, torch.float64, 1, False), ("count", count, torch.float64, 1, False),
                                ("valid", valid, torch.uint8, HW, True), ("warped", warped, torch.float32, 3 * HW, True),
                                ("lpips_in", lpips_in, torch.float32, 6 * HW, True)):
        if t is None and opt:
            continue
        if not torch.is_tensor(t) or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"consistency_pair: {name} must be a contiguous {dt} tensor of {n} values")
    if not float(min_opacity) > 0.0:
        raise ValueError("consistency_pair: min_opacity must be positive")
    if scratch is None:
        scratch = torch.empty(CONSISTENCY_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    if scratch.dtype != torch.float64 or scratch.numel() < CONSISTENCY_SCRATCH_DOUBLES or not scratch.is_contiguous():
        raise ValueError(f"consistency_pair: scratch must be a contiguous float64 tensor of {CONSISTENCY_SCRATCH_DOUBLES} values")
    _lib.need_cuda(frame_a, frame_b, depth_a, opacity_a, depth_b, opacity_b, pose_a, pose_b, sse, count, valid, warped, lpips_in, scratch)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    check(lib.lae_consistency_pair(ptr(frame_a), ptr(frame_b), _DTYPES[frame_a.dtype], ptr(depth_a), ptr(opacity_a), ptr(depth_b),
                                   ptr(opacity_b), ptr(pose_a), ptr(pose_b), fx, fy, cx, cy, H, W, float(min_opacity), ptr(scratch),
                                   ptr(sse), ptr(count), ptr(valid), ptr(warped), ptr(lpips_in), stream()), "consistency_pair")
    return sse, count


def consistency_numpy(frame_a, frame_b, depth_a, opacity_a, depth_b, opacity_b, pose_a, pose_b, intrinsics, H, W, min_opacity=0.5,
                      dtype=np.float64, valid=None):
    """numpy restatement of lae_consistency_pair with every quantity in `dtype` (float64 by default; np.float32 follows the
    kernel's precision, not its bits).  uint8 frames are taken as the kernel reads them, value * fp32(1 / 255); every other
    input is converted to `dtype` as it comes (fp32 arrays: exactly what the kernel reads).  `valid` (bool [H, W]) replaces the restatement's own decision in sse, count and lpips_in.
    -> dict, per pixel of b as [H, W, ...] arrays:
      valid     bool;  reason uint8: 0 valid, 1 no geometry at the pixel (transparent or behind a), 2 lands outside the frame,
                3 a right / lower neighbour without fw, 4 a tap without bw, 5 motion boundary, 6 occluded (the first that applies)
      fw        the forward flow (NaN where undefined);  landing = p + fw;  taps (x0, y0) int;  bw_mean the bilinear mean of bw
      warped    the bilinear mean of frame a at the landing point wherever that is inside the frame (whatever `valid`), else 0
      err       sum_c (warped_c - frame_b_c)^2 in float64 of the `dtype` values, wherever `warped` is defined, else 0
      occ_lhs / occ_rhs, bnd_lhs / bnd_rhs   the two sides of the two rules
      margin    the distance of the nearest decision from its threshold, each in its own units (the two rules: |lhs - rhs|; the
                four frame edges: pixels); inf where an undefined input decides
      lpips_in  [2, 3, H, W]
    and sse, count (float64 / int), warp_mse (NaN when count == 0)."""
    dt = np.dtype(dtype).type
    f32 = np.float32
    H, W = int(H), int(W)

    def frame(f):
        f = np.asarray(f)
        f = f.reshape(H, W, 3)
        return (f.astype(f32) * (f32(1.0) / f32(255.0)) if f.dtype == np.uint8 else f).astype(dt)

    Fa, Fb = frame(frame_a), frame(frame_b)
    fx, fy, cx, cy = (dt(v) for v in intrinsics)
    mo = dt(min_opacity)
    gx, gy = np.meshgrid(np.arange(W, dtype=dt), np.arange(H, dtype=dt))
    half, one = dt(0.5), dt(1.0)

    def points(P, D, A):
        P = np.asarray(P).reshape(4, 4).astype(dt)
        D, A = np.asarray(D).reshape(H, W).astype(dt), np.asarray(A).reshape(H, W).astype(dt)
        ok = A >= mo
        t = D / np.where(ok, A, one)
        xs, ys = ((gx + half) - cx) / fx, ((gy + half) - cy) / fy              # pinhole_ray
        nrm = np.sqrt((ys * ys + xs * xs) + one)
        dx, dy, dz = xs / nrm, ys / nrm, one / nrm
        X = np.stack([t * ((dz * P[k, 2] + dy * P[k, 1]) + dx * P[k, 0]) + P[k, 3] for k in range(3)], -1)
        return X, ok

    def project(P, X, ok):
        P = np.asarray(P).reshape(4, 4).astype(dt)
        v = X - P[:3, 3]
        q = [(P[2, k] * v[..., 2] + P[1, k] * v[..., 1]) + P[0, k] * v[..., 0] for k in range(3)]
        ok = ok & (q[2] > 0)
        qz = np.where(ok, q[2], one)
        return (fx * q[0] / qz + cx) - half, (fy * q[1] / qz + cy) - half, ok

    with np.errstate(all="ignore"):
        Xb, okb = points(pose_b, depth_b, opacity_b)
        lx, ly, def_b = project(pose_a, Xb, okb)
        Xa, oka = points(pose_a, depth_a, opacity_a)
        ux, uy, def_a = project(pose_b, Xa, oka)
        bwx, bwy = ux - gx, uy - gy
        fwx, fwy = lx - gx, ly - gy
        in_frame = def_b & (lx >= 0) & (lx <= dt(W - 1)) & (ly >= 0) & (ly <= dt(H - 1))
        x0 = np.where(in_frame, np.minimum(np.floor(np.where(in_frame, lx, 0)), W - 2), 0).astype(np.int64)
        y0 = np.where(in_frame, np.minimum(np.floor(np.where(in_frame, ly, 0)), H - 2), 0).astype(np.int64)
        wx, wy = lx - x0.astype(dt), ly - y0.astype(dt)
        taps_def = np.ones((H, W), bool)
        tap = []
        for k in range(4):
            rx, ry = x0 + (k & 1), y0 + (k >> 1)
            taps_def &= def_a[ry, rx]
            tap.append(np.concatenate([np.where(def_a[ry, rx], bwx[ry, rx], 0)[..., None],
                                       np.where(def_a[ry, rx], bwy[ry, rx], 0)[..., None], Fa[ry, rx]], -1))
        # the bilinear mean as two lerps along x and one along y, as the kernel forms it
        top = tap[0] + wx[..., None] * (tap[1] - tap[0])
        bot = tap[2] + wx[..., None] * (tap[3] - tap[2])
        mean = top + wy[..., None] * (bot - top)
        bmx, bmy = mean[..., 0], mean[..., 1]
        Fw = np.where(in_frame[..., None], mean[..., 2:], 0).astype(dt)
        # motion boundary: fw of the pixel against its right and lower neighbour, 0 in the last column / row
        right_def, down_def = np.ones((H, W), bool), np.ones((H, W), bool)
        right_def[:, :-1], down_def[:-1] = def_b[:, 1:], def_b[1:]
        nb_def = def_b & right_def & down_def
        dux, duy, dvx, dvy = (np.zeros((H, W), dt) for _ in range(4))
        dux[:, :-1], duy[:, :-1] = fwx[:, :-1] - fwx[:, 1:], fwy[:, :-1] - fwy[:, 1:]
        dvx[:-1], dvy[:-1] = fwx[:-1] - fwx[1:], fwy[:-1] - fwy[1:]
        mag = fwx * fwx + fwy * fwy
        bnd_lhs = (dux * dux + dvx * dvx) + (duy * duy + dvy * dvy)
        bnd_rhs = dt(0.01) * mag + dt(0.002)
        sx, sy = fwx + bmx, fwy + bmy
        occ_lhs = sx * sx + sy * sy
        occ_rhs = dt(0.01) * (mag + (bmx * bmx + bmy * bmy)) + dt(0.5)
        decided = in_frame & nb_def & taps_def
        bnd, occ = decided & (bnd_lhs > bnd_rhs), decided & (occ_lhs > occ_rhs)
        own_valid = decided & ~bnd & ~occ
        reason = np.select([~def_b, ~in_frame, ~nb_def, ~taps_def, bnd, occ], [1, 2, 3, 4, 5, 6], 0).astype(np.uint8)
        edge = np.minimum(np.minimum(np.abs(lx), np.abs(dt(W - 1) - lx)), np.minimum(np.abs(ly), np.abs(dt(H - 1) - ly)))
        rules = np.minimum(np.abs(bnd_lhs - bnd_rhs), np.abs(occ_lhs - occ_rhs))
        margin = np.full((H, W), np.inf)
        margin[def_b & ~in_frame] = edge[def_b & ~in_frame]
        margin[decided] = np.minimum(edge, rules)[decided]
        err = np.where(in_frame, ((Fw.astype(np.float64) - Fb.astype(np.float64)) ** 2).sum(-1), 0.0)
        use = own_valid if valid is None else np.asarray(valid).reshape(H, W).astype(bool)
        sse, count = float(err[use].sum()), int(use.sum())
        shift, scale = np.array(LPIPS_SHIFT, f32).astype(dt), np.array(LPIPS_SCALE, f32).astype(dt)
        x0_img = np.where(use[..., None], Fw, Fb)
        lp = np.stack([(((dt(2) * v - one) - shift) / scale).transpose(2, 0, 1) for v in (x0_img, Fb)]).astype(dt)
    nan = dt(np.nan)
    return {"valid": own_valid, "reason": reason, "fw": np.stack([np.where(def_b, fwx, nan), np.where(def_b, fwy, nan)], -1),
            "landing": np.stack([np.where(def_b, lx, nan), np.where(def_b, ly, nan)], -1), "taps": np.stack([x0, y0], -1),
            "bw_mean": np.stack([bmx, bmy], -1), "warped": Fw, "err": err, "occ_lhs": occ_lhs, "occ_rhs": occ_rhs,
            "bnd_lhs": bnd_lhs, "bnd_rhs": bnd_rhs, "margin": margin, "lpips_in": lp, "sse": sse, "count": count,
            "warp_mse": sse / count if count else float("nan")}


# ---------------------------------------------------------------- SSIM (csrc/ssim.hip; the definition: include/laenerf.h above lae_ssim)
def ssim_scratch_doubles(H, W):
    """the float64 values of scratch `ssim` needs for an H x W pair (lae_ssim_scratch_doubles, restated: no library call)"""
    H, W = int(H), int(W)
    tiles = -(-(H - 10) // SSIM_TILE_H) * -(-(W - 10) // SSIM_TILE_W) if H >= 11 and W >= 11 else 0
    return 4 * SSIM_MINMAX_BLOCKS + tiles


def ssim(pred, gt, H, W, data_range=None, out=None, map=None, scratch=None):
    """SSIM of one rendered view against its ground truth (lae_ssim; the reference's SSIMMeter, nerf/utils.py:259-293): pred, gt
    contiguous fp32 with H*W*3 values (`pred` and `gt_out` of eval_view as they are).  data_range a positive number, or None: from
    the data, max(max x - min x, max y - min y), on the device (two constant images: NaN).  out a float64 slot (allocated when
    None), map an optional fp32 [H-10, W-10, 3] that receives S per window position, scratch float64 with
    ssim_scratch_doubles(H, W) values.  No host read: the call can be captured.  -> out"""
    H, W = int(H), int(W)
    if H < 11 or W < 11:
        raise ValueError(f"ssim: H and W must be at least 11 (the window), got {H} x {W}")
    if H > 32768 or W > 32768 or 3 * H * W >= 2 ** 31:
        raise ValueError("ssim: H and W at most 32768 and H * W * 3 < 2^31")
    for name, t in (("pred", pred), ("gt", gt)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != 3 * H * W:
            raise ValueError(f"ssim: {name} must be a contiguous fp32 tensor of H x W x 3 values")
    L = 0.0
    if data_range is not None:
        L = float(data_range)
        if not (L > 0.0 and L < float("inf")):
            raise ValueError("ssim: data_range must be a positive finite number, or None for the data's own range")
    dev = pred.device
    need = ssim_scratch_doubles(H, W)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=dev)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float64, device=dev)
    for name, t, dt, n in (("out", out, torch.float64, 1), ("map", map, torch.float32, 3 * (H - 10) * (W - 10))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"ssim: {name} must be a contiguous {dt} tensor of {n} values")
    if not torch.is_tensor(scratch) or scratch.dtype != torch.float64 or scratch.numel() < need or not scratch.is_contiguous():
        raise ValueError(f"ssim: scratch must be a contiguous float64 tensor of at least {need} values")
    _lib.need_cuda(pred, gt, out, map, scratch)
    check(_lib.load().lae_ssim(ptr(pred), ptr(gt), H, W, L, ptr(scratch), ptr(out), ptr(map), stream()), "ssim")
    return out


def _ssim_window():
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) / 1.5) ** 2 / 2.0)
    return g / g.sum()


def _ssim_terms(x, y, data_range):
    """-> x, y as float64 [H, W, C], the window, and A1, A2, B1, B2, mx, my per window position"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 3 or x.shape != y.shape:
        raise ValueError("ssim_numpy: x and y must be two [H, W, C] arrays of one shape")
    H, W = x.shape[:2]
    if H < 11 or W < 11:
        raise ValueError(f"ssim_numpy: H and W must be at least 11 (the window), got {H} x {W}")
    if data_range is None:
        L = max(x.max() - x.min(), y.max() - y.min())
    else:
        L = float(data_range)
        if not L > 0.0:
            raise ValueError("ssim_numpy: data_range must be positive, or None for the data's own range")
    g = _ssim_window()

    def win(a):                                   # separable, horizontal then vertical, taps in ascending order
        t = sum(g[k] * a[:, k:k + W - 10] for k in range(11))
        return sum(g[k] * t[k:k + H - 10] for k in range(11))

    mx, my, exx, eyy, exy = win(x), win(y), win(x * x), win(y * y), win(x * y)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, (exx - mx * mx) + (eyy - my * my) + C2
    return x, y, g, L, A1, A2, B1, B2, mx, my


def ssim_numpy(x, y, data_range=None, full=False):
    """float64 restatement of lae_ssim: x, y [H, W, C] -> the mean of S over the C (H - 10)(W - 10) window values (full=True: and the
    map S [H-10, W-10, C]).  data_range None: from the data; a range of 0 (two constant images) gives NaN, as 0 / 0 does in torch.
    ValueError below 11 pixels."""
    _, _, _, L, A1, A2, B1, B2, _, _ = _ssim_terms(x, y, data_range)
    if L == 0.0:
        S = np.full(A1.shape, np.nan)
    else:
        S = (A1 * A2) / (B1 * B2)
    return (float(S.mean()), S) if full else float(S.mean())


def ssim_grad_numpy(x, y, data_range=1.0):
    """float64 restatement of lae_ssim_patch_backward for one image: d ssim_numpy(x, y, data_range) / d x, [H, W, C]"""
    if data_range is None:
        raise ValueError("ssim_grad_numpy: the data rule has no gradient here; give a positive data_range")
    x, y, g, _, A1, A2, B1, B2, mx, my = _ssim_terms(x, y, data_range)
    H, W = x.shape[:2]
    S = (A1 * A2) / (B1 * B2)
    Dm = (2 * my * A2 - 2 * my * A1) / (B1 * B2) - S * (2 * mx / B1 - 2 * mx / B2)
    Dxx = -S / B2
    Dxy = 2 * A1 / (B1 * B2)

    def spread(D):                                # the transpose of the forward pass: every window's value back over its pixels
        t = np.zeros((H,) + D.shape[1:])
        for k in range(11):
            t[k:k + H - 10] += g[k] * D
        out = np.zeros(x.shape)
        for k in range(11):
            out[:, k:k + W - 10] += g[k] * t
        return out

    return (spread(Dm) + 2 * x * spread(Dxx) + y * spread(Dxy)) / S.size
