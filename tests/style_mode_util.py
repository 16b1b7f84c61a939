"""Synthetic edit views with the image arrays of the stylization terms (shared by test_style_mode_cpu.py and
test_gpu_style_mode.py): each view is a rectangular edit region with holes in an H x W image, its crop terms computed by
edit_dataset._crop_terms, the reference's rules."""
import numpy as np
import torch

H_IMG, W_IMG = 24, 30


def make_image_view(box, seed, H=H_IMG, W=W_IMG, smooth=True, w8_low=False, df=0.6 / 1024):
    """box = (x0, x1, y0, y1) INCLUSIVE bounds of the region (the crop is then rows x0..x1-1, columns y0..y1-1); w8_low: every weight
    below 0.98, so the depth TV weights and their maxima are 0"""
    from laenerf_amd.editing.edit_dataset import _crop_terms
    g = torch.Generator().manual_seed(seed)
    x0, x1, y0, y1 = box
    keep = torch.rand(x1 - x0 + 1, y1 - y0 + 1, generator=g) > 0.25
    keep[0, 0] = keep[-1, -1] = True
    ii, jj = keep.nonzero(as_tuple=True)
    mask = ((ii + x0) * W + (jj + y0)).long()
    K = mask.numel()
    w8s = (0.9 + 0.1 * torch.rand(K, generator=g)) if not w8_low else torch.full((K,), 0.9)
    w8s[torch.rand(K, generator=g) < 0.9] = 0.99 if not w8_low else 0.9
    target = torch.rand(K, 3, generator=g)
    depth = 1.0 + torch.rand(K, generator=g)
    dist = torch.rand(K, generator=g) if smooth else None
    crop = _crop_terms(H, W, mask, w8s, target, depth, dist)
    c = torch.rand(3, generator=g) * 0.4 - 0.2
    x = c + (torch.rand(K, 3, generator=g) - 0.5) * 0.25
    d = torch.nn.functional.normalize(torch.randn(K, 3, generator=g), dim=-1)
    return dict(x_term=x, dirs=d, targets=target, depth_factor=torch.tensor(df), indices=mask, **crop)


# crops larger and smaller than a 16-pixel S, a one-pixel-high crop, a one-pixel-wide crop, odd row counts
BOXES = [(2, 21, 3, 27), (5, 9, 6, 12), (10, 11, 4, 25), (3, 20, 14, 15), (0, 23, 0, 29), (7, 14, 9, 22)]


def make_image_views(boxes=BOXES, seed=0, **kw):
    return [make_image_view(b, seed * 100 + k, **kw) for k, b in enumerate(boxes)]


def striped_style(h=40, w=52, period=6):
    """a synthetic style image [3,h,w]: diagonal colour stripes"""
    yy, xx = np.mgrid[0:h, 0:w]
    s = ((xx + yy) // period) % 2
    img = np.stack([0.9 * s + 0.05, 0.2 + 0.6 * (1 - s), 0.5 * np.ones_like(s, dtype=np.float64)]).astype(np.float32)
    return torch.from_numpy(img)
