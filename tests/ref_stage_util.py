"""Synthetic registered views for the Ref-NPR second stage (shared by test_ref_stage_cpu.py and test_gpu_ref_stage.py): an edit
region with holes in an H x W image, its crop terms by edit_dataset._crop_terms (the reference's rules), opacity weights in
[0.9, 1), and a registration of none, all or a third of its rows -- the keys register_views returns."""
import torch

H_REF, W_REF = 70, 83                      # ph, pw = 4, 5 with a fractional resize scale


def make_mask(H, W, seed, border=False):
    """flat pixel indices (ascending) of a region with holes; border=True: the region touches every border of the image"""
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(H, W, generator=g) > 0.3
    if border:
        keep[0, :] = keep[-1, :] = True
        keep[:, 0] = keep[:, -1] = True
    else:
        keep[:3] = keep[-4:] = False
        keep[:, :2] = keep[:, -5:] = False
    idx = keep.flatten().nonzero(as_tuple=True)[0]
    if idx.numel() % 16 == 0:
        idx = idx[:-1]                      # K is never a multiple of the MLP tile
    return idx


def make_ref_view(seed, H=H_REF, W=W_REF, reg="some", border=False, recolour=None, colour=None, df=0.6 / 1024):
    """reg: 'none' (R = 0), 'all' (R = K) or 'some' (a third of the rows; a few of them with weight 0).  recolour: a function of the
    registered rows' ground truth giving ref_targets (default: random colours).  colour: a function of the points x [K,3] giving the
    ground truth (default: random colours, which no network can fit)"""
    from laenerf_amd.editing.edit_dataset import _crop_terms
    g = torch.Generator().manual_seed(seed)
    mask = make_mask(H, W, seed, border)
    K = mask.numel()
    w8s = 0.9 + 0.0999 * torch.rand(K, generator=g)
    w8s[torch.rand(K, generator=g) < 0.8] = 0.99           # mostly opaque: the depth TV weights (>= 0.98 over four pixels) are not all zero
    gx = torch.Generator().manual_seed(seed + 7919)
    c = torch.rand(3, generator=gx) * 0.4 - 0.2
    x = c + (torch.rand(K, 3, generator=gx) - 0.5) * 0.25
    d = torch.nn.functional.normalize(torch.randn(K, 3, generator=gx), dim=-1)
    target = torch.rand(K, 3, generator=g) if colour is None else colour(x)
    depth = 1.0 + torch.rand(K, generator=g)
    crop = _crop_terms(H, W, mask, w8s, target, depth)
    h, w = crop["cut_gt"].shape[:2]
    if reg == "none":
        rows = torch.zeros(0, dtype=torch.long)
    elif reg == "all":
        rows = torch.arange(K)
    else:
        rows = torch.randperm(K, generator=g)[:K // 3].sort().values
    R = rows.numel()
    tw = torch.rand(R, generator=g)
    tw[torch.rand(R, generator=g) < 0.1] = 0.0
    ref_targets = torch.rand(R, 3, generator=g) if recolour is None else recolour(target[rows])
    image = torch.zeros(H * W, 4)
    image[mask, :3], image[mask, 3] = target, 1.0
    return dict(x_term=x, dirs=d, targets=target, depth_factor=torch.tensor(df), indices=mask, w8s=w8s, ref_targets=ref_targets,
                target_weights=tw, indices_ray_reg=rows, style_guide=0.1 + 0.9 * torch.rand(h, w, generator=g), image=image.view(H, W, 4),
                **crop)


def make_ref_views(seed=0, regs=("none", "all", "some"), **kw):
    return [make_ref_view(seed * 100 + k, reg=r, **kw) for k, r in enumerate(regs)]
