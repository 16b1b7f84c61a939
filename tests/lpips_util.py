"""fp64 torch restatement of LPIPS v0.1 (alex) for the tests: lpips' normalize_tensor, NetLinLayer (a 1x1 conv without bias),
spatial_average and the sum over the five layers, written from the package's published definition."""
import torch


def head_fp64(feats, lins):
    """feats: five [2B, C, h, w] tensors (pairs = consecutive rows), lins: five [C] -> [B] float64"""
    total = 0
    for f, w in zip(feats, lins):
        f = f.double()
        f0, f1 = f[0::2], f[1::2]
        n0 = torch.sqrt((f0 * f0).sum(1, keepdim=True))
        n1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
        d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
        total = total + (d * w.double().view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return total


def lpips_fp64(lp, in0, in1):
    """the whole metric in fp64: lpips(in0, in1, normalize=True) with the trunk and heads of `lp` (a metrics.LPIPS); in0 / in1
    [B,3,H,W] in [0,1]"""
    shift = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float64, device=in0.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float64, device=in0.device).view(1, 3, 1, 1)
    x = torch.stack([in0.double(), in1.double()], 1).reshape(-1, *in0.shape[1:])
    h = ((2 * x - 1) - shift) / scale
    feats = []
    for i, layer in enumerate(lp.trunk):
        if isinstance(layer, torch.nn.Conv2d):
            h = torch.nn.functional.conv2d(h, layer.weight.double(), layer.bias.double(), layer.stride, layer.padding)
        else:
            h = layer(h)
        if i in (1, 4, 7, 9, 11):
            feats.append(h)
    return head_fp64(feats, lp.lins)
