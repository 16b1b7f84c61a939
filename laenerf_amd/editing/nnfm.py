"""Nearest-neighbour feature matching (NNFM: ARF, Ref-NPR) on the HIP kernels of csrc/nnfm.hip.

The reference carries the loss in editing/semantic_encoder.py:83-164 (`nn_feat_replace`, `argmin_cos_distance`, `cos_loss`) and
editing/ref_loss.py (`NNFMLoss`); its working pipeline never calls it.  Per content position i the nearest style position
z_i = argmin_j (1 - a^_i . b^_j) under the matching normalization v / (sqrt(sum v^2 + 1e-8) + 1e-8), then
loss = mean_i (1 - cos(x_i, s_{z_i})) with cos_loss's normalization v / (|v| + 1e-8); the gradient flows through x only (the match
is a constant of the step, as argmin is in autograd).

Features are fp32 and channel-major [n, C, N], what StyleNetwork.features returns flattened; n independent matching problems:
    match="concat": n = 1, C = L * C'  (ARF, ref_loss.NNFMLoss: the layers concatenated)
    match="layer":  n = L              (SemanticEncoder.nn_feat_replace: one matching per layer)

The kernels never write the Na x Nb distance matrix: the matcher keeps a running best per content row in the MFMA accumulators'
layout (fp16 unit vectors, fp32 accumulation), the loss and its gradient read the original fp32 features.  One departure from the
reference: a content position whose feature vector is exactly zero contributes 1 to the loss and a zero gradient (autograd gives
NaN there through sqrt at 0).

`nnfm_numpy` restates the reference in float64 on the CPU; every test compares against it.
"""
import numpy as np
import torch
from torch.autograd import Function

__all__ = ["nnfm_pack", "nnfm_match", "nnfm_loss", "nnfm_numpy", "nnfm_workspace_bytes"]


def _backend():
    from ..backend import nnfm_backend
    return nnfm_backend


def nnfm_workspace_bytes(n, C, Na, Nb):
    """bytes one loss evaluation needs beside its inputs (the packed content side + the matcher's partial results); host only"""
    return _backend().workspace_bytes(int(n), int(C), int(Na), int(Nb))


def _as_problems(f, match="layer"):
    """[L, C, h, w] / [L, C, N] / [C, N] features -> contiguous fp32 [n, C, N]"""
    if match not in ("concat", "layer"):
        raise ValueError("nnfm: match must be 'concat' or 'layer'")
    if f.dim() == 4:
        f = f.flatten(2)
    if f.dim() == 2:
        f = f[None]
    if f.dim() != 3:
        raise ValueError("nnfm: features must be [L, C, h, w], [n, C, N] or [C, N]")
    f = f.float().contiguous()
    if match == "concat":
        f = f.reshape(1, f.shape[0] * f.shape[1], f.shape[2])
    return f


def nnfm_pack(feats):
    """fp32 [n, C, N] -> the matcher's operand: unit vectors in fp16, position-major [n, N_pad, C_pad] (zero padding)"""
    feats = _as_problems(feats)
    n, C, N = feats.shape
    be = _backend()
    packed = torch.empty(be.packed_bytes(n, C, N) // 2, dtype=torch.float16, device=feats.device)
    be.pack(feats, n, C, N, packed)
    return packed.view(n, -1, (C + 31) // 32 * 32)


def _match(a, b, packed_b, want_d):
    """a [n, C, Na], b [n, C, Nb] fp32 contiguous -> z [n, Na] int32 (, d [n, Na]).  The packed content side and the partial
    results live in the backend's grow-only scratch buffer (it grows only outside a stream capture)."""
    from ..backend import _workspace
    n, C, Na = a.shape
    Nb = b.shape[2]
    if b.shape[0] != n or b.shape[1] != C:
        raise ValueError(f"nnfm: content {tuple(a.shape)} and style {tuple(b.shape)} differ in n or C")
    be = _backend()
    z = torch.empty(n, Na, dtype=torch.int32, device=a.device)
    d = torch.empty(n, Na, dtype=torch.float32, device=a.device) if want_d else None
    if Na == 0:
        return z, d
    if packed_b is None:
        packed_b = nnfm_pack(b)
    elif tuple(packed_b.shape) != (n, (Nb + 63) // 64 * 64, (C + 31) // 32 * 32) or packed_b.dtype != torch.float16:
        # a side packed in the other arrangement (or of other features) can be large enough in bytes and still be another matrix
        raise ValueError(f"nnfm: the packed style side is {tuple(packed_b.shape)} {packed_b.dtype}, the style features {tuple(b.shape)} "
                         f"pack to {(n, (Nb + 63) // 64 * 64, (C + 31) // 32 * 32)} float16 (nnfm_pack in the same `match` arrangement)")
    part = (be.match_bytes(n, Na, Nb) + 255) // 256 * 256
    ws = _workspace(a.device, be.workspace_bytes(n, C, Na, Nb))
    packed_a = ws[part:]
    be.pack(a, n, C, Na, packed_a)
    be.match(packed_a, packed_b, n, Na, Nb, C, z, d, ws)
    return z, d


def nnfm_match(a, b, return_distance=False, packed_b=None):
    """content a [n, C, Na], style b [n, C, Nb] -> z [n, Na] int32: the nearest style position under the cosine distance (the lowest
    index among equal cosines); with return_distance also d [n, Na] = 1 - cosine of the match (fp16 operands, fp32 sums).
    packed_b: nnfm_pack(b), to pack a fixed style side once."""
    a, b = _as_problems(a), _as_problems(b)
    z, d = _match(a, b, packed_b, return_distance)
    return (z, d) if return_distance else z


class _nnfm_loss(Function):
    @staticmethod
    def forward(ctx, x, s, packed_s):
        n, C, Na = x.shape
        Nb = s.shape[2]
        z, _ = _match(x, s, packed_s, False)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        stats = torch.empty(4, n * Na, dtype=torch.float32, device=x.device)
        _backend().loss_forward(x, s, z, n, C, Na, Nb, loss, stats)
        ctx.save_for_backward(x, s, z, stats)
        ctx.mark_non_differentiable(z)
        return loss[0], z

    @staticmethod
    def backward(ctx, g_loss, _g_z):
        x, s, z, stats = ctx.saved_tensors
        n, C, Na = x.shape
        dx = torch.empty_like(x)
        _backend().loss_backward(x, s, z, stats, g_loss.float().reshape(1).contiguous(), n, C, Na, s.shape[2], dx)
        return dx, None, None


def nnfm_loss(x, style, packed_style=None, match="concat", return_match=False):
    """NNFM loss of the content features x against the style features ([L, C, h, w] or [L, C, N] each, fp32): a scalar whose
    gradient reaches x.  packed_style: nnfm_pack of the style features in the same `match` arrangement.  return_match: also z."""
    xs, ss = _as_problems(x, match), _as_problems(style, match)
    if xs.shape[2] == 0:
        raise ValueError("nnfm_loss: no content positions")
    loss, z = _nnfm_loss.apply(xs, ss, packed_style)
    return (loss, z) if return_match else loss


def nnfm_numpy(x, s, z=None):
    """The reference in float64 on the CPU.  x [n, C, Na], s [n, C, Nb] -> (z [n, Na] int64, loss, dx [n, C, Na], cos [n, Na, Nb]):
    z = argmax of the matching cosines `cos` (argmin_cos_distance's normalization; first index among equals, as torch.argmin),
    loss = cos_loss(x, gather(s, z)) and dx its gradient with respect to x.  z given: loss and dx at that match.  A zero content
    vector contributes 1 and a zero gradient (module docstring)."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    if x.ndim == 2:
        x, s = x[None], s[None]
    n, C, Na = x.shape
    an = x / (np.sqrt((x * x).sum(1, keepdims=True) + 1e-8) + 1e-8)
    bn = s / (np.sqrt((s * s).sum(1, keepdims=True) + 1e-8) + 1e-8)
    cos = np.einsum("nci,ncj->nij", an, bn)
    if z is None:
        z = cos.argmax(2)
    z = np.asarray(z).astype(np.int64).reshape(n, Na)
    t = np.take_along_axis(s, np.broadcast_to(z[:, None, :], (n, C, Na)), 2)
    na = np.sqrt((x * x).sum(1, keepdims=True))
    nt = np.sqrt((t * t).sum(1, keepdims=True))
    sa = na + 1e-8
    th = t / (nt + 1e-8)
    dot = (x * th).sum(1, keepdims=True)
    loss = float((1.0 - dot / sa).mean())
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = -(th / sa - dot * x / (na * sa * sa)) / (n * Na)
    dx = np.where(na > 0, dx, 0.0)
    return z, loss, dx, cos
