"""Time nearest-neighbour feature matching (csrc/nnfm.hip) against the reference-shaped torch chain and print one JSON line
(README "Stylize").

Per shape (n, C, Na, Nb) -- default (1, 768, 4096, 4096), the stylization's own size with the layers concatenated, and
(3, 256, 4096, 4096), one matching per layer -- on seeded Gaussian features:
  pack_ms / match_ms / loss_fwd_ms / loss_bwd_ms   each kernel entry alone (pack: the content side; the style side is packed once)
  fused_ms                                         nnfm_loss forward + backward (pack, match, loss, gradient) through autograd
  match_share_of_peak                              2 n Na Nb C / match time over the fp16 matrix-core peak (2.5e15 FLOP/s dense)
  torch_ms                                         the reference-shaped chain on the same tensors, forward + backward: fp32,
                                                   argmin_cos_distance's formulas (normalize, matmul, 1 - ., argmin), torch.gather,
                                                   cos_loss, autograd
  fused_peak_mib / torch_peak_mib                  torch.cuda.max_memory_allocated above the level before the call (inputs excluded);
                                                   the fused figure includes the whole grow-only scratch buffer that holds the
                                                   workspace (workspace_buffer_mib: allocated at 1.5 x the request that grew it),
                                                   of which the kernels use workspace_mib
  z_agree                                          share of positions where both paths chose the same index
and a StyleTrainer image step (every term on), graph-replayed, with loss="gram" and loss="nnfm": step_gram_ms / step_nnfm_ms.
Device times are CUDA-event intervals around `--reps` repetitions after `--warmup` ones, as tools/style_mode_bench.py takes them.

    python tools/nnfm_bench.py [--reps 50] [--warmup 10] [--size 256] [--no-trainer]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FP16_PEAK = 2.5e15


def torch_chain(x, s):
    """forward + backward of the reference's chain; -> (loss, z)"""
    x = x.detach().requires_grad_(True)
    with torch.no_grad():
        b = s / (((s * s).sum(1, keepdim=True) + 1e-8).sqrt() + 1e-8)
        a = x / (((x * x).sum(1, keepdim=True) + 1e-8).sqrt() + 1e-8)
        d_mat = 1.0 - torch.matmul(a.transpose(2, 1), b)
        z = torch.argmin(d_mat, 2)
    t = torch.gather(s, 2, z[:, None, :].expand(-1, s.shape[1], -1))
    a_tmp = x / ((x * x).sum(1, keepdim=True).sqrt() + 1e-8)
    b_tmp = t / ((t * t).sum(1, keepdim=True).sqrt() + 1e-8)
    loss = (1.0 - (a_tmp * b_tmp).sum(1)).mean()
    loss.backward()
    return loss.detach(), z


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_shape(shape, reps, warmup, timed):
    from laenerf_amd.backend import _workspace, nnfm_backend as be
    from laenerf_amd.editing import nnfm_loss, nnfm_pack
    n, C, Na, Nb = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(n, C, Na, device=dev, generator=g)
    s = torch.randn(n, C, Nb, device=dev, generator=g)
    out = {"shape": list(shape)}
    out["torch_peak_mib"] = peak_mib(lambda: torch_chain(x, s))      # before the fused path allocates its grow-only workspace
    packed_s = nnfm_pack(s)
    xg = x.clone().requires_grad_(True)

    def fused():
        xg.grad = None
        nnfm_loss(xg, s, packed_style=packed_s, match="layer").backward()
    fused()
    torch.cuda.synchronize()
    ws_bytes = be.workspace_bytes(n, C, Na, Nb)
    ws = _workspace(dev, ws_bytes)                                   # the grow-only scratch buffer the warm call above allocated
    out["workspace_mib"] = ws_bytes / 2 ** 20                        # what the kernels need ...
    out["workspace_buffer_mib"] = ws.numel() / 2 ** 20               # ... and what the buffer that holds it really takes (1.5 x at growth)
    out["fused_peak_mib"] = peak_mib(fused) + ws.numel() / 2 ** 20
    part = (be.match_bytes(n, Na, Nb) + 255) // 256 * 256
    packed_a = ws[part:]
    z = torch.empty(n, Na, dtype=torch.int32, device=dev)
    loss = torch.empty(1, device=dev)
    stats = torch.empty(4, n * Na, device=dev)
    dx = torch.empty_like(x)
    one = torch.ones(1, device=dev)
    out["pack_ms"] = timed(lambda: be.pack(x, n, C, Na, packed_a), reps, warmup)
    out["match_ms"] = timed(lambda: be.match(packed_a, packed_s, n, Na, Nb, C, z, None, ws), reps, warmup)
    out["loss_fwd_ms"] = timed(lambda: be.loss_forward(x, s, z, n, C, Na, Nb, loss, stats), reps, warmup)
    out["loss_bwd_ms"] = timed(lambda: be.loss_backward(x, s, z, stats, one, n, C, Na, Nb, dx), reps, warmup)
    out["fused_ms"] = timed(fused, reps, warmup)
    out["match_share_of_peak"] = 2.0 * n * Na * Nb * C / (out["match_ms"] * 1e-3) / FP16_PEAK
    out["torch_ms"] = timed(lambda: torch_chain(x, s), reps, warmup)
    lt, zt = torch_chain(x, s)
    out["z_agree"] = float((zt.int() == z).float().mean())
    out["loss_fused"], out["loss_torch"] = float(loss), float(lt)
    return out


def bench_trainer(S, reps, warmup, timed):
    from laenerf_amd.editing import EditSet, LAENeRF, StyleNetwork, StyleTrainer
    from laenerf_amd.editing.style_network import vgg19_features
    from style_mode_bench import make_views
    dev = torch.device("cuda", 0)
    side = 141
    H, W = side + 40, side + 60
    views = make_views(8, H, W, (side, side))
    torch.manual_seed(0)
    vgg = vgg19_features(14).to(dev)
    for layer in vgg:                                  # He-scaled weights: features of order one, as a trained VGG gives
        if isinstance(layer, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.zeros_(layer.bias)
    yy, xx = np.mgrid[0:300, 0:400]
    style_img = torch.from_numpy(np.stack([((xx + yy) // 12) % 2, ((xx - yy) // 20) % 2, np.full_like(xx, 1) * 0.5]).astype(np.float32))
    out = {}
    for kind in ("gram", "nnfm"):
        net = StyleNetwork(style_img, vgg, size=S, generator=torch.Generator().manual_seed(0), loss=kind)
        params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=1.0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                                 offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2, tv_weight=1e-3, tv_depth_guide=True,
                                 depth_disc_weight=1e-3, smooth_trans_weight=1e-3, warmup_iterations=-1, crop_size=S)
        torch.manual_seed(0)
        enc = LAENeRF(params, dir_encoding="sphere_harmonics").to(dev)
        es = EditSet.from_views(views, image_hw=(H, W), device=dev)
        tr = StyleTrainer(enc, es, params, iters=reps + warmup + 32, distill_palette_steps=-1, graph=True, style_net=net)
        tr.train(warmup + 16)
        torch.cuda.synchronize()
        out[f"step_{kind}_ms"] = timed(lambda: tr.train(1), reps, 0)
        out[f"capture_error_{kind}"] = tr.capture_error
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=256, help="crop_size S of the trainer step")
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("n", "C", "Na", "Nb"))
    ap.add_argument("--no-trainer", action="store_true")
    args = ap.parse_args()
    from style_mode_bench import timed
    shapes = [tuple(s) for s in args.shape] if args.shape else [(1, 768, 4096, 4096), (3, 256, 4096, 4096)]
    out = {"shapes": [bench_shape(s, args.reps, args.warmup, timed) for s in shapes]}
    if not args.no_trainer:
        out["trainer"] = bench_trainer(args.size, args.reps, args.warmup, timed)

    def rnd(v):
        if isinstance(v, float):
            return float("%.4g" % v)
        if isinstance(v, dict):
            return {k: rnd(u) for k, u in v.items()}
        if isinstance(v, list):
            return [rnd(u) for u in v]
        return v
    print(json.dumps(rnd(out)))


if __name__ == "__main__":
    main()
