"""Recolored views of a trained LAENeRF palette network: the display path of the reference's GUI (`test_gui_styleenc`,
nerf/utils.py:1230-1331, called from nerf/gui.py:617-640) and its evaluation (`eval_style_predictor`, nerf/gui.py:659-714, by way
of `val_gui_styleenc`, nerf/utils.py:1333-1386).

What the palette network predicts at a pixel depends on the pose only; the palette edits (colours, blend weights, biases) change
only the final recomposition.  So a view is prepared once per pose -- get_rays, the edit-grid render, the compaction of the hit
pixels (`lae_recolor_compact`: the reference's host-synchronising `nonzero()`), the two MLPs -- and every edit is ONE
`lae_recolor_compose` launch over the whole image: no host sync, no allocation when `out` is given, capturable in a HIP graph
(palette / weights / biases are device tensors).  The rules and the two deviations from the reference (fp32 instead of fp16 palette
product and sums; zero weights instead of 0/0 = NaN where every edited weight clamps to 0) are stated in include/laenerf.h;
`compose_numpy` restates them.
"""
import numpy as np
import torch

from ..backend import raymarching_backend as _rm
from ..backend import style_backend as _backend
from ..rays import get_rays

__all__ = ["RecolorView", "render_recolored", "recolor_views", "compose_numpy", "MODES"]

MODES = {"preview": 0, "weights": 1, "offsets": 2, "eval": 3}          # include/laenerf.h LAE_RECOLOR_*
_NO_OFFSETS, _TANH = 1, 2


def _flags(use_offsets, offset_act):
    if offset_act not in ("raw", "tanh"):
        raise ValueError("offset_act: 'raw' (get_offsets, the reference's display path) or 'tanh' (LAENeRF.forward)")
    return (0 if use_offsets else _NO_OFFSETS) | (_TANH if offset_act == "tanh" else 0)


def _bg_host(bg_color):
    v = bg_color.detach().flatten().tolist() if torch.is_tensor(bg_color) else np.atleast_1d(np.asarray(bg_color, np.float32)).tolist()
    v = [float(x) for x in v]
    if len(v) not in (1, 3):
        raise ValueError("bg_color: one number or three")
    return v * 3 if len(v) == 1 else v


class RecolorView:
    """One pose of a trained scene, ready to be recolored.  `renderer`: the NeRFRenderer of the scene; `style_enc`: the trained
    LAENeRF.  prepare() once per pose, then compose() per palette edit."""

    def __init__(self, renderer, style_enc):
        self.renderer, self.style_enc = renderer, style_enc
        self.H = self.W = None
        self._defaults = {}

    @torch.no_grad()
    def prepare(self, pose, intrinsics, H, W, edit_grid, bg_color, perturb_ray_dirs=False):
        """get_rays -> edit-grid render (fp16 autocast, scale_depth off) -> lae_recolor_compact -> ONE host read of K (the MLP
        launch sizes; the reference's nonzero() syncs here too) -> the frame loop's status -> the palette network's logits and raw
        offsets of the K edit pixels (eval mode).  Returns K."""
        enc = self.style_enc
        dev = enc.color_palette.device
        pose = torch.as_tensor(pose, dtype=torch.float32).to(dev).reshape(1, 4, 4)
        rays = get_rays(pose, intrinsics, H, W, -1, perturb_ray_dirs=perturb_ray_dirs)
        rays_o, rays_d = rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3)
        bg = torch.tensor(_bg_host(bg_color), dtype=torch.float32, device=dev)
        with torch.autocast("cuda", dtype=torch.float16):
            res = self.renderer.render_eval(rays_o, rays_d, bg_color=bg, perturb=False, scale_depth=False, dens_grid=edit_grid,
                                            image_hw=(H, W))
        N = H * W
        Np = (N + 15) // 16 * 16
        indices = torch.empty(N, dtype=torch.int32, device=dev)
        slot_map = torch.empty(N, dtype=torch.int32, device=dev)
        x_term = torch.empty(Np, 3, dtype=torch.float32, device=dev)
        dirs = torch.empty(Np, 3, dtype=torch.float32, device=dev)
        alpha = torch.empty(N, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _backend.recolor_compact(res["depth"], res["weights_sum"], rays_o, rays_d, N, indices, slot_map, x_term, dirs, alpha, count)
        K = int(count.item())
        if _rm.render_frame_last_status() == 1:
            raise RuntimeError("RecolorView.prepare: a cross-stream wait of the edit-grid render timed out; its outputs are NaN -- "
                               "prepare the view again")
        Kp = (K + 15) // 16 * 16
        if K:
            was_training = enc.training
            enc.eval()
            try:
                with torch.autocast("cuda", dtype=torch.float16):
                    w_logits, o_raw, _ = enc._logits(x_term[:Kp], dirs[:Kp] if enc.dir_encoding is not None else None)
            finally:
                enc.train(was_training)
        else:                                                              # nothing hit: compose never reads a logit
            w_logits = o_raw = torch.zeros(16, 16, dtype=torch.float16, device=dev)
        self.H, self.W, self.K = H, W, K
        self.indices, self.slot_map, self.x_term, self.dirs, self.alpha = indices[:K], slot_map, x_term[:K], dirs[:K], alpha
        self.w_logits, self.o_raw = w_logits.contiguous(), o_raw.contiguous()
        self.base = res["image"].reshape(N, 3).contiguous()
        self.bg = bg
        return K

    def _default_edit(self, mask, n_active, dev):
        """palette rows of the active bases (get_color_palette() without its boolean-mask sync), ones, zeros"""
        if mask not in self._defaults:
            idx = torch.tensor([j for j in range(16) if (mask >> j) & 1], dtype=torch.long, device=dev)
            self._defaults = {mask: (idx, torch.ones(n_active, device=dev), torch.zeros(n_active, device=dev))}
        return self._defaults[mask]

    @torch.no_grad()
    def compose(self, palette=None, p_weights=None, p_bias=None, mode="preview", k=0, use_offsets=True, offset_act="raw", out=None,
                out_u8=None):
        """One lae_recolor_compose launch: the prepared view under a palette edit -> [H, W, 3] fp32 (`out` if given).
        palette [n_active, 3], p_weights / p_bias [n_active]: fp32 device tensors (default: the network's active palette, ones,
        zeros).  mode: 'preview' (test_gui_styleenc), 'weights' (base k), 'offsets', 'eval' (eval_style_predictor).  out_u8
        [H, W, 3] uint8 (optional) receives (out * 255).byte()."""
        if self.H is None:
            raise RuntimeError("RecolorView.compose: prepare() a view first")
        if mode not in MODES:
            raise ValueError(f"mode: one of {sorted(MODES)}")
        enc = self.style_enc
        P, mask = enc.num_color_bases, int(enc._active_mask)
        n_active = bin(mask).count("1")
        dev = self.base.device
        if palette is None or p_weights is None or p_bias is None:
            idx, ones, zeros = self._default_edit(mask, n_active, dev)
            palette = torch.index_select(enc.color_palette.detach(), 0, idx) if palette is None else palette
            p_weights = ones if p_weights is None else p_weights
            p_bias = zeros if p_bias is None else p_bias
        if tuple(palette.shape) != (n_active, 3) or p_weights.numel() != n_active or p_bias.numel() != n_active:
            raise ValueError(f"compose: palette [{n_active}, 3], p_weights / p_bias [{n_active}] (the active bases)")
        if mode == "weights" and not 0 <= k < n_active:
            raise ValueError(f"compose: k must index an active base (0..{n_active - 1})")
        N = self.H * self.W
        if out is None:
            out = torch.empty(self.H, self.W, 3, dtype=torch.float32, device=dev)
        _backend.recolor_compose(self.slot_map, N, self.w_logits, self.o_raw, P, mask, palette, p_weights, p_bias, self.alpha, self.base,
                                 self.bg, MODES[mode], k, _flags(use_offsets, offset_act), out, out_u8)
        return out.view(self.H, self.W, 3)


def render_recolored(renderer, style_enc, pose, intrinsics, H, W, edit_grid, bg_color, perturb_ray_dirs=False, **compose_kwargs):
    """prepare + compose in one call (test_gui_styleenc, nerf/utils.py:1230-1331) -> [H, W, 3] fp32"""
    view = RecolorView(renderer, style_enc)
    view.prepare(pose, intrinsics, H, W, edit_grid, bg_color, perturb_ray_dirs=perturb_ray_dirs)
    return view.compose(**compose_kwargs)


@torch.no_grad()
def recolor_views(renderer, style_enc, poses, intrinsics, H, W, edit_grid, bg_color, palette=None):
    """eval_style_predictor's loop (nerf/gui.py:689-714): mode 'eval' over `poses` -> [n, H, W, 3] uint8 on the device, the
    images the reference writes as PNGs ((out * 255).byte())"""
    dev = style_enc.color_palette.device
    poses = torch.as_tensor(poses, dtype=torch.float32).to(dev).reshape(-1, 4, 4)
    imgs = torch.empty(poses.shape[0], H, W, 3, dtype=torch.uint8, device=dev)
    out = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    view = RecolorView(renderer, style_enc)
    for i in range(poses.shape[0]):
        view.prepare(poses[i], intrinsics, H, W, edit_grid, bg_color)
        view.compose(palette=palette, mode="eval", out=out, out_u8=imgs[i])
    return imgs


def compose_numpy(slot_map, w_logits, o_raw, active_mask, palette, p_weights, p_bias, alpha, base, bg, mode="preview", k=0,
                  use_offsets=True, offset_act="raw"):
    """lae_recolor_compose restated in numpy (include/laenerf.h): every operation one fp32 rounding in the kernel's order, exp / tanh
    in float64 rounded once.  slot_map [N]; w_logits / o_raw [K_pad, >= 16 or >= 3] fp16; palette [n_active, 3]; p_weights / p_bias
    [n_active]; alpha [>= K]; base [N, 3] (unused by 'eval'); bg [3].  -> [N, 3] fp32"""
    f32 = np.float32
    slot = np.asarray(slot_map).reshape(-1).astype(np.int64)
    N = slot.size
    bg = np.asarray(bg, f32).reshape(3)
    out = np.broadcast_to(bg, (N, 3)).copy() if mode == "eval" else np.asarray(base, f32).reshape(N, 3).copy()
    sel = np.nonzero(slot >= 0)[0]
    if sel.size == 0:
        return out
    s = slot[sel]
    t = np.asarray(alpha, f32).reshape(-1)[s]
    u = (f32(1) - t)[:, None]
    o = np.asarray(o_raw)[s, :3].astype(f32)
    if offset_act == "tanh":
        o = np.tanh(o.astype(np.float64)).astype(f32)
    if mode == "offsets":
        out[sel] = (o * f32(0.5) + f32(0.5)) + u * bg
        return out
    cols = [j for j in range(16) if (int(active_mask) >> j) & 1 and j < np.asarray(w_logits).shape[1]]
    lg = np.asarray(w_logits)[s][:, cols].astype(f32)
    e = np.exp((lg - lg.max(1, keepdims=True)).astype(np.float64)).astype(f32)
    tot = e[:, 0].copy()
    for j in range(1, len(cols)):
        tot = tot + e[:, j]
    w = e / tot[:, None]
    if mode == "weights":
        out[sel] = w[:, k:k + 1] + u * bg
        return out
    pal = np.asarray(palette, f32).reshape(len(cols), 3)
    if mode == "preview" and use_offsets:
        w = np.maximum(np.asarray(p_bias, f32).reshape(1, -1) + np.asarray(p_weights, f32).reshape(1, -1) * w, f32(0))
        ws = w[:, 0].copy()
        for j in range(1, len(cols)):
            ws = ws + w[:, j]
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(ws[:, None] > 0, w / ws[:, None], f32(0)).astype(f32)
    acc = w[:, 0:1] * pal[0]
    for j in range(1, len(cols)):
        acc = acc + w[:, j:j + 1] * pal[j]
    if mode == "eval":
        out[sel] = np.clip(acc + o, f32(0), f32(1)) * t[:, None] + bg * u
    elif use_offsets:
        out[sel] = np.clip(o + acc, f32(0), f32(1)) + u * bg
    else:
        out[sel] = np.clip(acc, f32(0), f32(1)) + u * bg
    return out
