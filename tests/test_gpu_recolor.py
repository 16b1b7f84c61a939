"""-m gpu: recolored views of a trained palette network (laenerf_amd.editing.recolor; nerf/utils.py:1230-1386, nerf/gui.py:617-714):
the compaction against torch's nonzero and expressions bit for bit, the compose kernel against its numpy restatement, the whole
path against the reference-shaped operator chain and against LAENeRF.forward, and edits replayed from a captured graph."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import DEV, N, T
from test_gpu_edit_dataset import poses_looking_at_origin
from test_gpu_frame import make

pytestmark = pytest.mark.gpu

H = W = 96
INTR = np.array([133.3, 133.3, 48.0, 48.0], np.float32)


def style_encoder(P=8, seed=3):
    from laenerf_amd.editing import LAENeRF
    torch.manual_seed(seed)
    params = SimpleNamespace(bound=1, num_palette_bases=P, style_weight=0)
    m = LAENeRF(params, dir_encoding="sphere_harmonics").to(DEV)
    m.encoder.embeddings.data.uniform_(-1.0, 1.0)                            # logits that prefer different bases in different places
    return m.eval()


def scene(O, empty_edit=False):
    from laenerf_amd import synthetic as S
    net, r = make(bound=1, seed=2)
    r.density_scale = 30.0
    dens = S.sphere_density_grid()
    coords = O.morton3D_invert(np.arange(128 ** 3, dtype=np.int32))
    keep = (coords[:, 0] >= 64) & (not empty_edit)
    edit = T(S.pack_bits_np(np.where(keep[None], dens, 0), 10.0))           # the x > 0 half of the sphere
    return r, edit


def compact(depth, ws, o, d):
    from laenerf_amd.backend import style_backend as B
    n = depth.numel()
    np_ = (n + 15) // 16 * 16
    out = dict(indices=torch.full((n,), -7, dtype=torch.int32, device=DEV), slot_map=torch.full((n,), -7, dtype=torch.int32, device=DEV),
               x_term=torch.full((np_, 3), float("nan"), device=DEV), dirs=torch.full((np_, 3), float("nan"), device=DEV),
               alpha=torch.full((n,), float("nan"), device=DEV), count=torch.full((1,), -1, dtype=torch.int32, device=DEV))
    B.recolor_compact(depth, ws, o, d, n, out["indices"], out["slot_map"], out["x_term"], out["dirs"], out["alpha"], out["count"])
    return out


@pytest.mark.parametrize("n,kind", [(1080 * 1920, "mixed"), (800 * 800, "mixed"), (12345, "mixed"), (12345, "none"), (12345, "all"),
                                    (1, "all"), (1, "none"), (1023, "mixed")])
def test_compaction_equals_torch_nonzero_and_expressions(n, kind):
    g = torch.Generator(device=DEV).manual_seed(n)
    depth = torch.rand(n, device=DEV, generator=g) * 4
    if kind == "mixed":
        r = torch.rand(n, device=DEV, generator=g)
        depth[r < 0.3] = 0.0
        depth[(r >= 0.3) & (r < 0.35)] = float("nan")                     # NaN -> 0: not an edit pixel
        depth[(r >= 0.35) & (r < 0.37)] = -0.0
        depth[(r >= 0.37) & (r < 0.38)] = float("inf")
    elif kind == "none":
        depth[: n // 2] = 0.0
        depth[n // 2:] = float("nan")
    else:
        depth = depth + 0.5
    ws = torch.rand(n, device=DEV, generator=g)
    o = torch.randn(n, 3, device=DEV, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=DEV, generator=g), dim=-1)
    res = compact(depth, ws, o, d)
    dd = torch.zeros_like(depth)
    dd[~depth.isnan()] = depth[~depth.isnan()]                              # utils.py:1265-1266
    x_term = o + dd[..., None] * d                                          # :1268
    idx = dd.flatten().nonzero(as_tuple=True)[0]                            # :1270
    K = int(res["count"].item())
    assert K == idx.numel() == {"none": 0, "all": n}.get(kind, K)
    assert torch.equal(res["indices"][:K].long(), idx)
    sm = res["slot_map"]
    assert torch.equal(sm[idx].long(), torch.arange(K, device=DEV))        # the slot map inverts the index list ...
    other = torch.ones(n, dtype=torch.bool, device=DEV)
    other[idx] = False
    assert bool((sm[other] == -1).all())                                   # ... and marks every other pixel
    assert torch.equal(res["x_term"][:K].view(torch.int32), x_term[idx].view(torch.int32))
    assert torch.equal(res["dirs"][:K], d[idx]) and torch.equal(res["alpha"][:K], ws[idx])
    Kp = (K + 15) // 16 * 16
    assert bool((res["x_term"][K:Kp] == 0).all()) and bool((res["dirs"][K:Kp] == 0).all())
    assert bool(res["x_term"][Kp:].isnan().all())                           # nothing written past the padding


def random_compose_inputs(seed, n=5000, P=8, mask=0xff):
    rng = np.random.default_rng(seed)
    edit = rng.random(n) < 0.5
    K = int(edit.sum())
    slot = np.full(n, -1, np.int32)
    slot[edit] = rng.permutation(K)
    Kp = (K + 15) // 16 * 16
    n_active = bin(mask).count("1")
    alpha = rng.random(Kp).astype(np.float32)
    pick = rng.random(Kp)
    alpha[pick < 0.25] = 0.0                                                   # alphas in {0, 1, random}
    alpha[pick > 0.75] = 1.0
    return dict(slot_map=slot, w_logits=(rng.standard_normal((Kp, 16)) * 3).astype(np.float16),
                o_raw=(rng.standard_normal((Kp, 16)) * 0.7).astype(np.float16), active_mask=mask, P=P,
                palette=rng.random((n_active, 3)).astype(np.float32), p_weights=(rng.random(n_active) * 2).astype(np.float32),
                p_bias=(rng.standard_normal(n_active) * 0.2).astype(np.float32), alpha=alpha,
                base=rng.random((n, 3)).astype(np.float32), bg=rng.random(3).astype(np.float32))


def kernel_compose(c, mode, k=0, flags=0, u8=True):
    from laenerf_amd.backend import style_backend as B
    from laenerf_amd.editing.recolor import MODES
    n = c["slot_map"].size
    out = torch.full((n, 3), float("nan"), device=DEV)
    out_u8 = torch.full((n, 3), 77, dtype=torch.uint8, device=DEV) if u8 else None
    B.recolor_compose(T(c["slot_map"]), n, T(c["w_logits"]), T(c["o_raw"]), c["P"], c["active_mask"], T(c["palette"]), T(c["p_weights"]),
                      T(c["p_bias"]), T(c["alpha"]), T(c["base"]), T(c["bg"]), MODES[mode], k, flags, out, out_u8)
    return out, out_u8


@pytest.mark.parametrize("mask,P", [(0xff, 8), (0b10110101, 8), (0b1, 8), (0xffff, 16), (0b100000000100, 12)])
def test_compose_equals_compose_numpy(mask, P):
    from laenerf_amd.editing.recolor import compose_numpy
    for seed in range(2):
        c = random_compose_inputs(seed, P=P, mask=mask)
        n_active = c["palette"].shape[0]
        cases = [("preview", 0, True, "raw"), ("preview", 0, False, "raw"), ("preview", 0, True, "tanh"), ("weights", n_active - 1, True, "raw"),
                 ("weights", 0, True, "raw"), ("offsets", 0, True, "raw"), ("offsets", 0, True, "tanh"), ("eval", 0, True, "raw")]
        if seed == 1:
            c["p_bias"][:] = -10.0                                             # every edited weight clamps to 0
        for mode, k, use_offsets, act in cases:
            flags = (0 if use_offsets else 1) | (2 if act == "tanh" else 0)
            out, out_u8 = kernel_compose(c, mode, k, flags)
            npc = {key: v for key, v in c.items() if key != "P"}
            want = compose_numpy(**npc, mode=mode, k=k, use_offsets=use_offsets, offset_act=act)
            got = N(out)
            assert np.isfinite(got).all(), (mode, act)
            assert np.abs(got - want).max() <= 2e-7, (mode, k, use_offsets, act, np.abs(got - want).max())
            assert torch.equal(out_u8, (out * 255).byte()), (mode, act)      # write_png((out * 255).byte()) of the kernel's own output


def test_compose_rejects_bad_arguments():
    c = random_compose_inputs(0, n=64)
    with pytest.raises(RuntimeError):
        kernel_compose(c, "weights", k=8)                                  # k indexes the 8 active bases
    c["active_mask"] = 0
    with pytest.raises(RuntimeError):
        kernel_compose(c, "preview")


def reference_chain(r, enc, pose, edit, bg, mode, palette, p_weights=None, p_bias=None):
    """the reference's lines (utils.py:1230-1311 / :1333-1386 + gui.py:706-714) on the repository's operators under fp16 autocast"""
    from laenerf_amd.rays import get_rays
    rays = get_rays(pose[None], INTR, H, W, -1)
    o, d = rays["rays_o"].view(-1, 3), rays["rays_d"].view(-1, 3)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        res = r.render_eval(o, d, bg_color=bg, scale_depth=False, dens_grid=edit, image_hw=(H, W))
        preds, depth, pred_t = res["image"], res["depth"], res["weights_sum"]
        dd = torch.zeros_like(depth)
        dd[~depth.isnan()] = depth[~depth.isnan()]
        x_term = o + dd[..., None] * d
        idx = dd.flatten().nonzero(as_tuple=True)
        w = enc.get_weights(x_term[idx])
        off = enc.get_offsets(x_term[idx], d[idx])
        if mode == "preview":
            pw = torch.clamp_min(p_bias[None] + p_weights[None] * w, 0)
            pw /= pw.sum(-1)[..., None]
            pred = torch.clamp(off.half() + pw.half() @ palette.half(), 0, 1)
            pred = pred + (1 - pred_t[idx].detach()[..., None]) * bg
            img = preds.clone()
            img[idx] = pred.float()
        else:
            alpha = pred_t[idx][..., None]
            cpred = torch.clamp((w @ palette.half()) + off, 0, 1)
            img = (torch.ones((H * W, 3), dtype=torch.float32, device=DEV) * bg)
            img[idx] = (cpred * alpha + img[idx] * (1 - alpha)).float()
    return img.view(H, W, 3), idx[0]


def test_end_to_end_equals_the_reference_chain(O):
    from laenerf_amd.editing import RecolorView, recolor_views
    r, edit = scene(O)
    enc = style_encoder()
    poses = T(poses_looking_at_origin(2, 3.2, seed=1))
    bg = torch.tensor([0.2, 0.5, 0.9], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    palette = torch.rand(8, 3, device=DEV, generator=g)
    p_weights = torch.rand(8, device=DEV, generator=g) * 2
    p_bias = torch.randn(8, device=DEV, generator=g) * 0.1
    view = RecolorView(r, enc)
    for i in range(2):
        K = view.prepare(poses[i], INTR, H, W, edit, bg)
        want, idx = reference_chain(r, enc, poses[i], edit, bg, "preview", palette, p_weights, p_bias)
        assert 100 < K < H * W // 2
        assert torch.equal(view.indices.long(), idx)                          # the same edit pixels
        got = view.compose(palette, p_weights, p_bias)
        assert (got - want).abs().max().item() <= 2e-3
        others = view.slot_map < 0
        assert torch.equal(got.view(-1, 3)[others], want.view(-1, 3)[others])   # the render's own pixels, bit for bit
        want_e, _ = reference_chain(r, enc, poses[i], edit, bg, "eval", palette)
        got_e = view.compose(palette, mode="eval")
        assert (got_e - want_e).abs().max().item() <= 2e-3
    imgs = recolor_views(r, enc, poses, INTR, H, W, edit, bg, palette=palette)
    assert imgs.shape == (2, H, W, 3) and imgs.dtype == torch.uint8
    assert torch.equal(imgs[1], (got_e * 255).byte())


def test_identity_edit_with_tanh_equals_the_trained_model(O):
    from laenerf_amd.editing import RecolorView
    r, edit = scene(O)
    enc = style_encoder()
    pose = T(poses_looking_at_origin(1, 3.2, seed=4))[0]
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    view = RecolorView(r, enc)
    K = view.prepare(pose, INTR, H, W, edit, bg)
    assert K > 100
    got = view.compose(offset_act="tanh").view(-1, 3)[view.indices.long()]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        pred = enc(view.x_term, view.dirs)
    t = view.alpha[:K][:, None]
    want = torch.clamp(pred.float(), 0, 1) + (1 - t) * bg
    assert (got - want).abs().max().item() <= 1e-3


def test_edits_replay_from_a_graph_and_touch_only_edit_pixels(O):
    from laenerf_amd.editing import RecolorView
    r, edit = scene(O)
    enc = style_encoder()
    pose = T(poses_looking_at_origin(1, 3.2, seed=1))[0]
    bg = torch.tensor([0.3, 0.3, 0.3], device=DEV)
    view = RecolorView(r, enc)
    K = view.prepare(pose, INTR, H, W, edit, bg)
    assert K > 100
    g = torch.Generator(device=DEV).manual_seed(1)
    palette = enc.get_color_palette().detach().clone()
    p_weights, p_bias = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    out = torch.empty(H, W, 3, device=DEV)
    out_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        view.compose(palette, p_weights, p_bias, out=out, out_u8=out_u8)    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        view.compose(palette, p_weights, p_bias, out=out, out_u8=out_u8)
    before = view.compose(palette, p_weights, p_bias).clone()
    palette.copy_(torch.rand(8, 3, device=DEV, generator=g))                  # a palette and weight edit, in place
    p_weights.copy_(torch.rand(8, device=DEV, generator=g) * 2)
    graph.replay()
    torch.cuda.synchronize()
    eager = view.compose(palette, p_weights, p_bias)
    assert torch.equal(out, eager) and torch.equal(out_u8, (eager * 255).byte())
    changed = (eager != before).any(-1).view(-1)
    edit_px = view.slot_map >= 0
    assert bool(changed.any()) and not bool((changed & ~edit_px).any())        # only edit pixels move
    assert torch.equal(eager.view(-1, 3)[~edit_px], view.base[~edit_px])


def test_a_view_without_edit_pixels_returns_the_base_image(O):
    from laenerf_amd.editing import RecolorView, render_recolored
    r, edit = scene(O, empty_edit=True)
    enc = style_encoder()
    pose = T(poses_looking_at_origin(1, 3.2, seed=1))[0]
    bg = torch.tensor([0.1, 0.7, 0.4], device=DEV)
    view = RecolorView(r, enc)
    assert view.prepare(pose, INTR, H, W, edit, bg) == 0
    img = view.compose(torch.rand(8, 3, device=DEV))
    assert torch.equal(img.view(-1, 3), view.base)
    assert bool((view.compose(mode="eval") == bg).all())
    assert torch.equal(render_recolored(r, enc, pose, INTR, H, W, edit, bg), img)
