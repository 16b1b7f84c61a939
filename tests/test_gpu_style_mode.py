"""-m gpu: LAENeRF's stylization step (nerf/utils.py:997-1033) on the device: the image kernels (csrc/style_image.hip) against the
reference's torch block, one full step against an autograd chain of the reference's step, graph replay against eager steps across
the warm-up gate, the NaN skip of a zero depth-discontinuity maximum, and a short stylization fit followed by distill_images."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import DEV, N
from style_mode_util import H_IMG, W_IMG, make_image_view, make_image_views, striped_style

pytestmark = pytest.mark.gpu

STYLE_TOL = {"pred": 1e-3, "w_hat": 1e-4, "o_hat": 5e-4, "loss": 1e-5, "g_wn": 1e-3, "g_on": 1e-3, "g_pal": 2e-3, "g_table": 1e-3}
ALL = 1 | 2 | 4 | 8 | 16 | 32


def _set(views):
    from laenerf_amd.editing import EditSet
    return EditSet.from_views(views, image_hw=(H_IMG, W_IMG), device=DEV)


def _ref(view, pred, S, flags, requires_grad=False):
    from laenerf_amd.editing.style_image import reference_image_terms
    t = lambda k: view[k].to(DEV)
    return reference_image_terms(pred, t("indices"), view["cut_min_max_xy"].tolist(), H_IMG, W_IMG, t("cut_gt"), t("cut_tv_h"), t("cut_tv_v"),
                                 t("cut_smooth_trans"), S, flags)


def _kernel_forward(es, pred16, cap, m, S, flags):
    from laenerf_amd.backend import style_backend
    from laenerf_amd.editing.style_image import image_blocks
    vgg = torch.full((3, S, S), float("nan"), device=DEV)
    terms = torch.full((3,), float("nan"), device=DEV)
    style_backend.style_image_forward(es, pred16, cap, m, S, vgg if flags & 32 else None, flags, image_blocks(es.max_crop_pixels), terms)
    return vgg, terms


def _kernel_backward(es, pred16, cap, m, S, gv, gt, flags):
    from laenerf_amd.backend import style_backend
    g = torch.full((cap, 3), float("nan"), device=DEV)
    style_backend.style_image_backward(es, pred16, cap, m, S, gv, gt, flags, g)
    return g


@pytest.mark.parametrize("S", [16, 40])
@pytest.mark.parametrize("flags", [ALL, 1 | 32, 1 | 2 | 8 | 16 | 32])
def test_image_forward_matches_the_torch_block(S, flags):
    from laenerf_amd.editing.style_trainer import capacity_for
    views = make_image_views(seed=1)
    es = _set(views)
    g = torch.Generator(device=DEV).manual_seed(2)
    worst = {"vgg": 0.0, "tv": 0.0, "smooth": 0.0, "disc": 0.0}
    for v, view in enumerate(views):
        K = view["x_term"].shape[0]
        cap = capacity_for(K) + 16                                           # K < cap: the pad rows hold garbage the kernels must skip
        _, _, _, m = es.sample(cap, step=v)
        pred16 = torch.rand(cap, 3, device=DEV, generator=g).half()
        vgg, terms = _kernel_forward(es, pred16, cap, m, S, flags)
        r_vgg, tv, sm, dc = _ref(view, pred16[:K], S, flags)
        if flags & 32:
            worst["vgg"] = max(worst["vgg"], float((vgg - r_vgg).abs().max()))
        for k, (name, want) in enumerate((("tv", tv), ("smooth", sm), ("disc", dc))):
            got, want = float(terms[k]), float(want)
            worst[name] = max(worst[name], abs(got - want) / max(abs(want), 1e-30) if want else abs(got))
    print("image forward: worst deviations", worst)
    assert worst["vgg"] <= 1e-6
    for name in ("tv", "smooth", "disc"):
        assert worst[name] <= 1e-5, worst


def test_image_backward_matches_autograd_and_is_deterministic():
    from laenerf_amd.editing.style_trainer import capacity_for
    views = make_image_views(seed=3)
    es = _set(views)
    S = 24
    g = torch.Generator(device=DEV).manual_seed(4)
    for v, view in enumerate(views):
        K = view["x_term"].shape[0]
        cap = capacity_for(K) + 16
        _, _, _, m = es.sample(cap, step=v)
        pred16 = torch.rand(cap, 3, device=DEV, generator=g).half()
        gv = torch.randn(3, S, S, device=DEV, generator=g)
        gt = torch.randn(3, device=DEV, generator=g)
        p = pred16[:K].float().requires_grad_(True)
        r_vgg, tv, sm, dc = _ref(view, p, S, ALL)
        ((r_vgg * gv).sum() + gt[0] * tv + gt[1] * sm + gt[2] * dc).backward()
        want = p.grad
        got = _kernel_backward(es, pred16, cap, m, S, gv, gt, ALL)
        dev = float((got[:K] - want).abs().max() / want.abs().max())
        assert dev <= 1e-4, (v, dev)
        assert torch.equal(got[K:], torch.zeros_like(got[K:]))               # pad rows: exactly 0
        again = _kernel_backward(es, pred16, cap, m, S, gv, gt, ALL)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        if v == 0:
            out = torch.empty_like(got)
            from laenerf_amd.backend import style_backend
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                style_backend.style_image_backward(es, pred16, cap, m, S, gv, gt, ALL, out)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), out.view(torch.int32))


def _model(seed, P=8):
    from laenerf_amd.editing import LAENeRF
    params = SimpleNamespace(bound=1, num_palette_bases=P, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(seed)
    m = LAENeRF(params, dir_encoding="sphere_harmonics").to(DEV)
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m, params


def _style_net(S=32, seed=0, he=False):
    from laenerf_amd.editing import StyleNetwork
    from laenerf_amd.editing.style_network import vgg19_features
    torch.manual_seed(seed)
    vgg = vgg19_features(14).to(DEV)
    if he:                                     # He-scaled weights: features of order one, as a trained VGG gives (torch's default is ~100x smaller)
        for layer in vgg:
            if isinstance(layer, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
                torch.nn.init.zeros_(layer.bias)
    return StyleNetwork(striped_style(), vgg, size=S, generator=torch.Generator().manual_seed(seed))


def _style_params(params, **kw):
    p = SimpleNamespace(**vars(params))
    p.__dict__.update(dict(style_weight=1e3, tv_weight=1e-3, tv_depth_guide=True, depth_disc_weight=1e-3, smooth_trans_weight=1e-3,
                           warmup_iterations=-1, crop_size=32))
    p.__dict__.update(kw)
    return p


def test_one_style_step_matches_the_reference_chain():
    from laenerf_amd.editing.style_image import style_image
    from laenerf_amd.editing.style_trainer import capacity_for
    m, base = _model(6)
    m.train()
    params = _style_params(base, style_weight=1.0)                          # the reference chain's fp16 dL/dpred must not overflow
    net = _style_net()
    views = make_image_views(seed=6)
    es = _set(views)
    v = 4                                                                    # the full-image crop
    K = views[v]["x_term"].shape[0]
    cap = capacity_for(K)
    x, d, t, k = es.sample(cap, step=v)
    w = {"style": params.style_weight, "tv": params.tv_weight, "sm": params.smooth_trans_weight, "dc": params.depth_disc_weight}
    with torch.autocast("cuda", dtype=torch.float16):
        loss, pred, _, _, pred32 = m.forward_train_loss(x, d, t, params, None, with_palet_loss=True, m_dev=k, with_pred32=True)
    vgg_in, terms = style_image(pred32, pred, es, cap, k, 32, ALL, 4)
    style = net.loss_from_input(vgg_in)
    total = loss + (style.half() * w["style"]).float() + (terms[0].half() * w["tv"]).float() + (terms[1].half() * w["sm"]).float() \
        + (terms[2].half() * w["dc"]).float()
    (total * 128.0).backward()
    params_of = (("table", m.encoder.embeddings), ("wn", m.weight_net.weights), ("on", m.offset_net.weights), ("pal", m.color_palette))
    got = {key: (p.grad / 128.0).clone() for key, p in params_of}
    got_terms = torch.stack((style, terms[0], terms[1], terms[2])).detach().clone()
    m.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        rp, rw, ro = m.forward_train(x[:K], d[:K])
        ref = torch.nn.functional.mse_loss(rp.float(), t[:K])
        ref = ref + m.weights_loss(rw.float(), params).half()
        ref = ref + m.offset_loss(ro.float(), params).half()
        ref = ref + m.palet_loss(params).half()
    r_vgg, tv, sm, dc = _ref(views[v], rp, 32, ALL)
    r_style = net.loss_from_input(r_vgg)
    ref = ref + r_style.half() * w["style"] + tv.half() * w["tv"] + sm.half() * w["sm"] + dc.half() * w["dc"]
    (ref * 128.0).backward()
    want_terms = torch.stack((r_style, tv, sm, dc)).detach()
    finite = {key: (bool(torch.isfinite(got[key]).all()), bool(torch.isfinite(p.grad).all())) for key, p in params_of}
    assert all(a and b for a, b in finite.values()), finite
    dev = {"loss": abs(total.item() - ref.item()) / abs(ref.item()),
           "terms": float(((got_terms - want_terms).abs() / want_terms.abs()).max())}
    for key, p in params_of[1:]:
        r = N(p.grad) / 128.0
        dev["g_" + key] = float(np.abs(N(got[key]) - r).max() / np.abs(r).max())
    gt_, rt = N(got["table"]), N(m.encoder.embeddings.grad) / 128.0
    dev["g_table"] = float(np.linalg.norm(gt_ - rt) / np.linalg.norm(rt))
    print("style step vs the reference chain:", {key: float("%.3g" % val) for key, val in dev.items()})
    assert dev["terms"] <= 1e-4, dev
    for key, val in dev.items():
        if key in STYLE_TOL:
            assert val < STYLE_TOL[key], dev


def _train(graph, steps=64, seed=7):
    from laenerf_amd.editing import StyleTrainer
    m, base = _model(seed)
    params = _style_params(base, warmup_iterations=16)                      # the gate opens at step 32
    es = _set(make_image_views(seed=seed))
    tr = StyleTrainer(m, es, params, iters=steps, distill_palette_steps=-1, seed=3, graph=graph, style_net=_style_net())
    tr.train(steps)
    torch.cuda.synchronize()
    return tr


def test_graph_replay_equals_eager_steps_across_the_warmup_gate():
    a, b = _train(True), _train(False)
    la, lb = a.losses(), b.losses()
    ta, tb = a.terms(), b.terms()
    assert np.all(ta[:32] == 0) and np.all(ta[32:, 0] > 0)                 # no image terms before the gate, the style term after
    rel = lambda x, y: float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))
    dev = {"loss": rel(la, lb), "terms": rel(ta, tb)}
    for (pa, *_), (pb, *_) in zip(a.opt.items, b.opt.items):
        dev[str(tuple(pa.shape))] = rel(N(pa.float()), N(pb.float()))
    ident = np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and all(torch.equal(pa, pb) for (pa, *_), (pb, *_) in zip(a.opt.items, b.opt.items))
    print("graph vs eager over 64 steps:", dev, "bit-identical:", ident, "captures:", a.captures, "capture_error:", a.capture_error)
    for val in dev.values():
        assert val <= 1e-6, dev


def test_zero_depth_discontinuity_maximum_is_skipped():
    from laenerf_amd.editing import StyleTrainer
    m, base = _model(8)
    params = _style_params(base, style_weight=0, tv_weight=1e-3)
    views = [make_image_view((2, 21, 3, 27), 81), make_image_view((3, 15, 4, 20), 82, w8_low=True)]
    es = _set(views)
    assert N(es.image["vmax"])[1].tolist() == [0.0, 0.0]
    tr = StyleTrainer(m, es, params, iters=16, distill_palette_steps=-1, seed=1, graph=False)
    tr.train(16)
    n_bad = int((tr._sched[:16] == 1).sum())
    lo = tr.losses()
    assert np.isnan(lo[tr._sched[:16] == 1]).all() and np.isfinite(lo[tr._sched[:16] == 0]).all()
    assert tr.steps_skipped == n_bad, (tr.steps_skipped, n_bad)


def test_stylization_lowers_the_gram_term_then_distills():
    from laenerf_amd.editing import StyleTrainer, distill_images
    from test_gpu_distill import network_case
    m, base = _model(9)
    params = _style_params(base, style_weight=1e3, tv_weight=0, depth_disc_weight=0, smooth_trans_weight=0, tv_depth_guide=False)
    es = _set(make_image_views(seed=9))
    tr = StyleTrainer(m, es, params, iters=320, distill_palette_steps=-1, seed=2, graph=True, lr=1e-2, style_net=_style_net(seed=9, he=True))
    tr.train(320)
    st = tr.terms()[:, 0]
    first, last = float(st[:32].mean()), float(st[-32:].mean())
    print(f"Gram term: first 32 steps {first:.4g}, last 32 {last:.4g}, factor {first / last:.3g}; capture_error {tr.capture_error}")
    assert last * 2 < first
    c, s, data = network_case(5)
    out = distill_images(data, m, s)
    assert torch.isfinite(out.images.float()).all()
