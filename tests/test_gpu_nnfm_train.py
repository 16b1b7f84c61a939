"""-m gpu: the NNFM style loss inside the stylization step (StyleTrainer with image terms): one step against the reference-shaped
chain with nnfm_numpy's gradient, graph replay against eager steps across the warm-up gate, a short fit, the colour-matched target,
and the unchanged Gram path.  Built on the helpers of style_mode_util and test_gpu_style_mode (a small random VGG, S = 32: 8 x 8
positions, 3 x 256 channels)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import DEV, N
from style_mode_util import make_image_views, striped_style
from test_gpu_style_mode import ALL, STYLE_TOL, _model, _ref, _set, _style_params

pytestmark = pytest.mark.gpu


def _style_net(S=32, seed=0, he=False, **kw):
    """test_gpu_style_mode._style_net with the StyleNetwork's keyword arguments open"""
    from laenerf_amd.editing import StyleNetwork
    from laenerf_amd.editing.style_network import vgg19_features
    torch.manual_seed(seed)
    vgg = vgg19_features(14).to(DEV)
    if he:
        for layer in vgg:
            if isinstance(layer, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
                torch.nn.init.zeros_(layer.bias)
    return StyleNetwork(striped_style(), vgg, size=S, generator=torch.Generator().manual_seed(seed), **kw)


class _given_gradient(torch.autograd.Function):
    """a scalar with a given value whose gradient with respect to `feats` is a given tensor (nnfm_numpy's, at a fixed match)"""

    @staticmethod
    def forward(ctx, feats, value, grad):
        ctx.save_for_backward(grad)
        return value.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def _nnfm_reference(net, vgg_in, z):
    """the NNFM term of the VGG input from torch ops (the VGG) plus nnfm_numpy (float64 loss and gradient at the match z)"""
    from laenerf_amd.editing import nnfm_numpy
    from laenerf_amd.editing.nnfm import _as_problems
    feats = net.features(vgg_in)
    f = _as_problems(feats, net.nnfm_match)
    s = _as_problems(net.nnfm_target, net.nnfm_match)
    _, loss64, dx64, _ = nnfm_numpy(N(f), N(s), z=N(z))
    grad = torch.from_numpy(dx64).to(DEV, torch.float32).reshape(feats.shape)
    return _given_gradient.apply(feats, torch.tensor(loss64, dtype=torch.float32, device=DEV), grad)


@pytest.mark.parametrize("match", ["concat", "layer"])
def test_one_nnfm_style_step_matches_the_reference_chain(match):
    from laenerf_amd.editing import nnfm_match
    from laenerf_amd.editing.nnfm import _as_problems
    from laenerf_amd.editing.style_image import style_image
    from laenerf_amd.editing.style_trainer import capacity_for
    m, base = _model(6)
    m.train()
    params = _style_params(base, style_weight=1.0)
    net = _style_net(he=True, loss="nnfm", nnfm_match=match)
    assert tuple(net.nnfm_target.shape) == (3, 256, 64)
    views = make_image_views(seed=6)
    es = _set(views)
    v = 4
    K = views[v]["x_term"].shape[0]
    cap = capacity_for(K)
    x, d, t, k = es.sample(cap, step=v)
    w = {"style": params.style_weight, "tv": params.tv_weight, "sm": params.smooth_trans_weight, "dc": params.depth_disc_weight}
    with torch.autocast("cuda", dtype=torch.float16):
        loss, pred, _, _, pred32 = m.forward_train_loss(x, d, t, params, None, with_palet_loss=True, m_dev=k, with_pred32=True)
    vgg_in, terms = style_image(pred32, pred, es, cap, k, 32, ALL, 4)
    style = net.loss_from_input(vgg_in)
    with torch.no_grad():
        z = nnfm_match(_as_problems(net.features(vgg_in), match), _as_problems(net.nnfm_target, match))     # the step's own match
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
    r_style = _nnfm_reference(net, r_vgg, z)
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
    print(f"nnfm ({match}) style step vs the reference chain:", {key: float("%.3g" % val) for key, val in dev.items()}, "style term", float(style.detach()))
    assert float(style.detach()) > 0
    assert dev["terms"] <= 1e-4, dev
    for key, val in dev.items():
        if key in STYLE_TOL:
            assert val < STYLE_TOL[key], dev


def _train(graph, steps=64, seed=7, **net_kw):
    from laenerf_amd.editing import StyleTrainer
    m, base = _model(seed)
    params = _style_params(base, warmup_iterations=16)                      # the gate opens at step 32
    es = _set(make_image_views(seed=seed))
    tr = StyleTrainer(m, es, params, iters=steps, distill_palette_steps=-1, seed=3, graph=graph, style_net=_style_net(**net_kw))
    tr.train(steps)
    torch.cuda.synchronize()
    return tr


def _same_bits(a, b):
    return np.array_equal(a.losses().view(np.uint32), b.losses().view(np.uint32)) and \
        np.array_equal(a.terms().view(np.uint32), b.terms().view(np.uint32)) and \
        all(torch.equal(pa, pb) for (pa, *_), (pb, *_) in zip(a.opt.items, b.opt.items))


def test_nnfm_graph_replay_equals_eager_steps_across_the_warmup_gate():
    a, b = _train(True, loss="nnfm"), _train(False, loss="nnfm")
    ta = a.terms()
    assert np.all(ta[:32] == 0) and np.all(ta[32:, 0] > 0)                 # no image terms before the gate, the NNFM term after
    print("nnfm graph vs eager over 64 steps: captures", a.captures, "capture_error", a.capture_error,
          "largest loss difference", float(np.abs(a.losses() - b.losses()).max()))
    assert a.capture_error is None and a.captures >= 1                     # the NNFM step runs inside the captured image-step graph
    assert _same_bits(a, b)


def test_stylization_lowers_the_nnfm_term():
    from laenerf_amd.editing import StyleTrainer
    m, base = _model(9)
    params = _style_params(base, style_weight=1.0, tv_weight=0, depth_disc_weight=0, smooth_trans_weight=0, tv_depth_guide=False)
    es = _set(make_image_views(seed=9))
    tr = StyleTrainer(m, es, params, iters=64, distill_palette_steps=-1, seed=2, graph=True, lr=1e-2,
                      style_net=_style_net(seed=9, he=True, loss="nnfm"))
    tr.train(64)
    st = tr.terms()[:, 0]
    first, last = float(st[:16].mean()), float(st[-16:].mean())
    print(f"NNFM term: first 16 steps {first:.4g}, last 16 {last:.4g}; capture_error {tr.capture_error}")
    assert np.isfinite(st).all() and (st > 0).all()
    assert last < first


def test_match_color_and_reset_keep_the_nnfm_buffers_in_place():
    from laenerf_amd.editing import nnfm_pack
    from laenerf_amd.editing.nnfm import _as_problems
    net = _style_net(he=True, loss="nnfm", nnfm_match="layer")
    ptrs = (net.nnfm_target.data_ptr(), net.nnfm_packed.data_ptr())
    before = net.nnfm_target.clone()
    assert torch.equal(net.nnfm_packed, nnfm_pack(_as_problems(net.nnfm_style, "layer")))
    net.match_color(torch.rand(3, 50, device=DEV))
    assert (net.nnfm_target.data_ptr(), net.nnfm_packed.data_ptr()) == ptrs
    assert not torch.equal(net.nnfm_target, before)
    assert torch.equal(net.nnfm_packed, nnfm_pack(_as_problems(net.nnfm_target, "layer")))
    net.reset_target()
    assert (net.nnfm_target.data_ptr(), net.nnfm_packed.data_ptr()) == ptrs
    assert torch.equal(net.nnfm_target, before) and torch.equal(net.nnfm_packed, nnfm_pack(_as_problems(before, "layer")))


def test_a_style_side_packed_in_the_other_arrangement_is_refused():
    from laenerf_amd.editing import nnfm_loss, nnfm_pack
    from laenerf_amd.editing.nnfm import _as_problems
    x = torch.randn(3, 32, 64, device=DEV)
    s = torch.randn(3, 32, 64, device=DEV)
    by_layer, concat = nnfm_pack(_as_problems(s, "layer")), nnfm_pack(_as_problems(s, "concat"))
    assert by_layer.numel() == concat.numel()                       # the same byte count: only the shape tells them apart
    with pytest.raises(ValueError):
        nnfm_loss(x, s, packed_style=by_layer, match="concat")
    with pytest.raises(ValueError):
        nnfm_loss(x, s, packed_style=concat, match="layer")
    assert torch.equal(nnfm_loss(x, s, packed_style=concat, match="concat"), nnfm_loss(x, s, match="concat"))


def test_laenerf_builds_the_nnfm_style_network_from_params():
    from laenerf_amd.editing import LAENeRF
    from laenerf_amd.editing.style_network import vgg19_features
    params = SimpleNamespace(bound=1, num_palette_bases=4, style_weight=1.0, style_loss="nnfm", nnfm_match="layer")
    vgg = vgg19_features(14).to(DEV)
    m = LAENeRF(params, size=32, style_img=striped_style().to(DEV), vgg=vgg, style_generator=torch.Generator().manual_seed(1))
    assert m.style_transfer_net.loss_kind == "nnfm" and m.style_transfer_net.nnfm_match == "layer"
    params = SimpleNamespace(bound=1, num_palette_bases=4, style_weight=1.0)
    m = LAENeRF(params, size=32, style_img=striped_style().to(DEV), vgg=vgg, style_generator=torch.Generator().manual_seed(1))
    assert m.style_transfer_net.loss_kind == "gram" and not hasattr(m.style_transfer_net, "nnfm_target")


def test_gram_steps_keep_their_bits():
    # the default network, an explicit loss="gram" and the Gram formula as it stood before the switch: same kernels, same order
    from laenerf_amd.editing.style_network import gram_matrix
    a, b = _train(True, steps=48), _train(True, steps=48, loss="gram")
    assert _same_bits(a, b)
    net = _style_net()
    net.loss_from_input = lambda v: torch.nn.functional.mse_loss(gram_matrix(net.features(v)), net.gram_target)
    from laenerf_amd.editing import StyleTrainer
    m, base = _model(7)
    params = _style_params(base, warmup_iterations=16)
    c = StyleTrainer(m, _set(make_image_views(seed=7)), params, iters=48, distill_palette_steps=-1, seed=3, graph=True, style_net=net)
    c.train(48)
    torch.cuda.synchronize()
    assert _same_bits(a, c)
