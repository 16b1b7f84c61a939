"""-m gpu: the Ref-NPR second stage on the device (csrc/ref_stage.hip, editing/ref_stage.py, editing/semantic_encoder.py): the
registered terms against their float64 restatement, the criterion with the MSE switched off, one step of each phase against the
reference-shaped torch chain, the supervision's matches, graph replay against eager steps across the phase switch, save / resume,
and a short fit on recoloured views."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gpu_util import DEV, N
from laenerf_amd.editing.ref_stage import (GT, REF, RefEditSet, RefStyleTrainer, ref_stage_numpy, reference_ref_step)
from laenerf_amd.editing.semantic_encoder import SemanticEncoder, build_ref_supervision, vgg16_features
from laenerf_amd.editing.style_trainer import capacity_for
from ref_stage_util import H_REF, W_REF, make_ref_view, make_ref_views
from test_gpu_style_mode import STYLE_TOL, _model

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FS = 32                                          # feature_size: 8 x 8 positions at relu3, C = 256


def _he_vgg16(last, seed=0):
    """seeded He-initialised VGG-16 layers: features of order one, as a trained VGG gives"""
    torch.manual_seed(seed)
    vgg = vgg16_features(last)
    for layer in vgg:
        if isinstance(layer, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(layer.weight, nonlinearity="relu")
            torch.nn.init.zeros_(layer.bias)
    return vgg.to(DEV)


@functools.lru_cache(maxsize=None)
def _sem():
    return SemanticEncoder(_he_vgg16(29))


def _template(seed=11):
    """a synthetic template view: the painted image is a recoloured copy of the original on the mask"""
    v = make_ref_view(seed, reg="all")
    img = v["image"]
    x0, x1, y0, y1 = (int(b) for b in v["cut_min_max_xy"])
    painted = torch.zeros(H_REF, W_REF, 3)
    painted[..., 0], painted[..., 1], painted[..., 2] = img[..., 2], 1.0 - img[..., 0] * img[..., 3], img[..., 1]
    painted = painted * img[..., 3:]
    return {"painted": painted, "original": img[..., :3].clone(), "box": (x0, x1, y0, y1)}


@functools.lru_cache(maxsize=None)
def _case(seed=0):
    """three views (R = 0, R = K, 0 < R < K) with the real supervision, computed once and shared (never modified)"""
    views = make_ref_views(seed=seed)
    sup = build_ref_supervision(views, _template(), _sem(), feature_size=FS)
    return views, sup


def _params(base, **kw):
    p = SimpleNamespace(**vars(base))
    p.__dict__.update(dict(style_weight=0, tv_weight=1e-3, tv_depth_guide=True, depth_disc_weight=1e-3, smooth_trans_weight=0, intensity_weight=0,
                           warmup_iterations=16, mse_loss=6.0, cos_loss_factor=2.5, color_patch_loss=30.0, feature_size=FS))
    p.__dict__.update(kw)
    return p


def test_ref_terms_match_the_float64_restatement():
    """lae_ref_terms_forward / _backward on 70 x 83 views with R = 0, R = K and 0 < R < K, both modes, cap = capacity_for(K) + 16 with
    NaN in every pad row the kernels must not read.
    Bound of the two sums: the kernel forms residuals, squares and sums in fp64 (each term and each of the n additions within 2^-53)
    and rounds the mean to fp32 once (2^-24); the restatement carries n * 2^-53 of its own.  With n <= 3 * 6000 terms that is
    2^-24 + 2 n 2^-53 < 2 * 2^-24 relative -- far inside n_terms * 2^-24.  The gradient is formed in fp64 and rounded once as well:
    8 * 2^-24 relative per element."""
    from laenerf_amd.backend import ref_stage_backend as be
    views, sup = _case()
    es = RefEditSet.from_views(views, (H_REF, W_REF), supervision=sup, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    nan = float("nan")
    worst = {"sum": 0.0, "grad": 0.0}
    for v, view in enumerate(views):
        K = view["x_term"].shape[0]
        assert K % 16 and K > 256
        cap = capacity_for(K) + 16
        o = int(es.offsets_host[v])
        rh = es.ref_host
        for mode in (GT, REF):
            _, _, t, m = es.sample(cap, step=v)
            assert int(m) == K
            t[K:] = nan
            pred16 = torch.rand(cap, 3, device=DEV, generator=gen).half()
            pred16[K:] = nan
            g_predw = torch.randn(cap, 3, device=DEV, generator=gen)
            g_predw[K:] = nan
            g_terms = torch.randn(2, device=DEV, generator=gen)

            def run(gp=g_predw):
                p16 = torch.full((cap, 3), nan, dtype=torch.float16, device=DEV)
                p32 = torch.full((cap, 3), nan, device=DEV)
                resid = torch.full((es.n_out if mode == REF else 0, 3), nan, dtype=torch.float64, device=DEV)
                terms = torch.full((2,), nan, device=DEV)
                g = torch.full((cap, 3), nan, device=DEV)
                be.forward(es, pred16, cap, m, t, mode, p16, p32, resid, terms)
                be.backward(es, pred16, cap, m, t, mode, resid, gp, g_terms, g)
                return p16, p32, terms, g
            p16, p32, terms, g = run()
            want = ref_stage_numpy(N(pred16[:K]).astype(np.float16), rh["w8s16"][o:o + K], mode, target=N(t[:K]), ref_target=rh["ref_target"][o:o + K],
                                   ref_weight=rh["ref_weight"][o:o + K], R=rh["ref_count"][v], tap_row=rh["tap_row"][v], tap_w=rh["tap_w"][v],
                                   color_patch=rh["color_patch"][v], g_predw=N(g_predw[:K]), g_terms=N(g_terms))
            assert np.array_equal(p16[:K].cpu().numpy().view(np.uint16), want["predw"].view(np.uint16))           # pred': bit for bit
            assert torch.equal(p32[:K], p16[:K].float())
            assert not p16[K:].any() and not p32[K:].any()
            got_t = N(terms).astype(np.float64)
            for k in range(2):
                if want["terms"][k] == 0.0:
                    assert got_t[k] == 0.0, (v, mode, k, got_t)
                else:
                    worst["sum"] = max(worst["sum"], abs(got_t[k] - want["terms"][k]) / want["terms"][k])
            if mode == REF:
                assert want["terms"][1] > 0 and (rh["ref_count"][v] == 0) == (want["terms"][0] == 0.0)
            gg, gw = N(g[:K]).astype(np.float64), want["g_pred"]
            assert np.isfinite(gg).all() and (gw != 0).all()
            worst["grad"] = max(worst["grad"], float((np.abs(gg - gw) / np.abs(gw)).max()))
            assert torch.equal(g[K:], torch.zeros_like(g[K:]))                                                     # pad rows: exactly 0
            # no upstream gradient for pred': the two terms' parts alone
            _, _, _, g_none = run(None)
            w_none = ref_stage_numpy(N(pred16[:K]).astype(np.float16), rh["w8s16"][o:o + K], mode, target=N(t[:K]), ref_target=rh["ref_target"][o:o + K],
                                     ref_weight=rh["ref_weight"][o:o + K], R=rh["ref_count"][v], tap_row=rh["tap_row"][v], tap_w=rh["tap_w"][v],
                                     color_patch=rh["color_patch"][v], g_terms=N(g_terms))["g_pred"]
            gn = N(g_none[:K]).astype(np.float64)
            assert np.array_equal(gn == 0, w_none == 0)
            nz = w_none != 0
            if nz.any():
                worst["grad"] = max(worst["grad"], float((np.abs(gn - w_none)[nz] / np.abs(w_none)[nz]).max()))
            # two runs and one graph replay: the same bits
            again = run()
            for a, b in zip((p16, p32, terms, g), again):
                assert torch.equal(a[:K].view(torch.int16 if a.dtype == torch.float16 else torch.int32), b[:K].view(torch.int16 if b.dtype == torch.float16 else torch.int32))
            if v == 2:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    rep = run()
                graph.replay()
                torch.cuda.synchronize()
                for a, b in zip((p16, p32, terms, g), rep):
                    assert torch.equal(a[:K].view(torch.int16 if a.dtype == torch.float16 else torch.int32), b[:K].view(torch.int16 if b.dtype == torch.float16 else torch.int32))
    print("ref_terms vs float64: worst relative deviations", worst, "in units of 2^-24:", {k: val / U for k, val in worst.items()})
    assert worst["sum"] <= 2 * U
    assert worst["grad"] <= 8 * U


def test_criterion_with_the_mse_switched_off():
    """mse_weight = 0: FIN_LOSS is the fp16-rounded regularisers summed in the node's order, bit for bit (0 * mse + x = x); the parameter
    gradients are those of mse_weight = 1 minus the MSE's, the latter through the existing torch formulation.  Both operands of that
    difference carry STYLE_TOL relative to the full gradient, so the deviation is measured against the full gradient's size."""
    m, params = _model(21)
    m.train()
    views, _ = _case()
    es = RefEditSet.from_views(views, (H_REF, W_REF), device=DEV)
    K = views[2]["x_term"].shape[0]
    cap = capacity_for(K)
    x, d, t, k = es.sample(cap, step=2)
    keys = (("table", m.encoder.embeddings), ("wn", m.weight_net.weights), ("on", m.offset_net.weights), ("pal", m.color_palette))

    def grads(fn):
        m.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            loss = fn()
        (loss * (1.0 if getattr(loss, "terms", None) is not None else 128.0)).backward()
        return {key: (p.grad / 128.0).clone() for key, p in keys}, loss
    scale = torch.full((1,), 128.0, device=DEV)
    g0, l0 = grads(lambda: m.forward_train_loss(x, d, t, params, scale, with_palet_loss=True, m_dev=k, mse_weight=0.0)[0])
    fin = N(l0.terms).astype(np.float32)
    h = lambda val: np.float32(np.float16(val))
    want = np.float32(np.float32(h(fin[3] + fin[4]) + h(fin[5])) + h(fin[8]))
    assert fin[1] == want and fin[0] == np.float32(want * np.float32(128.0)), (fin, want)
    g1, l1 = grads(lambda: m.forward_train_loss(x, d, t, params, scale, with_palet_loss=True, m_dev=k)[0])
    f1 = N(l1.terms)
    assert f1[2] == fin[2] and f1[2] > 0                                       # FIN_MSE: still the diagnostic MSE
    assert f1[1] == np.float32(np.float32(np.float32(f1[2] + h(f1[3] + f1[4])) + h(f1[5])) + h(f1[8]))
    gm, _ = grads(lambda: torch.nn.functional.mse_loss(m.forward_train(x[:K], d[:K])[0].float(), t[:K]))
    dev = {}
    for key, _ in keys:
        full, want_g, got_g = N(g1[key]), N(g1[key]) - N(gm[key]), N(g0[key])
        assert np.isfinite(got_g).all()
        if key == "table":
            dev["g_table"] = float(np.linalg.norm(got_g - want_g) / np.linalg.norm(full))
        else:
            dev["g_" + key] = float(np.abs(got_g - want_g).max() / np.abs(full).max())
    print("mse_weight=0 gradients vs (mse_weight=1) - MSE:", {key: float("%.3g" % val) for key, val in dev.items()})
    for key, val in dev.items():
        assert val < STYLE_TOL[key], dev
    assert float(np.abs(N(g0["wn"])).max()) > 0

    # mse_w = 1.0 through the new entry points: the bits of the existing ones
    from laenerf_amd.backend import style_backend as sb
    gen = torch.Generator(device=DEV).manual_seed(5)
    M, P, mask = cap, 8, 0b10111011
    na = bin(mask).count("1")
    wl, ol = torch.randn(M, 16, device=DEV, generator=gen).half(), torch.randn(M, 16, device=DEV, generator=gen).half()
    pal = torch.rand(P, 3, device=DEV, generator=gen)
    pred, w_hat, o_hat = torch.empty(M, 3, dtype=torch.half, device=DEV), torch.empty(M, na, device=DEV), torch.empty(M, 3, dtype=torch.half, device=DEV)
    sb.palette_forward(wl, ol, pal, P, mask, M, pred, w_hat, o_hat)
    lw, reg_w = (1e-3, 1e-3, 1e-2), (1.0, 1e-2)
    up = torch.ones(1, device=DEV)
    g_pred = torch.randn(M, 3, device=DEV, generator=gen)
    out = []
    for mse_w in (None, 1.0):
        fin = torch.zeros(12, device=DEV)
        sb.style_loss_forward(pred, t, w_hat, o_hat, M, na, lw, scale, fin, reg_palette=pal, reg_w=reg_w, m_dev=k, mse_w=mse_w)
        gwl, gol, gp = torch.empty_like(wl), torch.empty_like(ol), torch.empty_like(pal)
        sb.style_loss_backward_image(wl, ol, pal, P, mask, M, t, fin, up, lw, g_pred, gwl, gol, gp, k, reg_w=reg_w, mse_w=mse_w)
        out.append((fin[:9].clone(), gwl, gol, gp))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32), b.view(torch.int16 if b.dtype == torch.float16 else torch.int32))
    assert float(out[0][0][2]) > 0


def _trainer(seed, graph, steps=64, views=None, sup=None, **kw):
    m, base = _model(seed)
    if views is None:
        views, sup = _case()
    es = RefEditSet.from_views(views, (H_REF, W_REF), supervision=sup, device=DEV)
    lr = kw.pop("lr", 1e-3)
    params = _params(base, **kw)
    sem = _sem() if params.cos_loss_factor > 0 else None
    return RefStyleTrainer(m, es, params, iters=steps, sem=sem, distill_palette_steps=-1, seed=3, graph=graph, lr=lr), views, sup


def _opt_grads(tr, scale):
    """the gradients as the trainer's FusedAdam holds them (fp16 accumulators of the table and the MLP weights, the palette's .grad)"""
    m = tr.enc
    names = {id(m.encoder.embeddings): "table", id(m.weight_net.weights): "wn", id(m.offset_net.weights): "on", id(m.color_palette): "pal"}
    out = {}
    for p, _, _, shadow, _ in tr.opt.items:
        g = shadow.grad_half.float() if shadow is not None else p.grad.float()
        if shadow is not None and p.grad is not None:
            g = g + p.grad.float()
        out[names[id(p)]] = (g / scale).clone()
    assert sorted(out) == ["on", "pal", "table", "wn"]
    return out


@pytest.mark.parametrize("phase", [REF, GT])
def test_one_step_matches_the_reference_chain(phase):
    """step_loss (the trainer's own sum) against reference_ref_step on the view with 0 < R < K: loss and terms within 1e-4 relative,
    parameter gradients within STYLE_TOL (tests/test_gpu_style_mode.py's tolerances for the same kind of comparison)."""
    tr, views, sup = _trainer(31, graph=False)
    m, es = tr.enc, tr.es
    m.train()
    v = 2
    s = int(np.nonzero(tr._sched == v)[0][0])
    K = views[v]["x_term"].shape[0]
    cap = capacity_for(K)
    es.step.fill_(s)
    scale = torch.full((1,), 128.0, device=DEV)
    total, loss, acc, reg, patch, cos, tv, disc = tr.step_loss(cap, phase == REF, scaler=scale)
    tr.opt.zero_grad()
    total.backward()
    got = _opt_grads(tr, 128.0)
    got_loss = float(total.detach()) / 128.0
    got_terms = {key: float(val.detach()) for key, val in (("reg", reg), ("patch", patch), ("cos", cos), ("tv", tv), ("disc", disc))}
    x, d, t, _ = es._buffers(cap)
    tr.opt.zero_grad()
    ref, want_terms = reference_ref_step(m, tr.params, x[:K], d[:K], t[:K], views[v], (H_REF, W_REF), phase, sem=_sem(), style_feat=es.style_feat,
                                         tmpl_z=es.tmpl_z[v], color_patch=sup["color_patch"][v].to(DEV))
    (ref * 128.0).backward()
    want = _opt_grads(tr, 128.0)
    dev = {"loss": abs(got_loss - ref.item()) / abs(ref.item())}
    for key, val in want_terms.items():
        val = float(val)
        if phase == GT and key != "reg":
            assert got_terms[key] == 0.0 and val == 0.0
        else:
            assert val != 0.0, key
            dev["term_" + key] = abs(got_terms[key] - val) / abs(val)
    for key in ("wn", "on", "pal"):
        r = N(want[key])
        assert np.isfinite(N(got[key])).all() and np.isfinite(r).all() and np.abs(r).max() > 0
        dev["g_" + key] = float(np.abs(N(got[key]) - r).max() / np.abs(r).max())
    gt_, rt = N(got["table"]), N(want["table"])
    dev["g_table"] = float(np.linalg.norm(gt_ - rt) / np.linalg.norm(rt))
    print("phase", phase, "step vs the reference chain:", {key: float("%.3g" % val) for key, val in dev.items()}, "terms", got_terms)
    for key, val in dev.items():
        assert val < (STYLE_TOL[key] if key in STYLE_TOL and key != "loss" else 1e-4), dev


def test_supervision_matches_within_the_fp16_margin():
    """build_ref_supervision: for every position the float64 cosine distance of the chosen template column is within the matcher's
    fp16 margin of the float64 best (tests/test_gpu_nnfm.py's criterion and its bound COS_TOL = 2^-8: fp16-rounded unit vectors move
    a cosine by at most 2^-10, fp32 accumulation by C * 2^-24, and two cosines are compared).  No index equality is asserted."""
    from laenerf_amd.editing.nnfm import nnfm_numpy
    from test_gpu_nnfm import COS_TOL
    views, sup = _case()
    sem = _sem()
    P = (FS // 4) ** 2
    assert tuple(sup["tmpl_z"].shape) == (len(views), 3, P) and sup["tmpl_z"].dtype == torch.int32
    assert tuple(sup["style_feat"].shape) == (3, 256, P) and tuple(sup["content_feat"].shape) == (3, 256, P)
    ph, pw = H_REF // 16, W_REF // 16
    assert tuple(sup["color_patch"].shape) == (len(views), 3, ph, pw) and sup["patch_hw"] == (ph, pw)
    content = N(sup["content_feat"])
    for v, view in enumerate(views):
        f = sem.encode_feats(view["cut_gt"].to(DEV).permute(2, 0, 1), (11, 13, 15), (FS, FS)).flatten(2)
        _, _, _, cosm = nnfm_numpy(N(f), content)
        z = N(sup["tmpl_z"][v]).astype(np.int64)
        assert z.min() >= 0 and z.max() < P
        chosen = np.take_along_axis(cosm, z[..., None], 2)[..., 0]
        worst = float((cosm.max(2) - chosen).max())
        assert worst <= COS_TOL, (v, worst)
        cols = N(sup["patch_mean_color"]).T                                     # [N5, 3]
        got = N(sup["color_patch"][v]).reshape(3, -1).T
        assert all((np.abs(cols - c).sum(1) == 0).any() for c in got)            # values only from patch_mean_color's columns


def _run(graph, steps=64, **kw):
    tr, _, _ = _trainer(41, graph, steps, **kw)
    tr.train(steps)
    torch.cuda.synchronize()
    return tr


def _same(a, b):
    ok = np.array_equal(a.losses().view(np.uint32), b.losses().view(np.uint32)) and np.array_equal(a.terms().view(np.uint32), b.terms().view(np.uint32)) \
        and np.array_equal(a.mse().view(np.uint32), b.mse().view(np.uint32))
    return ok and all(torch.equal(pa, pb) for (pa, *_), (pb, *_) in zip(a.opt.items, b.opt.items))


def test_graph_replay_equals_eager_steps_across_the_phase_switch():
    a, b = _run(True), _run(False)
    ta = a.terms()
    print("graph vs eager over 64 steps: captures", a.captures, "cache misses", a.cache_misses, "capture_error:", a.capture_error)
    assert ta.shape == (64, 6) and np.all(ta[:32] == 0) and np.all(ta[32:, 4] > 0) and np.all(ta[32:, 5] > 0)    # gt phase, then cos and patch
    assert np.isfinite(a.losses()).all() and a.captures > 0
    assert all(isinstance(k[1], bool) for k in a.graphs) and {k[1] for k in a.graphs} == {False, True} or a.capture_error is not None
    assert _same(a, b)


def test_save_and_resume_continue_bit_for_bit(tmp_path):
    from laenerf_amd.editing import EditSet, StyleTrainer
    whole = _run(True)
    first, _, _ = _trainer(41, True, 64)
    first.train(24)
    path = str(tmp_path / "ref_stage.pt")
    first.save_checkpoint(path)
    second, views, _ = _trainer(43, True, 64)                                 # fresh objects, other initial weights
    second.load_checkpoint(path)
    second.train(40)
    torch.cuda.synchronize()
    assert second.global_step == 64
    assert np.array_equal(second.losses().view(np.uint32), whole.losses()[24:].view(np.uint32))
    assert np.array_equal(second.terms().view(np.uint32), whole.terms()[24:].view(np.uint32))
    assert all(torch.equal(pa, pb) for (pa, *_), (pb, *_) in zip(second.opt.items, whole.opt.items))
    m, base = _model(44)
    plain = StyleTrainer(m, EditSet.from_views(views, image_hw=(H_REF, W_REF), device=DEV), _params(base), iters=64, distill_palette_steps=-1, seed=3)
    with pytest.raises(ValueError, match="class"):
        plain.load_checkpoint(path)


def test_fit_lowers_the_registered_term_only_with_its_weight():
    """200 steps on four views whose ground truth is a smooth function of the points and whose ref_targets are a recoloured copy of
    it (channels rotated), all rows registered; the switch to the ref phase is at step 32.  Compared: the mean registered MSE of the
    16 steps from the switch and of the last 16.
    Margins, decided from one run on an MI355X (lr 1e-2): with mse_loss = 6 the term went 0.0533 -> 0.0374 (0.70 of its value at
    the switch; asserted: below 0.85); with mse_loss = 0 nothing pulls towards the recoloured targets and it went 0.0656 -> 0.0673
    (1.03; asserted: not below 0.95)."""
    recolour = lambda c: c[:, [1, 2, 0]]
    colour = lambda x: 0.5 + 0.45 * torch.sin(12.0 * x + torch.tensor([0.0, 2.0, 4.0]))         # smooth in the points: learnable
    views = [make_ref_view(700 + k, reg="all", recolour=recolour, colour=colour) for k in range(4)]
    out = {}
    for name, w in (("with", 6.0), ("without", 0.0)):
        tr, _, _ = _trainer(51, True, 200, views=views, sup=None, mse_loss=w, cos_loss_factor=0.0, color_patch_loss=0.0, tv_weight=0.0,
                            depth_disc_weight=0.0, lr=1e-2)
        tr.train(200)
        r = tr.mse()
        out[name] = (float(r[32:48].mean()), float(r[-16:].mean()))
    print("registered MSE at the switch -> at the end:", out)
    assert out["with"][1] < 0.85 * out["with"][0]                # observed 0.70
    assert out["without"][1] >= 0.95 * out["without"][0]         # observed 1.03
