"""Per-pixel weights and a second colour target in the fused training step, as far as no GPU is needed: the float64 restatement
(composite_train_step_numpy with pixel_weights / second_target) against central finite differences of its own loss and against the
reference's three lines (nerf/utils.py:523-526) in torch float64, the argument checks of every layer (library entry, operator,
ResidentImages, Trainer), the Trainer's config() keys, and the header / binding pair of the new symbols."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from step_args import null_step
from test_criterion_cpu import _cpu_trainer

T_THRESH = 1e-4
STEPS = (70, 1, 33, 64, 65, 12)                     # 6 rays, up to 70 samples (two passes of 64)
LAMBDA_2, LAMBDA_DEPTH, W_DIST, W_OPAC = 0.5, 0.37, 0.25, 0.05


def small_case(seed=3):
    """6 rays without an early stop (the optical depth of a ray stays below 3: T > 0.05 >> T_thresh, so the loss is smooth in every
    input), indices a permutation, weights in [0, 2] with one exact 0 and one exact 1"""
    rng = np.random.default_rng(seed)
    N, M = len(STEPS), sum(STEPS)
    rays = np.zeros((N, 3), np.int32)
    rays[:, 0], rays[:, 2] = rng.permutation(N), STEPS
    rays[:, 1] = np.concatenate([[0], np.cumsum(STEPS)[:-1]])
    deltas = np.stack([rng.uniform(0.005, 0.02, M), rng.uniform(0.005, 0.03, M)], -1)
    sig = rng.uniform(0, 2.0, M)
    sig[0:70] = rng.uniform(0, 3.0, 70)
    w = rng.uniform(0, 2, N)
    w[1], w[4] = 0.0, 1.0
    z = rng.uniform(0.5, 3.0, N)
    z[2] = 0.0
    s4 = rng.uniform(0, 1, (N, 4))
    s4[3, 3] = 1.0
    return dict(sigmas=sig, rgbs=rng.uniform(0, 1, (M, 3)), deltas=deltas, rays=rays, N=N, M=M, bg=rng.uniform(0, 1, (N, 3)),
                target=rng.uniform(0, 1, (N, 3)), w=w, s4=s4, z=z, nears=rng.uniform(0.2, 1.0, N))


def _restated(c, sigmas=None, rgbs=None, bg=None, channels=4, scale=1.0, **kw):
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    return composite_train_step_numpy(c["sigmas"] if sigmas is None else sigmas, c["rgbs"] if rgbs is None else rgbs, c["deltas"], c["rays"],
                                      c["target"], T_THRESH, bg=c["bg"] if bg is None else bg, z=c["z"], nears=c["nears"],
                                      depth_weight=LAMBDA_DEPTH, distort_weight=W_DIST, opacity_weight=W_OPAC, scale=scale,
                                      pixel_weights=c["w"], second_target=c["s4"][:, :channels], second_weight=LAMBDA_2, **kw)


def _fd(f, x, h=1e-6):
    """central differences of the scalar f over every element of x"""
    g = np.zeros_like(x)
    it = np.nditer(x, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        hi, lo = x.copy(), x.copy()
        hi[i] += h
        lo[i] -= h
        g[i] = (f(hi) - f(lo)) / (2 * h)
    return g


@pytest.mark.parametrize("channels", [3, 4])
def test_sample_gradients_against_finite_differences(channels):
    """grad_sigmas and grad_rgbs of the restatement (every term on, scale 8) against central differences of its loss.  Tolerance: the
    loss is O(1) in float64, so a difference quotient with h = 1e-6 carries ~1e-16 / 1e-6 = 1e-10 of rounding and O(h^2) = 1e-12 of
    truncation relative to the third derivative: atol 1e-8 is two orders above both, rtol 1e-6 covers the large entries"""
    c = small_case()
    scale = 8.0
    f = _restated(c, channels=channels, scale=scale)
    gs = _fd(lambda s: _restated(c, sigmas=s, channels=channels)["loss"], c["sigmas"]) * scale
    gc = _fd(lambda r: _restated(c, rgbs=r, channels=channels)["loss"], c["rgbs"]) * scale
    for name, a, b in (("grad_sigmas", f["grad_sigmas"], gs), ("grad_rgbs", f["grad_rgbs"], gc)):
        print(f"{channels} channels {name}: max abs difference {np.abs(a - b).max():.3e}, largest gradient {np.abs(b).max():.3e}")
        assert np.abs(b).max() > 1e-3 and np.allclose(a, b, rtol=1e-6, atol=1e-8), name


def test_grad_image_against_finite_differences():
    """d loss / d image_out cannot be perturbed directly; with a 3-channel second target the background enters the loss through
    image_out = image + (1 - weights_sum) * bg alone, so d loss / d bg = grad_image * (1 - weights_sum)"""
    c = small_case()
    f = _restated(c, channels=3)
    rest = 1 - f["weights_sum"]
    assert (rest > 0.04).all()
    g = _fd(lambda b: _restated(c, bg=b, channels=3)["loss"], c["bg"])
    assert np.allclose(f["grad_image"] * rest[:, None], g, rtol=1e-6, atol=1e-9)
    only_w = _restated_weights_only(c)
    assert not only_w["grad_image"][c["w"] == 0].any() and only_w["grad_image"][c["w"] != 0].all()


def _restated_weights_only(c):
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    return composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"], pixel_weights=c["w"])


def test_loss_against_the_references_three_lines():
    """loss = pow(w (pred - gt), 2).mean() + style_weight_d * pow((1 - w / 2) (gt_style - pred), 2).mean() + depth_weight_d * depth term
    (nerf/utils.py:523-531), gt_style = style[..., :3] * a + bg * (1 - a) (:511), in torch float64 on the restatement's own image"""
    c = small_case()
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    f = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"], z=c["z"], nears=c["nears"],
                                   depth_weight=1e-3, pixel_weights=c["w"], second_target=c["s4"], second_weight=LAMBDA_2)
    pred, gt = torch.tensor(f["image_out"]), torch.tensor(c["target"])
    weights, style, bg = torch.tensor(c["w"])[:, None], torch.tensor(c["s4"]), torch.tensor(c["bg"])
    gt_style = style[..., :3] * style[..., 3:] + bg * (1 - style[..., 3:])
    colour = ((weights * (pred - gt)) ** 2).mean()
    loss_style = (((1 - weights / 2) * (gt_style - pred)) ** 2).mean()
    z = torch.tensor(c["z"])
    depth_term = (((z > 0).double() * (torch.tensor(f["depth"]) - (z - torch.tensor(c["nears"])))) ** 2).mean()
    loss = colour + LAMBDA_2 * loss_style + 1e-3 * depth_term
    assert np.isclose(f["loss"], float(loss), rtol=1e-13, atol=0)
    assert np.isclose(f["second"], float(loss_style), rtol=1e-13, atol=0) and f["second"] > 1e-3
    # the pieces: ones and no second target are the call without the arguments
    plain = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"])
    ones = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"], pixel_weights=np.ones(c["N"]))
    for k in ("loss", "grad_image", "grad_sigmas", "grad_rgbs"):
        assert np.array_equal(plain[k], ones[k]), k
    assert plain["second"] == 0
    a1 = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"],
                                    second_target=np.concatenate([c["s4"][:, :3], np.ones((c["N"], 1))], 1), second_weight=LAMBDA_2)
    c3 = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg"],
                                    second_target=c["s4"][:, :3], second_weight=LAMBDA_2)
    assert a1["loss"] == c3["loss"] and np.array_equal(a1["grad_sigmas"], c3["grad_sigmas"])
    with pytest.raises(ValueError, match="mse"):
        composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, loss="huber", pixel_weights=c["w"])


# ---------------------------------------------------------------------------------------------------------------- arguments
BAD_WEIGHTS = [-1.0, float("inf"), float("nan")]


def check_weighted_einval(step):
    """every LAE_EINVAL case of the weight term, before any launch (and before the NULL checks: -3 is what a valid call on NULL buffers
    gives): the criterion term with the entropy off and the weight term with every pointer NULL but the ones given"""
    def rc(kind=0, w=None, w_dtype=2, t2=None, t2_dtype=2, channels=3, lam=0.5, t2_part=None, N=4, with_crit=True):
        return null_step(step, N=N, crit=(kind, 0.1, 0.1, 0, None, None, None) if with_crit else None,
                         weight=(w, w_dtype, t2, t2_dtype, channels, None, lam, t2_part))
    buf = torch.zeros(16)
    p = buf.data_ptr()
    assert rc() == -3                                                                # neither plane: the criterion term's own answer on NULL pointers
    assert rc(w=p) == -3 and rc(t2=p, t2_part=p) == -3
    for kind in (1, 2, 3):                                                           # weights or a second target with another criterion
        assert rc(kind=kind, w=p) == -1
        assert rc(kind=kind, t2=p, t2_part=p) == -1
        assert rc(kind=kind) == -3                                                   # ... which alone is fine
    for lam in BAD_WEIGHTS:
        assert rc(t2=p, t2_part=p, lam=lam) == -1
        assert rc(w=p, lam=lam) == -3                                                # the weight counts only with the second target
    for ch in (0, 1, 2, 5):
        assert rc(t2=p, t2_part=p, channels=ch) == -1
    for dt in (0, 3, -1):                                                            # uint8 and unknown codes
        assert rc(w=p, w_dtype=dt) == -1
        assert rc(t2=p, t2_part=p, t2_dtype=dt) == -1
        assert rc(t2=p, t2_part=p, w_dtype=dt) == -3                                 # not looked at without the plane
    assert rc(t2=p, t2_part=p, lam=-1.0, N=0) == -1                                  # checked before the N == 0 return
    assert rc(w=p, N=0) == 0
    # without a criterion term the weight term means MSE: the same answers
    assert rc(w=p, with_crit=False) == -3 and rc(w=p, w_dtype=0, with_crit=False) == -1 and rc(w=p, N=0, with_crit=False) == 0
    assert rc(t2=p, t2_part=p, channels=5, with_crit=False) == -1


def test_library_entry_refuses_invalid_arguments_before_any_launch(hip_lib):
    check_weighted_einval(hip_lib.lae_composite_rays_train_step)


def test_symbols_in_header_and_binding(hip_lib):
    from laenerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "laenerf.h")).read()
    # the step: its 27 base arguments, the four terms, the stream
    for name, n_args in (("lae_composite_rays_train_step", 27 + 4 + 1), ("lae_composite_rays_train_backward_blend_ex", 24),
                         ("lae_composite_rays_train_forward_blend", 20), ("lae_ref_distill_init", 11), ("lae_ref_distill_scatter", 21)):
        m = re.search(r"LAE_API\s+int\s+" + name + r"\s*\(([^;]*)\);", src)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name]), name
        assert hasattr(hip_lib, name)
    step = re.search(r"LAE_API\s+int\s+lae_composite_rays_train_step\s*\(([^;]*)\);", src).group(1).split(",")
    assert [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0] for a in step[-5:-1]] == [f"const {n}*" for n in _lib.TERM_STRUCTS]
    assert _lib.SIGNATURES["lae_composite_rays_train_step"][-5:] == [_lib.vp] * 5
    # the four term structs: the header's fields, names in order and C types, are the binding's
    assert list(_lib.TERM_STRUCTS) == ["lae_depth_term", "lae_dist_term", "lae_crit_term", "lae_weight_term"]
    ctype = lambda c: _lib.vp if c.endswith("*") else {"int": _lib.i32, "float": _lib.f32}[c]
    for name, cls in _lib.TERM_STRUCTS.items():
        m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{([^}]*)\}\s*" + name + r"\s*;", src)
        assert m, name
        decls = [re.sub(r"\s+", " ", d).strip() for d in m.group(1).split(";") if d.strip()]
        fields = [(d.rsplit(" ", 1)[1], ctype(d.rsplit(" ", 1)[0])) for d in decls]
        assert fields == list(cls._fields_), name
        assert len(fields) == {"lae_depth_term": 7, "lae_dist_term": 5, "lae_crit_term": 7, "lae_weight_term": 8}[name]


def _data(**kw):
    from laenerf_amd.data import ResidentImages
    img = np.zeros((2, 4, 5, 4), np.uint8)
    return ResidentImages(img, np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), (10.0, 10.0, 2.5, 2.0), device="cpu", **kw)


def test_resident_images_planes():
    d = _data()
    assert d.pixel_weights is None and d.second_target is None
    w = np.random.default_rng(0).uniform(0, 2, (2, 4, 5))
    d = _data(pixel_weights=w.astype(np.float16), second_target=np.zeros((2, 4, 5, 4), np.float32))
    assert d.pixel_weights.dtype == torch.float16 and d.second_target.dtype == torch.float32
    assert d.set_pixel_weights(w).dtype == torch.float32                              # float64 is stored as fp32
    assert np.array_equal(d.pixel_weights.numpy(), w.astype(np.float32))
    assert d.set_second_target(torch.zeros(2, 4, 5, 3, dtype=torch.bfloat16)).dtype == torch.float32
    assert d.set_pixel_weights(None) is None and d.set_second_target(None) is None and d.pixel_weights is None
    for bad in (np.zeros((2, 4, 5), np.uint8), np.zeros((2, 4, 5), np.int64)):
        with pytest.raises(ValueError, match="floating"):
            d.set_pixel_weights(bad)
    with pytest.raises(ValueError, match="floating"):
        d.set_second_target(np.zeros((2, 4, 5, 4), np.uint8))
    for bad in (np.zeros((2, 4, 4), np.float32), np.zeros((1, 4, 5), np.float32), np.zeros((2, 4, 5, 1), np.float32)):
        with pytest.raises(ValueError, match="pixel_weights must be"):
            _data(pixel_weights=bad)
    for bad in (np.zeros((2, 4, 5), np.float32), np.zeros((2, 4, 5, 2), np.float32), np.zeros((2, 5, 4, 3), np.float32)):
        with pytest.raises(ValueError, match="second_target must be"):
            _data(second_target=bad)


def _weighted_trainer(planes=("pixel_weights", "second_target"), **kw):
    from laenerf_amd.trainer import Trainer
    r = types.SimpleNamespace(fused_post_ops=kw.pop("fused", True), density_grid=torch.zeros(1), aabb_train=torch.zeros(6), min_near=0.2, bound=1,
                              grid_size=128, density_thresh=10.0, density_scale=1)
    opt = types.SimpleNamespace(param_groups=[{}], device_lr=False)
    data = types.SimpleNamespace(error_map=kw.pop("map", None), n_img=6, H=48, W=40, C=4, mode="image", bg="random", color_space="srgb",
                                 **{p: torch.zeros(1) for p in planes})
    return Trainer(r, opt, data, 100, 1e-2, **kw)


def test_trainer_refuses_and_config():
    from laenerf_amd.checkpoint import check_config
    default = _cpu_trainer().config()
    assert "pixel_weights" not in default and "second_weight" not in default
    assert _weighted_trainer().config() == default                                   # planes on the data alone change nothing
    both = _weighted_trainer(pixel_weights=True, second_weight=0.5, depth_weight=None).config()
    assert both["pixel_weights"] is True and both["second_weight"] == 0.5
    assert [n for n, _, _ in check_config(default, both)] == ["pixel_weights", "second_weight"]
    assert check_config(both, _weighted_trainer(pixel_weights=True, second_weight=0.5).config()) == []
    assert [n for n, _, _ in check_config(both, _weighted_trainer(pixel_weights=True, second_weight=0.25).config())] == ["second_weight"]
    only = _weighted_trainer(pixel_weights=True).config()
    assert only["pixel_weights"] is True and "second_weight" not in only
    with pytest.raises(ValueError, match="weight plane"):
        _weighted_trainer(planes=("second_target",), pixel_weights=True)
    with pytest.raises(ValueError, match="second target"):
        _weighted_trainer(planes=("pixel_weights",), second_weight=0.5)
    for kw in (dict(pixel_weights=True), dict(second_weight=0.5)):
        for loss in ("l1", "huber", "mape"):
            with pytest.raises(ValueError, match="loss='mse'"):
                _weighted_trainer(loss=loss, **kw)
        with pytest.raises(ValueError, match="error_map='ema'"):
            _weighted_trainer(error_map="ema", map=torch.zeros(1), **kw)
        with pytest.raises(ValueError, match="fused_post_ops"):
            _weighted_trainer(fused=False, **kw)
        _weighted_trainer(error_map="fixed", map=torch.zeros(1), **kw)               # a fixed map is no EMA: allowed
    for w in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="second_weight"):
            _weighted_trainer(second_weight=w)


def test_operator_layers_refuse():
    from laenerf_amd.raymarching import raymarching as rm
    from laenerf_amd.renderer import NeRFRenderer
    w = torch.ones(4)
    for loss in ("l1", "huber", "mape"):
        with pytest.raises(ValueError, match="loss='mse'"):
            rm.composite_rays_train_blend_mse(*([None] * 7), loss=loss, pixel_weights=w)
        with pytest.raises(ValueError, match="loss='mse'"):
            NeRFRenderer.shade_train(types.SimpleNamespace(fused_post_ops=True), None, gt=w, loss=loss, second_target=torch.ones(4, 3))
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="second_weight"):
            rm.composite_rays_train_blend_mse(*([None] * 7), second_target=torch.ones(4, 3), second_weight=bad)
    with pytest.raises(RuntimeError, match="float16 or float32"):
        rm.composite_rays_train_blend_mse(*([None] * 7), pixel_weights=torch.ones(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="3 or 4"):
        rm.composite_rays_train_blend_mse(*([None] * 7), second_target=torch.ones(4, 2))
    with pytest.raises(RuntimeError, match="need gt"):
        NeRFRenderer.shade_train(types.SimpleNamespace(fused_post_ops=True), None, gt=None, pixel_weights=w)
    with pytest.raises(RuntimeError, match="without a second target"):
        rm.finish_second_loss(types.SimpleNamespace())
