"""Trainer / StyleTrainer / DistillSet checkpoints: a run that is saved, loaded into fresh objects and continued equals the
uninterrupted run bit for bit (torch.equal, never a tolerance: any state that was not carried shows up as a difference)."""
import os

import numpy as np
import pytest
import torch

import checkpoint_util as U
from gpu_util import DEV

pytestmark = pytest.mark.gpu

REFERENCE_KEYS = {"epoch", "global_step", "stats", "mean_count", "mean_density", "model", "optimizer", "lr_scheduler", "scaler"}


# ---------------------------------------------------------------------------------------------------------------- 1
# (N, M): (8, 40) inside the first, host-sized group, before any mean_count; (32, 48) a group boundary; (40, 40) mid-group: the resumed
# run finishes the group eagerly, then replays graphs
@pytest.mark.parametrize("n,m", [(8, 40), (32, 48), (40, 40)])
@pytest.mark.parametrize("config,graph", [("plain", True), ("ema", True), ("depth", True)])
def test_resume_equals_uninterrupted(tmp_path, config, graph, n, m):
    _resume_case(tmp_path, config, graph, n, m)


def test_resume_equals_uninterrupted_eager(tmp_path):
    _resume_case(tmp_path, "plain", False, 40, 40)


def _resume_case(tmp_path, config, graph, n, m):
    a = U.make_trainer(config, graph=graph).train(n + m)
    want, rng_a = U.snapshot(a)[:2], torch.cuda.get_rng_state(DEV).clone()
    b = U.make_trainer(config, graph=graph).train(n)
    path = b.save_checkpoint(str(tmp_path / "run.pth"))
    assert path == str(tmp_path / "run.pth") and os.path.exists(path)
    c = U.fresh_for_resume(config, graph=graph)
    assert not torch.equal(c.opt.items[0][0], b.opt.items[0][0])              # nothing equal by accident
    c.load_checkpoint(path)
    assert c.global_step == n and c.losses().size == 0
    c.train(m)
    U.assert_same_state(want, c)
    assert torch.equal(rng_a, torch.cuda.get_rng_state(DEV))
    U.assert_same_tail(a, c, m)
    if config == "ema":
        assert int(c.ema.device_count()[0]) == (n + m) // 5 and int(a.ema.device_count()[0]) == (n + m) // 5
    if config == "depth":
        assert c.depth_losses().size == m and c.distort_losses().size == m
    print(f"resume {config} graph={graph} ({n}, {m}): captures A {a.captures} C {c.captures}, warm groups C {c.warm_groups}, "
          f"mean_count {c.r.mean_count}")
    if graph:
        assert c.captures >= 1                      # the resumed run went back to replaying captured groups
    else:
        assert c.captures == 0


# ---------------------------------------------------------------------------------------------------------------- 2
def test_load_into_a_used_trainer(tmp_path):
    a = U.make_trainer("ema").train(48)
    want = U.snapshot(a)[:2]
    b = U.make_trainer("ema").train(32)
    path = b.save_checkpoint(str(tmp_path / "used.pth"))
    b.train(16)
    b.load_checkpoint(path)
    assert b.global_step == 32 and b.graphs == {}
    b.train(16)
    U.assert_same_state(want, b)
    U.assert_same_tail(a, b, 16)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_a_refused_load_changes_nothing(tmp_path):
    other_rays = U.make_trainer("plain", num_rays=1024).train(20)
    p_rays = other_rays.save_checkpoint(str(tmp_path / "rays.pth"))
    other_table = U.make_trainer("plain", log2_hashmap_size=15).train(20)
    p_table = other_table.save_checkpoint(str(tmp_path / "table.pth"))

    tr = U.make_trainer("plain", net_seed=3, torch_seed=5, seed=8).train(24)
    stats = {k: (list(v) if isinstance(v, list) else v) for k, v in tr.stats.items()}
    before = U.snapshot(tr)
    for path, field in ((p_rays, "num_rays"), (p_table, "encoder.embeddings")):
        with pytest.raises(ValueError, match=field):
            tr.load_checkpoint(path)
        after = U.snapshot(tr)
        U.assert_same_state(before, after)
        assert torch.equal(before[2], after[2]) and tr.stats == stats and tr.losses().size == 24
    # the refused trainer still continues its own run
    with pytest.warns(UserWarning, match="num_rays"):
        tr.load_checkpoint(p_rays, strict_config=False)
    assert tr.global_step == 20 and tr.num_rays == U.RAYS
    for x, y in zip(tr.opt.items, other_rays.opt.items):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
    tr.train(16)
    assert tr.losses().shape == (16,) and np.isfinite(tr.losses()).all()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_the_file(tmp_path):
    from laenerf_amd import checkpoint as C
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    tr = U.make_trainer("ema").train(32)
    d = tmp_path / "ckpts"
    path = tr.save_checkpoint(str(d))
    assert os.path.basename(path) == C.checkpoint_name("ngp", 32 // 5) == "ngp_ep0006.pth"
    ck = torch.load(path, weights_only=True)
    assert set(ck) == REFERENCE_KEYS | {"ema", C.KEY}
    assert ck["epoch"] == 6 and ck["global_step"] == 32 and ck["mean_count"] == tr.r.mean_count and ck["mean_density"] == tr.r.mean_density
    model = ck["model"]
    assert not any(k.startswith("model.") for k in model)
    assert {"encoder.embeddings", "density_grid", "density_bitfield", "step_counter"} <= set(model)
    assert any(k.startswith("sigma_net.") for k in model) and any(k.startswith("color_net.") for k in model)
    assert set(ck["scaler"]) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    assert ck["scaler"]["scale"] == tr.opt.get_scale()
    assert {"last_epoch", "base_lrs", "_last_lr"} <= set(ck["lr_scheduler"]) and ck["lr_scheduler"]["last_epoch"] == 32
    assert set(ck["optimizer"]) == {"state", "param_groups"} and set(ck["ema"]) >= {"decay", "num_updates", "shadow_params"}
    extra = ck[C.KEY]
    assert extra["format"] == C.FORMAT and extra["lae_version"] and extra["config"]["num_rays"] == U.RAYS
    assert torch.equal(extra["optimizer_words"], tr.opt.dev_state.cpu())
    # a second renderer's own load_state_dict takes the file's dict
    torch.manual_seed(77)
    r2 = NeRFRenderer(NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV), bound=1).to(DEV)
    r2.load_state_dict(torch.load(path, weights_only=True))
    for (k, x), (_, y) in zip(sorted(r2.state_dict().items()), sorted(tr.r.state_dict().items())):
        assert torch.equal(x, y), k
    # full=False: the reference's short file
    short = torch.load(tr.save_checkpoint(str(tmp_path / "short.pth"), full=False), weights_only=True)
    assert not {"optimizer", "lr_scheduler", "scaler", "ema"} & set(short) and "optimizer_words" not in short[C.KEY]

    # best: nothing without a result; written once a result improves, EMA weights in `model`, no density_grid, live weights untouched
    assert tr.save_checkpoint(str(d), best=True) is None and not os.path.exists(d / "ngp.pth")
    live = [p.detach().clone() for p in tr.r.parameters()]
    shadow_tables = [sh.half.clone() for *_, sh, _ in tr.opt.items if sh is not None]
    res = tr.evaluate_one_epoch(tr.data)
    n_px = tr.data.n_img * 3 * tr.data.H * tr.data.W
    mse = float(np.sum(10.0 ** (-np.asarray(res["psnr"], np.float64) / 10.0)) / tr.data.n_img)
    assert len(tr.stats["results"]) == 1 and tr.stats["results"][0] == pytest.approx(mse, rel=1e-6) and n_px > 0
    best = tr.save_checkpoint(str(d), best=True)
    assert best == str(d / "ngp.pth") and tr.stats["best_result"] == tr.stats["results"][0]
    bk = torch.load(best, weights_only=True)
    assert "density_grid" not in bk["model"] and "density_bitfield" in bk["model"]
    names = [k for k, _ in tr.r.state_dict(reference_layout=True).items()]
    ema_of = {id(p): s for p, s in zip(tr.ema.params, tr.ema.shadow_params)}
    for k, p in tr.r.named_parameters():
        key = k[len("model."):] if k.startswith("model.") else k
        assert key in names and torch.equal(bk["model"][key], ema_of[id(p)].cpu()), k
    assert any(not torch.equal(s, p.detach()) for p, s in zip(tr.ema.params, tr.ema.shadow_params))
    for p, q in zip(tr.r.parameters(), live):
        assert torch.equal(p.detach(), q)
    for t, q in zip([sh.half for *_, sh, _ in tr.opt.items if sh is not None], shadow_tables):
        assert torch.equal(t, q)
    tr.stats["results"].append(tr.stats["results"][0] * 2)                    # no improvement: nothing is written
    os.remove(best)
    assert tr.save_checkpoint(str(d), best=True) is None and not os.path.exists(best)

    # rotation: three saves leave the newest two
    tr.train(5)
    second = tr.save_checkpoint(str(d))
    tr.train(5)
    third = tr.save_checkpoint(str(d))
    assert sorted(os.listdir(d)) == sorted(os.path.basename(p) for p in (second, third)) and len({path, second, third}) == 3
    assert tr.stats["checkpoints"] == [second, third] and C.latest_checkpoint(str(d)) == third
    # ... and a directory loads its latest file
    c = U.fresh_for_resume("ema")
    c.load_checkpoint(str(d))
    assert c.global_step == 42
    U.assert_same_state(tr, c)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_reference_shaped_file(tmp_path):
    """what the reference's save_checkpoint(full=True) writes: no `laenerf_amd` entry; torch.optim.Adam, GradScaler and torch_ema
    state dicts.  Every part is restored; exactness is not promised for such a file."""
    from laenerf_amd import checkpoint as C
    src = U.make_trainer("ema").train(32)
    # a real torch.optim.Adam over the same four parameter groups, stepped a few times
    from laenerf_amd.network import NeRFNetwork
    torch.manual_seed(5)
    twin = NeRFNetwork(bound=1, log2_hashmap_size=16).to(DEV)
    adam = torch.optim.Adam(twin.get_params(U.LR), betas=(0.9, 0.99), eps=1e-15)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(3):
        for g in adam.param_groups:
            for p in g["params"]:
                p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
        adam.step()
    shadows = [torch.randn(p.shape, device=DEV, generator=gen) for p in src.ema.params]
    ck = {"epoch": 5, "global_step": 32, "stats": {"loss": [0.5], "valid_loss": [], "results": [0.25], "checkpoints": [], "best_result": 0.25},
          "mean_count": src.r.mean_count, "mean_density": src.r.mean_density,
          "model": {k: v.detach().cpu().clone() for k, v in src.r.state_dict(reference_layout=True).items()},
          "optimizer": adam.state_dict(),
          "lr_scheduler": C.scheduler_to_reference(32, [U.LR] * 4, U.ITERS),
          "scaler": {"scale": 4096.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 17},
          "ema": {"decay": 0.95, "num_updates": 4, "shadow_params": shadows, "collected_params": None}}
    path = str(tmp_path / "ngp_ep0005.pth")
    torch.save(ck, path)
    c = U.fresh_for_resume("ema")
    c.load_checkpoint(str(tmp_path))                                         # the directory's latest
    for k, v in c.r.state_dict(reference_layout=True).items():
        assert torch.equal(v.cpu(), ck["model"][k]), k
    for *_, sh, _ in c.opt.items:
        if sh is not None:
            assert sh.version is not None
    for (p, m, v, sh, _), q in zip(c.opt.items, [p for g in adam.param_groups for p in g["params"]]):
        assert torch.equal(m, adam.state[q]["exp_avg"]) and torch.equal(v, adam.state[q]["exp_avg_sq"])
        if sh is not None:
            assert torch.equal(sh.half, p.detach().half())
    assert c.opt.steps_taken == 3 and c.opt.get_scale() == 4096.0 and int(c.opt.dev_state[1]) == 17
    assert all(torch.equal(x, y) for x, y in zip(c.ema.shadow_params, shadows)) and int(c.ema.device_count()[0]) == 4
    assert c.global_step == 32 and int(c.data.step) == 32 and c.stats["best_result"] == 0.25 and c.stats["results"] == [0.25]
    assert c.r.mean_count == src.r.mean_count > 0 and c.r.mean_density == src.r.mean_density
    c.train(16)
    assert c.graph and c.losses().shape == (16,) and np.isfinite(c.losses()).all() and c.global_step == 48


# ---------------------------------------------------------------------------------------------------------------- 6
def test_model_only(tmp_path):
    src = U.make_trainer("ema").train(48)
    path = src.save_checkpoint(str(tmp_path / "m.pth"))
    want = src.evaluate(range(2))
    c = U.fresh_for_resume("ema")
    own_step = c.global_step
    c.load_checkpoint(path, model_only=True)
    assert c.global_step == own_step and not c.started
    assert c.evaluate(range(2)) == want
    assert all(torch.equal(x, y) for x, y in zip(c.ema.shadow_params, src.ema.shadow_params))
    # extract_mesh(64) at its default threshold, and at lower ones: the young scene may have no surface at 10, and one of the
    # comparisons must be of a real mesh
    sizes = []
    for kw in ({}, {"threshold": 1.0}, {"threshold": 0.1}):
        (v0, f0), (v1, f1) = src.r.extract_mesh(64, **kw), c.r.extract_mesh(64, **kw)
        assert np.array_equal(np.asarray(v0), np.asarray(v1)) and np.array_equal(np.asarray(f0), np.asarray(f1))
        sizes.append(len(f0))
    print("model_only: triangles per threshold", sizes)
    assert max(sizes) > 0


# ---------------------------------------------------------------------------------------------------------------- 7
STYLE_COUNTS = [300, 310, 700, 720, 1500, 333]                # test_gpu_style_train.py's small edit set: five sizes, four bucket capacities


def _style_trainer(kind, model_seed, seed, graph=True):
    """kind 'points': the point losses with the palette distillation before step 48 of 64; 'tv': tv_weight > 0 (and the depth terms) on
    an edit set with image arrays, the image terms on from step 32 (warm-up 16), no style network"""
    from laenerf_amd.editing import StyleTrainer
    if kind == "points":
        from test_gpu_style_train import make_model, make_set
        m, params = make_model(seed=model_seed)
        return StyleTrainer(m, make_set(STYLE_COUNTS, seed=6), params, iters=64, distill_palette_steps=32, seed=seed, graph=graph)
    from style_mode_util import make_image_views
    from test_gpu_style_mode import _model, _set, _style_params
    m, base = _model(model_seed)
    params = _style_params(base, style_weight=0, tv_weight=1e-3, warmup_iterations=16)
    return StyleTrainer(m, _set(make_image_views(seed=7)), params, iters=64, distill_palette_steps=-1, seed=seed, graph=graph)


def _style_state(tr):
    out = {}
    for i, (p, m, v, *_) in enumerate(tr.opt.items):
        out[f"param{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = p.detach().clone(), m.clone(), v.clone()
    out["words"], out["es_step"], out["active"] = tr.opt.dev_state.clone(), tr.es.step.clone(), tr.enc.active_palets.clone()
    return out


# save points: before the palette distillation (step 48) and after it; past the warm-up of the image terms
@pytest.mark.parametrize("kind,n", [("points", 24), ("points", 56), ("tv", 40)])
def test_style_trainer_resume_equals_uninterrupted(tmp_path, kind, n):
    total = 64
    a = _style_trainer(kind, 6, 9).train(total)
    b = _style_trainer(kind, 6, 9).train(n)
    path = b.save_checkpoint(str(tmp_path / "style.pth"))
    ck = torch.load(path, weights_only=True)
    assert ck["global_step"] == n and ck["distilled"] == (kind == "points" and n >= 48)
    c = _style_trainer(kind, 77, 1234)
    assert not torch.equal(c.opt.items[0][0], b.opt.items[0][0]) and not np.array_equal(c._sched, b._sched)
    c.load_checkpoint(path)
    assert c.global_step == n and c.losses().size == 0 and c.es.seed == b.es.seed
    c.train(total - n)
    sa, sc = _style_state(a), _style_state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert a.enc._active_mask == c.enc._active_mask and a.distilled == c.distilled and c.global_step == total
    assert np.array_equal(c.losses().view(np.uint32), a.losses()[n:].view(np.uint32)) and np.isfinite(c.losses()).all()
    assert np.array_equal(c.mse().view(np.uint32), a.mse()[n:].view(np.uint32))
    assert np.array_equal(c.terms().view(np.uint32), a.terms()[n:].view(np.uint32))
    assert torch.equal(a.gen.get_state(), c.gen.get_state()) and np.array_equal(a._sched, c._sched)
    if kind == "points":
        assert a.distilled and bin(a.enc._active_mask).count("1") <= 8
    else:
        assert (a.terms()[32:, 1] > 0).all() and (a.terms()[:32] == 0).all()          # the tv term was on across the save point
    caps = [c.cap_of_step(k) for k in range(n, total)]
    if max(caps.count(k) for k in set(caps)) >= 2:                            # a capacity met twice: its second step is a captured graph
        assert c.captures >= 1
    # a configuration that differs is refused, and the refused trainer is unchanged
    d = _style_trainer(kind, 6, 9)
    d.iters += 1
    keep = _style_state(d)
    with pytest.raises(ValueError, match="iters"):
        d.load_checkpoint(path)
    for k, v in _style_state(d).items():
        assert torch.equal(v, keep[k]), k


def test_laenerf_state_dict_carries_what_forward_and_recolor_read(tmp_path):
    from test_gpu_style_train import make_model
    tr = _style_trainer("points", 6, 9).train(16)
    enc = tr.enc
    mask = torch.tensor([True, False, True, True, False, True, True, True], device=DEV)
    enc.set_active_palets(mask)
    enc.set_color_palette(torch.rand(int(mask.sum()), 3, device=DEV))         # a palette edit: the original palette is kept aside
    assert enc.original_color_palette is not None and "original_color_palette" in enc.state_dict()
    path = tr.save_checkpoint(str(tmp_path / "enc.pth"))
    g = torch.Generator().manual_seed(4)
    x = ((torch.rand(1000, 3, generator=g) - 0.5) * 0.5).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(1000, 3, generator=g), dim=-1).to(DEV)
    enc.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want = enc(x, d)
    fresh, _ = make_model(seed=31)
    assert fresh.original_color_palette is None and "original_color_palette" not in fresh.state_dict()
    fresh.load_state_dict(torch.load(path, weights_only=True)["model"])
    fresh.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        got = fresh(x, d)
    want, got = (want if isinstance(want, (tuple, list)) else (want,)), (got if isinstance(got, (tuple, list)) else (got,))
    assert len(want) == len(got) and all(torch.equal(p, q) for p, q in zip(want, got))
    assert torch.equal(fresh.active_palets, mask) and fresh._active_mask == enc._active_mask == 0b11101101
    assert torch.equal(fresh.original_color_palette, enc.original_color_palette)
    assert torch.equal(fresh.color_palette.detach(), enc.color_palette.detach())
    # model_only through the trainer, and a file without the original palette clears one
    other = _style_trainer("points", 55, 3)
    other.load_checkpoint(path, model_only=True)
    assert other.global_step == 0 and other.enc._active_mask == 0b11101101
    assert torch.equal(other.enc.original_color_palette, enc.original_color_palette)
    plain, _ = make_model(seed=32)
    other.enc.load_state_dict(plain.state_dict())
    assert other.enc.original_color_palette is None and other.enc._active_mask == 0xff


# ---------------------------------------------------------------------------------------------------------------- 8
def test_distill_set_save_load(tmp_path):
    from laenerf_amd.editing import DistillSet, distill_images
    from test_gpu_distill import network_case, style_encoder
    c, s, data = network_case(5)
    s.depth = torch.rand(s.R, device=DEV)
    path = str(tmp_path / "distill.npz")
    s.save(path)
    t = DistillSet.load(path, device=DEV)
    for k in ("img_idx", "pix", "w", "pred", "x_term", "dirs", "dist", "depth", "counts", "offsets", "view_img"):
        x, y = getattr(s, k), getattr(t, k)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), k
    for k in ("counts_host", "offsets_host", "view_img_host"):
        assert np.array_equal(getattr(s, k), getattr(t, k)) and getattr(s, k).dtype == getattr(t, k).dtype, k
    assert (s.occluded, s.n_img, s.V, s.R) == (t.occluded, t.n_img, t.V, t.R) and t.occluded == [2]
    enc = style_encoder()
    pal = torch.rand(8, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    a, b = distill_images(data, enc, s, palette=pal), distill_images(data, enc, t, palette=pal)
    assert torch.equal(a.images, b.images) and not torch.equal(a.images.float(), data.images.float() / 255)
    # a set without the optional arrays
    s.dist = s.depth = None
    s.save(path)
    u = DistillSet.load(path, device=DEV)
    assert u.dist is None and u.depth is None and torch.equal(u.w, s.w)
