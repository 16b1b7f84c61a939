"""-m gpu: bench.grouped_pipeline -- the two-stream grouped scheme the benchmark's flower_step, sparse_step and style_step objects
are measured on (the headline runs an inline copy of the same scheme) -- computes the step it claims to.

Per group of G batches the scheme replays two captured graphs: the march + the position-only half of the hash-grid backward (the
plan) on a side stream, `groups_ahead` groups early, and encoder + head, compositing + criterion, backward and FusedAdam on the main
stream.  State the two streams share: the optimizer's touched-lines bitmap (the plan writes it, Adam reads it), the library's
grow-only workspaces, the renderer's 16-entry step-counter ring (with G = 8 and two groups ahead the side stream's marches use the
counters of the batches the main stream is shading) and the march noise drawn inside the side graphs.  A race there would not
crash: it would train another model.  So, bit for bit after 13 groups (more than three turns of the 4-group ring, one break in the
step numbers so that the re-entry path runs):
  1. the pipeline (noise on) against the same graphs replayed in the same order on ONE stream (no overlap);
  2. the pipeline with a noise-free march against the eager, unsplit train step;
  3. the LAENeRF palette step with its plan on the side stream against its eager step without a plan.
Every test also shows that it compared something: parameters moved, losses finite, samples marched, a touched bitmap neither
empty nor full, GradScaler decisions inside the window (growth_interval 4: the scale doubles after four clean steps until the
fp16 gradients overflow, then a step is skipped and the scale halves)."""
from types import SimpleNamespace

import pytest
import torch

import bench
from bench import grouped_pipeline
from gpu_util import DEV

pytestmark = pytest.mark.gpu

G = 8
N_BATCHES = 4 * G                        # P = 4 groups, two of them ahead: the side stream wraps round the group ring
N_RAYS = 4096
GROWTH_INTERVAL = 4
# step numbers at which a group starts: six groups, group 2 of the second turn skipped (the scheme re-enters at group 3),
# seven more -- 13 groups of 8 steps
SCHEDULE = [k * G for k in range(6)] + [k * G for k in range(7, 14)]
BATCH_ORDER = [i % N_BATCHES for i0 in SCHEDULE for i in range(i0, i0 + G)]


@pytest.fixture(autouse=True)
def _default_side_stream(monkeypatch):
    monkeypatch.delenv("LAE_BENCH_SIDE_PRIO", raising=False)          # the A/B switch would bypass concurrent_side_stream


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    diff = {k: int((_bits(a[k]) != _bits(b[k])).sum()) for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))}
    assert not diff, f"{what}: bytes that differ {diff}"


def _state(opt, r=None):
    """everything a step leaves behind: parameters, Adam moments, fp16 shadow tables and their gradient accumulators, the
    touched-lines bitmaps, persistent fp32 gradients, the device optimizer state (loss scale, tracker, found_inf, step, skipped)
    and the renderer's step-counter ring"""
    st = {}
    for j, (p, m, v, sh, _) in enumerate(opt.items):
        st[f"param{j}"], st[f"exp_avg{j}"], st[f"exp_avg_sq{j}"] = p.detach().clone(), m.clone(), v.clone()
        if sh is not None:
            st[f"shadow{j}"], st[f"grad_acc{j}"] = sh.half.clone(), sh.grad_half.clone()
            if getattr(sh, "touched_lines", None) is not None:
                st[f"touched{j}"] = sh.touched_lines.clone()
        elif p.grad is not None:
            st[f"grad{j}"] = p.grad.clone()
    st["dev_state"] = opt.dev_state.clone()
    if r is not None:
        st["step_counter"] = r.step_counter.clone()
    return st


def _scaler(st):
    """(loss scale, steps skipped) of a device optimizer state (include/laenerf.h: word 0 the scale, word 8 the skipped steps)"""
    return float(st["dev_state"][:1].view(torch.float32)), int(st["dev_state"][8])


def _assert_power(init, final, losses, n_samples):
    moved = [k for k in init if k.startswith("param")]
    assert moved and all(not torch.equal(init[k], final[k]) for k in moved), "a parameter did not move"
    assert losses.numel() == len(BATCH_ORDER) and torch.isfinite(losses).all()
    assert min(n_samples) > 0
    if "step_counter" in final:
        assert int(final["step_counter"][:, 0].min()) > 0                  # every slot of the ring holds a march's samples
    touched = [final[k] for k in final if k.startswith("touched")]
    assert touched
    for t in touched:
        assert bool((t != 0).any()) and bool((t != -1).any()), "touched bitmap empty or full"
    (s0, k0), (s1, k1) = _scaler(init), _scaler(final)
    print(f"loss scale {s0:g} -> {s1:g}, skipped steps {k0} -> {k1}")
    assert s1 != s0 or k1 > k0, "no GradScaler decision in the window"


def _record_losses(opt, value_of):
    """FusedAdam.backward / step wrapped on this instance: after every step its loss value goes into slot (k mod N_BATCHES), k
    counting the steps issued -- under grouped_pipeline's capture, the batch index (as Trainer.losses reads them)"""
    slots = torch.full((N_BATCHES,), float("nan"), device=DEV)
    cls, pending, k = type(opt), [], [0]

    def backward(loss):
        cls.backward(opt, loss)
        pending.append(loss)

    def step():
        cls.step(opt)
        with torch.no_grad():
            slots[k[0] % N_BATCHES].copy_(value_of(pending.pop()).reshape(()))
        k[0] += 1
    opt.backward, opt.step = backward, step
    return slots


def _drive(step, slots):
    """issue SCHEDULE's groups through step(i); -> the per-step losses in issue order"""
    hist = []
    for i0 in SCHEDULE:
        for i in range(i0, i0 + G):
            step(i)
        b0 = i0 % N_BATCHES
        hist.append(slots[b0:b0 + G].clone())                  # main stream, behind the group's replay
    torch.cuda.synchronize()                                   # the side stream's groups ahead included
    return torch.cat(hist)


# ---------------------------------------------------------------------------------------------------- NeRF train step
def _scene(kind):
    """bench.sparse_step / bench.flower_step: (bound, packed occupancy, rays of batch b, seed)"""
    from laenerf_amd import synthetic as S
    if kind == "sparse":
        return 1, S.pack_bits_np(S.lego_sparse_density_grid(), 10.0), lambda b: S.lego_like_rays(N_RAYS, seed=700 + b, n_views=1), 77
    return 2, S.pack_bits_np(S.flower_density_grid(), 10.0), lambda b: S.flower_like_rays(N_RAYS, seed=5 + b), 99


def _nerf_setup(kind):
    """as bench._pipelined_train_step prepares a scene: model, FusedAdam(eps=1e-15), occupancy, 4G batches, 17 sizing steps,
    update_mean_count"""
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    from laenerf_amd.renderer import NeRFRenderer
    bound, bits, make_rays, seed = _scene(kind)
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=bound).to(DEV)
    r = NeRFRenderer(net, bound=bound, min_near=0.2).to(DEV)
    r.density_bitfield = torch.from_numpy(bits).to(DEV)
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, growth_interval=GROWTH_INTERVAL)
    batches = []
    for b in range(N_BATCHES):
        o, d = make_rays(b)
        batches.append((torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), torch.rand(N_RAYS, 3, device=DEV)))
    net.train()
    for i in range(17):
        o, d, gt = batches[i]
        with torch.autocast("cuda", dtype=torch.float16):
            res = r.render_train(o, d, bg_color=1, perturb=True, max_steps=1024, gt=gt, scaler=opt)
        opt.backward(res["loss"])
        opt.step()
    r.update_mean_count()
    assert r.mean_count > 0
    return r, opt, batches


@pytest.mark.parametrize("kind", ["sparse", "flower"])
def test_pipeline_equals_its_serial_replay(kind, monkeypatch):
    """the default scheme (march with noise + plan two groups ahead on the side stream) against the same scheme with the side
    stream patched to the current stream: the same graphs, the same RNG replay order, no overlap"""
    chosen = []
    real = bench.concurrent_side_stream

    def recorded(*a, **k):
        out = real(*a, **k)
        chosen.append(out)
        return out
    runs = {}
    for mode in ("pipelined", "serial"):
        monkeypatch.setattr(bench, "concurrent_side_stream",
                            recorded if mode == "pipelined" else (lambda *a, **k: (torch.cuda.current_stream(), None)))
        r, opt, batches = _nerf_setup(kind)
        init = _state(opt, r)
        slots = _record_losses(opt, lambda loss: loss.unscaled)
        step, n_samples = grouped_pipeline(r, opt, batches, G)
        losses = _drive(step, slots)
        runs[mode] = (init, _state(opt, r), losses, list(n_samples))
        del step, r, opt, batches
    assert len(chosen) == 1 and chosen[0][0] != torch.cuda.current_stream()
    print(kind, "side stream:", chosen[0][1])
    (init, got, losses, n), (init_s, ref, losses_s, n_s) = runs["pipelined"], runs["serial"]
    _assert_same(init, init_s, "state after set-up")
    _assert_same(got, ref, "state after the window")
    assert torch.equal(_bits(losses), _bits(losses_s)) and n == n_s
    _assert_power(init, got, losses, n)


@pytest.mark.parametrize("kind", ["sparse", "flower"])
def test_pipeline_equals_the_eager_step_without_noise(kind):
    """march (perturb=False) + plan on the side stream, shading / backward / Adam on the main one, against the unsplit eager step
    (render_train -> backward -> step, the backward planning for itself) over the same batches in the same order"""
    r, opt, batches = _nerf_setup(kind)
    init = _state(opt)
    slots = _record_losses(opt, lambda loss: loss.unscaled)

    def ahead_fn(batch):
        return r.march_train(batch[0], batch[1], perturb=False, max_steps=1024, plan_backward=True)

    def step_fn(batch, marched):
        with torch.autocast("cuda", dtype=torch.float16):
            res = r.shade_train(marched, bg_color=1, gt=batch[2], scaler=opt)
        opt.backward(res["loss"])
        opt.step()
        return res["n_samples"]
    step, n_samples = grouped_pipeline(r, opt, batches, G, ahead_fn=ahead_fn, step_fn=step_fn)
    losses = _drive(step, slots)
    got, n = _state(opt), [n_samples[b] for b in BATCH_ORDER]
    del step, r, opt, batches

    r, opt, batches = _nerf_setup(kind)
    _assert_same(init, _state(opt), "state after set-up")
    ref_losses, ref_n = [], []
    for b in BATCH_ORDER:
        o, d, gt = batches[b]
        with torch.autocast("cuda", dtype=torch.float16):
            res = r.render_train(o, d, bg_color=1, perturb=False, max_steps=1024, gt=gt, scaler=opt)
        opt.backward(res["loss"])
        opt.step()
        ref_losses.append(res["loss"].unscaled.clone().reshape(()))
        ref_n.append(res["n_samples"])
    _assert_same(got, _state(opt), "state after the window")
    assert torch.equal(_bits(losses), _bits(torch.stack(ref_losses))) and n == ref_n
    _assert_power(init, got, losses, n)


# ---------------------------------------------------------------------------------------------------- LAENeRF palette step
STYLE_POINTS = 8192


def _style_setup():
    """bench.style_step's model, optimizer and views (STYLE_POINTS points each) and its three warm-up steps"""
    from laenerf_amd.editing import LAENeRF
    from laenerf_amd.optim import FusedAdam
    params = SimpleNamespace(bound=1, num_palette_bases=8, style_weight=0, weight_loss_uniform=1e-3, weight_loss_non_uniform=1e-3,
                             offset_loss=1e-2, palette_loss_valid=1.0, palette_loss_distinct=1e-2)
    torch.manual_seed(7)
    m = LAENeRF(params, dir_encoding="sphere_harmonics").to(DEV)
    m.train()
    opt = FusedAdam(m, param_groups=m.get_params(1e-3), betas=(0.9, 0.999), eps=1e-8, growth_interval=GROWTH_INTERVAL)
    views = []
    for _ in range(N_BATCHES):
        v = torch.randn(STYLE_POINTS, 3, device=DEV)
        views.append((v / v.norm(dim=-1, keepdim=True) * 0.3 * torch.rand(STYLE_POINTS, 1, device=DEV) ** (1 / 3),
                      torch.nn.functional.normalize(torch.randn(STYLE_POINTS, 3, device=DEV), dim=-1),
                      torch.rand(STYLE_POINTS, 3, device=DEV)))

    def body(view, plan=None):
        x, d, target = view
        with torch.autocast("cuda", dtype=torch.float16):
            loss, pred, w, o = m.forward_train_loss(x, d, target, params, opt, with_palet_loss=True, plan=plan)
        opt.backward(loss)
        opt.step()
        return loss
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            body(views[i], m.plan_backward(views[i][0]) if i else None)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return m, opt, views, body


def test_style_step_pipeline_equals_the_eager_step_without_a_plan():
    """style_step's arrangement (ahead_fn = LAENeRF.plan_backward on the side stream, step_fn = forward_train_loss -> backward ->
    step) against the eager step that plans for itself"""
    m, opt, views, body = _style_setup()
    assert m.ffmlp_shadows and m.plan_backward(views[0][0]) is not None          # the arrangement style_step pipelines
    init = _state(opt)
    slots = _record_losses(opt, lambda loss: loss.terms[1])

    def step_fn(view, plan):
        body(view, plan)
        return STYLE_POINTS
    step, n_points = grouped_pipeline(None, opt, views, G, ahead_fn=lambda view: m.plan_backward(view[0]), step_fn=step_fn)
    losses = _drive(step, slots)
    got = _state(opt)
    del step, m, opt, views, body

    m, opt, views, body = _style_setup()
    _assert_same(init, _state(opt), "state after set-up")
    ref_losses = [body(views[b]).terms[1].clone().reshape(()) for b in BATCH_ORDER]
    _assert_same(got, _state(opt), "state after the window")
    assert torch.equal(_bits(losses), _bits(torch.stack(ref_losses)))
    _assert_power(init, got, losses, n_points)
