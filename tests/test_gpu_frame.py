"""-m gpu: the device-resident inference loop (lae_render_frame) against the operator-by-operator loop of
NeRFRenderer.run_cuda / run_cuda_distill (nerf/renderer.py:335-387, 394-480) on the same kernels, against the oracle's
loop, and against the vectors captured from the reference's unmodified renderer (tests/golden/make_golden.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
from gpu_util import DEV, N, T

pytestmark = pytest.mark.gpu

# HIP frame loop against the ORACLE's loop (fp16 MLPs on both sides; what differs is the fp32 accumulate of the MFMA against the
# oracle FFMLP's and __expf against expf): bounds = ~2x the deviation observed on the MI355X box (printed by the tests), all well
# inside north_star's 1e-4 RGB -- rounds 1-3 asserted 3e-3 here
ORACLE_LOOP_TOL = {"weights_sum": 2e-6, "image": 1.5e-5, "depth": 2.5e-6}      # observed 8.9e-7 / 7.0e-6 / 1.1e-6


def make(bound=1, log2_T=14, seed=0, table_amp=0.5):
    from laenerf_amd import synthetic as S
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=bound, log2_hashmap_size=log2_T).to(DEV)
    net.encoder.embeddings.data.uniform_(-table_amp, table_amp)        # densities spread over orders of magnitude:
    r = NeRFRenderer(net, bound=bound, min_near=0.2).to(DEV)           # rays terminate after very different step counts
    C = r.cascade
    r.density_bitfield = T(S.pack_bits_np(S.sphere_density_grid(cascade=C, bound=float(bound)), 10.0))
    net.eval(); r.eval()
    return net, r


def rays(n, seed, bound=1):
    from laenerf_amd import synthetic as S
    o, d = S.lego_like_rays(n, seed=seed, radius=3.2 if bound == 1 else 2.6)
    return T(o), T(d)


@pytest.mark.parametrize("bound,n", [(1, 5000), (2, 3001), (1, 1), (1, 17)])
def test_frame_loop_equals_operator_loop(bound, n):
    net, r = make(bound=bound)
    o, d = rays(n, seed=3, bound=bound)
    with torch.autocast("cuda", dtype=torch.float16):
        a = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=False)
        b = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=True, want_stats=True)
    # same kernels' arithmetic, same schedule: only the order of the alive list differs -> per-ray results identical
    hit = N(a["weights_sum"]) > 0
    assert hit.sum() > 0 or n < 20
    for k in ("image", "weights_sum"):
        assert np.array_equal(N(a[k]), N(b[k])), k
    assert np.array_equal(N(a["depth"])[hit], N(b["depth"])[hit])           # missed rays: 0/0 = NaN in both
    assert np.array_equal(np.isnan(N(a["depth"])), np.isnan(N(b["depth"])))
    st = b["stats"]
    assert 1 <= st["iterations"] <= 1024 and st["iterations_launched"] >= st["iterations"]
    assert st["rows"] >= n                                                   # the first iteration runs every ray once


def test_frame_loop_perturb_and_thresholds():
    net, r = make(bound=1, seed=1)
    o, d = rays(4096, seed=5)
    with torch.autocast("cuda", dtype=torch.float16):
        for T_thresh, max_steps in ((1e-2, 1024), (1e-4, 64)):
            torch.manual_seed(11)
            a = r.render_eval(o, d, bg_color=torch.tensor([0.2, 0.4, 0.6], device=DEV), perturb=True, max_steps=max_steps,
                              T_thresh=T_thresh, frame_loop=False)
            torch.manual_seed(11)
            b = r.render_eval(o, d, bg_color=torch.tensor([0.2, 0.4, 0.6], device=DEV), perturb=True, max_steps=max_steps,
                              T_thresh=T_thresh, frame_loop=True)
            assert np.array_equal(N(a["image"]), N(b["image"]))
            assert np.array_equal(N(a["weights_sum"]), N(b["weights_sum"]))
        # per-ray background
        bg = torch.rand(4096, 3, device=DEV)
        a = r.render_eval(o, d, bg_color=bg, frame_loop=False)
        b = r.render_eval(o, d, bg_color=bg, frame_loop=True)
        assert np.array_equal(N(a["image"]), N(b["image"]))
        # lookahead marcher in-line instead of on the side stream: same results
        from laenerf_amd.backend import raymarching_backend as rb
        rb.render_frame_set_overlap(False)
        try:
            f = r.render_eval(o, d, bg_color=bg, frame_loop=True)
        finally:
            rb.render_frame_set_overlap(True)
        assert np.array_equal(N(f["image"]), N(b["image"]))
        # two frames back to back on the same stream (the second starts while the first's tail is still queued)
        c = r.render_eval(o, d, bg_color=bg, frame_loop=True)
        e = r.render_eval(o, d, bg_color=bg, frame_loop=True)
        assert np.array_equal(N(c["image"]), N(b["image"])) and np.array_equal(N(e["image"]), N(b["image"]))


def test_frame_loop_row_budget():
    """more rows per iteration than the reference's N: fewer iterations, the same per-ray sample sequences (only the
    rounding of rays_t between iterations may differ)"""
    net, r = make(bound=1, seed=3)
    o, d = rays(6000, seed=2)
    with torch.autocast("cuda", dtype=torch.float16):
        a = r.render_eval(o, d, bg_color=1, frame_loop=True, want_stats=True)
        b = r.render_eval(o, d, bg_color=1, frame_loop=True, want_stats=True, row_budget=4 * 6000)
        c = r.render_eval(o, d, bg_color=1, frame_loop=True, want_stats=True, row_budget=3)      # below N: clamped to N
    assert b["stats"]["iterations"] < a["stats"]["iterations"]
    assert all(c["stats"][k] == a["stats"][k] for k in ("iterations", "rows"))      # launched iterations depend on host timing
    assert np.array_equal(N(c["image"]), N(a["image"]))
    assert np.abs(N(a["image"]) - N(b["image"])).max() < 1e-5
    assert np.abs(N(a["weights_sum"]) - N(b["weights_sum"])).max() < 1e-5
    hit = N(a["weights_sum"]) > 0
    assert np.abs(N(a["depth"])[hit] - N(b["depth"])[hit]).max() < 1e-5


def test_frame_loop_distill():
    from laenerf_amd import synthetic as S
    net, r = make(bound=1, seed=2)
    o, d = rays(4000, seed=7)
    g = S.sphere_density_grid(radius=0.35, boxes=False)
    edit = T(S.pack_bits_np(g, 10.0)) & r.density_bitfield                  # edit region: a subset of the occupied cells
    with torch.autocast("cuda", dtype=torch.float16):
        a = r.render_distill(o, d, edit, frame_loop=False)
        b = r.render_distill(o, d, edit, frame_loop=True)
        a2 = r.render_distill(o, d, edit, grow_grid=True, frame_loop=False)
        b2 = r.render_distill(o, d, edit, grow_grid=True, frame_loop=True)
    assert N(a["weights_edit"]).max() > 0
    for x, y in ((a, b), (a2, b2)):
        for k in ("image", "depth", "depth_edit", "weights_edit", "weights", "x_term"):
            assert np.array_equal(N(x[k]), N(y[k])), k


def test_frame_loop_vs_oracle_loop(O):
    """256 rays: the oracle's march / encode / MLP / composite driven by the reference's loop schedule"""
    net, r = make(bound=1, log2_T=12, seed=4)
    net.encoder.embeddings.data = net.encoder.embeddings.data.half().float()
    n = 256
    o, d = rays(n, seed=9)
    with torch.autocast("cuda", dtype=torch.float16):
        got = r.render_eval(o, d, bg_color=1, max_steps=1024, T_thresh=1e-4, frame_loop=True, want_stats=True)
    on, dn, bits = N(o), N(d), N(r.density_bitfield)
    nears, fars = O.near_far_from_aabb(on, dn, [-1, -1, -1, 1, 1, 1], 0.2)
    th = O.to_f16_bits(N(net.encoder.embeddings))
    ws_h, wc_h = O.to_f16_bits(N(net.sigma_net.weights)), O.to_f16_bits(N(net.color_net.weights))
    offs = N(net.encoder.offsets)
    wsum, depth, image = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    alive, rays_t = np.arange(n, dtype=np.int32), nears.copy()
    step, rows, iters = 0, 0, 0
    while step < 1024 and alive.size > 0:
        n_alive = alive.size
        n_step = max(min(n // n_alive, 8), 1)
        xyzs, dirs, deltas = O.march_rays(n_alive, n_step, alive, rays_t, on, dn, 1.0, bits, 1, 128, nears, fars,
                                          np.zeros(n_alive, np.float32))[:3]
        m = n_alive * n_step
        pad = (-m) % 128
        enc, _ = O.grid_encode_forward((xyzs[:m] + 1) / 2, th, offs, net.encoder.per_level_scale, 16, f16=True, out_blc=True)
        h, _ = O.ffmlp_forward(np.concatenate([enc, np.zeros((pad, 32), np.uint16)]), ws_h, 32, 16, 64, 2)
        hf = O.from_f16_bits(h)[:m]
        sigma = np.exp(hf[:, 0]).astype(np.float32)
        sh, _ = O.sh_encode_forward(dirs[:m], 4)
        cin = O.to_f16_bits(np.concatenate([sh, hf[:, 1:], np.zeros((m, 1), np.float32)], 1))
        oc, _ = O.ffmlp_forward(np.concatenate([cin, np.zeros((pad, 32), np.uint16)]), wc_h, 32, 16, 64, 3)
        rgb = (1 / (1 + np.exp(-O.from_f16_bits(oc)[:m, :3]))).astype(np.float32)
        O.composite_rays(n_alive, n_step, alive, rays_t, sigma, rgb, deltas[:m], wsum, depth, image, 1e-4)
        alive = alive[alive >= 0]
        step += n_step; rows += m; iters += 1
    image = image + (1 - wsum)[:, None]
    assert got["stats"]["iterations"] == iters and got["stats"]["rows"] == rows      # schedule and row counts: exact
    hit = wsum > 0
    dref = np.clip(depth - nears, 0, None)[hit] / (fars - nears)[hit]
    dev = {"weights_sum": float(np.abs(N(got["weights_sum"]) - wsum).max()), "image": float(np.abs(N(got["image"]) - image).max()),
           "depth": float(np.abs(N(got["depth"])[hit] - dref).max())}
    print("frame loop vs oracle loop, max abs deviation:", {k: float("%.3g" % v) for k, v in dev.items()})
    for k, v in dev.items():
        assert v < ORACLE_LOOP_TOL[k], dev


@pytest.mark.parametrize("tag", ["b1", "b2"])
def test_frame_loop_vs_reference_capture(tag):
    """vectors from the reference's unmodified nerf/renderer.py run_cuda / run_cuda_distill (fp32 table there, fp16 here)"""
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.renderer import NeRFRenderer
    g = golden("e2e_" + tag)
    bound = int(g["bound"])
    net = NeRFNetwork(bound=bound, num_levels=16, log2_hashmap_size=10).to(DEV)
    net.encoder.embeddings.data = T(g["table"])
    net.sigma_net.weights.data = T(g["sigma_w"])
    net.color_net.weights.data = T(g["color_w"])
    r = NeRFRenderer(net, bound=bound, min_near=0.2).to(DEV)
    r.density_bitfield = T(g["bitfield"])
    net.eval()
    o, d = T(g["rays_o"]), T(g["rays_d"])
    with torch.autocast("cuda", dtype=torch.float16):
        ev = r.render_eval(o, d, bg_color=1, max_steps=256, frame_loop=True)
        ds = r.render_distill(o, d, T(g["edit_bitfield"]), max_steps=256, frame_loop=True)
    # north_star tolerance 1e-4; measured 2.0e-5 / 1.8e-5 (tools/fp16_table_delta.py: the fixture tables are fp16-representable,
    # so what differs from the capture is the half accumulate of the encoder and the fp16 MLP arithmetic)
    assert np.abs(N(ev["image"]) - g["eval_image"]).max() < 1e-4
    for k, ref in (("image", "dist_image"), ("weights", "dist_weights"), ("weights_edit", "dist_weights_edit")):
        assert np.abs(N(ds[k]) - g[ref]).max() < 1e-4, k


def test_frame_loop_refuses_capture_and_cpu():
    net, r = make(bound=1)
    o, d = rays(256, seed=1)
    with torch.autocast("cuda", dtype=torch.float16):
        r.render_eval(o, d, frame_loop=True)                                   # warm: workspace allocation
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError):
            with torch.cuda.graph(gph):
                r.render_eval(o, d, frame_loop=True)
    torch.cuda.synchronize()


def test_tiled_ray_order_returns_the_same_image():
    from laenerf_amd import synthetic as S
    net, r = make(bound=1, seed=6)
    o, d = S.frame_rays(64, 96)
    o, d = T(o), T(d)
    with torch.autocast("cuda", dtype=torch.float16):
        a = r.render_eval(o, d, bg_color=1)
        b = r.render_eval(o, d, bg_color=1, image_hw=(64, 96))            # rendered in 8x4 pixel tiles, returned in scanline order
        c = r.render_eval(o, d, bg_color=1, image_hw=(64, 96), tile_hw=(16, 16), frame_loop=False)
    for k in ("image", "weights_sum"):
        assert np.array_equal(N(a[k]), N(b[k])) and np.array_equal(N(a[k]), N(c[k])), k


def test_render_frame_argument_errors():
    """lae_render_frame through the stub: bad arguments raise, nothing falls back"""
    from laenerf_amd import raymarching as rm
    net, r = make(bound=1)
    o, d = rays(64, seed=2)
    enc = net.encoder
    table = enc.embeddings.detach().half()
    ws, wc = net.sigma_net.weights.detach().half(), net.color_net.weights.detach().half()
    args = (o, d, r.aabb_infer, 0.2, r.density_bitfield, 1, 1, 128, table, enc.offsets, enc.per_level_scale, 16, ws, wc)
    res = rm.render_frame(*args, bg_color=1)                                   # sanity: the direct call works
    assert res["image"].shape == (64, 3)
    with pytest.raises(RuntimeError):
        rm.render_frame(*args, max_n_step=9)                                   # more steps per iteration than the lookahead records
    with pytest.raises(RuntimeError):
        rm.render_frame(*args, max_steps=0)
    with pytest.raises(RuntimeError):
        rm.render_frame(o, d, r.aabb_infer, 0.2, r.density_bitfield, 1, 1, 128, enc.embeddings.detach(), enc.offsets,
                        enc.per_level_scale, 16, ws, wc)                       # fp32 table
    with pytest.raises(RuntimeError):
        rm.render_frame(*args[:4], r.density_bitfield.cpu(), *args[5:])        # bitfield on the CPU: no fallback


def test_frames_on_two_streams():
    """frames issued from different torch streams share the library's mirror / side stream: the second waits for the first"""
    net, r = make(bound=1, seed=8)
    o, d = rays(3000, seed=4)
    with torch.autocast("cuda", dtype=torch.float16):
        ref = r.render_eval(o, d, bg_color=1)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        outs = []
        for st in (s1, s2, s1, s2):
            with torch.cuda.stream(st):
                outs.append(r.render_eval(o, d, bg_color=1))
        torch.cuda.synchronize()
    for res in outs:
        assert np.array_equal(N(res["image"]), N(ref["image"]))


def test_side_stream_is_chosen_by_a_timed_handshake():
    """round 5: with the first frame of a caller stream the library times 16 hand-overs through its own store / poll kernels on its
    side-stream candidates (the highest-priority one first; streams of the caller's class are created when that one is not concurrent
    or slow -- which happens once the process uses a few more streams: a 9.8 ms frame took 23 ms) and takes the first prompt one.
    Here: eight other streams in use, a frame on a NEW caller stream -> a probe record whose chosen candidate is concurrent and at
    most as slow as every other candidate measured; same image as the in-line loop bit for bit."""
    from laenerf_amd.backend import raymarching_backend as B
    net, r = make(bound=1, seed=8)
    o, d = rays(3000, seed=4)
    busy = [torch.cuda.Stream() for _ in range(8)]
    for st in busy:
        with torch.cuda.stream(st):
            torch.zeros(16, device=DEV).add_(1)
    torch.cuda.synchronize()
    with torch.autocast("cuda", dtype=torch.float16):
        B.render_frame_set_overlap(False)
        try:
            ref = r.render_eval(o, d, bg_color=1)
        finally:
            B.render_frame_set_overlap(True)
        caller = torch.cuda.Stream()
        caller.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(caller):
            res = r.render_eval(o, d, bg_color=1)
        torch.cuda.synchronize()
    assert np.array_equal(N(res["image"]), N(ref["image"]))
    probe = B.render_frame_probe()
    print("side-stream probe:", probe)
    assert B.render_frame_mode() == 1 and probe["in_use"] >= 0
    us = probe["handshake_us"]
    measured = [v for v in us if v >= 0]
    assert us[probe["in_use"]] >= 0 and us[probe["in_use"]] <= min(measured) + 1e-3
    assert us[probe["in_use"]] < 400.0 or all(v >= 400.0 for v in measured)  # a slow stream is only kept when no prompt one was found


@pytest.mark.parametrize("kind", ["opaque", "empty"])
def test_frame_loop_ends_when_every_ray_dies_at_once(kind):
    """all rays terminate in the first iteration (opaque field) or never find a sample (empty bitfield): n_alive drops to 0
    in one step. The host must treat an observed n_alive == 0 as the end of the frame even if the done flag of the same
    mirror update is not visible yet (regression: a zero-workgroup launch, 'invalid configuration argument')"""
    net, r = make(bound=2, seed=2, table_amp=0.5)
    if kind == "opaque":
        net.sigma_net.weights.data.abs_().mul_(8.0)                          # huge densities everywhere
    else:
        r.density_bitfield = torch.zeros_like(r.density_bitfield)
    for n in (64, 300, 2048):
        o, d = rays(n, seed=n, bound=2)
        with torch.autocast("cuda", dtype=torch.float16):
            a = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=False)
            for rep in range(40):                                            # the race is a matter of timing: many short frames
                b = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=True, want_stats=(rep % 2 == 0))
                assert np.array_equal(N(a["image"]), N(b["image"]))
                assert np.array_equal(N(a["weights_sum"]), N(b["weights_sum"]))


@pytest.mark.parametrize("bound,density", [(1, 0.004), (2, 0.002), (2, 0.05), (1, 0.0), (2, 0.0)])
def test_frame_loop_on_sparse_random_occupancy(bound, density):
    """the lookahead's "nothing ahead" test (coarse occupancy field, csrc/frame.hip k_frame_coarse_*) must never end a walk
    that still has a sample in front of it: isolated occupied cells scattered over every cascade (most rays cross long empty
    stretches between hits, many graze marked coarse cells), rays from outside the volume, from inside it, axis-parallel and
    nearly axis-parallel ones -- frame loop and operator loop bit for bit"""
    net, r = make(bound=bound, seed=7, table_amp=0.3)
    rng = np.random.default_rng(11)
    bits = (rng.random(r.cascade * 128 ** 3) < density)
    bits[-64:] = True                                                       # the top level's far corner: cells positions clamp into
    targets = None
    if density == 0.0:
        # the dangerous case for an early stop: a volume that is empty except for 40 isolated cells per cascade (and one
        # small box), with rays aimed exactly at those cells from far away -- most of each ray's path passes the test
        from laenerf_amd import synthetic as S
        cx, cy, cz = S._morton_inverse_table(128)
        targets = []
        for c in range(r.cascade):
            pick = rng.choice(128 ** 3, 40, replace=False)
            bits[c * 128 ** 3 + pick] = True
            b_c = min(2.0 ** c, float(bound))
            ctr = np.stack([cx[pick], cy[pick], cz[pick]], 1).astype(np.float32)
            targets.append(((ctr + 0.5) / 128 * 2 - 1) * b_c)
            box = (np.abs(cx - 40) < 3) & (np.abs(cy - 90) < 3) & (np.abs(cz - 64) < 3)
            bits[c * 128 ** 3 + np.nonzero(box)[0]] = True
        targets = np.concatenate(targets).astype(np.float32)
    packed = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    r.density_bitfield = T(packed)
    n = 6000
    o, d = rays(n, seed=9, bound=bound)
    o, d = N(o).copy(), N(d).copy()
    # a third of the rays start inside the volume with random directions
    k = n // 3
    o[:k] = rng.uniform(-0.6 * bound, 0.6 * bound, (k, 3)).astype(np.float32)
    dd = rng.standard_normal((k, 3)).astype(np.float32)
    d[:k] = dd / np.linalg.norm(dd, axis=1, keepdims=True)
    # axis-parallel and nearly axis-parallel rays (a zero / tiny direction component: 1 / d is inf / huge)
    for j, ax in enumerate((0, 1, 2)):
        base = k + 40 * j
        o[base:base + 40] = rng.uniform(-0.5 * bound, 0.5 * bound, (40, 3)).astype(np.float32)
        v = np.zeros((40, 3), np.float32); v[:, ax] = np.where(rng.random(40) < 0.5, 1.0, -1.0)
        v[20:, (ax + 1) % 3] = 1e-4
        d[base:base + 40] = v / np.linalg.norm(v, axis=1, keepdims=True)
    if targets is not None:                                                 # the last 2000 rays: from a sphere around the volume at a target cell
        m = 2000
        tg = targets[rng.integers(0, len(targets), m)] + rng.uniform(-0.3, 0.3, (m, 3)).astype(np.float32) * (2.0 * bound / 128)
        src = rng.standard_normal((m, 3)).astype(np.float32)
        src = src / np.linalg.norm(src, axis=1, keepdims=True) * (2.5 * bound)
        v = tg - src
        o[-m:] = src; d[-m:] = v / np.linalg.norm(v, axis=1, keepdims=True)
    o, d = T(o), T(d)
    with torch.autocast("cuda", dtype=torch.float16):
        a = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=False)
        b = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=True, want_stats=True)
    hit = N(a["weights_sum"]) > 0
    assert hit.mean() > (0.3 if targets is None else 0.2)
    if targets is not None:
        assert hit[-2000:].mean() > 0.8                                     # the aimed rays do find their isolated cell (outer-cascade cells inside the inner box are never probed)
    for key in ("image", "weights_sum"):
        assert np.array_equal(N(a[key]), N(b[key])), key
    assert np.array_equal(N(a["depth"])[hit], N(b["depth"])[hit])
    assert np.array_equal(np.isnan(N(a["depth"])), np.isnan(N(b["depth"])))


_AB_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import test_gpu_frame as F
net, r = F.make(bound={bound})
o, d = F.rays({n}, seed=5, bound={bound})
with torch.autocast("cuda", dtype=torch.float16):
    a = r.render_eval(o, d, bg_color=1, max_steps=1024, frame_loop=True)
torch.cuda.synchronize()
h = hashlib.sha256()
for k in ("image", "depth", "weights_sum"):
    h.update(a[k].float().contiguous().cpu().numpy().tobytes())
print("HASH", h.hexdigest())
"""


@pytest.mark.parametrize("bound,n", [(1, 40000), (2, 20011)])
def test_lookahead_variants_render_the_same_bits(bound, n):
    """the lookahead's A/B switches (stragglers finished by the finishing kernel or inside the lane kernel, visits of an empty
    stretch probed together or one by one, coarse-field early stop, emit path, encoder schedule) change WHEN probes are issued and WHO walks a ray, never a sample: the
    frame must come out bit for bit the same.  The switches are read once per process: fresh child processes."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    hashes = {}
    for name, env in (("default", {}), ("in-wave stragglers", {"LAE_FRAME_FINISH_QUEUE": "0"}), ("plain visits", {"LAE_FRAME_SPEC": "0"}),
                      ("queue everything up to 48", {"LAE_FRAME_COOP_MAX": "48"}),
                      # round 4: the "nothing ahead" test off, rows stored straight from the lanes, the training cost table for the
                      # encoder's XCD schedule / the finest level in halves, stragglers of the first walk handed over, hand-over
                      # of whole waves after 4 lane rounds
                      ("no coarse field", {"LAE_FRAME_COARSE": "0"}),
                      ("training schedule", {"LAE_GRID_FWD_FRAME_SCHED": "0"}), ("level halves", {"LAE_GRID_FWD_FRAME_SCHED": "2"}),
                      ("lookahead in line", {"LAE_FRAME_OVERLAP": "0"}),
                      ("whole waves never handed over", {"LAE_FRAME_ADMIT_CAP": "0"}), ("one worst-case encoder launch", {"LAE_FRAME_GRID_TAIL": "0"}),
                      ("overflow launch always", {"LAE_GRID_FWD_TAIL_MIN": "0"}), ("host one iteration ahead", {"LAE_FRAME_LAG": "1"}), ("general emit kernel at 8 samples per ray", {"LAE_FRAME_EMIT8": "0"}), ("host six iterations ahead", {"LAE_FRAME_LAG": "6"}), ("handed over after one round", {"LAE_FRAME_ADMIT_ROUND": "1", "LAE_FRAME_ADMIT_CAP": "100000"})):
        e = dict(os.environ, **env)
        out = subprocess.run([sys.executable, "-c", _AB_SCRIPT.format(root=ROOT, bound=bound, n=n)], capture_output=True, text=True, timeout=600, env=e)
        lines = [l for l in out.stdout.splitlines() if l.startswith("HASH ")]
        assert out.returncode == 0 and len(lines) == 1, (name, out.stdout[-1000:], out.stderr[-2000:])
        hashes[name] = lines[0]
    assert len(set(hashes.values())) == 1, hashes


_AB_DISTILL_SCRIPT = r"""
import hashlib, sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import test_gpu_frame as F
from laenerf_amd import synthetic as S
net, r = F.make(bound=1, seed=2)
o, d = F.rays({n}, seed=7)
edit = F.T(S.pack_bits_np(S.sphere_density_grid(radius=0.35, boxes=False), 10.0)) & r.density_bitfield
KEYS = ("image", "depth", "depth_edit", "weights_edit", "weights", "x_term")
with torch.autocast("cuda", dtype=torch.float16):
    b = r.render_distill(o, d, edit, frame_loop=True)
    a = r.render_distill(o, d, edit, frame_loop=False) if {oploop} else None
torch.cuda.synchronize()
h = hashlib.sha256()
for k in KEYS:
    h.update(b[k].float().contiguous().cpu().numpy().tobytes())
print("HASH", h.hexdigest())
print("EDITED", int((b["weights_edit"] > 0).sum()))
if a is not None:
    print("OPLOOP", " ".join(k for k in KEYS if np.array_equal(F.N(a[k]), F.N(b[k]))))
"""
AB_DISTILL_RAYS = 1000


def test_emit_variants_render_the_same_distill_bits():
    """The distill render (edit grid: k_frame_emit<true> / k_frame_emit8<true> / k_frame_head<true>) of test_frame_loop_distill's
    scene in fresh child processes (the switches are read once per process): the default, where the late iterations -- the
    host's bound of n_alive at or below an eighth of the row budget -- go through k_frame_emit8<true>, and LAE_FRAME_EMIT8=0,
    where k_frame_emit<true> writes the same rows.  Same bits; and the default run equals the operator loop
    (k_composite_infer<true>, eight samples per ray in the late iterations) array for array.
    1000 rays.  The host takes k_frame_emit8 once its lagging bound of n_alive is at most an eighth of the row budget (n_lb >= 8),
    i.e. at most 125 rays here; of the counts traced (1000 / 2000 / 4000) this is the smallest, and no smaller one was tried, so
    it is an upper bound of the smallest count that reaches the kernel, not that count.  Emit launches of the default run (one kernel
    trace of the child script per count on an MI355X; the counts move by a launch or two from run to run with the host's lag):
    1000 rays, 97 iterations: k_frame_emit<true> 63, k_frame_emit8<true> 34, k_frame_emit<false> 0, k_frame_emit8<false> 0;
    2000 rays: 64 / 29 / 0 / 0; 4000 rays: 66 / 28 / 0 / 0."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    hashes, keys = {}, None
    for name, env, oploop in (("default", {}, 1), ("general emit kernel at 8 samples per ray", {"LAE_FRAME_EMIT8": "0"}, 0)):
        out = subprocess.run([sys.executable, "-c", _AB_DISTILL_SCRIPT.format(root=ROOT, n=AB_DISTILL_RAYS, oploop=oploop)],
                             capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out.stdout.splitlines() if l.startswith(("HASH ", "EDITED ", "OPLOOP "))}
        assert out.returncode == 0 and "HASH" in lines, (name, out.stdout[-1000:], out.stderr[-2000:])
        assert int(lines["EDITED"]) > 0, name
        hashes[name] = lines["HASH"]
        if oploop:
            keys = lines["OPLOOP"].split()
    assert len(set(hashes.values())) == 1, hashes
    assert keys == ["image", "depth", "depth_edit", "weights_edit", "weights", "x_term"], keys


def _degrade_child(env):
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    e = dict(os.environ, **env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "frame_degrade_child.py")], capture_output=True, text=True, timeout=600, env=e)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (env, out.stdout[-1000:], out.stderr[-3000:])
    warnings = [l for l in out.stderr.splitlines() if "laenerf_amd: render_frame:" in l]
    return json.loads(lines[0]), warnings


def test_frame_loop_degrades_to_the_inline_lookahead_instead_of_failing():
    """The overlapped frame loop orders its two streams with polled words, which needs them to run side by side (the reference's
    loop, nerf/renderer.py:335-387, has no such requirement).  Fresh child processes (the environment must be set before the
    first HIP call): (a) default; (b) dispatch serialised (AMD_SERIALIZE_KERNEL=3) and (c) every stream on ONE hardware queue
    (GPU_MAX_HW_QUEUES=1 with the side stream at the caller's priority -- at its default, high, priority it has a queue of
    its own): the probe finds out, frames are rendered in line; (d) as (c) with the probe skipped (LAE_FRAME_OVERLAP=1) and a
    short wait time-out: the first frame's handshake gives up, the frame is poisoned, rendered AGAIN in line inside the same
    call, and the process stays in line; (e) 40 live torch streams, the frame on one of them.  Every frame of every child has
    the same bits; at most one warning per process."""
    base, w0 = _degrade_child({})
    assert base["mode"] == 1 and not w0 and all(f["finite"] and f["status"] == 0 for f in base["frames"])
    sha = base["frames"][0]["sha"]
    assert all(f["sha"] == sha for f in base["frames"])
    report = {"default": base}

    def same_bits(res):
        assert [f["sha"] for f in res["frames"]] == [sha, sha] and all(f["finite"] for f in res["frames"]), res
        assert all(f["status"] == 0 for f in res["frames"]), res        # lae_render_frame_last_status after the synchronise: completed
    ser, w1 = _degrade_child({"AMD_SERIALIZE_KERNEL": "3"})
    same_bits(ser)
    assert ser["mode"] == 0 and len(w1) == 1 and "do not run concurrently" in w1[0]
    alias = {"GPU_MAX_HW_QUEUES": "1", "LAE_FRAME_SIDE_PRIO": "0"}
    one_q, w2 = _degrade_child(alias)
    same_bits(one_q)
    assert (one_q["mode"] == 1 and not w2) or (one_q["mode"] == 0 and len(w2) == 1)   # side by side after all, or said so once
    hung, w3 = _degrade_child(dict(alias, LAE_FRAME_OVERLAP="1", LAE_FRAME_WAIT_SPINS_LOG2="16"))
    same_bits(hung)
    if one_q["mode"] == 0:                                      # the queues really alias on this box: the give-up path ran
        assert hung["mode"] == 0 and len(w3) == 1 and "timed out" in w3[0]
    many, w4 = _degrade_child({"LAE_TEST_LIVE_STREAMS": "40"})
    same_bits(many)
    assert len(w4) <= 1
    inline, w5 = _degrade_child({"LAE_FRAME_OVERLAP": "0"})
    same_bits(inline)
    assert inline["mode"] == 0 and not w5
    report.update({"serialised dispatch": (ser, w1), "one hw queue": (one_q, w2), "one hw queue, probe skipped": (hung, w3),
                   "40 live streams": (many, w4), "in line": inline})
    print("frame-loop degrade paths:", report)


def _neighbour_check(*args):
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mfma_neighbour_check.py"), *args], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, TMPDIR="/tmp"))
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-1500:], out.stderr[-3000:])
    return json.loads(lines[0])


def test_kernels_keep_their_bits_beside_a_process_that_keeps_the_matrix_pipe_busy():
    """gfx950 packed-fp32 erratum (laenerf_amd/build.py): beside another wave's MFMA instructions a packed-fp32
    instruction whose low result takes SRC1's high half can read that half as zero.  This was round 4's unexplained "two-process
    fault"; the reference's flow shares a GPU between trainer and renderer (nerf/gui.py:1985-2028).  In a fresh child process, with
    tools/ubench/bin/spinner (back-to-back v_mfma loops) as a SECOND PROCESS on the GPU: the fp16 hash-grid backward, the fp32
    hash-grid forward with dy_dx, the SH encoder, a palette step's gradients and an inference frame must keep the bits they have
    alone.  Where a library built with the compiler's defaults (packed fp32 on) is at hand (tools/grid_loop_fault.sh / the line in
    DESIGN.md leave one), the same check must FAIL on it -- the test has teeth.  tools/suite_beside_mfma.sh runs the whole parity
    suite this way (profiles/r5_suite_beside_mfma.txt)."""
    import os
    from conftest import ROOT
    res = _neighbour_check("--reps", "25")
    print("beside an MFMA neighbour:", res)
    assert res["ok"] is True, res
    raw = os.path.join(ROOT, "tools", "ubench", "bin", "liblaenerf_raw.so")
    from laenerf_amd import _lib
    if os.path.exists(raw) and os.path.getmtime(raw) >= os.path.getmtime(_lib.SO_PATH):       # a probe build of THESE sources (a stale one lacks newer entry points)
        bad = _neighbour_check("--reps", "25", "--lib", raw)
        print("library with packed fp32 on:", bad)
        assert bad["ok"] is False and bad["grid_backward_fp16"]["runs_that_differ"] > 0 and bad["grid_forward_fp32_dy_dx"]["runs_that_differ"] > 0, bad


def test_two_processes_rendering_frames_keep_their_bits():
    """round 4's two-rank soak inside the suite (tools/two_rank_soak.sh ran outside it): two PROCESSES render the same frame on
    one GPU, 120 and 360 times; every frame of both must equal its process's first frame bit for bit (tools/grid_loop_fault.py)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "grid_loop_fault.py"), "--frames", "120", "--neighbour", "same"],
                         capture_output=True, text=True, timeout=900, env=dict(os.environ, TMPDIR="/tmp"))
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-1500:], out.stderr[-3000:])
    j = json.loads(lines[0])
    assert j["frames_that_differ"] == 0 and j["neighbour_result"]["frames_that_differ"] == 0, j
    assert j["neighbour_result"]["frames"] == 360
