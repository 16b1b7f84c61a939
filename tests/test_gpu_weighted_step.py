"""Per-pixel weights and a second colour target in the fused training step: the WGT flavour of k_composite_train_step through
lae_composite_rays_train_step and its weight term.  Cases: N in {1, 5, 67} (below, across and no multiple of the 4 rays of a workgroup); rays of
0, 1, 63, 64, 65 and 130 samples (the passes of 64) and one that stops early on T_thresh; planes gathered through duplicated pix_inds
or, with pix_inds = NULL, by the ray; a tail of rows no ray owns; every output buffer poisoned with NaN.  The float64 restatement is
pinned by test_weighted_step_cpu.py.

Measured on an MI355X against float64 (test_against_the_fp64_restatement prints them; worst over N in {1, 5, 67} and 3 / 4 channels):
grad_image 5.8e-8 relative (bound 1e-6), grad_sigmas 8.9e-8 absolute (bound 3e-5 at these gradients), grad_rgbs 3.0e-8 absolute (bound
1e-6), the total and the second term within 1e-7 relative (bound 1e-5)."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, N as NP, T
from step_args import term_refs
from test_weighted_step_cpu import check_weighted_einval

pytestmark = pytest.mark.gpu

T_THRESH = 1e-4
SIZES = (1, 5, 67)
#          num_steps, kind: the first ray spans three passes, the first five hold an empty ray, a pass boundary and the early stop
PATTERN = [(130, "plain"), (0, "plain"), (65, "plain"), (100, "stop"), (1, "plain"), (63, "plain"), (64, "plain")]
TAIL_ROWS = 5
LAMBDA_2, LAMBDA_DEPTH, LAMBDA_DIST, LAMBDA_OPAC, SCALE = 0.5, 0.37, 0.25, 0.5, 1024.0
F16, F32 = 1, 2
TERMS = [(), ("depth",), ("dist",), ("opac",), ("scale", "bg_rays"), ("depth", "dist", "opac", "scale", "bg_rays")]


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def build(N, seed=31):
    rng = np.random.default_rng(seed + N)
    spec = [PATTERN[i % len(PATTERN)] for i in range(N)]
    owned = sum(s for s, _ in spec)
    M = owned + TAIL_ROWS
    sig = rng.uniform(0, 2.0, M).astype(np.float32)
    rays = np.zeros((N, 3), np.int32)
    rays[:, 0] = rng.permutation(N)
    off = 0
    for n, (steps, kind) in enumerate(spec):
        rays[n, 1:] = (off, steps)
        if kind == "stop":
            sig[off:off + steps] = rng.uniform(0, 60.0, steps)
        off += steps
    nears = rng.uniform(0.2, 1.0, N).astype(np.float32)
    P = 2 * N + 3                                                  # plane entries; pix_inds draws from them with repeats
    inds = rng.integers(0, P, N).astype(np.int64)
    if N >= 5:
        inds[3] = inds[0]                                          # at least one duplicate
    w = rng.uniform(0, 2, P).astype(np.float16).astype(np.float32)  # fp16-representable: the fp16 plane holds the same values
    s4 = rng.uniform(0, 1, (P, 4)).astype(np.float16).astype(np.float32)
    z = rng.uniform(0.5, 3.0, N).astype(np.float32)
    z[::4] = 0.0
    return dict(sigmas=sig, rgbs=rng.uniform(0, 1, (M, 3)).astype(np.float32),
                deltas=np.stack([rng.uniform(0.005, 0.02, M), rng.uniform(0.005, 0.03, M)], -1).astype(np.float32), rays=rays, rows_end=owned,
                M=M, N=N, P=P, nears=nears, fars=(nears + rng.uniform(1.0, 3.0, N)).astype(np.float32),
                bg_rays=rng.uniform(0, 1, (N, 3)).astype(np.float32), target=rng.uniform(0, 1, (N, 3)).astype(np.float32), inds=inds, w=w, s4=s4,
                z=z, spec=spec)


@pytest.fixture(scope="module")
def cases():
    from laenerf_amd import build as B
    B.build()
    out = {}
    for N in SIZES:
        c = build(N)
        t = {k: T(c[k]) for k in ("sigmas", "rgbs", "deltas", "rays", "nears", "fars", "bg_rays", "target", "inds", "w", "s4", "z")}
        t["rows_end"] = torch.tensor([c["rows_end"]], dtype=torch.int32, device=DEV)
        t["scale"] = torch.tensor([SCALE], device=DEV)
        out[N] = (c, t)
    return out


def _dt(t):
    return F16 if t.dtype == torch.float16 else F32


def step(c, t, terms=(), w=None, t2=None, inds=None, lam=LAMBDA_2, entry="weighted", target=None, check=True):
    """one call of lae_composite_rays_train_step through the binding table, always with the criterion term (MSE) and, unless
    entry="crit", with the weight term; every output poisoned -> the outputs; check=False leaves out the host reads (for a capture)"""
    from laenerf_amd import _lib
    p = _lib.ptr
    M, n = c["M"], c["N"]
    nb = (n + 3) // 4
    o = dict(ws=_nan(n), dp=_nan(n), im=_nan(n, 3), do=_nan(n), io=_nan(n, 3), gi=_nan(n, 3), gs=_nan(M), gc=_nan(M, 3), loss=_nan(2), part=_nan(nb))
    target = t["target"] if target is None else target
    args = [p(t["sigmas"]), p(t["rgbs"]), p(t["deltas"]), p(t["rays"]), M, n, T_THRESH, p(t["nears"]), p(t["fars"]),
            p(t["bg_rays"]) if "bg_rays" in terms else None, 1.0, 1.0, 1.0, p(t["rows_end"]), p(target), p(t["scale"]) if "scale" in terms else None,
            p(o["ws"]), p(o["dp"]), p(o["im"]), p(o["do"]), p(o["io"]), p(o["gi"]), p(o["gs"]), p(o["gc"]), p(o["loss"]), p(o["part"]), 0]
    depth = dist = weight = None
    if "depth" in terms:
        o["gd"], o["dpart"] = _nan(n), _nan(nb)
        depth = (p(t["z"]), F32, None, LAMBDA_DEPTH, 0, p(o["gd"]), p(o["dpart"]))
    if "dist" in terms:
        o["ds"], o["gx"], o["xpart"] = _nan(n), _nan(n), _nan(nb)
        dist = (LAMBDA_DIST, 0, p(o["ds"]), p(o["gx"]), p(o["xpart"]))
    if "opac" in terms:
        o["op"], o["gw"], o["opart"] = _nan(n), _nan(n), _nan(nb)
        crit = (0, 0.1, LAMBDA_OPAC, 0, p(o["op"]), p(o["gw"]), p(o["opart"]))
    else:
        crit = (0, 0.1, 0.0, 0, None, None, None)
    if entry != "crit":                                            # "crit": no weight term
        if t2 is not None:
            o["tpart"] = _nan(nb)
        weight = (p(w), 0 if w is None else _dt(w), p(t2), 0 if t2 is None else _dt(t2), 0 if t2 is None else int(t2.shape[-1]), p(inds),
                  lam, p(o.get("tpart")))
    rc = _lib.load().lae_composite_rays_train_step(*args, *term_refs(depth, dist, crit, weight), _lib.stream())
    assert rc == 0, rc
    for k, v in o.items():
        assert not check or torch.isfinite(v).all(), k             # every output row is written
    return o


def _same(a, b, keys=None):
    assert keys is not None or a.keys() == b.keys()
    for k in (keys or a):
        assert torch.equal(a[k], b[k]), k


def _finish(parts, n_elem):
    from laenerf_amd.backend import raymarching_backend as B
    out = _nan(2)
    B.loss_finish(parts, parts.numel(), n_elem, None, out)
    return out


def test_the_cases_hold_what_they_claim(cases):
    c = cases[67][0]
    steps = {s for s, _ in c["spec"]}
    assert steps >= {0, 1, 63, 64, 65, 130} and any(k == "stop" for _, k in c["spec"])
    assert len(set(c["inds"].tolist())) < 67 and c["inds"].max() < c["P"] and c["inds"].min() >= 0
    assert {s for s, _ in cases[5][0]["spec"]} == {130, 0, 65, 100, 1} and cases[1][0]["spec"] == [(130, "plain")]
    assert c["w"].min() >= 0 and c["w"].max() <= 2 and c["w"].max() > 1.5 and c["w"].min() < 0.5


# ---------------------------------------------------------------------------------------------------------------- 1 bits
@pytest.mark.parametrize("terms", TERMS, ids=lambda v: "+".join(v) or "plain")
@pytest.mark.parametrize("N", SIZES)
def test_no_plane_and_a_plane_of_ones_are_the_crit_step(cases, N, terms):
    c, t = cases[N]
    old = step(c, t, terms, entry="crit")
    _same(old, step(c, t, terms))                                          # w_src == NULL && t2_src == NULL
    ones = torch.ones(c["P"], device=DEV)
    _same(old, step(c, t, terms, w=ones, inds=t["inds"]))
    _same(old, step(c, t, terms, w=ones.half(), inds=t["inds"]))
    _same(old, step(c, t, terms, w=ones[:N].contiguous()))                 # pix_inds == NULL: gathered by the ray


@pytest.mark.parametrize("N", SIZES)
def test_fp16_and_fp32_planes_and_alpha_one(cases, N):
    c, t = cases[N]
    terms = TERMS[-1]
    a = step(c, t, terms, w=t["w"], t2=t["s4"], inds=t["inds"])
    _same(a, step(c, t, terms, w=t["w"].half(), t2=t["s4"].half(), inds=t["inds"]))
    _same(a, step(c, t, terms, w=t["w"].half(), t2=t["s4"], inds=t["inds"]))
    s3 = t["s4"][:, :3].contiguous()
    s4 = torch.cat([s3, torch.ones(c["P"], 1, device=DEV)], 1).contiguous()
    b = step(c, t, terms, w=t["w"], t2=s3, inds=t["inds"])
    _same(b, step(c, t, terms, w=t["w"], t2=s4, inds=t["inds"]))
    _same(b, step(c, t, terms, w=t["w"], t2=s4.half(), inds=t["inds"]))
    assert not torch.equal(a["gi"], b["gi"])                               # the alpha of the first is not 1: the blend matters
    # pix_inds == NULL equals the gather done by hand
    wg, sg = t["w"][t["inds"]].contiguous(), t["s4"][t["inds"]].contiguous()
    _same(a, step(c, t, terms, w=wg, t2=sg))


# ---------------------------------------------------------------------------------------------------------------- 2 values
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("N", SIZES)
def test_against_the_fp64_restatement(cases, N, channels):
    """every term on, no loss scale: the family's absolute bounds (grad_rgbs 1e-6, grad_sigmas 3e-5) were set at scale 1
    (test_gpu_criterion.py's test_entropy_with_huber_against_the_fp64_restatement passes no scale) -- the float32 forward's error in
    image_out, ~1e-7, reaches the sample gradients times (w^2 + lambda u^2) * 2 / (3 N) * scale.  grad_image (rtol 1e-6, atol 0) is compared with the restatement's expression in float64 on the
    kernel's own float32 operands -- image_out and the blended second target --, as test_gpu_criterion.py compares the colour gradients
    on the kernel's own e (the forward's error is the forward tests' subject); the sample gradients and the two finished values with
    composite_train_step_numpy, with that file's bounds.  The relative bound holds although the gradient's two parts cancel on some
    elements, because the kernel rounds their difference once (include/laenerf.h)."""
    from laenerf_amd.raymarching.raymarching import composite_train_step_numpy
    c, t = cases[N]
    terms = ("depth", "dist", "opac", "bg_rays")
    s = t["s4"][:, :channels].contiguous()
    o = step(c, t, terms, w=t["w"], t2=s, inds=t["inds"])
    w, s2 = c["w"][c["inds"]], c["s4"][c["inds"]][:, :channels]
    ref = composite_train_step_numpy(c["sigmas"], c["rgbs"], c["deltas"], c["rays"], c["target"], T_THRESH, bg=c["bg_rays"], z=c["z"],
                                     nears=c["nears"], fars=c["fars"], depth_weight=LAMBDA_DEPTH, distort_weight=LAMBDA_DIST, scale=1.0,
                                     opacity_weight=LAMBDA_OPAC, pixel_weights=w, second_target=s2, second_weight=LAMBDA_2)
    # grad_image from the kernel's own blended image
    io, gt, bg = NP(o["io"]).astype(np.float64), c["target"].astype(np.float64), c["bg_rays"].astype(np.float64)
    w64, s64 = w.astype(np.float64)[:, None], s2.astype(np.float64)
    f32 = np.float32                                                       # the blend of the second target: the kernel's own float32 roundings
    t2 = ((s2[:, :3] * s2[:, 3:] + c["bg_rays"] * (f32(1) - s2[:, 3:])) if channels == 4 else s2).astype(np.float64)
    assert s2.dtype == np.float32 and c["bg_rays"].dtype == np.float32
    u = 1 - 0.5 * w64
    want = ((w64 * (w64 * (io - gt)) - LAMBDA_2 * (u * (u * (t2 - io)))) * (2.0 / (3 * N)))
    gi = NP(o["gi"]).astype(np.float64)
    nz = want != 0
    rel = (np.abs(gi - want)[nz] / np.abs(want)[nz]).max()
    atol = 3e-5 * max(1.0, float(np.abs(ref["grad_image"]).max()), float(np.abs(ref["grad_ws"]).max()))
    err_s = np.abs(NP(o["gs"]).astype(np.float64) - ref["grad_sigmas"]).max()
    err_c = np.abs(NP(o["gc"]).astype(np.float64) - ref["grad_rgbs"]).max()
    second = _finish(o["tpart"], 3 * N)[1].item()
    print(f"N {N}, {channels} channels: grad_image max relative error {rel:.3e}; grad_sigmas max abs error {err_s:.3e} (atol {atol:.3e}, max "
          f"{np.abs(ref['grad_sigmas']).max():.3e}); grad_rgbs max abs error {err_c:.3e} (max {np.abs(ref['grad_rgbs']).max():.3e}); loss "
          f"{o['loss'][1].item():.7e} / {float(ref['loss']):.7e}; second {second:.7e} / {float(ref['second']):.7e}")
    assert np.allclose(gi, want, rtol=1e-6, atol=0)
    assert np.allclose(NP(o["gs"]), ref["grad_sigmas"], rtol=1e-4, atol=atol)
    assert np.allclose(NP(o["gc"]), ref["grad_rgbs"], rtol=1e-5, atol=1e-6)
    assert o["loss"][1].item() == pytest.approx(float(ref["loss"]), rel=1e-5)
    assert second == pytest.approx(float(ref["second"]), rel=1e-5) and second > 1e-4
    assert torch.equal(o["loss"][0], o["loss"][1])
    assert torch.equal(_finish(o["part"], 3 * N)[1], o["loss"][1])         # every finisher yields the total


@pytest.mark.parametrize("N", [5, 67])
def test_weight_zero_removes_the_colour_exactly(cases, N):
    """rays whose weight is 0: grad_image is exactly 0 there, and their sample gradients are those of the other terms alone -- the
    call without the weight term whose target at those rays is the ray's own blended pixel (e == 0 exactly), depth and entropy on"""
    c, t = cases[N]
    terms = ("depth", "opac", "scale", "bg_rays")
    w = t["w"].clone()
    zero_planes = torch.unique(t["inds"][::2])
    w[zero_planes] = 0.0
    o = step(c, t, terms, w=w, inds=t["inds"])
    masked_index = (w[t["inds"]] == 0).nonzero().flatten()                 # by ray index: what the kernel gathers at
    assert 0 < masked_index.numel() < N
    assert not o["gi"][masked_index].any() and o["gi"][(w[t["inds"]] != 0).nonzero().flatten()].any()
    target = t["target"].clone()
    target[masked_index] = o["io"][masked_index]
    other = step(c, t, terms, entry="crit", target=target)
    assert not other["gi"][masked_index].any()
    rays = c["rays"]
    seen = 0
    for index, off, steps in rays.tolist():
        if index in masked_index.tolist() and steps:
            assert torch.equal(o["gs"][off:off + steps], other["gs"][off:off + steps]), index
            assert torch.equal(o["gc"][off:off + steps], other["gc"][off:off + steps]) and not o["gc"][off:off + steps].any()
            seen += o["gs"][off:off + steps].abs().sum().item() > 0
    assert seen >= 1                                                        # the other terms do reach those samples
    # two targets that differ at the masked rays only: every gradient output has the same bits
    noisy = t["target"].clone()
    noisy[masked_index] = torch.rand(masked_index.numel(), 3, device=DEV)
    o2 = step(c, t, terms, w=w, inds=t["inds"], target=noisy)
    _same(o, o2, keys=("gs", "gc", "gi", "gd", "gw", "ws", "io"))
    assert torch.equal(o["loss"], o2["loss"])


# ---------------------------------------------------------------------------------------------------------------- 3 determinism
def test_two_calls_and_a_captured_replay_give_the_same_bits(cases):
    c, t = cases[67]
    terms = TERMS[-1]
    a = step(c, t, terms, w=t["w"], t2=t["s4"], inds=t["inds"])
    _same(a, step(c, t, terms, w=t["w"], t2=t["s4"], inds=t["inds"]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b = step(c, t, terms, w=t["w"], t2=t["s4"], inds=t["inds"], check=False)
    for v in b.values():
        v.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    _same(a, b)


# ---------------------------------------------------------------------------------------------------------------- 4 arguments
def test_every_einval_case():
    from laenerf_amd import _lib
    check_weighted_einval(_lib.load().lae_composite_rays_train_step)


def test_backend_wrapper_and_operator(cases):
    """the Python layers hand the same call down: backend.composite_rays_train_step(weight_sup=...) and
    composite_rays_train_blend_mse(pixel_weights=..., second_target=...) against the direct call"""
    from laenerf_amd.raymarching import raymarching as rm
    c, t = cases[67]
    direct = step(c, t, ("bg_rays",), w=t["w"], t2=t["s4"], inds=t["inds"])
    rays = t["rays"].clone()
    rays.rows_end = t["rows_end"]
    sig, col = t["sigmas"].clone().requires_grad_(), t["rgbs"].clone().requires_grad_()
    loss, ws, _, image = rm.composite_rays_train_blend_mse(sig, col, t["deltas"], rays, t["nears"], t["fars"], t["target"], bg_color=t["bg_rays"],
                                                           T_thresh=T_THRESH, pixel_weights=t["w"], pixel_inds=t["inds"], second_target=t["s4"],
                                                           second_weight=LAMBDA_2)
    loss.backward()
    assert torch.equal(loss.detach(), direct["loss"][0]) and torch.equal(ws, direct["ws"]) and torch.equal(image, direct["io"])
    assert torch.equal(sig.grad, direct["gs"]) and torch.equal(col.grad, direct["gc"])
    assert torch.equal(rm.finish_second_loss(loss), _finish(direct["tpart"], 3 * 67)[1])
