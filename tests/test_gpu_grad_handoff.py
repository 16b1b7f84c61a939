"""-m gpu: the hand-off from the field backward to Adam -- the reduction of the MLP weight-gradient slabs (and the deferred loss value)
riding in the hash-grid accumulate pass (lae_nerf_field_backward), and the gradient accumulator's "dirty" word that lets that pass
skip the old values of a zeroed accumulator.  Every comparison is bit for bit."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from gpu_util import DEV, T

pytestmark = pytest.mark.gpu

SIGMA_W, COLOR_W = 64 * (32 + 64 + 16), 64 * (32 + 128 + 16)


@contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value                     # putenv: the library reads the switch with getenv at every call
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def field_case(O, M, seed=0, **grid_kw):
    """random inputs of one field backward: M samples, the head's 16 x 2 feature layout, a table of grid_kw's levels"""
    rng = np.random.default_rng(seed)
    offsets, pls = O.grid_offsets(input_dim=3, level_dim=2, align_corners=False, **grid_kw)
    L = offsets.shape[0] - 1
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = dict(M=M, L=L, S=float(np.log2(pls)), H=grid_kw.get("base_resolution", 16), n_entries=int(offsets[-1]),
             offsets_host=np.ascontiguousarray(offsets.astype(np.int32)), offsets=T(offsets.astype(np.int32)),
             x=T(rng.uniform(0, 1, (M, 3)).astype(np.float32)), dirs=T(d),
             enc=T((rng.standard_normal((16, M, 2)) * 0.1).astype(np.float16)),
             h=T((rng.standard_normal((M, 16)) * 0.1).astype(np.float16)),
             rgbs=T(rng.uniform(0.05, 0.95, (M, 3)).astype(np.float32)),
             ws=T((rng.standard_normal(SIGMA_W) * 0.1).astype(np.float16)), wc=T((rng.standard_normal(COLOR_W) * 0.1).astype(np.float16)),
             grad_sigmas=T((rng.standard_normal(M) * 1e-3).astype(np.float32)),
             grad_rgbs=T((rng.standard_normal((M, 3)) * 1e-3).astype(np.float32)),
             partials=T(rng.uniform(0, 1, 1061).astype(np.float32)), scale=T(np.array([1024.0], np.float32)),
             gws0=T((rng.standard_normal(SIGMA_W) * 1e-2).astype(np.float16)), gwc0=T((rng.standard_normal(COLOR_W) * 1e-2).astype(np.float16)))
    return c


def field_backward(c, accumulate=0, table0=None, dirty=None, grad_sigmas=None, grad_rgbs=None):
    """lae_nerf_field_backward on fresh outputs -> dict of everything it writes"""
    from laenerf_amd import _lib
    from laenerf_amd._lib import ptr
    M, L = c["M"], c["L"]
    out = dict(gws=c["gws0"].clone() if accumulate else torch.full((SIGMA_W,), 7.0, device=DEV, dtype=torch.half),
               gwc=c["gwc0"].clone() if accumulate else torch.full((COLOR_W,), 7.0, device=DEV, dtype=torch.half),
               table=torch.zeros(c["n_entries"], 2, device=DEV, dtype=torch.half) if table0 is None else table0.clone(),
               loss=torch.full((2,), float("nan"), device=DEV), wflag=torch.zeros(1, dtype=torch.int32, device=DEV),
               tflag=torch.zeros(1, dtype=torch.int32, device=DEV),
               grad_h=torch.empty(M, 16, device=DEV, dtype=torch.half), grad_enc=torch.empty(16, M, 2, device=DEV, dtype=torch.half))
    gs = c["grad_sigmas"] if grad_sigmas is None else grad_sigmas
    gr = c["grad_rgbs"] if grad_rgbs is None else grad_rgbs
    rc = _lib.load().lae_nerf_field_backward(
        ptr(gs), ptr(gr), ptr(c["enc"]), ptr(c["dirs"]), ptr(c["h"]), ptr(c["rgbs"]), ptr(c["ws"]), ptr(c["wc"]), M, 1.0,
        ptr(out["grad_h"]), ptr(out["grad_enc"]), ptr(out["gws"]), ptr(out["gwc"]), accumulate, ptr(out["wflag"]),
        ptr(c["partials"]), c["partials"].numel(), 3 * 4096, ptr(c["scale"]), ptr(out["loss"]),
        ptr(c["x"]), ptr(c["offsets"]), ptr(out["table"]), L, c["S"], c["H"], 0, 0, 0, 0.0, 1.0, c["offsets_host"].ctypes.data, None,
        ptr(out["tflag"]), None, ptr(dirty), _lib.stream())
    _lib.check(rc, "nerf_field_backward")
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.detach().cpu().numpy().view(np.uint16 if t.dtype == torch.half else np.uint32)


# bench shape: 257 792 samples, L = 16, T = 2^19 (4 000-odd partition tasks); small table: two levels = 65 partition tasks for the
# pass's 2 x CUs workgroups, so tail tasks are among the static first tickets and most workgroups start with none at all
CASES = {"bench": dict(M=257792, num_levels=16, log2_hashmap_size=19, desired_resolution=2048, base_resolution=16),
         "small": dict(M=4096, num_levels=2, log2_hashmap_size=19, desired_resolution=34, base_resolution=17)}


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", ["bench", "small"])
def test_ride_along_equals_separate_reduction(O, case, accumulate):
    """both weight gradients, the table gradient, loss_out[0..1] and the found_inf words: the same bits with the reduction riding in
    k_bwd_acc and with LAE_FIELD_NO_RIDE_ALONG=1 (k_dw_reduce2 launched on its own)"""
    kw = dict(CASES[case])
    c = field_case(O, kw.pop("M"), seed=3, **kw)
    ride = field_backward(c, accumulate)
    with env("LAE_FIELD_NO_RIDE_ALONG", "1"):
        plain = field_backward(c, accumulate)
    for k in ("gws", "gwc", "table", "loss", "wflag", "tflag", "grad_enc"):
        assert np.array_equal(bits(ride[k]), bits(plain[k])), k
    assert float(ride["gws"].float().abs().sum()) > 0 and float(ride["table"].float().abs().sum()) > 0
    assert not np.array_equal(bits(ride["gws"]), bits(torch.full((SIGMA_W,), 7.0, device=DEV, dtype=torch.half)))
    assert torch.isfinite(ride["loss"]).all() and int(ride["wflag"]) == 0 and int(ride["tflag"]) == 0
    # the loss block: the fixed-order sum k_loss_finish computes, scaled
    assert abs(float(ride["loss"][1]) - float(c["partials"].double().sum()) / (3 * 4096)) < 1e-6
    assert float(ride["loss"][0]) == float(ride["loss"][1]) * 1024.0


def test_nonfinite_gradients_are_still_reported(O):
    """a non-finite weight gradient (stored by a tail task) and a non-finite table gradient (stored by a partition task of the same
    launch) reach their found_inf words; then, end to end, Adam skips the step"""
    kw = dict(CASES["small"])
    c = field_case(O, kw.pop("M"), seed=4, **kw)
    gr = c["grad_rgbs"].clone(); gr[1234, 1] = float("inf")
    out = field_backward(c, grad_rgbs=gr)
    assert int(out["wflag"]) == 1 and not torch.isfinite(out["gwc"].float()).all()
    # a non-finite value already in the accumulator that the call adds to (test_grid_backward_reports_stored_nonfinite_values)
    table0 = torch.zeros(c["n_entries"], 2, device=DEV, dtype=torch.half); table0[: c["offsets_host"][1]] = float("inf")
    out = field_backward(c, table0=table0)
    assert int(out["tflag"]) == 1 and int(out["wflag"]) == 0 and torch.isfinite(out["gws"].float()).all()
    with env("LAE_FIELD_NO_RIDE_ALONG", "1"):
        plain = field_backward(c, table0=table0)
    assert np.array_equal(bits(out["table"]), bits(plain["table"]))

    net, opt, x, d, w = make_net()
    before = [p.detach().clone() for p in net.parameters()]
    fwd_bwd(net, opt, x, d, w, loss_factor=float("inf"))
    assert int(opt.dev_state[2].item()) == 1
    assert opt._check_tables(opt._tables())["n"] == 0          # reported by the backward: nothing left to scan
    opt.step()
    assert opt.steps_skipped == 1 and opt.steps_taken == 0
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert float(net.encoder.shadow.grad_half.float().abs().nan_to_num(1.0).sum()) == 0


# ---------------------------------------------------------------------------------------------------------- the dirty word
def make_net(seed=0, word=True):
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    torch.manual_seed(seed)
    net = NeRFNetwork(bound=1, log2_hashmap_size=15).to(DEV)
    net.encoder.embeddings.data.uniform_(-0.1, 0.1)
    net.train()
    opt = FusedAdam(net, param_groups=net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, init_scale=128.0)
    assert net.encoder.shadow.grad_dirty is not None and int(net.encoder.shadow.grad_dirty) == 1
    if not word:
        net.encoder.shadow.grad_dirty = None               # no word: every backward reads the old values, as before
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand(8192, 3, device=DEV, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(8192, 3, device=DEV, generator=g), dim=1)
    w = torch.randn(8192, 3, device=DEV, generator=g)
    net.external_grad = (torch.randn(net.encoder.shadow.grad_half.shape, device=DEV, generator=g) * 1e-2).half()
    return net, opt, x, d, w


def fwd_bwd(net, opt, x, d, w, loss_factor=1.0):
    from laenerf_amd.field import nerf_field
    with torch.autocast("cuda", dtype=torch.float16):
        s, c = nerf_field(x, d, net.encoder, net.sigma_net, net.color_net, bound=1)
    loss = ((c * w).sum() * 1e-3 + (s * w[:, 0]).sum() * 1e-4) * loss_factor
    opt.scale(loss).backward()


def state(net, opt):
    return [t.detach().clone() for t in (net.encoder.shadow.grad_half, net.sigma_net.shadow.grad_half, net.color_net.shadow.grad_half,
                                         net.encoder.embeddings, net.sigma_net.weights, net.color_net.weights, opt.dev_state[:9])]


def same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def external(net):
    """someone else writes the accumulator, then says so the documented way"""
    sh = net.encoder.shadow
    sh.grad_half.copy_(net.external_grad)
    sh.unreported = True
    sh.mark_all_touched()


def seq_step_between(net, opt, a):                        # backward -> step -> backward
    fwd_bwd(net, opt, *a); opt.step(); fwd_bwd(net, opt, *a)


def seq_accumulate(net, opt, a):                          # backward -> backward -> step
    fwd_bwd(net, opt, *a); fwd_bwd(net, opt, *a); opt.step()


def seq_external(net, opt, a):                            # backward -> step -> external write + mark -> backward
    fwd_bwd(net, opt, *a); opt.step(); external(net); fwd_bwd(net, opt, *a)


SEQS = [seq_step_between, seq_accumulate, seq_external]


def test_dirty_word_sequences_equal_the_run_without_it():
    def word_of(net):
        return int(net.encoder.shadow.grad_dirty)
    finals = {}
    for word in (True, False):
        # backward -> step -> backward
        net, opt, *a = make_net(word=word)
        fwd_bwd(net, opt, *a)
        one = state(net, opt)
        assert not word or word_of(net) == 1
        opt.step()
        assert not word or word_of(net) == 0               # the apply kernel has zeroed the accumulator
        assert float(net.encoder.shadow.grad_half.float().abs().sum()) == 0
        fwd_bwd(net, opt, *a)
        assert not word or word_of(net) == 1
        finals[("step_between", word)] = state(net, opt)
        # backward -> backward -> step: the second backward accumulates on top, so it must read the old values
        net, opt, *a = make_net(word=word)
        fwd_bwd(net, opt, *a); fwd_bwd(net, opt, *a)
        two = state(net, opt)
        assert same(state(net, opt)[3:], one[3:]) and not torch.equal(two[0], one[0])
        assert torch.allclose(two[0].float(), 2 * one[0].float(), rtol=2e-3, atol=1e-6)
        opt.step()
        finals[("accumulate", word)] = [two[0]] + state(net, opt)
        # an external write followed by the documented mark, then backward: on top of what was written
        net, opt, *a = make_net(word=word)
        fwd_bwd(net, opt, *a); opt.step()
        external(net)
        ext = net.encoder.shadow.grad_half.clone()
        assert not word or word_of(net) == 1
        fwd_bwd(net, opt, *a)
        got = net.encoder.shadow.grad_half
        assert not torch.equal(got, ext)
        untouched = (finals[("step_between", word)][0].float().abs().sum(dim=1) == 0)
        assert torch.equal(got[untouched], ext[untouched])  # entries this batch does not reach keep the external values
        finals[("external", word)] = state(net, opt)
        # zero_grad(): the next backward overwrites
        net, opt, *a = make_net(word=word)
        fwd_bwd(net, opt, *a)
        opt.zero_grad()
        assert not word or word_of(net) == 0
        fwd_bwd(net, opt, *a)
        assert same(state(net, opt), one)
    for k in ("step_between", "accumulate", "external"):
        assert same(finals[(k, True)], finals[(k, False)]), k


@pytest.mark.parametrize("seq", SEQS, ids=lambda f: f.__name__)
def test_dirty_word_in_a_captured_graph(seq):
    """the sequence captured in ONE graph and replayed three times = the same sequence run eagerly three times: the word lives on
    the device, so a replay carries it from launch to launch"""
    net, opt, *a = make_net()
    for _ in range(4):                                     # one warm-up pass + three more, eagerly
        seq(net, opt, a)
    want = state(net, opt)

    net, opt, *a = make_net()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seq(net, opt, a)                                   # warm-up: workspaces, autograd's buffers
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seq(net, opt, a)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert same(state(net, opt), want)


def test_generic_atomic_backward_leaves_the_word_set(O):
    from laenerf_amd.backend import gridencoder_backend as G
    kw = dict(CASES["small"])
    c = field_case(O, kw.pop("M"), seed=6, **kw)
    M, L = c["M"], c["L"]
    grad = c["enc"][:L].contiguous()
    table_h = torch.zeros(c["n_entries"], 2, device=DEV, dtype=torch.half)

    def run(ge, dirty):
        G.grid_encode_backward(grad, c["x"], table_h, c["offsets"], ge, M, 3, 2, L, c["S"], c["H"], None, None, 0, False, 0,
                               offsets_host=c["offsets_host"], grad_dirty=dirty.data_ptr())
    dirty = torch.zeros(1, dtype=torch.int32, device=DEV)
    G.set_backward_mode(1)
    try:
        ge = torch.zeros(c["n_entries"], 2, device=DEV, dtype=torch.half)
        run(ge, dirty)
        assert int(dirty) == 1 and float(ge.float().abs().sum()) > 0
    finally:
        G.set_backward_mode(0)
    # the binned pass after it: the word says "written", so it adds on top; with a cleared word it would start from zero
    once = torch.zeros(c["n_entries"], 2, device=DEV, dtype=torch.half)
    clean = torch.zeros(1, dtype=torch.int32, device=DEV)
    run(once, clean)
    assert int(clean) == 1
    before = ge.clone()
    run(ge, dirty)
    hit = once.float().abs().sum(dim=1) > 0
    assert hit.any() and not torch.equal(ge[hit], once[hit]) and torch.equal(ge[~hit], before[~hit])
    assert torch.allclose(ge.float(), before.float() + once.float(), rtol=2e-3, atol=1e-4)
