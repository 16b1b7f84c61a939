"""-m gpu: the kernels of csrc/optimizer.hip through the C ABI, against the restatements of tests/optim_util.py (pinned on the CPU by
tests/test_optim_cpu.py): an exact first step bit for bit at every size that takes another path (4-wide body, scalar tail, second and
third trip of the capped grid-stride loop), the general step within a counted number of roundings of float64, the touched-lines
contract with poisoned untouched lines, the non-finite scan at its bit-pattern and position edges, k_begin over 40 steps against the
GradScaler rules, and the two EMA launches.  Every buffer a launch may write is poisoned first and carries guard elements behind
its end; S = sweep(4) (sweep(8) for the scan) is what one pass of a capped launch covers.

Worst measured error / bound on one MI355X (printed by the tests; the bounds are optim_util.step_ratios / ema_ratio):
    general step (n = 4099 and S + 1027, fp16 / fp32 gradients, steps 1 .. 10^7), weight_decay 0:     p' 0.692   m' 0.135   v' 0.198
    the same with weight_decay 0.01:                                                                 p' 0.698   m' 0.144   v' 0.197
    eight tensors with eight learning rates:                                                         p' 0.681   m' 0.120   v' 0.184
    FusedAdam, three groups, weight_decay 0.01, first step:                                          p' 0.245   m' 0.026   v' 0.004
    touched lines (n = 1129 and S + 53):                                                             p' 0.692   m' 0.135   v' 0.197
    EMA update:                                                                                      0.998
The p' figure is the final rounding of p' alone on an element whose update is small: half an ulp of p in [0.09, 0.11] is up to 0.694
of 2^-24 |p'| (general_inputs says why p is kept there).  On the error of u = p' - p itself, the kernel's statement order in numpy
float32 (optim_util.adam1_f32, on the CPU) uses 12.5 of the bound's 32 half-ulps of u without weight decay and 20.2 with it where
|u| > 1e-4; where m' cancels the error of u is not relative to u at all (millions of half-ulps of a tiny u) and the first term
takes it.  The EMA figure is likewise the final rounding where shadow and
parameter nearly agree, just above a power of two; the bound's second term covers the two roundings before it in full.
One of the breaks these tests were tried against changes no result: `n4 = n & ~7` in ema_segs only moves up to four more elements
from the 4-wide loop to the scalar tail, which handles up to 256 per tensor with the same arithmetic.
"""
import functools

import numpy as np
import pytest
import torch

import optim_util as OU
from gpu_util import DEV

pytestmark = pytest.mark.gpu

PAD = 32                                   # guard elements behind every buffer
NAN = np.float32("nan")
GRAD_SENTINEL = 3.0                        # a gradient nobody may read or zero
SHADOW_SENTINEL = np.int16(0x5555)         # fp16 bits of a shadow entry nobody may write
HYPER = dict(beta1=0.9, beta2=0.99, eps=1e-15)
STEPS0 = [0, 9, 999, 99999, 10 ** 7 - 1]   # preset step counts: the step taken is one more
SIZES = {"1": lambda S: 1, "2": lambda S: 2, "3": lambda S: 3, "4": lambda S: 4, "5": lambda S: 5, "7": lambda S: 7, "9": lambda S: 9,
         "1023": lambda S: 1023, "1025": lambda S: 1025, "S": lambda S: S, "S+1": lambda S: S + 1, "2S+5": lambda S: 2 * S + 5}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = host(a) if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} differ, first at {bad[0]}: got {g[bad[0]]:#x}, want {w[bad[0]]:#x}"


def padded(a, guard):
    """device copy of `a` followed by PAD guard elements"""
    return dev(np.concatenate([np.ascontiguousarray(a), np.full(PAD, guard, a.dtype)]))


class Seg:
    """one parameter tensor's buffers, each n elements + guards: p, m, v fp32, g fp16 / fp32, shadow fp16 (poisoned with NaN) or None"""

    def __init__(self, p, m, v, g, shadow=True):
        self.n = len(p)
        if shadow is True:
            shadow = np.full(self.n, np.float16("nan"))
        host_side = {"p": (np.asarray(p, np.float32), NAN), "m": (np.asarray(m, np.float32), NAN), "v": (np.asarray(v, np.float32), NAN),
                     "g": (g, g.dtype.type(GRAD_SENTINEL))}
        if shadow is not None:
            host_side["shadow"] = (shadow.view(np.int16), SHADOW_SENTINEL)
        self.before, self.last = {}, None
        for name, (a, guard) in host_side.items():
            full = np.concatenate([np.ascontiguousarray(a), np.full(PAD, guard, a.dtype)])
            t = dev(full)
            if name == "shadow":
                t, full = t.view(torch.float16), full.view(np.float16)
            setattr(self, name, t)
            self.before[name], self.before["guard_" + name] = full[:self.n], full[self.n:]
        if shadow is None:
            self.shadow = None

    def read(self):
        """-> the n elements of every buffer; the guard elements behind them must be untouched"""
        out = {}
        for name in ("p", "m", "v", "g", "shadow"):
            t = getattr(self, name)
            if t is None:
                continue
            a = host(t)
            assert_bits(a[self.n:], self.before["guard_" + name], f"guard elements behind {name}")
            out[name] = a[:self.n]
        self.last = out
        return out


def run_apply(entry, segs, st, lrs, hyper, weight_decay=0.0, touched=None, dirty=None):
    """entry "single": lae_adam_apply per tensor; "multi": one lae_adam_apply_multi.  lrs: device fp32 tensor, one word per tensor"""
    lr_at = [lrs.data_ptr() + 4 * i for i in range(len(segs))]
    if entry == "single":
        assert touched is None and dirty is None
        for s, lr in zip(segs, lr_at):
            assert OU.apply(s.p, s.m, s.v, s.g, s.shadow, st, lr, hyper["beta1"], hyper["beta2"], hyper["eps"], weight_decay, n=s.n) == 0
    else:
        assert OU.apply_multi([s.p for s in segs], [s.m for s in segs], [s.v for s in segs], [s.g for s in segs], [s.shadow for s in segs], st,
                              lr_at, hyper["beta1"], hyper["beta2"], hyper["eps"], weight_decay, touched=touched, dirty=dirty,
                              sizes=[s.n for s in segs]) == 0
    torch.cuda.synchronize()


def begun_state(hyper, scale, step0=0, found_inf=0):
    st = OU.new_state(scale=scale, step=step0, found_inf=found_inf)
    assert OU.begin(st, hyper["beta1"], hyper["beta2"]) == 0
    return st


# ------------------------------------------------------------------ 1. exact first step
def exact_state():
    E = OU.EXACT
    st = begun_state(E, E["scale"])
    d, _ = OU.read_state(st)
    assert (d["skip"], d["step"], d["inv_bc1"], d["bc2_sqrt"], d["inv_scale"]) == (0, 1, 2.0, 0.5, 2.0 ** -7)
    return st


def check_exact(c, seg, what, keep=None):
    o = seg.read()
    k = slice(None) if keep is None else keep
    for name, want in (("p", c["p1"]), ("m", c["m1"]), ("v", c["v1"]), ("shadow", c["shadow1"])):
        assert_bits(o[name][k], want[k], f"{what}: {name}")
    assert_bits(o["g"], np.zeros_like(c["g"]), f"{what}: gradient zeroed")
    return o


@pytest.mark.parametrize("grad", ["half", "float"])
@pytest.mark.parametrize("size", list(SIZES))
def test_exact_first_step_bit_for_bit(size, grad):
    """p' = p - lr sign(g), m' = g / (2 scale), v' = (g / scale)^2 / 4, shadow = half(p'), grad = 0: every intermediate exact"""
    n = SIZES[size](OU.sweep(4))
    c = OU.exact_case(n, grad == "half")
    z = np.zeros(n, np.float32)
    lrs = dev(np.array([OU.EXACT["lr"]], np.float32))
    outs = []
    for entry in ("single", "multi"):
        seg = Seg(c["p"], z, z, c["g"])
        run_apply(entry, [seg], exact_state(), lrs, OU.EXACT)
        outs.append(check_exact(c, seg, f"{entry} n={n}"))
    for name in ("p", "m", "v", "shadow", "g"):
        assert_bits(outs[0][name], outs[1][name], f"lae_adam_apply against lae_adam_apply_multi: {name}")


def test_exact_first_step_with_weight_decay():
    """weight_decay 2^-3: p' = p - lr sign(g / scale + wd p); the sign is not sign(g) on more than a third of the elements"""
    n, E = 4099, OU.EXACT
    c = OU.exact_case(n, False, weight_decay=True)
    k = c["keep"]
    assert (np.sign(c["u"]) != c["sign_g"])[k].mean() > 1 / 3 and (~k).sum() < 8
    z = np.zeros(n, np.float32)
    lrs = dev(np.array([E["lr"]], np.float32))
    for entry in ("single", "multi"):
        seg = Seg(c["p"], z, z, c["g"])
        run_apply(entry, [seg], exact_state(), lrs, E, weight_decay=E["weight_decay"])
        check_exact(c, seg, f"weight decay, {entry}", keep=k)


@pytest.mark.parametrize("grad", ["half", "float"])
def test_zero_gradient_keeps_the_parameter_bits(grad):
    """g = 0, m = v = 0, eps = 1e-15: 0 / eps = 0 and p - lr * 0 keeps every bit of p, the sign of -0.0 included"""
    p = np.array([-0.0, 0.0, 1.5, -2.25, 1e-40, -1e-40, 0.1, -1024.0, 3.0e-5], np.float32)
    z = np.zeros(len(p), np.float32)
    lrs = dev(np.array([1e-2], np.float32))
    for entry in ("single", "multi"):
        seg = Seg(p, z, z, np.zeros(len(p), np.float16 if grad == "half" else np.float32))
        run_apply(entry, [seg], begun_state(HYPER, 1024.0), lrs, HYPER)
        o = seg.read()
        for name, want in (("p", p), ("m", z), ("v", z), ("shadow", p.astype(np.float16)), ("g", seg.before["g"])):
            assert_bits(o[name], want, name)


# ------------------------------------------------------------------ 2. general step against float64
@functools.lru_cache(maxsize=4)
def general_inputs(n, grad_half, seed=0):
    """p around 0.1, m around 1e-3, v around 1e-6, the gradient around 1e-3 times the loss scale 1024.
    The p' bound of optim_util.step_ratios needs two things of the inputs, both about elements whose m' cancels (u small, so the
    bound is its first term 2^-24 |p'| alone).  (1) p in [0.09, 0.11]: half an ulp there is 2^-28, at most 0.70 of 2^-24 |p'|, so
    the final rounding leaves 0.30 * 0.09 * 2^-24 = 0.027 * 2^-24 of slack (just above 0.125 it would leave none).  (2) the error
    of u that is not relative to u stays below that: m' = 0 means g = -9 m, the roundings of g - m, of the product and (with
    weight decay, |wd p| <= 1.1e-3) of g itself put at most 0.2 * 2^-24 * (9.9 |m| + 2.2e-3) into m'; v' >= max(0.99e-6, 0.81 m^2)
    gives |m| / denom <= 1.1 bc2 and 2.2e-3 / denom <= 2.2 bc2 (bc2 = sqrt(1 - beta2^step), lr bc2 / bc1 <= 1.0 lr for these betas),
    so u is off by at most lr * 0.2 * (10.9 + 2.2) * 2^-24 = 2.6 lr * 2^-24: 0.008 * 2^-24 at LR = 3e-3."""
    rng = np.random.default_rng([n, int(grad_half), seed])
    p = (0.1 + 0.01 * (2.0 * rng.random(n) - 1.0)).astype(np.float32)
    m = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-6 * (1.0 + rng.random(n))).astype(np.float32)
    g = (1e-3 * 1024.0 * rng.standard_normal(n)).astype(np.float16 if grad_half else np.float32)
    for a in (p, m, v, g):
        a.setflags(write=False)
    return p, m, v, g


LR = 3e-3
SCALE = 1024.0


def reference_step(p, m, v, g, lr, weight_decay, step, hyper=HYPER):
    inv = np.float32(1.0 / SCALE)
    return (OU.adam_step_f64(p, m, v, g, lr, hyper["beta1"], hyper["beta2"], hyper["eps"], weight_decay, step, inv),
            OU.grad_magnitude_f64(p, g, weight_decay, inv))


def seg_ratios(seg, ref, g_mag, sel=None):
    """-> step_ratios of the segment's buffers (on the selected elements); also the shadow is half(p') of the p' the kernel wrote"""
    o = seg.read()
    s = slice(None) if sel is None else sel
    if seg.shadow is not None:
        assert_bits(o["shadow"][s], o["p"][s].astype(np.float16), "shadow = half(p')")
    b = seg.before
    return OU.step_ratios(o["p"][s], o["m"][s], o["v"][s], b["p"][s], b["m"][s], b["v"][s], g_mag[s], tuple(r[s] for r in ref))


@pytest.mark.parametrize("step0", STEPS0)
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("grad", ["half", "float"])
@pytest.mark.parametrize("size", ["4099", "S+1027"])
def test_general_step_against_float64(size, grad, weight_decay, step0):
    n = 4099 if size == "4099" else OU.sweep(4) + 4 * 256 + 3
    p, m, v, g = general_inputs(n, grad == "half")
    lr = LR
    ref, g_mag = reference_step(p, m, v, g, lr, weight_decay, step0 + 1)
    lrs = dev(np.array([lr], np.float32))
    for entry in ("single", "multi"):
        st = begun_state(HYPER, SCALE, step0)
        assert OU.read_state(st)[0]["step"] == step0 + 1
        seg = Seg(p, m, v, g, shadow=None if (entry == "single" and grad == "float") else True)      # a NULL shadow through lae_adam_apply too
        run_apply(entry, [seg], st, lrs, HYPER, weight_decay=weight_decay)
        r = seg_ratios(seg, ref, g_mag)
        print(f"general step n={n} grad={grad} wd={weight_decay} step={step0 + 1} {entry}: p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f} of the bound")
        assert max(r) <= 1.0, r
        assert_bits(seg.last["g"], np.zeros_like(g), "gradient zeroed")


def test_every_tensor_of_a_multi_call_reads_its_own_learning_rate():
    """eight tensors, eight learning-rate words: each matches the restatement with its own rate and with no neighbour's"""
    sizes = [1029, 0, 77, 4100, 5, 2051, 16, 333]
    halves = [True, False, False, True, True, False, True, False]
    shadows = [True, None, None, True, None, True, True, None]
    lr = [LR / 1.5 ** i for i in range(8)]
    lrs = dev(np.array(lr, np.float32))
    step0 = 9
    segs, inputs = [], []
    for i, (n, h, sh) in enumerate(zip(sizes, halves, shadows)):
        p, m, v, g = general_inputs(n, h, seed=100 + i)
        inputs.append((p, m, v, g))
        segs.append(Seg(p, m, v, g, shadow=sh))
    run_apply("multi", segs, begun_state(HYPER, SCALE, step0), lrs, HYPER)
    for i, (seg, (p, m, v, g)) in enumerate(zip(segs, inputs)):
        if seg.n == 0:
            seg.read()
            continue
        r = seg_ratios(seg, *reference_step(p, m, v, g, float(np.float32(lr[i])), 0.0, step0 + 1))
        print(f"tensor {i} (n={seg.n}): p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f} of the bound")
        assert max(r) <= 1.0, (i, r)
        for j in (i - 1, i + 1):
            if 0 <= j < 8:
                wrong = seg_ratios(seg, *reference_step(p, m, v, g, float(np.float32(lr[j])), 0.0, step0 + 1))
                assert wrong[0] > 1000.0, (i, j, wrong)
        assert_bits(seg.last["g"], np.zeros_like(g), "gradient zeroed")


def test_fused_adam_groups_have_their_own_rate_and_weight_decay():
    """FusedAdam(param_groups=...) with a rate per group and weight_decay 0.01: one step against the restatement, group by group; with
    weight decay no table gets a touched-lines bitmap"""
    from laenerf_amd.network import NeRFNetwork
    from laenerf_amd.optim import FusedAdam
    torch.manual_seed(7)
    net = NeRFNetwork(bound=1, log2_hashmap_size=12).to(DEV)
    net.encoder.embeddings.data.uniform_(-0.1, 0.1)
    groups = net.get_params(1e-2)
    for i, grp in enumerate(groups):
        grp["lr"] = 1e-2 * (i + 1)
    opt = FusedAdam(net, param_groups=groups, betas=(0.9, 0.99), eps=1e-15, weight_decay=0.01, init_scale=SCALE)
    assert net.encoder.shadow is not None and net.encoder.shadow.touched_lines is None
    assert len({gi for *_, gi in opt.items}) == len(opt.items) == 3
    rng = np.random.default_rng(21)
    before = []
    for p, m, v, shadow, gi in opt.items:
        g = (1e-3 * SCALE * rng.standard_normal(p.numel())).astype(np.float16)
        assert shadow is not None
        shadow.grad_half.copy_(dev(g).view_as(shadow.grad_half))
        shadow.unreported = True                         # written behind the operators' back: the optimizer scans it
        before.append((host(p).reshape(-1).copy(), g, gi))
    opt.step()
    torch.cuda.synchronize()
    assert opt.steps_taken == 1 and opt.steps_skipped == 0
    for (p, m, v, shadow, gi), (p0, g, _) in zip(opt.items, before):
        z = np.zeros_like(p0)
        got = (host(p).reshape(-1), host(m).reshape(-1), host(v).reshape(-1))
        ref, g_mag = reference_step(p0, z, z, g, 1e-2 * (gi + 1), 0.01, 1)
        r = OU.step_ratios(*got, p0, z, z, g_mag, ref)
        print(f"FusedAdam group {gi} (n={p0.size}): p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f} of the bound")
        assert max(r) <= 1.0, (gi, r)
        for other in {0, 1, 3} - {gi}:
            wrong, _ = reference_step(p0, z, z, g, 1e-2 * (other + 1), 0.01, 1)
            assert OU.step_ratios(*got, p0, z, z, g_mag, wrong)[0] > 1000.0, (gi, other)
        assert_bits(shadow.half.reshape(-1), got[0].astype(np.float16), "shadow table")
        assert float(shadow.grad_half.float().abs().sum()) == 0


# ------------------------------------------------------------------ 3. touched lines
def bitmap_words(lines):
    """bool per 16-parameter line -> the int32 words lae_adam_apply_multi reads (bit l & 31 of word l >> 5)"""
    w = np.zeros((len(lines) + 31) // 32, np.uint32)
    for l in np.flatnonzero(lines):
        w[l >> 5] |= np.uint32(1) << np.uint32(l & 31)
    return w.view(np.int32)


def touched_lines(n, variant):
    n_lines = (n + 15) // 16
    t = np.random.default_rng(5).random(n_lines) < 0.5
    t[[0, 31, 33, n_lines - 1]] = True
    t[[1, 32]] = False
    return t if variant == "a" else ~t


def touched_inputs(n, grad_half, lines, finite_fill):
    """general inputs; on untouched lines (unless finite_fill) NaN in p / m / v, the sentinels in the gradient and in the shadow"""
    p, m, v, g = (a.copy() for a in general_inputs(n, grad_half, seed=9))
    on = lines[np.arange(n) >> 4]
    shadow = np.full(n, np.float16("nan")).view(np.uint16)
    if not finite_fill:
        p[~on] = m[~on] = v[~on] = NAN
        g[~on] = GRAD_SENTINEL
        shadow[~on] = np.uint16(SHADOW_SENTINEL)
    return p, m, v, g, shadow.view(np.float16), on


@pytest.mark.parametrize("mode", ["step", "skip", "weight_decay"])
@pytest.mark.parametrize("grad", ["half", "float"])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_touched_lines_contract(variant, grad, mode):
    """n = 16 * 70 + 9: a partial last line, three bitmap words, both values at lines 31, 32, 33 and at the last line over the two
    variants.  A line whose bit is clear is neither read nor written (not even its gradient is zeroed); with weight decay the bitmap
    is ignored; a skipped step zeroes the gradient of the touched lines only; the dirty word is cleared, step or skip"""
    n = 16 * 70 + 9
    lines = touched_lines(n, variant)
    assert len(bitmap_words(lines)) == 3 and lines[31] != lines[32] and lines[33] != lines[32] and lines[-1] == (variant == "a")
    wd = 0.01 if mode == "weight_decay" else 0.0
    p, m, v, g, shadow, on = touched_inputs(n, grad == "half", lines, finite_fill=(mode == "weight_decay"))
    seg = Seg(p, m, v, g, shadow=shadow)
    p2, m2, v2, g2 = general_inputs(37, True, seed=10)
    other = Seg(p2, m2, v2, g2, shadow=None)                        # a second tensor with NULL bitmap and NULL dirty entries
    bitmap = dev(bitmap_words(lines))
    dirty = dev(np.array([1, 7, 7, 7], np.int32))
    lrs = dev(np.array([LR, 2e-3], np.float32))
    step0 = 9
    st = begun_state(HYPER, SCALE, step0, found_inf=int(mode == "skip"))
    d, _ = OU.read_state(st)
    assert d["skip"] == int(mode == "skip") and d["step"] == step0 + (mode != "skip")
    run_apply("multi", [seg, other], st, lrs, HYPER, weight_decay=wd, touched=[bitmap, None], dirty=[dirty.data_ptr(), None])
    assert host(dirty).tolist() == [0, 7, 7, 7]
    assert_bits(bitmap, bitmap_words(lines), "the bitmap is read only")
    o, b = seg.read(), seg.before
    upd = np.ones(n, bool) if mode == "weight_decay" else on          # the elements the launch works on
    for name in ("p", "m", "v", "g", "shadow"):
        assert_bits(o[name][~upd], b[name][~upd], f"untouched lines: {name}")
    assert_bits(o["g"][upd], np.zeros(int(upd.sum()), g.dtype), "gradient of the touched lines zeroed")
    oo = other.read()
    assert_bits(oo["g"], np.zeros_like(g2), "second tensor: gradient zeroed")
    if mode == "skip":
        for name in ("p", "m", "v", "shadow"):
            assert_bits(o[name], b[name], f"skipped step: {name}")
        for name in ("p", "m", "v"):
            assert_bits(oo[name], other.before[name], f"skipped step, second tensor: {name}")
        return
    assert (~upd).sum() > 16 * 20 or mode == "weight_decay"
    r = seg_ratios(seg, *reference_step(p, m, v, g, LR, wd, step0 + 1), sel=upd)
    r2 = seg_ratios(other, *reference_step(p2, m2, v2, g2, 2e-3, wd, step0 + 1))
    print(f"touched lines {variant} {grad} {mode}: p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f} of the bound")
    assert max(r) <= 1.0 and max(r2) <= 1.0, (r, r2)


def test_touched_lines_past_one_sweep():
    """n = S + 16 * 3 + 5 with every other line touched: the second trip of the loop looks its line up too"""
    n = OU.sweep(4) + 16 * 3 + 5
    lines = np.arange((n + 15) // 16) % 2 == 0
    p, m, v, g, shadow, on = touched_inputs(n, True, lines, finite_fill=False)
    seg = Seg(p, m, v, g, shadow=shadow)
    words = np.full((len(lines) + 31) // 32, 0x55555555, np.int32)
    assert np.array_equal(words, bitmap_words(np.arange(len(words) * 32) % 2 == 0))
    step0 = 9
    run_apply("multi", [seg], begun_state(HYPER, SCALE, step0), dev(np.array([LR], np.float32)), HYPER, touched=[dev(words)])
    o, b = seg.read(), seg.before
    for name in ("p", "m", "v", "g", "shadow"):
        assert_bits(o[name][~on], b[name][~on], f"untouched lines: {name}")
    assert_bits(o["g"][on], np.zeros(int(on.sum()), np.float16), "gradient of the touched lines zeroed")
    r = seg_ratios(seg, *reference_step(p, m, v, g, LR, 0.0, step0 + 1), sel=on)
    print(f"touched lines n={n}: p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f} of the bound")
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------ 4. the non-finite scan
HALF_BAD = [0x7c00, 0xfc00, 0x7e00, 0x7c01, 0xfdff]                 # +inf, -inf, a quiet NaN, a NaN with only the lowest mantissa bit, -NaN
FLOAT_BAD = [np.float32("inf"), np.float32("-inf"), np.float32("nan")]
STATE_POISON = np.array([1000 * i + 5 for i in range(16)], np.int32)


def poisoned_state(found_inf=0):
    w = STATE_POISON.copy()
    w[2] = found_inf
    return dev(w)


def found_inf_of(st, before_found_inf=0):
    """word 2 after a scan; every other word must be what it was"""
    w = host(st)
    want = STATE_POISON.copy()
    want[2] = w[2]
    assert np.array_equal(w, want), "the scan wrote a state word other than found_inf"
    return int(w[2])


def clean_buffer(n, half, guard_bad=True):
    """finite values of every magnitude, the largest finite ones included; the guard elements behind n are +inf (a scan that reads
    past n reports them)"""
    if half:
        pat = np.array([0x7bff, 0xfbff, 0x0001, 0x8000, 0x0000, 0x3c00, 0x7800, 0x03ff], np.uint16).view(np.float16)      # +-65504, subnormals, -0
    else:
        pat = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 1e-45, -1e-40, 0.0, 1.0, 2.0 ** 127, -0.0], np.float32)
    a = np.resize(np.roll(pat, 3), n)
    return padded(a, a.dtype.type("inf") if guard_bad else a.dtype.type(1))


def poke(buf, pos, value, half):
    """write one element by its bit pattern (fp16) or value (fp32); -> the old element"""
    view = buf.view(torch.int16) if half else buf
    old = view[pos].clone()
    view[pos] = int(np.array(value, np.uint16).view(np.int16)) if half else float(value)
    return old


def scan(entry, buf, n, st):
    if entry == "single":
        return OU.check(buf, st, n=n)
    a, b = dev(np.ones(100, np.float32)), dev(np.ones(37, np.float16))
    return OU.check_multi([a, buf, b], st, sizes=[100, n, 37])


@pytest.mark.parametrize("half", [True, False], ids=["half", "float"])
@pytest.mark.parametrize("entry", ["single", "multi"])
def test_scan_finds_one_bad_element_at_every_edge(entry, half):
    for n in (4096, 4099):                                          # n % 8 = 0 and 3: the 8-wide body alone, and body + tail
        buf = clean_buffer(n, half)
        st = poisoned_state()
        assert scan(entry, buf, n, st) == 0 and found_inf_of(st) == 0, "clean buffer"
        for pos in (0, 1, 7, 8, n - 1):
            for value in (HALF_BAD if half else FLOAT_BAD):
                old = poke(buf, pos, value, half)
                st = poisoned_state()
                assert scan(entry, buf, n, st) == 0
                assert found_inf_of(st) == 1, (n, pos, value)
                (buf.view(torch.int16) if half else buf)[pos] = old
        st = poisoned_state()
        assert scan(entry, buf, n, st) == 0 and found_inf_of(st) == 0, "the buffer is clean again"


@pytest.mark.parametrize("half", [True, False], ids=["half", "float"])
@pytest.mark.parametrize("entry", ["single", "multi"])
def test_scan_past_one_sweep(entry, half):
    """+inf at S8 - 1, S8 and S8 + 1, S8 = sweep(8): the last element of the first trip and the first ones of the second"""
    S8 = OU.sweep(8)
    for n in (S8 + 8, S8 + 11):
        buf = torch.ones(n + PAD, dtype=torch.float16 if half else torch.float32, device=DEV)
        buf[n:] = float("inf")
        st = poisoned_state()
        assert scan(entry, buf, n, st) == 0 and found_inf_of(st) == 0, "clean buffer"
        for pos in (S8 - 1, S8, S8 + 1):
            buf[pos] = float("inf")
            st = poisoned_state()
            assert scan(entry, buf, n, st) == 0
            assert found_inf_of(st) == 1, (n, pos)
            buf[pos] = 1.0


@pytest.mark.parametrize("half", [True, False], ids=["half", "float"])
def test_scan_reaches_the_last_element_of_the_eighth_tensor(half):
    sizes = [64, 5, 1027, 8, 2056, 1, 16, 4099]
    halves = [True, False, False, True, True, False, True, half]
    bufs = [clean_buffer(n, h) for n, h in zip(sizes, halves)]
    st = poisoned_state()
    assert OU.check_multi(bufs, st, sizes=sizes) == 0 and found_inf_of(st) == 0
    poke(bufs[7], sizes[7] - 1, 0x7c01 if half else np.float32("nan"), half)
    assert OU.check_multi(bufs, st, sizes=sizes) == 0 and found_inf_of(st) == 1


@pytest.mark.parametrize("half", [True, False], ids=["half", "float"])
@pytest.mark.parametrize("entry", ["single", "multi"])
def test_scan_leaves_finite_extremes_and_a_set_word_alone(entry, half):
    """+-65504, the smallest subnormal, -0 (fp16); +-FLT_MAX and subnormals (fp32): found_inf stays 0; a word already 1 stays 1"""
    for n in (8, 11, 4099):
        buf = clean_buffer(n, half)
        st = poisoned_state()
        assert scan(entry, buf, n, st) == 0 and found_inf_of(st) == 0, n
        st = poisoned_state(found_inf=1)
        assert scan(entry, buf, n, st) == 0 and found_inf_of(st) == 1, n


def test_return_codes_and_nothing_written():
    st = poisoned_state()
    f = [dev(np.ones(16, np.float32)) for _ in range(9)]
    h = dev(np.ones(16, np.float16))
    off = f[0].data_ptr() + 4                                       # 4 bytes off a 16-byte boundary
    lr = dev(np.array([1e-2], np.float32))
    hy = (0.9, 0.99, 1e-15, 0.0)
    count, step = dev(np.zeros(2, np.int32)), dev(np.array([4], np.int64))
    # the scan
    assert OU.check_multi(f, st) == OU.EINVAL                       # nine tensors
    assert OU.check_multi([off], st, sizes=[8], is_half=[0]) == OU.EINVAL
    assert OU.check(off, st, n=8, is_half=0) == OU.EINVAL
    assert OU.check_multi([h, None], st, sizes=[16, 8], is_half=[1, 0]) == OU.ENULL
    assert OU.check(None, st, n=8, is_half=0) == OU.ENULL
    # apply
    nine = [f[0]] * 9
    assert OU.apply_multi(nine, nine, nine, nine, [None] * 9, st, [lr] * 9, *hy) == OU.EINVAL
    assert OU.apply_multi([off], [f[1]], [f[2]], [f[3]], [None], st, [lr], *hy, sizes=[8]) == OU.EINVAL
    assert OU.apply_multi([f[0]], [f[1]], [f[2]], [f[3]], [h.data_ptr() + 4], st, [lr], *hy, sizes=[8]) == OU.EINVAL
    assert OU.apply_multi([f[0]], [f[1]], [f[2]], [None], [None], st, [lr], *hy, sizes=[8]) == OU.ENULL
    assert OU.apply(off, f[1], f[2], f[3], None, st, lr, *hy, n=8, is_half=0) == OU.EINVAL
    assert OU.apply(f[0], f[1], f[2], None, None, st, lr, *hy, n=8, is_half=0) == OU.ENULL
    # EMA
    assert OU.ema_multi(f, f, 0.5) == OU.EINVAL
    assert OU.ema_multi([off], [f[1]], 0.5, sizes=[8]) == OU.EINVAL
    assert OU.ema_multi([f[0]], [None], 0.5, sizes=[8]) == OU.ENULL
    assert OU.ema_gated(f, f, step, 4, count, 0.95, 1) == OU.EINVAL
    assert OU.ema_gated([f[0]], [off], step, 4, count, 0.95, 1, sizes=[8]) == OU.EINVAL
    assert OU.ema_gated([None], [f[1]], step, 4, count, 0.95, 1, sizes=[8]) == OU.ENULL
    assert OU.ema_gated([f[0]], [f[1]], step, 0, count, 0.95, 1) == OU.EINVAL            # epoch_len < 1
    torch.cuda.synchronize()
    assert found_inf_of(st) == 0 and host(count).tolist() == [0, 0]
    assert all(np.array_equal(host(t), np.ones(16, np.float32)) for t in f) and np.array_equal(host(h), np.ones(16, np.float16))


# ------------------------------------------------------------------ 5. k_begin
def ulps(a, b):
    """distance of two positive fp32 values in units of the last place"""
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


def found_inf_pattern():
    """40 steps: growth on the third finite step, an inf on the step that would have grown, two infs in a row, then a fixed
    pseudo-random tail"""
    head = [0, 0, 0, 0, 0, 1, 1, 0, 0, 0]
    return head + [int(x) for x in (np.random.default_rng(40).random(30) < 0.3)]


EXACT_WORDS = ("scale", "growth_tracker", "found_inf", "skip", "step", "inv_scale", "skipped")


def tiny_apply(st, betas):
    """an apply launch over five parameters: leaves the next step's bias corrections in words 9-13"""
    z = np.zeros(5, np.float32)
    seg = Seg(z, z, z, z, shadow=None)
    run_apply("multi", [seg], st, dev(np.array([1e-2], np.float32)), dict(beta1=betas[0], beta2=betas[1], eps=1e-15))


@pytest.mark.parametrize("use_scaler", [1, 0])
def test_begin_follows_the_gradscaler_rules_for_40_steps(use_scaler):
    betas, interval = (0.9, 0.99), 3
    pattern = found_inf_pattern()
    st = OU.new_state(scale=1024.0 if use_scaler else 1.0)
    py, _ = OU.read_state(st)
    events = set()
    for i, f in enumerate(pattern):
        st[2:3].fill_(f)
        if use_scaler and f and py["growth_tracker"] == interval - 1:
            events.add("inf on a growth step")
        if use_scaler and f and i and pattern[i - 1]:
            events.add("two infs in a row")
        assert OU.begin(st, betas[0], betas[1], interval, 2.0, 0.5, use_scaler) == 0
        before = py
        py = OU.scaler_begin(py, f, interval, 2.0, 0.5, use_scaler, betas=betas)
        if py["scale"] > before["scale"]:
            events.add("growth")
        d, _ = OU.read_state(st)
        assert {k: d[k] for k in EXACT_WORDS} == {k: py[k] for k in EXACT_WORDS}, i
        assert d["inv_scale"] == (float(np.float32(1.0 / before["scale"])) if use_scaler else 1.0)
        assert ulps(d["inv_bc1"], py["inv_bc1"]) <= 1 and ulps(d["bc2_sqrt"], py["bc2_sqrt"]) <= 1, (i, d, py)
        tiny_apply(st, betas)
    if use_scaler:
        assert events == {"inf on a growth step", "two infs in a row", "growth"} and 0 < py["skipped"] == sum(pattern)
    else:
        assert py["step"] == 40 and py["skipped"] == 0 and py["scale"] == 1.0 and py["growth_tracker"] == 0


def test_cached_bias_corrections_equal_the_recomputed_ones():
    """two state blocks through the same begin / apply sequence; one has word 11 zeroed before every begin, so it recomputes what the
    other takes from the words the previous apply left: bit-identical at every step"""
    betas, pattern = (0.9, 0.99), found_inf_pattern()
    a, b = OU.new_state(scale=1024.0), OU.new_state(scale=1024.0)
    cached = 0
    for i, f in enumerate(pattern):
        for st in (a, b):
            st[2:3].fill_(f)
        b[11:12].zero_()
        wa = host(a)
        cached += int(not f and wa[11] == wa[4] + 1)
        for st in (a, b):
            assert OU.begin(st, betas[0], betas[1], 3, 2.0, 0.5, 1) == 0
        wa, wb = host(a), host(b)
        assert np.array_equal(wa[:9], wb[:9]), (i, wa, wb)
        for st in (a, b):
            tiny_apply(st, betas)
        wa = host(a)
        assert wa[11] == wa[4] + 1 and np.array_equal(wa[12:14].view(np.float32), np.array(betas, np.float32))
    assert cached == len(pattern) - sum(pattern) - 1              # every taken step but the first came from the cache


def test_begin_follows_changed_betas_not_the_cache():
    st = OU.new_state(scale=1024.0, step=9)
    assert OU.begin(st, 0.9, 0.99) == 0
    tiny_apply(st, (0.9, 0.99))
    w = host(st)
    assert w[11] == 11                                               # the cache is for step 11, with the old betas
    assert OU.begin(st, 0.8, 0.95) == 0
    d, w2 = OU.read_state(st)
    a, b = OU.bias_corrections_f64(0.8, 0.95, 11)
    assert d["step"] == 11 and ulps(d["inv_bc1"], a) <= 1 and ulps(d["bc2_sqrt"], b) <= 1
    assert w2[5] != w[9] and w2[6] != w[10]


@pytest.mark.parametrize("step0", STEPS0)
def test_bias_corrections_over_a_long_horizon(step0):
    """recomputed at step0 + 1, from the cache at step0 + 2; at 10^7 both corrections are exactly 1"""
    betas = (0.9, 0.99)
    st = OU.new_state(scale=1024.0, step=step0)
    for step in (step0 + 1, step0 + 2):
        assert OU.begin(st, betas[0], betas[1]) == 0
        d, _ = OU.read_state(st)
        a, b = OU.bias_corrections_f64(betas[0], betas[1], step)
        assert d["step"] == step and ulps(d["inv_bc1"], a) <= 1 and ulps(d["bc2_sqrt"], b) <= 1, (d, a, b)
        if step >= 10 ** 7:
            assert d["inv_bc1"] == 1.0 and d["bc2_sqrt"] == 1.0
        tiny_apply(st, betas)
        assert host(st)[11] == step + 1


# ------------------------------------------------------------------ 6. EMA
def ema_inputs(n, seed):
    rng = np.random.default_rng([n, seed])
    return (0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.standard_normal(n)).astype(np.float32)


def test_ema_update_multi_against_float64():
    sizes = [1, 2, 3, 4, 5, 7, 1023, OU.sweep(4) + 3]
    worst = 0.0
    for n in sizes:
        s0, p0 = ema_inputs(n, 0)
        s, p = padded(s0, NAN), padded(p0, NAN)
        assert OU.ema_multi([s], [p], 0.05, sizes=[n]) == 0
        got, gp = host(s), host(p)
        assert_bits(gp, np.concatenate([p0, np.full(PAD, NAN)]), "param unchanged")
        assert_bits(got[n:], np.full(PAD, NAN), "guard elements behind the shadow")
        r = OU.ema_ratio(got[:n], s0, p0, 0.05)
        worst = max(worst, r)
        assert r <= 1.0, (n, r)
        assert not np.array_equal(got[:n], s0)
    # eight tensors of mixed sizes in one call
    sizes8 = [1029, 0, 77, 4100, 5, 2051, 16, 333]
    ins = [ema_inputs(n, 1 + i) for i, n in enumerate(sizes8)]
    ss, ps = [padded(a, NAN) for a, _ in ins], [padded(b, NAN) for _, b in ins]
    omd = float(np.float32(1.0 - 0.95))
    assert OU.ema_multi(ss, ps, omd, sizes=sizes8) == 0
    for n, (s0, p0), s, p in zip(sizes8, ins, ss, ps):
        got = host(s)
        assert_bits(host(p)[:n], p0, "param unchanged")
        assert_bits(got[n:], np.full(PAD, NAN), "guard elements behind the shadow")
        r = OU.ema_ratio(got[:n], s0, p0, omd)
        worst = max(worst, r)
        assert r <= 1.0, (n, r)
    print(f"EMA update: {worst:.3f} of the bound")


@pytest.mark.parametrize("use_num_updates", [1, 0])
@pytest.mark.parametrize("size,epoch_len", [("1029+5", 4), ("1", 4), ("S+3", 4), ("1029+5", 1)])
def test_ema_update_gated_counts_and_matches_the_plain_update(size, epoch_len, use_num_updates):
    """the int64 step counter goes 0 .. 13: only positive multiples of epoch_len update, count[0] advances once per update, the ticket
    count[1] is 0 after every launch, and the shadows are the bits lae_ema_update_multi gives with ema_one_minus_decay(decay, k)"""
    from laenerf_amd.optim import ema_one_minus_decay
    sizes = {"1029+5": [1029, 5], "1": [1], "S+3": [OU.sweep(4) + 3]}[size]
    decay = 0.95
    ins = [ema_inputs(n, 50 + i) for i, n in enumerate(sizes)]
    gated, plain = [padded(a, NAN) for a, _ in ins], [padded(a, NAN) for a, _ in ins]
    params = [padded(b, NAN) for _, b in ins]
    step, count = dev(np.zeros(1, np.int64)), dev(np.zeros(2, np.int32))
    k = 0
    for s in range(14):
        step.fill_(s)
        for p in params:                                             # the parameters move between steps (exactly: a power of two times them)
            p.mul_(0.5 if s % 2 else 2.0)
        assert OU.ema_gated(gated, params, step, epoch_len, count, decay, use_num_updates, sizes=sizes) == 0
        if s > 0 and s % epoch_len == 0:
            k += 1
            assert OU.ema_multi(plain, params, ema_one_minus_decay(decay, k, bool(use_num_updates)), sizes=sizes) == 0
        assert host(count).tolist() == [k, 0], (s, host(count))
        for a, b in zip(gated, plain):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"step {s}: gated against plain"
    assert k == (3 if epoch_len == 4 else 13) and int(host(step)[0]) == 13
    assert not np.array_equal(host(gated[0])[:sizes[0]], ins[0][0])
