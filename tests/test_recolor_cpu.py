"""The recolor rule of lae_recolor_compose (include/laenerf.h) as restated by `compose_numpy`, against the reference's expressions
(nerf/utils.py:1275-1311 test_gui_styleenc, nerf/gui.py:708-714 eval_style_predictor) in fp32 torch on the CPU."""
import numpy as np
import pytest
import torch

from laenerf_amd.editing.recolor import compose_numpy

MASKS = [0xff, 0b10110101, 0b1000, 0xffff]


def case(seed, N=700, P=8, mask=0xff, clamp_all=False):
    rng = np.random.default_rng(seed)
    edit = rng.random(N) < 0.6
    slot = np.full(N, -1, np.int32)
    K = int(edit.sum())
    slot[edit] = rng.permutation(K)                                       # any slot order: compose reads through the map
    Kp = (K + 15) // 16 * 16
    wl = (rng.standard_normal((Kp, 16)) * 3).astype(np.float16)
    orw = (rng.standard_normal((Kp, 16)) * 0.7).astype(np.float16)
    n_active = bin(mask & ((1 << P) - 1)).count("1")
    pal = rng.random((n_active, 3)).astype(np.float32)
    pw = (rng.random(n_active) * 2).astype(np.float32)
    pb = (rng.standard_normal(n_active) * 0.2).astype(np.float32)
    if clamp_all:
        pb = np.full(n_active, -10.0, np.float32)                         # every edited weight clamps to 0: sum(w') == 0
    alpha = rng.choice([0.0, 1.0, 0.5], size=Kp).astype(np.float32)
    rnd = rng.random(Kp) < 0.5
    alpha[rnd] = rng.random(int(rnd.sum())).astype(np.float32)
    base = rng.random((N, 3)).astype(np.float32)
    bg = rng.random(3).astype(np.float32)
    return dict(slot_map=slot, w_logits=wl, o_raw=orw, active_mask=mask & ((1 << P) - 1), palette=pal, p_weights=pw, p_bias=pb,
                alpha=alpha, base=base, bg=bg)


def reference_torch(c, mode, k=0, use_offsets=True, offset_act="raw", literal_division=False):
    """the reference's lines on fp32 CPU tensors (its fp16 casts left out: the rule computes in fp32)"""
    slot = torch.from_numpy(c["slot_map"]).long()
    idx = torch.nonzero(slot >= 0, as_tuple=True)[0]
    s = slot[idx]
    cols = [j for j in range(16) if (c["active_mask"] >> j) & 1]
    w = torch.softmax(torch.from_numpy(c["w_logits"].astype(np.float32))[s][:, cols], -1)       # get_weights
    o = torch.from_numpy(c["o_raw"].astype(np.float32))[s, :3]                                    # get_offsets (raw)
    if offset_act == "tanh":
        o = torch.tanh(o)
    t = torch.from_numpy(c["alpha"])[s]
    pal, bg = torch.from_numpy(c["palette"]), torch.from_numpy(c["bg"])
    if mode == "eval":                                                                            # gui.py:706-714
        img = torch.ones(slot.numel(), 3) * bg
        cpred = torch.clamp(w @ pal + o, 0, 1)
        img[idx] = cpred * t[:, None] + img[idx] * (1 - t[:, None])
        return img.numpy()
    img = torch.from_numpy(c["base"]).clone()
    if mode == "weights":                                                                         # utils.py:1275-1281
        pred = w[:, k][..., None].repeat((1, 3))
    elif mode == "offsets":                                                                       # :1282-1286
        pred = o * 0.5 + 0.5
    elif use_offsets:                                                                             # :1290-1302
        pw = torch.clamp_min(torch.from_numpy(c["p_bias"])[None] + torch.from_numpy(c["p_weights"])[None] * w, 0)
        tot = pw.sum(-1)[..., None]
        pw = pw / tot
        if not literal_division:
            pw = torch.where(tot > 0, pw, torch.zeros_like(pw))                                   # the stated deviation: 0/0 -> 0
        pred = torch.clamp(o + pw @ pal, 0, 1)
    else:                                                                                         # :1303-1308
        pred = torch.clamp(w @ pal, 0, 1)
    pred += (1 - t[..., None]) * bg                                                               # :1310-1311
    img[idx] = pred
    return img.numpy()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("mode,use_offsets", [("preview", True), ("preview", False), ("weights", True), ("offsets", True), ("eval", True)])
@pytest.mark.parametrize("offset_act", ["raw", "tanh"])
def test_compose_numpy_equals_the_reference_expressions(mask, mode, use_offsets, offset_act):
    P = 16 if mask > 0xff else 8
    for seed in range(3):
        c = case(seed, P=P, mask=mask)
        n_active = c["palette"].shape[0]
        k = seed % n_active
        got = compose_numpy(**c, mode=mode, k=k, use_offsets=use_offsets, offset_act=offset_act)
        want = reference_torch(c, mode, k, use_offsets, offset_act)
        assert got.dtype == np.float32 and got.shape == c["base"].shape
        assert np.abs(got - want).max() <= 1e-6
        other = c["slot_map"] < 0
        if mode == "eval":
            assert (got[other] == c["bg"]).all()
        else:
            assert np.array_equal(got[other], c["base"][other])


@pytest.mark.parametrize("mask", MASKS[:3])
def test_an_edit_that_clamps_every_weight_takes_the_weights_as_zero(mask):
    """the reference divides 0 / 0 there and shows NaN; the rule keeps the offsets alone"""
    c = case(5, mask=mask, clamp_all=True)
    got = compose_numpy(**c, mode="preview")
    assert np.isfinite(got).all()
    assert np.abs(got - reference_torch(c, "preview")).max() <= 1e-6
    literal = reference_torch(c, "preview", literal_division=True)
    edit = c["slot_map"] >= 0
    assert np.isnan(literal[edit]).all() and not np.isnan(literal[~edit]).any()
    s = c["slot_map"][edit]
    o = c["o_raw"][s, :3].astype(np.float32)
    u = (1 - c["alpha"][s])[:, None]
    assert np.abs(got[edit] - (np.clip(o, 0, 1) + u * c["bg"])).max() <= 1e-6


def test_identity_edit_equals_the_unedited_palette_product():
    """p_weights = 1, p_bias = 0: w' = w / sum(w), i.e. the network's own weights (to the rounding of a sum of ones)"""
    c = case(7)
    n = c["palette"].shape[0]
    c["p_weights"], c["p_bias"] = np.ones(n, np.float32), np.zeros(n, np.float32)
    got = compose_numpy(**c, mode="preview")
    slot = torch.from_numpy(c["slot_map"]).long()
    idx = torch.nonzero(slot >= 0, as_tuple=True)[0]
    w = torch.softmax(torch.from_numpy(c["w_logits"].astype(np.float32))[slot[idx]][:, :8], -1)
    o = torch.from_numpy(c["o_raw"].astype(np.float32))[slot[idx], :3]
    t = torch.from_numpy(c["alpha"])[slot[idx]]
    want = torch.clamp(o + w @ torch.from_numpy(c["palette"]), 0, 1) + (1 - t[:, None]) * torch.from_numpy(c["bg"])
    assert np.abs(got[idx.numpy()] - want.numpy()).max() <= 1e-6


def test_no_edit_pixel_returns_the_base_or_the_background():
    c = case(3)
    c["slot_map"][:] = -1
    assert np.array_equal(compose_numpy(**c, mode="preview"), c["base"])
    assert (compose_numpy(**c, mode="eval") == c["bg"]).all()
