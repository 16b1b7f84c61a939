"""Nearest-neighbour feature matching without a GPU: nnfm_numpy against the reference's recorded results
(tests/golden/nnfm_case.npz, written by tests/golden/make_golden_nnfm.py from the reference's semantic_encoder.py), the host
size helpers and argument validation of the lae_nnfm_* entry points, and the StyleNetwork switch."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from nnfm_util import GOLDEN_CASES, golden_inputs, match_margin


def test_nnfm_numpy_reproduces_the_reference_fixture():
    from laenerf_amd.editing import nnfm_numpy
    g = golden("nnfm_case")
    assert [tuple(r) for r in g["shapes"].tolist()] == list(GOLDEN_CASES)
    for k, shape in enumerate(GOLDEN_CASES):
        x, s = golden_inputs(int(g["seed"]), k, shape)
        z, loss, dx, cos = nnfm_numpy(x, s)
        assert cos.shape == (shape[0], shape[2], shape[3])
        assert np.array_equal(z, g[f"z{k}"])
        assert abs(loss - float(g[f"loss{k}"])) <= 1e-6 * abs(loss)                      # the reference computed in fp32
        assert np.abs(dx - g[f"dx{k}"]).max() <= 1e-6 * np.abs(dx).max()
        assert match_margin(x, s) >= float(g["margin"]) > 1e-3                           # what the generator chose the seed for
        z2, loss2, dx2, _ = nnfm_numpy(x, s, z=g[f"z{k}"])                               # at a given match
        assert np.array_equal(z2, z) and loss2 == loss and np.array_equal(dx2, dx)


def test_nnfm_numpy_gradient_is_the_derivative_and_zero_vectors_are_defined():
    from laenerf_amd.editing import nnfm_numpy
    rng = np.random.default_rng(3)
    x, s = rng.standard_normal((2, 5, 7)), rng.standard_normal((2, 5, 4))
    x[1, :, 2] = 0.0
    z, loss, dx, _ = nnfm_numpy(x, s)
    assert np.isfinite(loss) and np.isfinite(dx).all() and not dx[1, :, 2].any()
    h = 1e-6
    for idx in ((0, 1, 3), (1, 4, 0), (0, 0, 6)):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        num = (nnfm_numpy(xp, s, z=z)[1] - nnfm_numpy(xm, s, z=z)[1]) / (2 * h)
        assert abs(num - dx[idx]) <= 1e-8 + 1e-6 * abs(dx[idx])
    x0 = np.zeros((1, 5, 1))
    assert nnfm_numpy(x0, s[:1])[1] == 1.0                                               # a zero vector contributes 1


def test_workspace_size_is_small_and_monotone(hip_lib):
    ws = hip_lib.lae_nnfm_workspace_bytes
    full = ws(1, 768, 4096, 4096)
    assert 4096 * 768 * 2 <= full <= 16 << 20                                            # the distance matrix alone would be 64 MiB
    assert hip_lib.lae_nnfm_packed_bytes(1, 768, 4096) == 4096 * 768 * 2
    assert hip_lib.lae_nnfm_packed_bytes(2, 40, 70) == 2 * 128 * 64 * 2                  # N to 64 rows, C to 32 channels
    base = (2, 40, 70, 33)
    for axis, values in ((0, (1, 2, 3, 7)), (1, (1, 31, 32, 33, 64, 65, 768)), (2, (0, 1, 63, 64, 65, 130, 4096)),
                         (3, (1, 33, 255, 256, 257, 300, 4096, 4100))):
        sizes = []
        for v in values:
            a = list(base)
            a[axis] = v
            sizes.append(ws(*a))
        assert sizes == sorted(sizes), (axis, sizes)
        assert sizes[-1] > sizes[0], (axis, sizes)


def test_arguments_are_validated_before_any_launch(hip_lib):
    one = ctypes.c_void_p(256)
    L = hip_lib
    # Na == 0 (pack: N == 0): OK without touching pointers
    assert L.lae_nnfm_pack(None, 1, 8, 0, None, None) == 0
    assert L.lae_nnfm_match(None, None, 1, 0, 4, 8, None, None, None, None) == 0
    assert L.lae_nnfm_loss_forward(None, None, None, 1, 8, 0, 4, None, None, None) == 0
    assert L.lae_nnfm_loss_backward(None, None, None, None, None, 1, 8, 0, 4, None, None) == 0
    # NULL -> LAE_ENULL (d_best alone may be NULL)
    assert L.lae_nnfm_pack(None, 1, 8, 4, one, None) == -3
    assert L.lae_nnfm_pack(one, 1, 8, 4, None, None) == -3
    for hole in (0, 1, 6, 8):
        a = [one, one, 1, 4, 4, 8, one, one, one, None]
        a[hole] = None
        assert L.lae_nnfm_match(*a) == -3, hole
    for hole in (0, 1, 2, 7, 8):
        a = [one, one, one, 1, 8, 4, 4, one, one, None]
        a[hole] = None
        assert L.lae_nnfm_loss_forward(*a) == -3, hole
    for hole in (0, 1, 2, 3, 4, 9):
        a = [one, one, one, one, one, 1, 8, 4, 4, one, None]
        a[hole] = None
        assert L.lae_nnfm_loss_backward(*a) == -3, hole
    # C < 1, Nb < 1, n < 1 -> LAE_EINVAL
    assert L.lae_nnfm_pack(one, 1, 0, 4, one, None) == -1
    assert L.lae_nnfm_pack(one, 0, 8, 4, one, None) == -1
    assert L.lae_nnfm_match(one, one, 1, 4, 4, 0, one, one, one, None) == -1
    assert L.lae_nnfm_match(one, one, 1, 4, 0, 8, one, one, one, None) == -1
    assert L.lae_nnfm_match(one, one, 0, 4, 4, 8, one, one, one, None) == -1
    assert L.lae_nnfm_loss_forward(one, one, one, 1, 0, 4, 4, one, one, None) == -1
    assert L.lae_nnfm_loss_forward(one, one, one, 1, 8, 4, 0, one, one, None) == -1
    assert L.lae_nnfm_loss_backward(one, one, one, one, one, 1, 0, 4, 4, one, None) == -1
    assert L.lae_nnfm_loss_backward(one, one, one, one, one, 1, 8, 4, 0, one, None) == -1
    assert L.lae_nnfm_match(ctypes.c_void_p(8), one, 1, 4, 4, 8, one, one, one, None) == -1      # packed sides: 16-byte aligned


def _tiny_vgg(seed=0):
    from laenerf_amd.editing.style_network import vgg19_features
    torch.manual_seed(seed)
    return vgg19_features(2)


def test_style_network_rejects_an_unknown_loss_and_gram_is_unchanged():
    from laenerf_amd.editing import StyleNetwork
    from laenerf_amd.editing.style_network import gram_matrix, random_crop
    from style_mode_util import striped_style
    with pytest.raises(ValueError):
        StyleNetwork(striped_style(), _tiny_vgg(), style_layers=(0, 2), size=16, loss="bogus")
    with pytest.raises(ValueError):
        StyleNetwork(striped_style(), _tiny_vgg(), style_layers=(0, 2), size=16, nnfm_match="bogus")
    vgg = _tiny_vgg()
    net = StyleNetwork(striped_style(), vgg, style_layers=(0, 2), size=16, generator=torch.Generator().manual_seed(5))
    explicit = StyleNetwork(striped_style(), vgg, style_layers=(0, 2), size=16, generator=torch.Generator().manual_seed(5), loss="gram")
    assert net.loss_kind == "gram"
    assert sorted(dict(net.named_buffers())) == sorted(dict(explicit.named_buffers())) == ["gram_style", "gram_target", "image", "mean", "std"]
    # the buffers of the constructor as it was: the crop torchvision's RandomCrop rule draws from the generator, its Gram
    with torch.no_grad():
        crop = random_crop(striped_style(), 16, generator=torch.Generator().manual_seed(5))
        want = gram_matrix(net.features(net.normalize(crop)))
    assert torch.equal(net.gram_style, want) and torch.equal(net.gram_target, want) and torch.equal(explicit.gram_style, want)
    x = torch.rand(3, 16, 16)
    assert torch.equal(net.loss_from_input(x), torch.nn.functional.mse_loss(gram_matrix(net.features(x)), want))
