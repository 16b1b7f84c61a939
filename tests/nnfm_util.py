"""Inputs and float64 helpers shared by test_nnfm_cpu.py, test_gpu_nnfm.py and tests/golden/make_golden_nnfm.py."""
import numpy as np

GOLDEN_CASES = ((2, 40, 70, 33), (1, 64, 150, 97))          # (n, C, Na, Nb) of tests/golden/nnfm_case.npz
GOLDEN_SEEDS = range(256)                                    # the generator records the one whose matches are best separated


def match_margin(x, s):
    """smallest float64 gap between the best and the second-best matching cosine over all content positions (Nb >= 2)"""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    an = x / (np.sqrt((x * x).sum(1, keepdims=True) + 1e-8) + 1e-8)
    bn = s / (np.sqrt((s * s).sum(1, keepdims=True) + 1e-8) + 1e-8)
    c = np.sort(np.einsum("nci,ncj->nij", an, bn), 2)
    return float((c[..., -1] - c[..., -2]).min())


def golden_inputs(seed, k, shape):
    """content x [n, C, Na] and style s [n, C, Nb] of golden case k: fp32 standard normals from numpy.random.default_rng([seed, k])"""
    n, C, Na, Nb = shape
    rng = np.random.default_rng([int(seed), int(k)])
    x = rng.standard_normal((n, C, Na)).astype(np.float32)
    s = rng.standard_normal((n, C, Nb)).astype(np.float32)
    return x, s
