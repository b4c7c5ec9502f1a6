"""Float64 numpy restatement of GumbelQuantize.forward in its hard form (reference modules/vector_quantization/
quantize_vqgan.py:171-200 with F.gumbel_softmax's own arithmetic), the seeded inputs of the test cases, and the fixture loader.

    logits  l[n, k] = z_n . W_k + b_k
    scores  s[n, k] = (l[n, k] - log q[n, k]) / tau       (F.gumbel_softmax: gumbels = -exponential_().log(); (logits + gumbels) / tau)
    codes   argmax_k s, torch's rules (first index on ties, NaN is the maximum)
    KL      mean_n sum_k p log(p K + 1e-10), p = softmax(l)
    z_q     E[codes] in NCHW (the reference multiplies the row by fl(fl(1 - y) + y), within 2^-23 of 1)

Near-tie rule (tests/test_gumbel.py): a code is compared only where the float64 top-2 gap of s exceeds MARGIN = 8 * err_ref,
err_ref = max |s_f32(reference's own torch ops on the CPU) - s_f64| over every case and tau below, measured by
tools/gen_golden_gumbel.py and stored in the fixture's `meta`; the factor 8 covers the few-ulp differences of logf and of the
dot chain's order on the GPU.  At most SKIP_CAP of a case's tokens may be left out; the generator asserts that the reference
itself stays within that.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = "gumbel_quantize_B2.npz"
SKIP_CAP = 0.02
TAUS = (1.0, 0.5)
# name -> (B, C, H, W, K, d, seed); "golden" is stored in the fixture, the others are regenerated from their seeds
CASES = {
    "golden": (2, 64, 6, 6, 200, 16, 9101),       # N = 72: a partial wave, a wave that straddles the two images
    "odd": (1, 128, 5, 7, 37, 3, 9102),           # K % 4 != 0, a partial second tile, odd HW, unaligned q rows
    "wide": (3, 256, 8, 8, 1024, 256, 9103),
    "flat": (33, 64, 1, 1, 64, 16, 9104),         # HW == 1
}


def case_inputs(name):
    """z [B, C, H, W], W [K, C], b [K], E [K, d], q [B, K, H, W] (Exp(1)), float32: logits of standard deviation ~1.5"""
    B, C, H, Wd, K, d, seed = CASES[name]
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, C, H, Wd)).astype(np.float32)
    W = (rng.standard_normal((K, C)) * (1.5 / np.sqrt(C))).astype(np.float32)
    b = (0.5 * rng.standard_normal(K)).astype(np.float32)
    E = rng.standard_normal((K, d)).astype(np.float32)
    q = rng.standard_exponential((B, K, H, Wd)).astype(np.float32)
    q = np.maximum(q, np.float32(1e-30))
    return z, W, b, E, q


def load():
    g = dict(np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False))
    g["meta"] = json.loads(str(g["meta"]))
    return g


def inputs(name, g=None):
    """the case's inputs; "golden" from the fixture (its q is the reference's own captured draw at tau = TAUS[0])"""
    if name == "golden" and g is not None:
        return g["z"], g["W"], g["b"], g["E"], g["q"]
    return case_inputs(name)


def logits64(z, W, b):
    """[B, K, H, W] float64"""
    return np.einsum("bchw,kc->bkhw", z.astype(np.float64), W.astype(np.float64)) + b.astype(np.float64)[None, :, None, None]


def argmax_torch(s, axis=1):
    """first index among equal maxima; a NaN is the maximum and the first NaN wins"""
    nan = np.isnan(s)
    out = np.argmax(np.where(nan, -np.inf, s), axis=axis)
    has = nan.any(axis=axis)
    return np.where(has, np.argmax(nan, axis=axis), out)


def top2_gap(s, axis=1):
    srt = np.sort(s, axis=axis)
    return np.take(srt, -1, axis=axis) - np.take(srt, -2, axis=axis)


def forward(z, W, b, E, q, tau):
    """-> scores [B, K, H, W] f64 (the logits when q is None), codes [B, H, W] i64, KL mean (float), z_q [B, d, H, W] f32"""
    l = logits64(z, W, b)
    s = l if q is None else (l - np.log(q.astype(np.float64))) / float(tau)
    codes = argmax_torch(s, axis=1).astype(np.int64)
    K = W.shape[0]
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    p = e / e.sum(axis=1, keepdims=True)
    kl = float(np.sum(p * np.log(p * K + 1e-10), axis=1).mean())
    zq = np.ascontiguousarray(E[codes].transpose(0, 3, 1, 2))
    return s, codes, kl, zq
