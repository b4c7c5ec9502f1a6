"""numpy restatement of the scored / temperature-sampled code assignment of MaskVectorQuantize / VectorQuantize
(tests/test_maskvq.py, tools/gen_golden_maskvq.py): the perturbed scores in float64 from the fp32 `s / temp`, the top-2 gap per
token, which tokens may legitimately flip, and the loss.  Also the loader of the tests/golden/maskvq_*.npz fixtures.

The skip rule.  A sampled code is argmax_j fl(fl(s_j / temp) + g_j), g = -log(clamp(-log(clamp(u, 1e-20)), 1e-20)).  The division
is IEEE on both sides; what differs between two implementations is g (another logf) and nothing else.  G_ERR is the largest
|fp32 torch chain - float64 chain| of g over every u the fixtures hold, measured on the CPU by the generator: the device logf and
the host log each sit within a couple of ulp of the true value (the inner log's relative error becomes an absolute error of the
outer one), so either side's g is within 2 G_ERR of the float64 value; two competitors, plus one fp32 ulp of the best perturbed
score for the two roundings of the add:  a token may differ only if its float64 top-2 gap is below  4 G_ERR + ulp32(best).
At most SKIP_CAP of a fixture's tokens may be in that set (expected share ~1e-5: the gap density of Gumbel-perturbed scores at zero
is O(1)).

Cosine end to end (the module normalises on the GPU, the reference did on the CPU; the operands may differ in the last bit): each
cosine is within 2 ulp of 1.0 of the reference's, so a token may also differ when its top-2 gap of the reference's scores is below
4 ulp32(1.0) -- divided by temp in the perturbed domain."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a_l2_masked", "b_l2_flat", "c_cosine", "d_ties_l2", "d_ties_cos", "e_cosdist")
G_ERR = 5.2497209068747e-07      # measured by tools/gen_golden_maskvq.py (it asserts that no fixture exceeds it)
SKIP_CAP = 0.001
COS_ULPS = 4.0 * float(np.spacing(np.float32(1.0)))
SIDE_FIELDS = ("u1", "dist")
EPS32 = np.float32(1e-20)


def gumbel64(u):
    """the reference's gumbel_noise of fp32 uniforms, in float64"""
    eps = np.float64(EPS32)
    a = -np.log(np.maximum(np.asarray(u, np.float32).astype(np.float64), eps))
    return -np.log(np.maximum(a, eps))


def perturbed(s, temp, u):
    """float64 perturbed scores from the fp32 quotient s / temp"""
    q = (np.asarray(s, np.float32) / np.float32(temp)).astype(np.float64)
    return q + gumbel64(u)


def argmax_torch(v):
    """torch.argmax over the last axis: the first index among equal maxima, a NaN is the maximum and the first NaN wins"""
    v = np.asarray(v)
    nan = np.isnan(v)
    out = np.argmax(np.where(nan, -np.inf, v), axis=-1)
    has = nan.any(axis=-1)
    return np.where(has, np.argmax(nan, axis=-1), out).astype(np.int64)


def top2(v):
    """(best, best - second best) per row"""
    v = np.asarray(v, np.float64)
    t = np.partition(v, v.shape[-1] - 2, axis=-1)[..., -2:]
    return t[..., 1], t[..., 1] - t[..., 0]


def skip_sampled(s, temp, u, cosine_end_to_end=False):
    """bool [N]: tokens whose sampled code may differ between two correct implementations"""
    best, gap = top2(perturbed(s, temp, u))
    thr = 4.0 * G_ERR + np.spacing(np.abs(best).astype(np.float32)).astype(np.float64)
    if cosine_end_to_end:
        thr = thr + COS_ULPS / float(temp)
    return gap < thr


def skip_cosine_hard(s):
    """bool [N]: temp == 0, cosine end to end: the reference's two best cosines within 4 ulp of 1.0"""
    _, gap = top2(np.where(np.isnan(s), -np.inf, np.asarray(s, np.float64)))
    return gap < COS_ULPS


def loss_ref(x_rows, e_rows, beta, mask=None):
    """the reference's loss from token rows [N, D] and gathered rows [N, D] (mask [N] or None), in float64"""
    d2 = (np.asarray(e_rows, np.float64) - np.asarray(x_rows, np.float64)) ** 2
    if mask is None:
        m = d2.mean()
        return beta * m + m
    mk = np.asarray(mask, np.float64).reshape(-1, 1)
    m = (d2 * mk).mean()
    ratio = 1.0 / mk.mean()
    return ratio * beta * m + ratio * m


def load(tag):
    """the fixture `tag` as a dict; arrays too large for one file sit in maskvq_<tag>.<field><part>.npz side files"""
    g = dict(np.load(os.path.join(GOLDEN, "maskvq_%s.npz" % tag)))
    for field in SIDE_FIELDS:
        parts = int(g.get(field + "_parts", 0))
        if parts:
            g[field] = np.concatenate([np.load(os.path.join(GOLDEN, "maskvq_%s.%s%d.npz" % (tag, field, i)))["a"]
                                       for i in range(parts)], axis=0)
    return g
