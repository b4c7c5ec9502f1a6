"""numpy restatement of the soft code assignment (tests/test_soft_assign.py, tools/gen_golden_soft.py): the float64 softmax of
given fp32 distances, the p / q argmax that torch.multinomial computes from its exponential_ draw, and how close each token's
draw was.  Also the loader of the tests/golden/soft_assign_*.npz fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("d256_k96", "d64_k1024", "d256_k16384", "tiestress_k96")
FLIP_REL = 1e-4          # a token whose two best ratios are closer than this (relative) may legitimately flip


def scores(dist, temp):
    """s = (-d) / temp in fp32, as the reference's `-distances / temp` and the kernel"""
    return (-np.asarray(dist, np.float32)) / np.float32(temp)


def softmax64(dist, temp):
    """float64 softmax over the last axis of the fp32 scores of fp32 distances"""
    s = scores(dist, temp).astype(np.float64)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def draw(p, q):
    """argmax_j p[n, j] / q[n, j], the first index on ties"""
    return np.argmax(np.asarray(p, np.float64) / np.asarray(q, np.float64), axis=-1).astype(np.int64)


def ratio_gap(p, q):
    """per token: (best - second best) / best of p / q"""
    r = np.asarray(p, np.float64) / np.asarray(q, np.float64)
    top = np.partition(r, r.shape[-1] - 2, axis=-1)[..., -2:]
    return (top[..., 1] - top[..., 0]) / top[..., 1]


def skip_set(p, q):
    """bool [N]: tokens whose draw may flip under an error of the soft codes"""
    return ratio_gap(p, q) < FLIP_REL


def q_from_bits(qbits):
    """the fixtures keep the upper 16 bits of each fp32 variate: exactly an fp32 number"""
    return (np.asarray(qbits, np.uint32) << np.uint32(16)).view(np.float32)


def load(tag):
    """the fixture `tag` as a dict; arrays too large for one file sit in soft_assign_<tag>.<field><part>.npz side files"""
    g = dict(np.load(os.path.join(GOLDEN, "soft_assign_%s.npz" % tag)))
    for field in ("dist", "dist_oracle", "soft", "qbits"):
        parts = int(g.get(field + "_parts", 0))
        if parts:
            g[field] = np.concatenate([np.load(os.path.join(GOLDEN, "soft_assign_%s.%s%d.npz" % (tag, field, i)))["a"]
                                       for i in range(parts)], axis=0)
    g["q"] = q_from_bits(g["qbits"])
    return g
