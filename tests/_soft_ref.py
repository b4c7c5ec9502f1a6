"""numpy restatement of the soft code assignment (tests/test_soft_assign.py, tests/test_soft_assign_shapes.py,
tools/gen_golden_soft.py): the float64 softmax of given fp32 distances, the p / q argmax that torch.multinomial computes from its
exponential_ draw, how close each token's draw was, the allowance of the soft codes and the launcher's choice of kernel form.
Also the loader of the tests/golden/soft_assign_*.npz fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("d256_k96", "d64_k1024", "d256_k16384", "tiestress_k96")
FLIP_REL = 1e-4          # a token whose two best ratios are closer than this (relative) may legitimately flip


def scores(dist, temp):
    """s = (-d) / temp in fp32, as the reference's `-distances / temp` and the kernel"""
    with np.errstate(over="ignore"):
        return (-np.asarray(dist, np.float32)) / np.float32(temp)


def softmax64(dist, temp):
    """float64 softmax over the last axis of the fp32 scores of fp32 distances; a NaN score, or a row maximum of -inf, makes
    the row NaN as in torch"""
    s = scores(dist, temp).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def softmax32_error(dist, temp):
    """e_ref: max |torch.softmax of the fp32 scores on the CPU (the reference's own op) - softmax64|"""
    import torch
    p32 = torch.softmax(torch.from_numpy(np.ascontiguousarray(scores(dist, temp))), dim=-1).numpy()
    return float(np.abs(p32.astype(np.float64) - softmax64(dist, temp)).max())


def ulp32(v):
    """the spacing of fp32 at v"""
    return float(np.spacing(np.float32(v)))


def soft_allowance(dist, temp):
    """max(4 e_ref, 4 ulp32(largest p)): the factor is tests/test_soft_assign.py's; the floor is there because e_ref falls below
    one ulp of p at small K (exactly 0 at K = 1) while the kernel rounds three times (one expf, the fp32 cast of the double sum,
    one division: about 2.5 ulp of p)"""
    return max(4.0 * softmax32_error(dist, temp), 4.0 * ulp32(softmax64(dist, temp).max()))


def kernel_form(D, K, soft, dist, q, aligned=True):
    """dvq_vq_soft_assign_flat_f32 + dvq_launch_soft_assign restated: (kernel width, WANT_DIST, WANT_S, V) of a call.  soft, dist,
    q: whether the pointer is given; aligned: whether every given pointer of {soft or the workspace, q} is 16-byte aligned.
    V = 4 / 1: the row form of phase B, None where it does not run."""
    Dp = D if D in (64, 128, 256) else min(w for w in (64, 128, 256) if w >= D)
    want_s = bool(soft) or bool(q)                   # sbuf = soft, or the workspace when q comes without soft
    vec = K % 4 == 0 and aligned
    return (Dp, bool(dist), want_s, (4 if vec else 1) if want_s else None)


def draw(p, q):
    """argmax_j p[n, j] / q[n, j], the first index on ties; a row of NaN draws 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.argmax(np.asarray(p, np.float64) / np.asarray(q, np.float64), axis=-1).astype(np.int64)


def ratio_gap(p, q):
    """per token: (best - second best) / best of p / q; a single code has no second best: 1"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.asarray(p, np.float64) / np.asarray(q, np.float64)
    if r.shape[-1] == 1:
        return np.ones(r.shape[:-1])
    top = np.partition(r, r.shape[-1] - 2, axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
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
