"""numpy restatement of the lucidrains-style quantizer (dynamicvectorquantization_amd/lucid.py; tests/test_lucid.py,
tools/gen_golden_lucid.py): hard and sampled codes from the assign's bit-exact distances, the training step of both codebooks
(cluster_size EMA, the new embed, code expiry), the losses, the orthogonal regulariser in float64.  Also the loader of the
tests/golden/lucid_*.npz fixtures.

Codes.  The reference scores with s = -cdist (torch's matmul form of the distance, clamped at 0, square-rooted); the kernels score
with s = -sqrt(max(d, 0)) of the assign's own distance d (ATen-order norms, sequential-k FMA chain).  At temp = 0 the code is
argmax s = argmin d.  At temp > 0 the code is argmax fl(fl(s / temp) + g); two correct implementations may disagree where the float64
top-2 gap of the perturbed scores is below
    2 (S_ERR / temp + G_ERR) + ulp32(best)
-- each competitor's score is within S_ERR of the float64 distance on either side (S_ERR: the larger of max |reference fp32 dist -
float64| and max |-sqrt(oracle d) - float64| over the fixture, measured by the generator and stored in the .npz), its noise within
G_ERR (tests/_maskvq_ref.py), plus one fp32 ulp of the best perturbed score for the roundings of the add.  At most SKIP_CAP of a
fixture's tokens may be in that set."""
import collections
import os

import numpy as np

from tests._maskvq_ref import G_ERR, SKIP_CAP, argmax_torch, gumbel64, perturbed, top2  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("a_euclid", "b_euclid_flat", "c_cosine", "d_ties")
ORTHO_SETS = ("n96_d64_init", "n96_d64_trained", "n100_d256_init", "n100_d256_trained", "n1024_d128_init", "n1024_d128_trained",
              "n96_d64_dup_zero")
PART_BYTES = 720 << 10


def load(name):
    """tests/golden/lucid_<name>.npz as a dict; arrays too large for one file sit in lucid_<name>.<field><part>.npz side files"""
    g = dict(np.load(os.path.join(GOLDEN, "lucid_%s.npz" % name)))
    for key in [k for k in g if k.endswith("_parts")]:
        field = key[:-len("_parts")]
        g[field] = np.concatenate([np.load(os.path.join(GOLDEN, "lucid_%s.%s%d.npz" % (name, field, i)))["a"]
                                   for i in range(int(g[key]))], axis=0)
    return g


def rows_of(x, layout):
    """the reference's `flatten` [N, D] of the module input"""
    if layout == "nchw":
        return np.ascontiguousarray(x.reshape(x.shape[0], x.shape[1], -1).transpose(0, 2, 1)).reshape(-1, x.shape[1])
    if layout == "bdn":
        return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, x.shape[1])
    return x.reshape(-1, x.shape[-1])


def l2norm(a):
    """F.normalize(a, p = 2, dim = -1) in the array's precision"""
    a = np.asarray(a)
    n = np.sqrt((a.astype(np.float64) ** 2).sum(axis=-1, keepdims=True)).astype(a.dtype)
    return a / np.maximum(n, a.dtype.type(1e-12))


def cdist_scores(d):
    """s = -sqrt(d < 0 ? 0 : d) in fp32 from the assign's distances d [N, K]; a NaN stays a NaN"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return -np.sqrt(np.where(d < 0, np.float32(0), d)).astype(np.float32)


def argmin_torch(d):
    """the assign's code: the first index among equal minima, a NaN is the minimum and the first NaN wins"""
    return argmax_torch(-np.asarray(d))


def skip_sampled(s, temp, u, s_err):
    """bool [N]: tokens whose sampled code may differ between two correct implementations (module docstring)"""
    best, gap = top2(perturbed(s, temp, u))
    thr = 2.0 * (float(s_err) / float(temp) + G_ERR) + np.spacing(np.abs(best).astype(np.float32)).astype(np.float64)
    return gap < thr


def commit_loss(x_rows, e_rows, weight):
    """commitment_weight * mse(quantize, x), in float64"""
    return float(weight) * float(((np.asarray(e_rows, np.float64) - np.asarray(x_rows, np.float64)) ** 2).mean())


def ortho64(t):
    """orthogonal_loss_fn of t [n, d] and its gradient, in float64"""
    t = np.asarray(t, np.float64)
    n = t.shape[0]
    nrm = np.maximum(np.sqrt((t ** 2).sum(-1, keepdims=True)), 1e-12)
    c = t / nrm
    m = c @ c.T - np.eye(n)
    loss = (m ** 2).sum() / n ** 2
    g = (4.0 / n ** 2) * (m @ c)
    return loss, (g - c * (c * g).sum(-1, keepdims=True)) / nrm


def ortho64_heads(t):
    """orthogonal_loss_fn of t [h, n, d] in float64: the mean of the heads' losses, each head's gradient divided by h"""
    parts = [ortho64(th) for th in t]
    return float(np.mean([p[0] for p in parts])), np.stack([p[1] for p in parts]) / len(parts)


OrthoGeom = collections.namedtuple("OrthoGeom", "T gx gy idle s0 S tper last")


def ortho_geometry(h, n):
    """dvq_ortho_grid and dvq_ortho_backward_slices (csrc/ortho_loss.hip) restated.  T: 32-row tiles; forward grid gx x gy x h
    (four column tiles per workgroup, OL_ROWCHUNK = 8 row tiles per chunk), idle: waves of the last forward workgroup without a
    column tile; s0: the first estimate of the backward slice count (about 1024 waves, at most 8, at most T), S: the count after
    rounding the tiles per slice (tper) up, last: the column tiles of the last slice"""
    T = (n + 31) // 32
    gx, gy = (T + 3) // 4, (T + 7) // 8
    s0 = min(max(1024 // max(T * h, 1), 1), 8, T)
    tper = (T + s0 - 1) // s0
    S = (T + tper - 1) // tper
    return OrthoGeom(T, gx, gy, 4 * gx - T, s0, S, tper, T - (S - 1) * tper)


def ortho_workspace_bytes(h, n, d):
    """dvq_ortho_loss_workspace_bytes restated: the larger of the forward partials (one double per workgroup) and the backward
    slices' partial gradients (S x [h, n, d] floats), rounded up to 256 bytes"""
    g = ortho_geometry(h, n)
    return (max(g.gx * g.gy * h * 8, g.S * h * n * d * 4) + 255) // 256 * 256


def train_step(kind, rows, codes, embed, embed_avg, cluster_size, decay, eps, threshold, picks):
    """one training-mode update in float64 -> (embed' [K, D], cluster_size' [K], expired [K] bool).
    kind 0 (Euclidean): embed' = embed_avg / (((cs' + eps) / (sum cs' + K eps)) * sum cs').
    kind 1 (cosine): m = normalize(per-code mean of the normalised rows), normalize(embed) where a code has no token;
    embed' = embed * decay + (1 - decay) * m.
    Both: the j-th code with cs' < threshold takes normalize(rows)[picks[j]]."""
    K = embed.shape[0]
    rows = np.asarray(rows, np.float64)
    embed = np.asarray(embed, np.float64)
    counts = np.bincount(np.asarray(codes).reshape(-1), minlength=K).astype(np.float64)
    cs = np.asarray(cluster_size, np.float64) * decay + (1.0 - decay) * counts
    if kind == 0:
        tot = cs.sum()
        new = np.asarray(embed_avg, np.float64) / ((((cs + eps) / (tot + K * eps)) * tot)[:, None])
    else:
        rn = l2norm(rows)
        sums = np.zeros_like(embed)
        np.add.at(sums, np.asarray(codes).reshape(-1), rn)
        mean = l2norm(sums / np.where(counts == 0, 1.0, counts)[:, None])
        mean = np.where((counts == 0)[:, None], l2norm(embed), mean)
        new = embed * decay + (1.0 - decay) * mean
    expired = (cs < threshold) if threshold > 0 else np.zeros(K, bool)
    if expired.any():
        new = new.copy()
        new[expired] = l2norm(rows)[np.asarray(picks)[:int(expired.sum())]]
    return new, cs, expired
