"""numpy float32 restatement of the fixed summation order of include/dvq.h (dvq_code_sums_det, dvq_vq_backward_codebook_det_f32),
and the shapes / code patterns tests/test_deterministic_stats.py runs.  Every addition below is ONE float32 operation on float32
operands (numpy adds float32 arrays in float32), in the documented order:
  tiles of TILE consecutive tokens; in a tile a code's members in ascending token index, in runs of RUN; a run summed from its first
  member on; the runs added in order; the tile partials added in ascending tile index from the first tile that has a member."""
import functools

import numpy as np

TILE, RUN = 2048, 32


def det_sums(v, codes, K, tile=TILE, run=RUN):
    """v [N, D] float32, codes [N] int -> (counts [K] float32, sums [K, D] float32) in the documented order"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    N, D = v.shape
    sums = np.zeros((K, D), np.float32)
    have = np.zeros(K, bool)
    counts = np.zeros(K, np.int64)
    for t0 in range(0, N, tile):
        c = np.asarray(codes[t0:t0 + tile])
        for j in np.unique(c):
            if j < 0 or j >= K:
                continue
            members = t0 + np.nonzero(c == j)[0]                 # ascending token index
            counts[j] += members.size
            partial = None
            for r0 in range(0, members.size, run):
                acc = v[members[r0]].copy()
                for m in members[r0 + 1:r0 + run]:
                    acc = acc + v[m]
                partial = acc if partial is None else partial + acc
            sums[j] = partial if not have[j] else sums[j] + partial
            have[j] = True
    assert sums.dtype == np.float32
    return counts.astype(np.float32), sums


def det_grad(z, E, codes, mask, g_loss, coef_scale, tile=TILE, run=RUN):
    """g_weight [K, D] = fl(c * S), c = -fl(g_loss * coef_scale), S the documented sum of fl(fl(z - E[code]) * mask)"""
    z = np.asarray(z, np.float32)
    K = E.shape[0]
    ok = (codes >= 0) & (codes < K)
    e = E[np.where(ok, codes, 0)]
    m = np.ones(z.shape[0], np.float32) if mask is None else np.asarray(mask, np.float32)
    val = ((z - e).astype(np.float32) * m[:, None]).astype(np.float32)
    _, S = det_sums(val, codes, K, tile, run)
    c = np.float32(-(np.float32(g_loss) * np.float32(coef_scale)))
    return (c * S).astype(np.float32)


def scatter_f64(v, codes, K):
    """the same sums by a float64 scatter-add (what the 1e-5 criterion of the atomic kernels is measured against)"""
    ok = (codes >= 0) & (codes < K)
    out = np.zeros((K, v.shape[1]), np.float64)
    np.add.at(out, codes[ok], v[ok].astype(np.float64))
    return np.bincount(codes[ok], minlength=K).astype(np.float64), out


# (N, D, K, pattern): the cases of the issue
CASES = [
    (130, 64, 97, "uniform"),
    (2048, 16, 3, "uniform"),          # every code is long (more than 128 members of the tile)
    (2049, 256, 1024, "uniform"),      # one token in the second tile
    (6221, 64, 97, "one"),             # all tokens on one code
    (6221, 64, 97, "half"),            # half the tokens on one code
    (6221, 4, 4100, "uniform"),        # more codes than a tile has tokens
    (4200, 96, 1024, "dual"),          # dual-grain: runs of four equal codes
]
CASE_IDS = ["%dx%d_K%d_%s" % c for c in CASES]
# B x HW with HW % 4 != 0 where N has such a factorisation
NCHW_OF = {130: (2, 65), 2048: (1024, 2), 2049: (3, 683), 6221: (1, 6221), 4200: (8, 525)}


def make_codes(N, K, pattern, seed):
    rng = np.random.default_rng(seed)
    if pattern == "uniform":
        c = rng.integers(0, K, N)
    elif pattern == "one":
        c = np.full(N, 5 % K)
    elif pattern == "half":
        c = rng.integers(0, K, N)
        c[rng.permutation(N)[:N // 2]] = 3 % K
    elif pattern == "dual":
        c = np.repeat(rng.integers(0, K, (N + 3) // 4), 4)[:N]
    else:
        raise ValueError(pattern)
    c = c.astype(np.int64)
    c[::53] = -1                                                  # every 53rd code is -1, every 97th is K: both ignored
    c[::97] = K
    return c


@functools.lru_cache(maxsize=None)
def case_inputs(i):
    """(v [N, D] float32, codes [N] int64) of case i, values spread over a few binades so that the order of additions shows"""
    N, D, K, pattern = CASES[i]
    rng = np.random.default_rng(1000 + i)
    v = (rng.standard_normal((N, D)) * np.exp2(rng.integers(-3, 4, (N, 1)))).astype(np.float32)
    return v, make_codes(N, K, pattern, 2000 + i)


def narrow(v, dtype):
    """float32 values rounded to a torch 16-bit dtype and widened again (exact): what the kernel sums for such latents"""
    import torch
    return torch.from_numpy(v).to(dtype).to(torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def case_reference(i, dtype_name):
    import torch
    v, codes = case_inputs(i)
    if dtype_name != "float32":
        v = narrow(v, getattr(torch, dtype_name))
    return det_sums(v, codes, CASES[i][2])
