"""numpy / float64 restatement of what csrc/code_stats.hip computes (flat and grain form) and of EMAVectorQuantizer's EMA
step, plus the seeded cases tools/gen_golden_taming.py and tests/test_taming.py share.  TEST INFRASTRUCTURE ONLY.

Perplexity, the kernel's recipe (include/dvq.h, dvq_code_stats_f32): p_j = fl32(count_j) / fl32(n), t_j = fl32(p_j * fl32(log(
fl32(p_j + 1e-10)))), H = sum of the t_j, perplexity = exp(-H).  `perplexity_f32` keeps the fp32 roundings of p and t and sums
in float64; `perplexity_f64` is the same statistic in real arithmetic (float64 throughout) -- the two agree to a few 1e-7, far
inside the 1e-5 the tests allow against either."""
import zlib

import numpy as np

from dynamicvectorquantization_amd import synth

GOLDEN_FILE = "taming_%s.npz"
BETA = 0.25
DECAY, EPS = 0.99, 1e-5

# name -> (B, D, H, W, K): the class cases.  a: one 128-token block of the wide kernel; b: N % 128 != 0 and HW % 4 != 0 (the EMA
# accumulate's fallback form), D = 64; n: the narrow path at the codebook size taming-style VectorQuantizer(16384, 4) models use
CASES = {"a": (2, 256, 8, 8, 1024), "b": (3, 64, 5, 7, 96), "n": (2, 4, 3, 5, 16384)}
SEQ = (2, 64, 37, 96)                        # VectorQuantizer2Seq: B, D, L, K


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def case_inputs(name):
    """-> z [B, D, H, W], E [K, D] (trained-like), gw [B, D, H, W] (the weight of z_q in the scalar that is back-propagated),
    cs0 [K] (positive cluster sizes the EMA cases start from)"""
    B, D, H, W, K = CASES[name]
    seed = 8100 + 10 * sorted(CASES).index(name)
    E = synth.codebook_trained(K, D, seed=seed)
    z = synth.z_tokens(E, B, H, W, seed + 1)
    gw = synth.normal(seed + 2, z.shape)
    cs0 = synth.uniform(seed + 3, (K,), 0.5, 4.0)
    return z, E, gw, cs0


def seq_inputs():
    B, D, L, K = SEQ
    E = synth.codebook_default_init(K, D, seed=8190)
    z = (synth.z_tokens(synth.codebook_trained(K, D, seed=8191), B, 1, L, 8192) * np.float32(0.002)).reshape(B, D, L)
    return z, E


def rows_of(z):
    """[B, D, *spatial] -> token rows [N, D], the reference's 'b c h w -> (b h w) c'"""
    B, D = z.shape[:2]
    return np.ascontiguousarray(np.moveaxis(z.reshape(B, D, -1), 1, 2)).reshape(-1, D)


def onehot(codes, K):
    codes = np.asarray(codes, np.int64).reshape(-1)
    out = np.zeros((codes.size, K), np.float32)
    ok = (codes >= 0) & (codes < K)
    out[np.nonzero(ok)[0], codes[ok]] = 1.0
    return out


def _perplexity(counts, n, f32):
    counts = np.asarray(counts, np.int64)
    if n == 0:
        return 1.0
    if f32:
        p = counts.astype(np.float32) / np.float32(n)
        t = p * np.log((p + np.float32(1e-10)).astype(np.float32)).astype(np.float32)
        return float(np.exp(-np.sum(t.astype(np.float32).astype(np.float64))))
    p = counts.astype(np.float64) / float(n)
    return float(np.exp(-np.sum(p * np.log(p + 1e-10))))


def flat_stats(codes, K):
    """-> dict(counts [K] int64, n_used, n_tokens, perplexity (float64 statistic), perplexity_f32 (the kernel's roundings))"""
    codes = np.asarray(codes, np.int64).reshape(-1)
    ok = (codes >= 0) & (codes < K)
    counts = np.bincount(codes[ok], minlength=K).astype(np.int64)
    n = codes.size
    return dict(counts=counts, n_used=int((counts > 0).sum()) if n else 0, n_tokens=n,
                perplexity=_perplexity(counts, n, False), perplexity_f32=_perplexity(counts, n, True))


def grain_stats(codes, grain, G, K):
    """codes [B, H, W], grain [B, hc, wc] -> dict(counts [G, K], n_tokens [G], n_used [G], perplexity [G], perplexity_f32 [G]):
    position (y, x) counts iff y % s == 0 and x % s == 0 with s = (H / hc) >> g, g the grain of its cell; cells with a grain
    outside [0, G) are ignored; written as plain loops on purpose"""
    codes, grain = np.asarray(codes, np.int64), np.asarray(grain, np.int64)
    B, H, W = codes.shape
    hc, wc = grain.shape[1:]
    S = H // hc
    assert H == hc * S and W == wc * S and S == 1 << (G - 1)
    counts = np.zeros((G, K), np.int64)
    n_tokens = np.zeros(G, np.int64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                g = int(grain[b, y // S, x // S])
                if not 0 <= g < G:
                    continue
                s = S >> g
                if y % s or x % s:
                    continue
                n_tokens[g] += 1
                c = int(codes[b, y, x])
                if 0 <= c < K:
                    counts[g, c] += 1
    return dict(counts=counts, n_tokens=n_tokens,
                n_used=np.array([(counts[g] > 0).sum() if n_tokens[g] else 0 for g in range(G)], np.int64),
                perplexity=np.array([_perplexity(counts[g], int(n_tokens[g]), False) for g in range(G)]),
                perplexity_f32=np.array([_perplexity(counts[g], int(n_tokens[g]), True) for g in range(G)]))


def ema_step(z, codes, cluster_size, embed_avg, decay=DECAY, eps=EPS):
    """one EMAVectorQuantizer training update in float64 (quantize_vqgan.py:438-446 with EmbeddingEMA's three methods):
    -> (cluster_size', embed_avg', weight')"""
    rows = rows_of(z).astype(np.float64)
    codes = np.asarray(codes, np.int64).reshape(-1)
    K, D = embed_avg.shape
    counts = np.bincount(codes, minlength=K).astype(np.float64)
    sums = np.zeros((K, D))
    np.add.at(sums, codes, rows)
    cs = np.asarray(cluster_size, np.float64) * decay + (1.0 - decay) * counts
    avg = np.asarray(embed_avg, np.float64) * decay + (1.0 - decay) * sums
    n = cs.sum()
    smoothed = (cs + eps) / (n + K * eps) * n
    return cs, avg, avg / smoothed[:, None]


def zipf_codes(seed, N, K, a=1.1):
    """a skewed draw: P(j) ~ (j + 1)^-a by inversion of the cumulative weights"""
    w = np.arange(1, K + 1, dtype=np.float64) ** -a
    cdf = np.cumsum(w) / w.sum()
    u = synth.uniform(seed, (N,)).astype(np.float64)
    return np.minimum(np.searchsorted(cdf, u), K - 1).astype(np.int64)


def flat_cases():
    """name -> (codes [N] int64, K): the flat kernel's cases"""
    out = {}
    for N, K in ((1, 1), (257, 5), (1024, 1024), (4099, 16384), (3000, 40000), (513, 1023)):
        out["%dx%d" % (N, K)] = (synth.randint(8300 + K % 97, (N,), K), K)
    out["all_equal"] = (np.full(4096, 777, np.int64), 1024)
    out["zipf"] = (zipf_codes(8350, 65536, 1024), 1024)
    c = synth.randint(8360, (1000,), 64)
    c[::7] = -1
    c[3::11] = 64
    c[5] = 1 << 40
    out["out_of_range"] = (c, 64)
    out["empty"] = (np.zeros(0, np.int64), 33)
    return out


def grain_map(seed, B, hc, wc, G, probs=None):
    u = synth.uniform(seed, (B, hc, wc))
    probs = probs or [1.0 / G] * G
    edges = np.cumsum(probs)
    return np.minimum(np.searchsorted(edges, u, side="right"), G - 1).astype(np.int64)
