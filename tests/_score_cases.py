"""Case tables, seeded inputs and the rules of comparison for the scored / sampled assign (csrc/vq_sample.hip) and the Gumbel sweep
(csrc/vq_gumbel.hip) away from the shapes of their golden fixtures.  Shared by the CPU checks (tests/test_score_cases.py) and the GPU
tests (tests/test_score_assign_shapes.py, tests/test_gumbel_shapes.py); everything here is numpy, torch on the CPU and the oracle.

Scores.  The kernels' MFMA chain is the oracle's sequential-k fmaf chain bit for bit, so the fp32 score of every metric is
reproduced on the CPU:  L2  s = -d, d = oracle.token_distances;  CDIST  s = -sqrt(d < 0 ? 0 : d) (_lucid_ref.cdist_scores);
DOT  s = oracle.token_dots;  Gumbel logit  l = fl(oracle.token_dots(z, W) + b).

Scored assign, rules.  Without noise the codes equal `argmax_torch` of those scores on every token, ties and NaN included.  With
noise the code is argmax fl(fl(s / temp) + g(u)); the division is IEEE on both sides, only g (two logf) differs between two correct
implementations.  The rule is tests/_maskvq_ref.py's: a token may differ only where the float64 top-2 gap of fp32(s / temp) + g64(u)
is below 4 G + ulp32(best), with G = max(_maskvq_ref.G_ERR, the largest |fp32 torch CPU chain of g - float64 chain| over the case's
OWN u) -- the special uniforms of the noise-edge cases (u == 1.0: g = 46.05, half an ulp there is 1.9e-6) exceed the constant that
was measured over ordinary uniforms.  At most _maskvq_ref.SKIP_CAP of a case's tokens may be in that set; a seed that violates the
cap is replaced, never excused.

Gumbel sweep, rules.  Without q the codes equal `argmax_torch` of the fp32 logits.  With q: float64 s = (l32 + g64) / tau,
g = -log q; a token may differ only where the top-2 gap is below 4 Gq / tau + 4 ulp32(best): Gq = max |fp32 torch CPU -log(q) -
float64| over the case's q for each competitor on either side, and four ulps for the add and the divide of two competitors.  Cap:
_gumbel_ref.SKIP_CAP.  KL: |kl - kl64| <= 1e-5 T, kl64 = mean_n A'/S - log S + log kl_K in float64 from the fp32 logits and
T = the float64 mean over tokens of |A'/S| + |log S| + |log kl_K| (A' = sum e^(l-m) (l-m), S = sum e^(l-m)): the project's 1e-5,
relative to the terms the kernel adds rather than to their difference, which cancels to 0 at near-uniform logits (`kl64`)."""
import collections

import numpy as np
import torch

from dynamicvectorquantization_amd import synth
from tests import _gumbel_ref as GR
from tests import _maskvq_ref as R
from tests._lucid_ref import cdist_scores, l2norm

KERNEL_WIDTHS = (64, 128, 256)
METRICS = ("l2", "dot", "cdist")
TEMPS = (1.0, 0.25)

# noise: "none" (u == nullptr), "aligned" (u as allocated: 16-byte reads when K % 4 == 0, scalar reads otherwise), "offset" (u 4 bytes
# off a 16-byte boundary: scalar reads by alignment)
ScoreCase = collections.namedtuple("ScoreCase", "name D K shape metric noise temps seed")

_seed = [8601]


def _next_seed():
    _seed[0] += 3                                   # (seed, seed + 1, seed + 2: codebook, tokens, uniforms)
    return _seed[0] - 3


def _score_table():
    every, k_edges, n_edges = [], [], []
    for D in KERNEL_WIDTHS:                         # every instantiation: NCHW [3, D, 5, 7], HW = 35: a wave straddles images
        for metric in METRICS:
            for K, noise in ((100, "none"), (100, "aligned"), (33, "aligned"), (100, "offset")):
                if metric == "cdist" and noise == "none":
                    continue                        # the cdist entry point requires u (temp == 0 is the plain assign)
                every.append(ScoreCase("every-D%d-%s-K%d-%s" % (D, metric, K, noise), D, K, (3, D, 5, 7), metric, noise,
                                       () if noise == "none" else TEMPS, _next_seed()))
    for metric in METRICS:                          # K edges: K <= 4 leaves lane half 1 without a code, K % 32 in 1..4 a last tile
        for K in (1, 3, 4, 5, 8, 31, 32, 33, 64, 65):   # with codes in half 0 only, K % 4 != 0 reads u scalar
            for noise in ("none", "aligned"):
                if metric == "cdist" and noise == "none":
                    continue
                k_edges.append(ScoreCase("k-%s-K%d-%s" % (metric, K, noise), 64, K, (33, 64), metric, noise,
                                         () if noise == "none" else TEMPS, _next_seed()))
    shapes = [(N, 128) for N in (1, 31, 32, 127, 128, 129)] + [(2, 128, 1, 1), (5, 128, 3, 3), (1, 128, 13, 11)]
    for shape in shapes:                            # N edges: one token, partial / full waves and workgroups, HW == 1 with four dims
        for noise in ("none", "aligned"):
            n_edges.append(ScoreCase("n-%s-%s" % ("x".join(map(str, shape)), noise), 128, 36, shape, "l2", noise,
                                     () if noise == "none" else (1.0,), _next_seed()))
    return tuple(every), tuple(k_edges), tuple(n_edges)


EVERY, K_EDGES, N_EDGES = _score_table()
DUPLICATE = (6, 25)                                 # noise-edge case: codebook row 25 (lane half 0) is a copy of row 6 (half 1), u too
TIE_TOKENS = [2, 8, 11, 14, 17, 20]                 # (rows n % 3 == 2: no 1.0 and no 1 - 2^-24 among their uniforms)
NOISE_EDGE = ScoreCase("noise-edges", 64, 40, (48, 64), "l2", "aligned", (0.05, 1.0, 20.0), _next_seed())
SCORE_CASES = EVERY + K_EDGES + N_EDGES + (NOISE_EDGE,)
BY_NAME = {c.name: c for c in SCORE_CASES}
assert len(BY_NAME) == len(SCORE_CASES)

_CACHE = {}


def cached(key, make):
    """computed once, shared by the tests that need it and never written to afterwards"""
    if key not in _CACHE:
        val = make()
        for a in (val.values() if isinstance(val, dict) else [val]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def ntokens(shape):
    return int(shape[0] * np.prod(shape[2:], dtype=np.int64))


def to_layout(rows, shape):
    """token rows [N, D] -> the tensor of `shape` ([N, D] itself, or NCHW [B, D, *spatial]) that holds them"""
    if len(shape) == 2:
        return np.ascontiguousarray(rows)
    B, D = shape[:2]
    return np.ascontiguousarray(rows.reshape(B, -1, D).transpose(0, 2, 1)).reshape(shape)


def to_rows(x):
    """the inverse of to_layout"""
    if x.ndim == 2:
        return np.ascontiguousarray(x)
    B, D = x.shape[:2]
    return np.ascontiguousarray(x.reshape(B, D, -1).transpose(0, 2, 1)).reshape(-1, D)


def kernel_form(case):
    """(D, METRIC, NOISE, VEC) of the vq_score_assign_kernel instantiation the launcher picks for this case
    (dvq_launch_score_assign: vec = K % 4 == 0 and u 16-byte aligned)"""
    if case.noise == "none":
        return (case.D, case.metric, False, False)
    return (case.D, case.metric, True, case.noise == "aligned" and case.K % 4 == 0)


def scores32(oracle, rows, E, metric):
    """the kernel's fp32 scores [N, K], bit for bit"""
    if metric == "dot":
        return np.stack([oracle.token_dots(r, E) for r in rows])
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.stack([oracle.token_distances(r, E) for r in rows])
    return -d if metric == "l2" else cdist_scores(d)


def g_err(u):
    """the G of the skip rule for the uniforms u: the reference's own fp32 chain on the CPU against the float64 chain"""
    t = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32))
    g32 = -torch.log((-torch.log(t.clamp(min=1e-20))).clamp(min=1e-20))
    return max(R.G_ERR, float(np.abs(g32.numpy().astype(np.float64) - R.gumbel64(u)).max()))


def skip_sampled(s, temp, u, G):
    """_maskvq_ref.skip_sampled with the case's own G: bool [N], tokens whose sampled code may differ"""
    if np.shape(s)[-1] == 1:
        return np.zeros(np.shape(s)[0], bool)        # one code: nothing to flip to
    with np.errstate(invalid="ignore", over="ignore"):
        best, gap = R.top2(R.perturbed(s, temp, u))
        thr = 4.0 * G + np.spacing(np.abs(best).astype(np.float32)).astype(np.float64)
        return gap < thr


def sampled_codes(s, temp, u):
    with np.errstate(invalid="ignore", over="ignore"):
        return R.argmax_torch(R.perturbed(s, temp, u))


def noise_edge_u(N, K, seed):
    """ordinary uniforms with the special values of the noise's clamps among them, at rotating columns: 0, a subnormal, 1e-20 and
    1e-10 in every row (g = -3.8 .. -3.1: they lose), exactly 1.0 in rows n % 3 == 0 (a = 0 clamps to 1e-20, g = 46.05: it wins at
    temp >= 1), 1 - 2^-24 in rows n % 3 == 1 (g = 16.6), neither in rows n % 3 == 2; row 5 constant"""
    u = synth.uniform(seed, (N, K)).copy()
    cols = [k for k in range(K) if k not in DUPLICATE]           # (the duplicated pair's columns are made equal afterwards)
    for n in range(N):
        special = [0.0, 1e-42, 1e-20, 1e-10] + [[1.0], [1.0 - 2.0 ** -24], []][n % 3]
        for i, v in enumerate(special):
            u[n, cols[(7 * n + 5 * i) % len(cols)]] = np.float32(v)      # (5 i distinct for i < 6)
    u[5] = np.float32(0.37)
    return u


def score_inputs(case, oracle):
    """dict: E [K, D], rows [N, D], x (the case's layout), u [N, K] or None, s [N, K] fp32 scores, G, and per temp
    want / skip"""
    def make():
        E = synth.codebook_trained(case.K, case.D, seed=case.seed).copy()
        N = ntokens(case.shape)
        rows = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, case.seed + 1)[0, :, :, 0].T)
        u = None
        if case.noise != "none":
            u = noise_edge_u(N, case.K, case.seed + 2) if case is NOISE_EDGE else synth.uniform(case.seed + 2, (N, case.K))
        if case is NOISE_EDGE:
            first, second = DUPLICATE
            E[second] = E[first]                    # a duplicated row (tile 0, the other lane half) with equal noise: the first wins
            u[:, second] = u[:, first]
            rows[TIE_TOKENS] = E[first] + np.float32(0.05) * rows[TIE_TOKENS]     # tokens next to the duplicated row ...
            u[TIE_TOKENS, first] = u[TIE_TOKENS, second] = np.float32(0.995)       # ... whose noise favours the pair at every temp
        if case.metric == "dot":
            rows, E = l2norm(rows), l2norm(E)
        out = {"E": E, "rows": rows, "x": to_layout(rows, case.shape), "u": u, "s": scores32(oracle, rows, E, case.metric)}
        out["hard"] = R.argmax_torch(out["s"])
        if u is not None:
            out["G"] = g_err(u)
            # the duplicate's perturbed score is the same bits as the first's in any implementation (same inputs, same operations):
            # an exact tie that the first index wins, not a near tie -- the gap is taken without that column
            cols = np.arange(case.K) != DUPLICATE[1] if case is NOISE_EDGE else np.ones(case.K, bool)
            for temp in case.temps:
                out["want", temp] = sampled_codes(out["s"], temp, u)
                out["skip", temp] = skip_sampled(out["s"][:, cols], temp, u[:, cols], out["G"])
        return out
    return cached(("score", case.name), make)


SPECIAL_TEMPS = (1.0, 20.0)
SPECIAL_BOOKS = ("plain", "nan_one", "nan_three", "inf_row", "all_inf")
SPECIAL_NAN_ROWS = (23, 36, 9)                      # tile 0 half 1, tile 1, tile 0 half 0: the first NaN is 9
SPECIAL_INF_ROW, SPECIAL_INF_CHANNEL = 7, 2
SPECIAL_ORDINARY = 3                                # tokens from here on are ordinary, with a negative channel SPECIAL_INF_CHANNEL


def special_inputs(metric, oracle):
    """D = 64, K = 40, 12 token rows against five codebooks, with noise.  Token 0 holds a NaN (every score NaN: code 0), token 1
    is zero, token 2 equals codebook row `J`, chosen so that the oracle's distance of that row to itself is NEGATIVE (the CDIST
    score clamps it; a NaN there would win) and given u = 1e-10 at J so that J loses at temp 20; the others are ordinary with
    channel 2 negative, so that a codebook row with +inf there has the dot -inf and the score -inf under every metric.
    -> dict: rows, u, J, G and per book: E, s, hard, (want, temp), (skip, temp)"""
    def make():
        D, K, N, seed = 64, 40, 12, 8590
        E0 = synth.codebook_trained(K, D, seed=seed).copy()
        rows = np.ascontiguousarray(synth.z_tokens(E0, 1, N, 1, seed + 1)[0, :, :, 0].T)
        u = synth.uniform(seed + 2, (N, K)).copy()
        self_d = np.array([oracle.token_distances(E0[j], E0)[j] for j in range(K)])
        J = int(np.argmax(self_d < 0))
        rows[0, 5] = np.nan
        rows[1] = 0.0
        rows[2] = E0[J]
        u[2, J] = np.float32(1e-10)
        c = SPECIAL_INF_CHANNEL
        rows[SPECIAL_ORDINARY:, c] = -np.abs(rows[SPECIAL_ORDINARY:, c]) - np.float32(0.1)
        out = {"rows": rows, "u": u, "J": J, "self_d": self_d, "G": g_err(u)}
        for book in SPECIAL_BOOKS:
            E = E0.copy()
            if book == "nan_one":
                E[SPECIAL_NAN_ROWS[1], 1] = np.nan
            elif book == "nan_three":
                for j in SPECIAL_NAN_ROWS:
                    E[j, j % D] = np.nan
            elif book == "inf_row":
                E[SPECIAL_INF_ROW, c] = np.inf
            elif book == "all_inf":
                E[:, c] = np.inf
            s = scores32(oracle, rows, E, metric)
            out[book, "E"], out[book, "s"], out[book, "hard"] = E, s, R.argmax_torch(s)
            for temp in SPECIAL_TEMPS:
                out[book, "want", temp] = sampled_codes(s, temp, u)
                out[book, "skip", temp] = skip_sampled(s, temp, u, out["G"])
        return out
    return cached(("special", metric), make)


PADDED_WIDTHS = (32, 96, 160, 224)


def padded_inputs(D, oracle):
    """a width served by zero padding: K = 36, 70 tokens; E, rows, u, their zero-padded copies Ep, rp at the next kernel width and,
    per metric, the scores at that width with hard and (want, temp), (skip, temp) for TEMPS"""
    def make():
        K, N, seed = 36, 70, 8500 + D
        Dp = min(w for w in KERNEL_WIDTHS if w >= D)
        E = synth.codebook_trained(K, D, seed=seed)
        rows = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, seed + 1)[0, :, :, 0].T)
        u = synth.uniform(seed + 2, (N, K))
        Ep, rp = np.zeros((K, Dp), np.float32), np.zeros((N, Dp), np.float32)
        Ep[:, :D], rp[:, :D] = E, rows
        out = {"E": E, "rows": rows, "u": u, "Ep": Ep, "rp": rp, "G": g_err(u)}
        for metric in METRICS:
            sc = scores32(oracle, rp, Ep, metric)
            out[metric, "hard"] = R.argmax_torch(sc)
            for temp in TEMPS:
                out[metric, "want", temp] = sampled_codes(sc, temp, u)
                out[metric, "skip", temp] = skip_sampled(sc, temp, u, out["G"])
        return out
    return cached(("padded", D), make)


# ---- the Gumbel sweep ---------------------------------------------------------------------------------------------------------------

# bias: "normal" 0.5 N(0, 1); "ramp_up" + 0.75 k; "ramp_down" + 0.75 (K - 1 - k); "inf40" -inf on codes 0..39; "one" -inf on all
# codes but ONE_CODE; "allinf" -inf everywhere.  wstd: the logits' standard deviation.  kl_K None: K.  e_offset: embed 4 bytes off
GumbelCase = collections.namedtuple("GumbelCase", "name C K shape d noise tau bias wstd kl_K e_offset seed")
ONE_CODE = 77


def _gcase(name, C, K, shape, d, noise, seed, tau=1.0, bias="normal", wstd=1.5, kl_K=None, e_offset=False):
    return GumbelCase(name, C, K, shape, d, noise, tau, bias, wstd, kl_K, e_offset, seed)


def _gumbel_table():
    widths, ds, n_edges, stress = [], [], [], []
    seed = 9201
    for C in KERNEL_WIDTHS:                         # widths and small K (K <= 4: a lane half without a code), KL wanted
        for noise in (False, True):
            for i, K in enumerate((1, 3, 4, 5, 32, 33, 100)):
                widths.append(_gcase("w-C%d-K%d-%s" % (C, K, "q" if noise else "noq"), C, K, (3, C, 5, 7), (1, 8, 12, 16)[i % 4],
                                     noise, seed, tau=(1.0, 0.5)[i % 2]))
                seed += 1
    for d, off in ((1, False), (8, False), (12, False), (16, False), (8, True)):     # the z_q epilogues; d = 8 off alignment: scalar
        ds.append(_gcase("d%d%s" % (d, "-offset" if off else ""), 64, 33, (3, 64, 5, 7), d, True, seed, e_offset=off))
        seed += 1
    for shape, C, K in (((1, 128), 128, 36), ((129, 128), 128, 36), ((5, 128, 3, 3), 128, 36), ((128 * 257 + 1, 64), 64, 8)):
        n_edges.append(_gcase("n-%s" % "x".join(map(str, shape)), C, K, shape, 8, True, seed))
        seed += 1
    for name, kw in (("ramp_up", dict(bias="ramp_up")), ("ramp_down", dict(bias="ramp_down")), ("std30", dict(wstd=30.0)),
                     ("inf40", dict(bias="inf40")), ("one", dict(bias="one")), ("allinf", dict(bias="allinf")),
                     ("klK1", dict(bias="ramp_up", kl_K=1.0)), ("klK1000.5", dict(kl_K=1000.5))):
        stress.append(_gcase("kl-" + name, 64, 160, (3, 64, 5, 7), 16, True, seed, **kw))
        seed += 1
    return tuple(widths), tuple(ds), tuple(n_edges), tuple(stress)


G_WIDTHS, G_DS, G_N_EDGES, G_STRESS = _gumbel_table()
GUMBEL_CASES = G_WIDTHS + G_DS + G_N_EDGES + G_STRESS
G_BY_NAME = {c.name: c for c in GUMBEL_CASES}
assert len(G_BY_NAME) == len(GUMBEL_CASES)


def gumbel_bias(case, rng):
    K = case.K
    b = (0.5 * rng.standard_normal(K)).astype(np.float32)
    k = np.arange(K, dtype=np.float32)
    if case.bias == "ramp_up":
        b = b + np.float32(0.75) * k
    elif case.bias == "ramp_down":
        b = b + np.float32(0.75) * (np.float32(K - 1) - k)
    elif case.bias == "inf40":
        b[:40] = -np.inf
    elif case.bias == "one":
        keep = b[ONE_CODE]
        b[:] = -np.inf
        b[ONE_CODE] = keep
    elif case.bias == "allinf":
        b[:] = -np.inf
    else:
        assert case.bias == "normal"
    return b.astype(np.float32)


def kl64(l32, kl_K):
    """(kl, T, kl_ref) from the fp32 logits [N, K], in float64.  kl = mean_n A'/S - log S + log kl_K: sum_k p log(p kl_K) in the
    form whose terms T = mean_n |A'/S| + |log S| + |log kl_K| measures (m the row maximum, S = sum e^(l-m), A' = sum e^(l-m) (l-m),
    a term with e^(l-m) == 0 is 0).  kl_ref = the reference's expression, mean_n sum_k p log(p kl_K + 1e-10): the 1e-10 moves the
    value by at most 1e-10 K / kl_K (csrc/vq_gumbel.hip derives it; tests/test_score_cases.py asserts it for every case)"""
    l = np.asarray(l32, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = l.max(axis=1, keepdims=True)
        x = l - m
        e = np.exp(x)
        S = e.sum(axis=1)
        p = e / S[:, None]
        kl_ref = float(np.sum(p * np.log(p * float(kl_K) + 1e-10), axis=1).mean())
        A = np.where(e != 0.0, e * x, 0.0).sum(axis=1)
        A = np.where(np.isnan(e).any(axis=1), np.nan, A)
        kl = float((A / S - np.log(S) + np.log(float(kl_K))).mean())
        T = float((np.abs(A / S) + np.abs(np.log(S)) + abs(np.log(float(kl_K)))).mean())
    return kl, T, kl_ref


def kl32_chain_error(l32, kl_K, want):
    """|the reference's own fp32 torch chain on the CPU (softmax, log, sum, mean) - the float64 value|"""
    lt = torch.from_numpy(np.ascontiguousarray(l32, dtype=np.float32))
    p = lt.softmax(dim=1)
    got = float(torch.sum(p * torch.log(p * float(kl_K) + 1e-10), dim=1).mean())
    return abs(got - want)


def gumbel_inputs(case, oracle):
    """dict: z (the case's layout), W [K, C], b [K], E [K, d], q (the logits' layout [B, K, *spatial]) or None, l32 [N, K],
    hard / want / skip [N], Gq, kl, T, kl_K"""
    def make():
        rng = np.random.default_rng(case.seed)
        N = ntokens(case.shape)
        z = rng.standard_normal(case.shape).astype(np.float32)
        W = (rng.standard_normal((case.K, case.C)) * (case.wstd / np.sqrt(case.C))).astype(np.float32)
        b = gumbel_bias(case, rng)
        E = rng.standard_normal((case.K, case.d)).astype(np.float32)
        rows = to_rows(z)
        with np.errstate(invalid="ignore"):
            l32 = (np.stack([oracle.token_dots(r, W) for r in rows]) + b[None, :]).astype(np.float32)
        kl_K = float(case.K if case.kl_K is None else case.kl_K)
        kl, T, kl_ref = kl64(l32, kl_K)
        out = {"z": z, "W": W, "b": b, "E": E, "q": None, "l32": l32, "hard": R.argmax_torch(l32), "kl": kl, "T": T, "kl_K": kl_K,
               "kl_ref": kl_ref}
        if case.noise:
            qrows = np.maximum(rng.standard_exponential((N, case.K)).astype(np.float32), np.float32(1e-30))
            out["q"] = to_layout(qrows, (case.shape[0], case.K) + tuple(case.shape[2:]))
            q64 = qrows.astype(np.float64)
            out["Gq"] = float(np.abs((-torch.log(torch.from_numpy(qrows))).numpy().astype(np.float64) + np.log(q64)).max())
            with np.errstate(invalid="ignore", over="ignore"):
                s = (l32.astype(np.float64) - np.log(q64)) / float(case.tau)
                out["want"] = R.argmax_torch(s)
                if case.K == 1:
                    out["skip"] = np.zeros(N, bool)
                else:
                    best, gap = R.top2(s)
                    thr = 4.0 * out["Gq"] / float(case.tau) + 4.0 * np.spacing(np.abs(best).astype(np.float32)).astype(np.float64)
                    out["skip"] = gap < thr
        return out
    return cached(("gumbel", case.name), make)


SKIP_CAP = R.SKIP_CAP
GUMBEL_SKIP_CAP = GR.SKIP_CAP
