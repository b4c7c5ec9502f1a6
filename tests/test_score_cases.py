"""CPU checks behind tests/test_score_assign_shapes.py and tests/test_gumbel_shapes.py: the oracle's dot chain, what the case
tables of tests/_score_cases.py reach, and that the references alone stay within the skip caps (a seed that does not is replaced)."""
import numpy as np
import pytest

from dynamicvectorquantization_amd import synth
from tests import _score_cases as C

GROUPS = {"every": C.EVERY, "k_edges": C.K_EDGES, "n_edges": C.N_EDGES, "noise_edge": (C.NOISE_EDGE,)}
G_GROUPS = {"widths": C.G_WIDTHS, "d": C.G_DS, "n_edges": C.G_N_EDGES, "stress": C.G_STRESS}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("D", (64, 96, 128, 256))
def test_token_dots_is_the_chain_of_the_distances(D, oracle_mod):
    """token_distances == fl(fl(xn + en) - 2 token_dots) bit for bit (2 dot is exact, so the fused and the unfused form round
    once alike), and the chain's dot within D 2^-24 sum |x_k e_k| of the float64 dot"""
    K, N = 70, 9
    E = synth.codebook_trained(K, D, seed=8581)
    rows = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, 8582)[0, :, :, 0].T)
    en = oracle_mod.codebook_norms(E)
    xn = oracle_mod.sumsq_rows(rows)
    for n in range(N):
        dots = oracle_mod.token_dots(rows[n], E)
        assert dots.dtype == np.float32 and dots.shape == (K,)
        want = ((xn[n] + en).astype(np.float32) - np.float32(2.0) * dots).astype(np.float32)
        assert np.array_equal(_bits(oracle_mod.token_distances(rows[n], E)), _bits(want))
        exact = E.astype(np.float64) @ rows[n].astype(np.float64)
        mag = np.abs(E.astype(np.float64)) @ np.abs(rows[n].astype(np.float64))
        assert (np.abs(dots.astype(np.float64) - exact) <= D * 2.0 ** -24 * mag).all()
    z = np.zeros(D, np.float32)
    assert not oracle_mod.token_dots(z, E).any()
    e1 = np.zeros(D, np.float32)
    e1[D - 1] = 1.0                                                # the last channel is read
    assert np.array_equal(oracle_mod.token_dots(e1, E), E[:, D - 1])


def test_score_tables_reach_every_instantiation():
    """the launcher's choice restated for every case: all 24 reachable vq_score_assign_kernel<D, METRIC, NOISE, VEC> of the 27
    (the three <D, CDIST, false, false> are instantiated by launch_score but the cdist entry point requires u), and the
    shapes the docstrings promise"""
    forms = {C.kernel_form(c) for c in C.SCORE_CASES}
    want = {(D, m, n, v) for D in C.KERNEL_WIDTHS for m in C.METRICS for (n, v) in ((False, False), (True, True), (True, False))}
    want -= {(D, "cdist", False, False) for D in C.KERNEL_WIDTHS}
    assert forms == want and len(want) == 24
    assert {C.kernel_form(c) for c in C.EVERY} == want             # the first table alone reaches them
    for c in C.EVERY:
        assert C.ntokens(c.shape) == 105 and c.shape[2] * c.shape[3] == 35
        assert (c.K % 32 == 4) if c.K == 100 else (c.K % 32 == 1 and c.K % 4 != 0)     # a last tile with codes in half 0 only
    assert {c.K for c in C.K_EDGES} == {1, 3, 4, 5, 8, 31, 32, 33, 64, 65}
    assert {C.ntokens(c.shape) for c in C.N_EDGES} == {1, 2, 31, 32, 45, 127, 128, 129, 143}
    assert {(c.C, c.noise) for c in C.GUMBEL_CASES} == {(w, n) for w in C.KERNEL_WIDTHS for n in (False, True)}
    assert {c.K for c in C.G_WIDTHS} == {1, 3, 4, 5, 32, 33, 100} and {c.d for c in C.G_WIDTHS + C.G_DS} == {1, 8, 12, 16}
    assert max(C.ntokens(c.shape) for c in C.G_N_EDGES) > 256 * 128      # more than 256 KL partials
    assert len({c.seed for c in C.SCORE_CASES}) == len(C.SCORE_CASES) and len({c.seed for c in C.GUMBEL_CASES}) == len(C.GUMBEL_CASES)


@pytest.mark.parametrize("group", list(GROUPS))
def test_score_cases_stay_within_the_skip_cap(group, oracle_mod):
    worst_g, total = 0.0, 0
    for c in GROUPS[group]:
        inp = C.score_inputs(c, oracle_mod)
        assert inp["s"].shape == (C.ntokens(c.shape), c.K) and inp["x"].shape == c.shape
        assert np.isfinite(inp["s"]).all()
        if c.noise == "none":
            continue
        worst_g = max(worst_g, inp["G"])
        for temp in c.temps:
            skip = inp["skip", temp]
            total += int(skip.sum())
            assert skip.mean() <= C.SKIP_CAP, (c.name, temp, int(skip.sum()))
    print("%s: %d cases, %d tokens in skip sets, largest G %.3g" % (group, len(GROUPS[group]), total, worst_g))
    if group != "noise_edge":
        assert worst_g == C.R.G_ERR                                # ordinary uniforms stay under the measured constant


def test_noise_edge_case_holds_what_it_claims(oracle_mod):
    c = C.NOISE_EDGE
    inp = C.score_inputs(c, oracle_mod)
    u = inp["u"]
    first, second = C.DUPLICATE
    other = np.arange(len(u)) != 5
    for v in (0.0, 1e-42, 1e-20, 1e-10):
        assert (u == np.float32(v)).any(axis=1)[other].all()
    has_one, has_below = (u == np.float32(1.0)).any(axis=1), (u == np.float32(1.0 - 2.0 ** -24)).any(axis=1)
    assert has_one[other].sum() == 16 and has_below[other].sum() == 16 and not (has_one & has_below).any()
    assert not has_one[C.TIE_TOKENS].any() and not has_below[C.TIE_TOKENS].any()
    assert (inp["want", 1.0][has_one] == np.argmax(u == np.float32(1.0), axis=1)[has_one]).all()      # g = 46.05 wins at temp 1
    assert 0 < np.float32(1e-42) < np.finfo(np.float32).tiny       # a subnormal
    assert (u[5] == u[5, 0]).all()
    assert np.array_equal(inp["E"][first], inp["E"][second]) and np.array_equal(u[:, first], u[:, second])
    assert np.array_equal(_bits(inp["s"][:, first]), _bits(inp["s"][:, second]))
    assert inp["G"] > C.R.G_ERR                                    # u == 1.0 is outside what the constant was measured over
    won = [int((inp["want", t] == first).sum()) for t in c.temps]
    assert min(won) >= 1 and all(not (inp["want", t] == second).any() for t in c.temps)      # the tie is decided, for the first
    codes = {t: inp["want", t] for t in c.temps}
    assert not np.array_equal(codes[0.05], codes[20.0])            # the temperatures matter


@pytest.mark.parametrize("D", C.PADDED_WIDTHS)
def test_padded_width_cases_stay_within_the_skip_cap(D, oracle_mod):
    inp = C.padded_inputs(D, oracle_mod)
    for metric in C.METRICS:
        for temp in C.TEMPS:
            assert inp[metric, "skip", temp].mean() <= C.SKIP_CAP
    if D == 96:                                                    # zero channels change no bit of a score
        for metric in C.METRICS:
            assert np.array_equal(_bits(C.scores32(oracle_mod, inp["rows"], inp["E"], metric)),
                                  _bits(C.scores32(oracle_mod, inp["rp"], inp["Ep"], metric)))


@pytest.mark.parametrize("metric", C.METRICS)
def test_special_score_restatement(metric, oracle_mod):
    """what the special inputs must give, from the restatement alone"""
    sp = C.special_inputs(metric, oracle_mod)
    J, o = sp["J"], C.SPECIAL_ORDINARY
    assert sp["self_d"][J] < 0                                     # the clamp of the CDIST score is exercised
    for temp in C.SPECIAL_TEMPS:
        for book in C.SPECIAL_BOOKS:
            assert not sp[book, "skip", temp].any()
            assert sp[book, "want", temp][0] == 0                  # the all-NaN token
        assert (sp["nan_one", "want", temp][1:] == C.SPECIAL_NAN_ROWS[1]).all()
        assert (sp["nan_three", "want", temp][1:] == min(C.SPECIAL_NAN_ROWS)).all()
        assert np.isneginf(sp["inf_row", "s"][o:, C.SPECIAL_INF_ROW]).all()
        assert not (sp["inf_row", "want", temp][o:] == C.SPECIAL_INF_ROW).any()
        assert np.isneginf(sp["all_inf", "s"][o:]).all() and not sp["all_inf", "want", temp][o:].any()
    if metric == "cdist":
        s = sp["plain", "s"]
        assert np.isfinite(s[1:]).all() and s[2, J] == 0           # the zero token and the clamped self distance: no NaN
        assert sp["plain", "want", 20.0][2] != J                   # ... and a NaN there would have won


@pytest.mark.parametrize("group", list(G_GROUPS))
def test_gumbel_cases_stay_within_the_skip_cap(group, oracle_mod):
    worst, total = 0.0, 0
    for c in G_GROUPS[group]:
        inp = C.gumbel_inputs(c, oracle_mod)
        N = C.ntokens(c.shape)
        assert inp["l32"].shape == (N, c.K) and inp["z"].shape == c.shape
        if c.noise:
            assert inp["q"].shape == (c.shape[0], c.K) + tuple(c.shape[2:])
            worst = max(worst, inp["Gq"])
            total += int(inp["skip"].sum())
            assert inp["skip"].mean() <= C.GUMBEL_SKIP_CAP, (c.name, int(inp["skip"].sum()))
        if c.bias == "allinf":
            assert np.isnan(inp["kl"]) and not inp["hard"].any() and not inp["want"].any()
        else:
            assert np.isfinite(inp["kl"]) and np.isfinite(inp["T"]) and (inp["T"] > 0 or (c.K == 1 and inp["kl"] == 0))
            assert abs(inp["kl"] - inp["kl_ref"]) <= 1e-10 * c.K / inp["kl_K"] + 1e-15      # the reference's 1e-10 inside the log
        if c.bias == "one":
            assert abs(inp["kl"] - np.log(inp["kl_K"])) <= 1e-14 and (inp["want"] == C.ONE_CODE).all()
        if c.bias == "inf40":
            assert (inp["want"] >= 40).all()
        if c.bias == "ramp_up":                                    # every tile raises the maximum; the early terms underflow in fp32
            l = inp["l32"]
            assert (np.diff(l.reshape(len(l), 5, 32).max(axis=2), axis=1) > 0).all()
            assert (l[:, 0] - l.max(axis=1) < -104).all()
        if c.bias == "ramp_down":
            l = inp["l32"]
            assert (np.diff(l.reshape(len(l), 5, 32).max(axis=2), axis=1) < 0).all()
        if c.wstd == 30.0:
            assert 20.0 < inp["l32"].std() < 40.0
    print("%s: %d cases, %d tokens in skip sets, largest Gq %.3g" % (group, len(G_GROUPS[group]), total, worst))
