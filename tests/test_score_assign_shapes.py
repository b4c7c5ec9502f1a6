"""The scored / sampled assign (csrc/vq_sample.hip: vq_score_assign_kernel) away from the shapes of its golden fixtures: every
reachable instantiation <D, METRIC, NOISE, VEC>, K from 1 to 65 (a lane half without a code, last tiles with codes in one half
only, scalar reads of u), N from one token to a second workgroup, NCHW against row-major, u off 16-byte alignment, the special
values of the noise's clamps, special scores, and the widths served by zero padding.  Called at kernel level: quantize.score_assign
and lucid.cdist_sample_assign with a fresh _CodebookPrep.

Tables, inputs and rules: tests/_score_cases.py (its docstring derives them); tests/test_score_cases.py checks on the CPU what the
tables reach and that the references stay within the skip cap.  Expected codes: the oracle's fp32 scores (bit for bit the
kernel's), `argmax_torch` without noise -- exact on every token -- and the float64 perturbed scores with noise, outside the skip
set of the rule (empty in every case of the tables).

What the cases see.  Mistakes that stay in bounds were tried on scratch builds.  The `code < K` guard of the running argmax
dropped (a padded code may win): every case with K % 32 != 0 under L2 and CDIST fails, and DOT at K <= 5, in all three tables,
the padded widths and the special scores.  The scalar reads of u taking the padding default for the fourth code of each run: only
the scalar forms fail (K = 33, u off alignment, K % 4 != 0 in the K table), the 16-byte forms and the noise-free ones pass.  The
merge of the lane halves taking the last index among equal scores, tried together with the previous one: the noise edges and
the special scores fail as well."""
import numpy as np
import pytest
import torch

from tests import _score_cases as C


def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _off4(t):
    """the same values 4 bytes off a 16-byte boundary (a fresh buffer)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _run(metric, x, E, prep, temp=0.0, u=None):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.lucid import cdist_sample_assign
    from dynamicvectorquantization_amd.quantize import score_assign
    if metric == "cdist":
        return cdist_sample_assign(x, E, prep, temp, u)
    return score_assign(x, E, prep, _lib.METRIC_DOT if metric == "dot" else _lib.METRIC_L2, temp, u)


def _check_case(c, dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    inp = C.score_inputs(c, oracle_mod)
    x, E, prep = _t(inp["x"], dev), _t(inp["E"], dev), _CodebookPrep()
    out_shape = (c.shape[0],) + tuple(c.shape[2:])
    four_dims = len(c.shape) == 4
    rows = _t(inp["rows"], dev) if four_dims else None
    if c.noise == "none":
        got = _run(c.metric, x, E, prep)
        assert got.dtype == torch.int64 and tuple(got.shape) == out_shape
        assert np.array_equal(got.cpu().numpy().reshape(-1), inp["hard"])           # every token, no skip set
        if four_dims:
            assert torch.equal(_run(c.metric, rows, E, prep), got.reshape(-1))       # NCHW == row-major of the same tokens
        return
    u = _t(inp["u"], dev)
    assert u.data_ptr() % 16 == 0
    for temp in c.temps:
        got = _run(c.metric, x, E, prep, temp, _off4(u) if c.noise == "offset" else u)
        assert got.dtype == torch.int64 and tuple(got.shape) == out_shape
        g = got.cpu().numpy().reshape(-1)
        want, skip = inp["want", temp], inp["skip", temp]
        print("%s temp %g: %d of %d tokens in the skip set, %d differ, G %.3g" % (c.name, temp, skip.sum(), skip.size, (g != want).sum(), inp["G"]))
        assert skip.mean() <= C.SKIP_CAP
        assert np.array_equal(g[~skip], want[~skip])
        if c.noise == "offset":                                                     # scalar by alignment: the aligned run's codes
            assert torch.equal(_run(c.metric, x, E, prep, temp, u), got)
        if four_dims:
            assert torch.equal(_run(c.metric, rows, E, prep, temp, u), got.reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.EVERY])
def test_every_instantiation(name, dev, oracle_mod):
    _check_case(C.BY_NAME[name], dev, oracle_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.K_EDGES])
def test_k_edges(name, dev, oracle_mod):
    _check_case(C.BY_NAME[name], dev, oracle_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.N_EDGES])
def test_n_edges(name, dev, oracle_mod):
    _check_case(C.BY_NAME[name], dev, oracle_mod)


@pytest.mark.gpu
def test_noise_edges(dev, oracle_mod):
    """0, a subnormal, 1e-20, 1e-10, 1 - 2^-24 and exactly 1.0 among the uniforms, a constant row of u, and a duplicated codebook
    row with equal noise, which the first index wins (tests/test_score_cases.py: the tie is the winner for some tokens at every
    temp)"""
    c = C.NOISE_EDGE
    _check_case(c, dev, oracle_mod)
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    inp = C.score_inputs(c, oracle_mod)
    first, second = C.DUPLICATE
    for temp in c.temps:
        got = _run(c.metric, _t(inp["x"], dev), _t(inp["E"], dev), _CodebookPrep(), temp, _off4(_t(inp["u"], dev))).cpu().numpy()
        assert not (got == second).any() and (got[C.TIE_TOKENS] == first).sum() == (inp["want", temp][C.TIE_TOKENS] == first).sum() >= 1
        skip = inp["skip", temp]
        assert np.array_equal(got[~skip], inp["want", temp][~skip])                 # the scalar reads see the same special values


@pytest.mark.gpu
@pytest.mark.parametrize("metric", C.METRICS)
def test_special_scores(metric, dev, oracle_mod):
    """an all-NaN token gives code 0; a single NaN score wins and the first NaN wins; a codebook row with an inf scores -inf and
    never wins; every score -inf gives code 0; the zero token and a token equal to a code under CDIST (d slightly negative: clamped,
    not NaN).  The expected codes are the restatement's; tests/test_score_cases.py asserts that they are what this list says"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    sp = C.special_inputs(metric, oracle_mod)
    x, u = _t(sp["rows"], dev), _t(sp["u"], dev)
    for book in C.SPECIAL_BOOKS:
        E, prep = _t(sp[book, "E"], dev), _CodebookPrep()
        if metric != "cdist":
            assert np.array_equal(_run(metric, x, E, prep).cpu().numpy(), sp[book, "hard"]), book
        for temp in C.SPECIAL_TEMPS:
            assert not sp[book, "skip", temp].any()
            for uu in (u, _off4(u)):
                got = _run(metric, x, E, prep, temp, uu).cpu().numpy()
                assert np.array_equal(got, sp[book, "want", temp]), (book, temp, got, sp[book, "want", temp])


@pytest.mark.gpu
@pytest.mark.parametrize("D", C.PADDED_WIDTHS)
def test_padded_widths(D, dev, oracle_mod):
    """a width served by zero padding equals the explicitly zero-padded run at the next kernel width bit for bit, through both
    wrappers, with and without u; and the codes are the oracle's at the padded width"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    inp = C.padded_inputs(D, oracle_mod)
    E, Ep, rows, rp = inp["E"], inp["Ep"], inp["rows"], inp["rp"]
    Dp = Ep.shape[1]
    u = _t(inp["u"], dev)
    x4, x4p = C.to_layout(rows, (2, D, 5, 7)), C.to_layout(rp, (2, Dp, 5, 7))
    for metric in C.METRICS:
        for a, b in ((rows, rp), (x4, x4p)):
            pa, pb = _CodebookPrep(), _CodebookPrep()
            if metric != "cdist":
                got = _run(metric, _t(a, dev), _t(E, dev), pa)
                assert torch.equal(got, _run(metric, _t(b, dev), _t(Ep, dev), pb))
                assert np.array_equal(got.cpu().numpy().reshape(-1), inp[metric, "hard"])
            for temp in C.TEMPS:
                got = _run(metric, _t(a, dev), _t(E, dev), pa, temp, u)
                assert torch.equal(got, _run(metric, _t(b, dev), _t(Ep, dev), pb, temp, u))
                skip = inp[metric, "skip", temp]
                assert skip.mean() <= C.SKIP_CAP
                assert np.array_equal(got.cpu().numpy().reshape(-1)[~skip], inp[metric, "want", temp][~skip])
