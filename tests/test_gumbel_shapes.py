"""The Gumbel sweep (csrc/vq_gumbel.hip: vq_gumbel_assign_kernel<D, NOISE>, quantize.gumbel_assign) away from the four cases of
tests/test_gumbel.py: all six instantiations at K from 1 to 100 (K <= 4: the lane half without a code in the merge of the KL
state), d = 1, 8, 12, 16 and embed off 16-byte alignment (both z_q epilogues), one token to more than 256 KL partials, and the
KL state under stress: a maximum that rises on every tile while early terms underflow, a descending ramp, logits of standard
deviation 30, -inf logits on a lane's whole first tile, on all codes but one, on every code, and kl_K != K.

Tables, inputs and rules: tests/_score_cases.py (its docstring derives them; tests/test_score_cases.py holds the CPU checks).
Logits: fl(oracle.token_dots(z, W) + b), bit for bit the kernel's.  Codes: exact without q; with q outside the skip set of the
rule.  z_q: bit-equal to E[code].  KL: |kl - kl64| <= 1e-5 T; the observed |kl - kl64| / T is printed per case.

Measured on an MI355X: the largest |kl - kl64| / T over every case is 4.0e-8 (`kl-std30`; the ramps 2.3e-8 and 2.4e-8, the
ordinary cases below 1e-8), so no case needs more than the 1e-5 and none is compared against an fp32 chain instead.  One token of
all cases is in a skip set (`n-32897x64`).

What the cases see.  On a scratch build without the guard for a lane half without a code in `moved()` the KL is NaN exactly in
the cases with K <= 4 (all widths, with and without q) and in `kl-one`; every other case passes."""
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


def _prep(W, b, dev):
    from dynamicvectorquantization_amd import _lib
    K, Cc = W.shape
    nb = _lib.lib.dvq_gumbel_prep_bytes(K, Cc)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    Wt, bt = _t(W, dev), _t(b, dev)
    _lib.check(_lib.lib.dvq_gumbel_prepare_f32(Wt.data_ptr(), _lib.ptr(bt), K, Cc, buf.data_ptr(), nb, _lib.stream_ptr(dev)), "prepare")
    return buf


def _run(c, inp, dev, **kw):
    from dynamicvectorquantization_amd.quantize import gumbel_assign
    Et = _t(inp["E"], dev)
    if c.e_offset:
        Et = _off4(Et)
    else:
        assert Et.data_ptr() % 16 == 0
    return gumbel_assign(_t(inp["z"], dev), _prep(inp["W"], inp["b"], dev), Et, c.tau, _t(inp["q"], dev), kl_K=c.kl_K, **kw)


def _check_case(c, dev, oracle_mod):
    inp = C.gumbel_inputs(c, oracle_mod)
    zq, codes, kl = _run(c, inp, dev)
    N = C.ntokens(c.shape)
    assert codes.dtype == torch.int64 and tuple(codes.shape) == (c.shape[0],) + tuple(c.shape[2:])
    assert tuple(zq.shape) == (c.shape[0], c.d) + tuple(c.shape[2:]) and tuple(kl.shape) == (1,)
    got = codes.cpu().numpy().reshape(-1)
    assert got.min() >= 0 and got.max() < c.K
    if c.noise:
        skip = inp["skip"]
        assert skip.mean() <= C.GUMBEL_SKIP_CAP
        assert np.array_equal(got[~skip], inp["want"][~skip])
        left = int(skip.sum())
    else:
        assert np.array_equal(got, inp["hard"])                     # every token, ties and NaN included
        left = 0
    assert np.array_equal(C.to_rows(zq.cpu().numpy()).view(np.uint32), inp["E"][got].view(np.uint32))     # the codebook row itself
    klv, want, T = float(kl), inp["kl"], inp["T"]
    if np.isnan(want):
        assert np.isnan(klv)
        ratio = float("nan")
    else:
        err = abs(klv - want)
        ratio = err / T if T > 0 else (0.0 if err == 0 else float("inf"))
        assert err <= 1e-5 * T, (c.name, klv, want, T)
    print("%s: N %d, %d in the skip set, Gq %.3g, KL %.9g (float64 %.9g), T %.4g, |kl - kl64| / T %.3g" % (
        c.name, N, left, inp.get("Gq", 0.0), klv, want, T, ratio))
    return zq, codes, kl


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.G_WIDTHS])
def test_widths_and_small_k(name, dev, oracle_mod):
    _check_case(C.G_BY_NAME[name], dev, oracle_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.G_DS])
def test_zq_epilogues(name, dev, oracle_mod):
    c = C.G_BY_NAME[name]
    zq, codes, kl = _check_case(c, dev, oracle_mod)
    only = _run(c, C.gumbel_inputs(c, oracle_mod), dev, want_zq=False, want_kl=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], codes)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.G_N_EDGES])
def test_n_edges(name, dev, oracle_mod):
    _check_case(C.G_BY_NAME[name], dev, oracle_mod)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in C.G_STRESS])
def test_kl_stress(name, dev, oracle_mod):
    c = C.G_BY_NAME[name]
    zq, codes, kl = _check_case(c, dev, oracle_mod)
    inp = C.gumbel_inputs(c, oracle_mod)
    if c.bias == "allinf":
        assert not codes.any() and bool(torch.isnan(kl).all())
    if c.bias == "one":
        assert bool((codes == C.ONE_CODE).all())
    noq = _run(c._replace(noise=False), dict(inp, q=None), dev)    # the KL term does not depend on the noise: the same bits
    assert torch.equal(noq[2].view(torch.int32), kl.view(torch.int32))
    assert np.array_equal(noq[1].cpu().numpy().reshape(-1), inp["hard"])


@pytest.mark.gpu
def test_kl_is_deterministic(dev, oracle_mod):
    c = C.G_BY_NAME["kl-ramp_up"]
    inp = C.gumbel_inputs(c, oracle_mod)
    a, b = _run(c, inp, dev), _run(c, inp, dev)
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    big = C.G_BY_NAME["n-32897x64"]                                 # 258 partials: the finalize's second round, the same bits too
    inp = C.gumbel_inputs(big, oracle_mod)
    a, b = _run(big, inp, dev), _run(big, inp, dev)
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[1], b[1])
