"""Quantisation from given codes (csrc/vq_sample.hip: vq_apply_codes_kernel, quantize.apply_codes) at the widths, shapes, masks
and codes its fixtures never ran: D from 16 to 256 (the ABI takes any multiple of 16), one token to a second workgroup, NCHW
with a wave that straddles images, K = 1, fractional and all-zero masks, codes outside [0, K) -- the kernel documents that such a
code "leaves its token unquantised (z_q = z) and adds nothing to the loss" -- either output alone, and more than 256 loss partials.

Reference: zq bits are numpy's fp32 z + (e - z) (z itself for a code out of range); loss[0] is the float64 mean over N D of
fp32(e - z)^2 m, loss[1] = beta loss[0] + loss[0]; tolerance the project's 1e-5 relative (tests/test_maskvq.py); an all-zero mask
gives exactly 0 and a NaN in z a NaN loss.

What the cases see.  On a scratch build that quantised a token with a code out of range to row 0 (the `ok` guard of the
difference dropped; the read stays in bounds) the out-of-range tests fail at every width, and the many-partials test, which mixes such codes in; the
shape and mask tests pass."""
import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import synth
from tests import _score_cases as C

WIDTHS = (16, 48, 64, 128, 256)
SHAPES = lambda D: ((1, D), (127, D), (129, D), (3, D, 5, 7))
OUT_OF_RANGE = np.array([-1, None, 2 ** 40, np.iinfo(np.int64).min], dtype=object)      # None: K
BETA = 0.25


def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(D, shape, K, seed):
    N = C.ntokens(shape)
    E = synth.codebook_trained(K, D, seed=seed)
    rows = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, seed + 1)[0, :, :, 0].T)
    codes = synth.randint(seed + 2, (N,), K)
    return E, rows, codes


def _masks(N, seed):
    return {"none": None, "01": synth.bernoulli(seed, (N,), 0.6).astype(np.float32),
            "frac": synth.uniform(seed + 1, (N,), 0.0, 2.0), "zero": np.zeros(N, np.float32)}


def _reference(rows, E, codes, mask, K):
    """(zq rows fp32, loss[0] in float64)"""
    ok = (codes >= 0) & (codes < K)
    e = E[np.where(ok, codes, 0)]
    with np.errstate(invalid="ignore"):
        diff = np.where(ok[:, None], (e - rows).astype(np.float32), np.float32(0))
        zq = (rows + diff).astype(np.float32)
        sq = (diff * diff).astype(np.float32).astype(np.float64)
    m = np.ones(len(rows)) if mask is None else mask.astype(np.float64)
    return zq, float((sq * m[:, None]).mean())


def _check(rows, E, codes, mask, shape, dev, prep, what):
    from dynamicvectorquantization_amd.quantize import apply_codes
    K = E.shape[0]
    z = _t(C.to_layout(rows, shape), dev)
    ct = _t(codes, dev).reshape((shape[0],) + tuple(shape[2:]))
    mt = None if mask is None else _t(mask, dev).reshape(ct.shape)
    zq, loss = apply_codes(z, ct, _t(E, dev), prep, mt, BETA)
    want_zq, want = _reference(rows, E, codes, mask, K)
    assert tuple(zq.shape) == tuple(shape) and tuple(loss.shape) == (2,) and loss.dtype == torch.float32
    assert np.array_equal(_bits(C.to_rows(zq.cpu().numpy())), _bits(want_zq)), what
    l0, l1 = float(loss[0]), float(loss[1])
    if np.isnan(want):
        assert np.isnan(l0) and np.isnan(l1), what
    else:
        assert abs(l0 - want) <= 1e-5 * abs(want) and abs(l1 - (BETA * want + want)) <= 1e-5 * abs(BETA * want + want), (what, l0, want)
    if mask is not None and not mask.any() and not np.isnan(rows).any():
        assert l0 == 0.0 and l1 == 0.0, what
    only_loss = apply_codes(z, ct, _t(E, dev), prep, mt, BETA, want_zq=False)           # either output alone: the same bits
    only_zq = apply_codes(z, ct, _t(E, dev), prep, mt, BETA, want_loss=False)
    assert only_loss[0] is None and only_zq[1] is None
    assert torch.equal(only_zq[0].view(torch.int32), zq.view(torch.int32)), what
    assert torch.equal(only_loss[1].view(torch.int32), loss.view(torch.int32)), what
    return zq, loss


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_shapes_masks_and_partial_outputs(D, dev):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    prep = _CodebookPrep()
    for si, shape in enumerate(SHAPES(D)):
        for K in (1, 96):
            seed = 8700 + 40 * WIDTHS.index(D) + 8 * si + 4 * (K == 96)
            E, rows, codes = _inputs(D, shape, K, seed)
            for name, mask in _masks(len(rows), seed + 3).items():
                _check(rows, E, codes, mask, shape, dev, prep, (D, shape, K, name))


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_codes_out_of_range_leave_the_token_unquantised(D, dev):
    """-1, K, 2^40 and INT64_MIN among the codes (the kernel takes `ok ? cj : 0` for the row it reads and a zero difference for
    such a token): zq == z bit for bit there, nothing added to the loss"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, apply_codes
    prep = _CodebookPrep()
    for si, shape in enumerate(SHAPES(D)):
        for K in (1, 96):
            seed = 8900 + 40 * WIDTHS.index(D) + 8 * si + 4 * (K == 96)
            E, rows, codes = _inputs(D, shape, K, seed)
            N = len(rows)
            bad = np.array([K if v is None else v for v in OUT_OF_RANGE], dtype=np.int64)
            codes = codes.copy()
            where = np.arange(0, N, 3)
            codes[where] = bad[np.arange(len(where)) % len(bad)]
            for name, mask in _masks(N, seed + 3).items():
                if name == "zero":
                    continue
                zq, loss = _check(rows, E, codes, mask, shape, dev, prep, (D, shape, K, name))
                assert np.array_equal(_bits(C.to_rows(zq.cpu().numpy())[where]), _bits(rows[where]))
            # the loss is that of the in-range tokens alone: the same call with the others masked out, and codes in range there
            m = np.ones(N, np.float32)
            m[where] = 0.0
            safe = codes.copy()
            safe[where] = 0
            z = _t(C.to_layout(rows, shape), dev)
            ct = lambda a: _t(a, dev).reshape((shape[0],) + tuple(shape[2:]))
            l_bad = apply_codes(z, ct(codes), _t(E, dev), prep, None, BETA, want_zq=False)[1]
            l_safe = apply_codes(z, ct(safe), _t(E, dev), prep, ct(m), BETA, want_zq=False)[1]
            assert torch.equal(l_bad.view(torch.int32), l_safe.view(torch.int32))


@pytest.mark.gpu
def test_many_partials_and_nan(dev):
    """[38401, 16]: 301 workgroups, so the finalize's strided read of the partials runs a second round; a NaN in z gives a NaN
    loss and leaves every other token's zq alone"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    D, K, N = 16, 96, 38401
    assert (N + 127) // 128 > 256
    E, rows, codes = _inputs(D, (N, D), K, 9100)
    prep = _CodebookPrep()
    for name, mask in _masks(N, 9103).items():
        _check(rows, E, codes, mask, (N, D), dev, prep, name)
    codes = codes.copy()
    codes[::5] = np.array([-1, K, 2 ** 40, np.iinfo(np.int64).min], dtype=np.int64)[np.arange(len(codes[::5])) % 4]
    _check(rows, E, codes, _masks(N, 9103)["frac"], (N, D), dev, prep, "out of range")
    rows = rows.copy()
    assert 0 <= codes[N - 2] < K
    rows[N - 2, D - 1] = np.nan                                    # in the last workgroup, a token whose code is in range
    zq, loss = _check(rows, E, codes, None, (N, D), dev, prep, "nan")
    assert bool(torch.isnan(loss).all()) and int(torch.isnan(zq).sum()) == 1
    zq, loss = _check(rows, E, codes, _masks(N, 9103)["zero"], (N, D), dev, prep, "nan under a zero mask")
    assert bool(torch.isnan(loss).all())                           # NaN * 0 is NaN: as torch's mean of (e - z)^2 * mask
