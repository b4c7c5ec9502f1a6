"""The fused soft code assignment (dvq_vq_soft_assign_flat_f32, quantize.soft_assign, get_soft_codes of every quantizer) against
the reference's own ops (tests/golden/soft_assign_*.npz, written by tools/gen_golden_soft.py) and against the numpy restatement
tests/_soft_ref.py.  Tolerances are the fixtures': soft_tol = 4 e_ref, e_ref = the reference fp32 softmax's own distance from the
float64 softmax of the same distances; a drawn code may differ from the reference's only where the two best p / q are within 1e-4
relative (at most 1 % of the tokens, else the test fails)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _cases as C
from tests import _soft_ref as R
from dynamicvectorquantization_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIX = {}


def _fixture(tag):
    """fixture + its regenerated codebook, loaded once and shared (read-only) by the tests"""
    if tag not in _FIX:
        g = R.load(tag)
        K, D = int(g["K"]), int(g["D"])
        make = synth.codebook_trained if str(g["cb_kind"]) == "trained" else synth.codebook_default_init
        E = make(K, D, seed=int(g["cb_seed"]))
        assert C.crc(E) == g["cb_crc"], "the synthetic codebook does not regenerate bit-identically"
        for a in list(g.values()) + [E]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FIX[tag] = (g, E)
    return _FIX[tag]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_declared_and_exported():
    from dynamicvectorquantization_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvq.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dvq_vq_soft_assign_workspace_bytes", "dvq_vq_soft_assign_flat_f32"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert _lib.lib.dvq_version() >= 1100


def test_validation_without_gpu():
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    EINVAL, EUNSUPPORTED = -1, -2
    a = 256                                                        # a "pointer" that passes the alignment checks
    assert L.dvq_vq_soft_assign_workspace_bytes(200, 256, 96) >= 200 * 96 * 4
    assert L.dvq_vq_soft_assign_workspace_bytes(0, 256, 96) == 0
    assert L.dvq_vq_soft_assign_workspace_bytes(200, 100, 96) == 0

    def call(x=a, cb=a, prep=a, N=200, D=256, K=96, temp=1.0, q=0, soft=a, dist=0, codes=a, ws=0, ws_bytes=0):
        return L.dvq_vq_soft_assign_flat_f32(x, cb, prep, N, D, K, temp, q, soft, dist, codes, ws, ws_bytes, 0)

    for null in ("x", "cb", "prep", "codes"):
        assert call(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert call(temp=0.0) == EINVAL and b"temp" in L.dvq_last_error_string()
    assert call(temp=-1.0) == EINVAL
    assert call(temp=float("nan")) == EINVAL
    assert call(temp=float("inf")) == EINVAL
    assert call(N=0) == EINVAL
    assert call(D=100) == EUNSUPPORTED                              # the widths rule of every assign entry point (include/dvq.h)
    need = L.dvq_vq_soft_assign_workspace_bytes(200, 256, 96)
    assert call(soft=0, q=a, ws=a, ws_bytes=need - 1) == EINVAL and b"workspace" in L.dvq_last_error_string()
    assert call(soft=0, q=a, ws=0, ws_bytes=need) == EINVAL


@pytest.mark.parametrize("tag", R.FIXTURES)
def test_restatement_reproduces_the_reference(tag, oracle_mod):
    """_soft_ref from the fixture's stored distances (the long row: the CPU oracle's, which the generator found bit-equal to the
    reference's) and q gives the reference's soft codes within soft_tol and its drawn codes outside the skip set"""
    g, E = _fixture(tag)
    if "dist" in g:
        dist = g["dist"]
    else:
        assert bool(g["dist_bits_equal_oracle"])
        dist = np.stack([oracle_mod.token_distances(g["x"][n], E) for n in range(int(g["N"]))])
        assert C.crc(dist) == g["oracle_dist_crc"]
    p = R.softmax64(dist, float(g["temp"]))
    tol = float(g["soft_tol"])
    if "soft" in g:
        assert np.abs(p - g["soft"]).max() <= tol
    else:
        assert np.abs(p[g["soft_rows_idx"]] - g["soft_rows"]).max() <= tol
    skip = R.skip_set(p, g["q"])
    assert skip.mean() <= 0.01
    keep = ~skip
    assert np.array_equal(R.draw(p, g["q"])[keep], g["code_draw"][keep])
    assert np.array_equal(np.argmin(dist, axis=1), g["code_hard"])


# ---------------------------------------------------------------------------------------------------------------- GPU

def _run(dev, x, E, temp, q=None, want_soft=True, want_dist=False):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, soft_assign
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)
    return soft_assign(t(x), t(E), _CodebookPrep(), temp, t(q), want_soft, want_dist)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", R.FIXTURES)
def test_fixture(tag, dev):
    """distances: bitwise the reference's where the fixture stores them (every stored fixture records dist_bits_equal_oracle; were
    it false, the oracle's bits in `dist_oracle` are what is pinned)"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    g, E = _fixture(tag)
    x, temp, q, tol = g["x"], float(g["temp"]), g["q"], float(g["soft_tol"])
    N, K = int(g["N"]), int(g["K"])
    soft, hard, dist = _run(dev, x, E, temp, want_dist=True)
    soft_n, hard_n, dist_n = soft.cpu().numpy(), hard.cpu().numpy(), dist.cpu().numpy()
    assert soft_n.shape == (N, K) and hard_n.shape == (N,) and hard.dtype == torch.int64
    if "dist" in g:
        want = g["dist"] if bool(g["dist_bits_equal_oracle"]) else g["dist_oracle"]
        assert np.array_equal(dist_n.view(np.uint32), want.view(np.uint32))
    else:
        assert C.crc(dist_n) == g["oracle_dist_crc"]
    if "soft" in g:
        err = np.abs(soft_n - g["soft"]).max()
    else:
        err = np.abs(soft_n[g["soft_rows_idx"]] - g["soft_rows"]).max()
    print("%s: soft error %.3g (soft_tol %.3g), row sums within %.3g" % (tag, err, tol, np.abs(soft_n.astype(np.float64).sum(1) - 1).max()))
    assert err <= tol
    assert np.abs(soft_n.astype(np.float64).sum(1) - 1.0).max() <= K * tol
    assert np.array_equal(hard_n, g["code_hard"])
    xt, Et = torch.tensor(x, device=dev), torch.tensor(E, device=dev)
    assert torch.equal(vq_assign(xt, Et, _CodebookPrep(), want_zq=False, want_loss=False)[1], hard)
    # the draw
    skip = R.skip_set(soft_n, q)
    assert skip.mean() <= 0.01
    soft2, drawn, _ = _run(dev, x, E, temp, q=q)
    assert np.array_equal(drawn.cpu().numpy()[~skip], g["code_draw"][~skip])
    assert torch.equal(soft2, soft)                                  # two runs, and with / without q: the same bits
    none, drawn2, _ = _run(dev, x, E, temp, q=q, want_soft=False)
    assert none is None and torch.equal(drawn2, drawn)
    none, hard2, _ = _run(dev, x, E, temp, want_soft=False)
    assert none is None and torch.equal(hard2, hard)
    soft3, hard3, dist3 = _run(dev, x, E, temp, want_dist=True)
    assert torch.equal(soft3, soft) and torch.equal(hard3, hard) and torch.equal(dist3, dist)


@pytest.mark.gpu
def test_padded_width_equals_explicit_padding(dev):
    K, N = 96, 200
    E = synth.codebook_trained(K, 32, seed=7461)
    x = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, 7462)[0, :, :, 0].T)
    q = torch.empty(N, K).exponential_(1, generator=torch.Generator().manual_seed(5)).numpy()
    Ep, xp = np.zeros((K, 64), np.float32), np.zeros((N, 64), np.float32)
    Ep[:, :32], xp[:, :32] = E, x
    for qq in (None, q):
        a = _run(dev, x, E, 4.0, q=qq, want_dist=True)
        b = _run(dev, xp, Ep, 4.0, q=qq, want_dist=True)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert tuple(_run(dev, x.reshape(2, 100, 32), E, 4.0)[0].shape) == (2, 100, K)


@pytest.mark.gpu
def test_unaligned_k_takes_the_scalar_rows(dev):
    """K % 4 != 0: phase B reads its rows with 4-byte accesses; the first 94 codes of the fixture's codebook"""
    g, E = _fixture("d256_k96")
    K = 94
    soft, hard, dist = _run(dev, g["x"], E[:K], float(g["temp"]), want_dist=True)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), np.ascontiguousarray(g["dist"][:, :K]).view(np.uint32))
    p = R.softmax64(g["dist"][:, :K], float(g["temp"]))
    assert np.abs(soft.cpu().numpy() - p).max() <= float(g["soft_tol"])
    assert np.array_equal(hard.cpu().numpy(), np.argmin(g["dist"][:, :K], axis=1))


def _vq2(cls, K, D, E, dev):
    m = cls(K, D).to(dev).eval()
    m.codebook.weight.data[:-1].copy_(torch.tensor(E))
    m.invalidate_codebook_cache()
    return m


@pytest.mark.gpu
def test_seeded_draw_follows_torch_generator(dev):
    """torch.manual_seed governs get_soft_codes(stochastic=True) as it governs the torch chain of the parent commit (restated here:
    compute_distances, softmax, torch.multinomial): the draws agree on >= 99 % of the tokens (the chain's distances are a vendor GEMM
    at tolerance level, so a near-tied ratio may flip)"""
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    g, E = _fixture("d256_k96")
    m = _vq2(lambda K, D: VectorQuantize2(K, D, accept_image_fmap=False, channel_last=True), 96, 256, E, dev)
    x = torch.tensor(g["x"], device=dev)
    temp = float(g["temp"])
    torch.manual_seed(1234)
    soft, code = m.get_soft_codes(x, temp=temp, stochastic=True)
    torch.manual_seed(1234)
    d = m.codebook.compute_distances(x)
    p = torch.softmax(d / (-temp), dim=-1)
    want = torch.multinomial(p, 1).reshape(-1)
    assert code.shape == want.shape and code.dtype == torch.int64
    assert float((code == want).float().mean()) >= 0.99
    assert float((soft - p).abs().max()) < 1e-4
    torch.manual_seed(1234)
    assert torch.equal(m.get_soft_codes(x, temp=temp, stochastic=True)[1], code)
    # CPU tensors keep the torch chain
    sc, cc = m.cpu().get_soft_codes(x.cpu(), temp=temp)
    assert np.array_equal(cc.numpy(), g["code_hard"])


@pytest.mark.gpu
def test_rq_soft_codes(dev):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import soft_assign
    from dynamicvectorquantization_amd.rq import RQBottleneck
    K, D, B, h, w, depth = 96, 64, 2, 4, 4, 2
    rq = RQBottleneck((4, 4, D), (4, 4, depth), K).to(dev).eval()
    books = []
    for i, cb in enumerate(rq.codebooks):
        Ei = synth.codebook_trained(K, D, seed=7470 + i) * np.float32(1.0 if i == 0 else 0.3)
        cb.weight.data[:-1].copy_(torch.from_numpy(Ei))
        cb.invalidate_codebook_cache()
        books.append(Ei)
    z = synth.z_tokens(books[0], B, h, w, 7480)
    x = torch.from_numpy(np.ascontiguousarray(z.transpose(0, 2, 3, 1))).to(dev)
    soft, hard = rq.get_soft_codes(x, temp=8.0)
    assert soft.shape == (B, h, w, depth, K) and torch.equal(hard, rq.get_codes(x))
    N = B * h * w
    ws = next(iter(rq._ws.values()))
    for i in range(depth):
        if i == 0:
            r = x.reshape(N, D)
        else:
            off = _lib.lib.dvq_rq_residual_offset(N, D, depth, i)
            assert off > 0
            r = ws[off:off + N * D * 4].view(torch.float32).view(N, D)
        cb = rq.codebooks[i]
        s_i, c_i, _ = soft_assign(r.clone(), cb.weight[:-1], cb._prep, 8.0)
        assert torch.equal(soft[..., i, :].reshape(N, K), s_i) and torch.equal(hard[..., i].reshape(N), c_i)
    torch.manual_seed(7)
    s1, c1 = rq.get_soft_codes(x, temp=8.0, stochastic=True)
    torch.manual_seed(7)
    s2, c2 = rq.get_soft_codes(x, temp=8.0, stochastic=True)
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and int(c1.min()) >= 0 and int(c1.max()) < K
    assert torch.equal(s1[..., 0, :], soft[..., 0, :])               # depth 0 sees the same residual either way


@pytest.mark.gpu
def test_list_quantizer_soft_codes(dev):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2List
    g, E = _fixture("d256_k96")
    m = _vq2(VectorQuantize2List, 96, 256, E, dev)
    x = torch.tensor(g["x"], device=dev)
    soft, code = m.get_soft_codes(x, temp=float(g["temp"]))
    assert np.abs(soft.cpu().numpy() - g["soft"]).max() <= float(g["soft_tol"])
    assert np.array_equal(code.cpu().numpy(), g["code_hard"])
    soft3, code3 = m.get_soft_codes(x.reshape(2, 100, 256), temp=float(g["temp"]))
    assert soft3.shape == (2, 100, 96) and torch.equal(soft3.reshape(200, 96), soft) and torch.equal(code3.reshape(200), code)
