"""VectorQuantizer / EMAVectorQuantizer / VectorQuantizer2Seq and the code-usage statistics under them (csrc/code_stats.hip,
`dvq_code_stats_f32`, `dvq_code_stats_grain_f32`, quantize.code_usage).

References: the reference's own outputs in tests/golden/taming_*.npz (tools/gen_golden_taming.py, which also asserts that the
oracle reproduces the reference's codes and z_q: the pin) and the numpy / float64 restatement tests/_taming_ref.py.

Bounds: counts, n_used, the one-hot matrix, codes and z_q are compared for equality.  Perplexity: 1e-5 relative, the project's
scalar tolerance (the kernel's recipe deviates from this torch build's by < 1e-6: tools/gen_golden_taming.py prints it), and
bit-equal from run to run (a pure function of the counts).  Loss: _cases.loss_close.  Gradients: 1e-6 (z) / 1e-5 (codebook) of
the largest entry, as tests/test_autograd_and_training.py applies them.  EMA parameters: max |got - ref| / max |ref| < 1e-5,
the bound of tests/test_ema_stats.py (include/dvq.h: float atomics, rounding-level parity).

The codebook gradient is compared bit for bit with VectorQuantizer2(legacy=True)'s: at the shapes used here (at most two 64-token
tiles) a code row receives at most two atomic adds onto zero, and fp32 addition of two terms is commutative."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import synth
from tests import _cases as C
from tests import _taming_ref as R

EINVAL, EUNSUPPORTED = -1, -2
CASE_NAMES = sorted(R.CASES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _golden(name):
    return np.load(os.path.join(C.GOLDEN, R.GOLDEN_FILE % name))


def _close(got, ref, rel):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() <= rel * max(1e-30, np.abs(ref).max())


def _case(name):
    g = _golden(name)
    z, E, gw, cs0 = R.case_inputs(name)
    assert C.crc(z) == g["z_crc"] and C.crc(E) == g["E_crc"] and C.crc(gw) == g["gw_crc"] and C.crc(cs0) == g["cs0_crc"], \
        "synthetic inputs do not regenerate bit-identically"
    assert tuple(int(v) for v in g["shape"]) == R.CASES[name]
    return g, z, E, gw, cs0


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_symbols_version_and_imports():
    from dynamicvectorquantization_amd import _lib
    header = open(os.path.join(os.path.dirname(C.GOLDEN), "..", "include", "dvq.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("dvq_code_stats_f32", "dvq_code_stats_grain_f32"):
        assert "DVQ_API" in header and n + "(" in header, n
        assert hasattr(raw, n) and n in _lib.EXPORTS and getattr(_lib.lib, n).argtypes is not None
    assert _lib.lib.dvq_version() >= 1500
    from dynamicvectorquantization_amd.quantize import (CodeUsage, EmbeddingEMA, EMAVectorQuantizer, VectorQuantizer,  # noqa: F401
                                                        VectorQuantizer2Seq, code_usage)
    assert VectorQuantizer.want_encodings is True and EMAVectorQuantizer.want_encodings is True
    with pytest.raises(_lib.DvqError):
        code_usage(torch.zeros(4, dtype=torch.int64), 8)                  # CPU tensors raise, as everywhere


def test_abi_validation_without_gpu():
    """fake "pointers": every call below is refused before anything is launched"""
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    a = 256

    def flat(codes=a, N=10, K=8, counts=a, n_used=a, perp=a, onehot=0):
        return L.dvq_code_stats_f32(codes, N, K, counts, n_used, perp, onehot, 0)

    for null in ("codes", "counts", "n_used", "perp"):
        assert flat(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert flat(K=0) == EINVAL and flat(K=-3) == EINVAL and flat(N=-1) == EINVAL
    assert flat(K=1 << 20) == EUNSUPPORTED

    def grain(codes=a, grain=a, B=2, H=32, W=32, hc=16, wc=16, G=2, K=8, counts=a, n_tokens=a, n_used=a, perp=a):
        return L.dvq_code_stats_grain_f32(codes, grain, B, H, W, hc, wc, G, K, counts, n_tokens, n_used, perp, 0)

    for null in ("codes", "grain", "counts", "n_tokens", "n_used", "perp"):
        assert grain(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert grain(K=0) == EINVAL and grain(B=0) == EINVAL and grain(hc=0) == EINVAL
    assert grain(G=1) == EINVAL and grain(G=4) == EINVAL
    assert grain(G=3) == EINVAL and b"grain map" in L.dvq_last_error_string()       # 32 / 16 != 4
    assert grain(hc=8, wc=8) == EINVAL and grain(hc=16, wc=8) == EINVAL and grain(H=33) == EINVAL and grain(W=30) == EINVAL
    assert grain(K=1 << 20) == EUNSUPPORTED


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_reference_perplexity(name):
    g, *_ = _case(name)
    K = R.CASES[name][4]
    for tag in ("vq", "ema"):
        codes = g[tag + "_codes"].astype(np.int64)
        s = R.flat_stats(codes, K)
        ref = float(g[tag + "_perplexity"])
        assert abs(s["perplexity"] - ref) <= 1e-5 * ref and abs(s["perplexity_f32"] - ref) <= 1e-5 * ref
        assert s["n_used"] == int(g[tag + "_n_used"])
        enc = R.onehot(codes, K)
        assert C.crc(enc) == g[tag + "_onehot_crc"]
        p32 = s["counts"].astype(np.float32) / np.float32(codes.size)
        assert np.array_equal(_bits(p32), _bits(torch.mean(torch.from_numpy(enc), dim=0).numpy()))     # the recipe's p_j


def test_state_dict_keys_and_shapes():
    from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer, VectorQuantizer, VectorQuantizer2Seq
    g = _golden("b")
    B, D, H, W, K = R.CASES["b"]
    m = VectorQuantizer(K, D, R.BETA)
    assert sorted(m.state_dict().keys()) == json.loads(str(g["vq_state_keys"]))
    lo, hi = float(m.embedding.weight.detach().min()), float(m.embedding.weight.detach().max())
    assert -1.0 / K <= lo and hi <= 1.0 / K
    e = EMAVectorQuantizer(K, D, R.BETA)
    assert sorted(e.state_dict().keys()) == json.loads(str(g["ema_state_keys"]))
    assert {k: list(v.shape) for k, v in e.state_dict().items()} == json.loads(str(g["ema_state_shapes"]))
    emb = e.embedding
    assert all(isinstance(p, torch.nn.Parameter) and not p.requires_grad for p in (emb.weight, emb.cluster_size, emb.embed_avg))
    assert emb.update is True and torch.equal(emb.weight, emb.embed_avg) and float(emb.cluster_size.abs().max()) == 0.0
    assert float(emb.weight.std()) > 0.5                                     # randn, not the uniform init
    s = VectorQuantizer2Seq(R.SEQ[3], R.SEQ[1], R.BETA)
    assert sorted(s.state_dict().keys()) == json.loads(str(_golden("seq")["state_keys"]))


def test_ema_remap_constructor_does_not_crash(tmp_path):
    from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer
    path = str(tmp_path / "used.npy")
    np.save(path, np.array([5, 2, 9, 2], np.int64))
    e = EMAVectorQuantizer(12, 4, 0.25, remap=path, unknown_index="extra")
    assert e.re_embed == 5 and "used" in e.state_dict()
    inds = torch.tensor([[2, 9, 7, 5]])
    assert e.remap_to_used(inds).tolist() == [[1, 2, 4, 0]]                  # first occurrence; unknown -> the extra slot
    assert e.unmap_to_all(torch.tensor([[1, 2, 4, 0]])).tolist() == [[2, 9, 5, 5]]


def test_grain_rule_by_hand_and_against_the_permuter():
    # 2 images, 4 x 4 codes, 2 x 2 cells: image 0 = cells (coarse, fine / fine, coarse), image 1 all coarse
    codes = np.arange(32, dtype=np.int64).reshape(2, 4, 4) % 7
    grain = np.array([[[0, 1], [1, 0]], [[0, 0], [0, 0]]], np.int64)
    s = R.grain_stats(codes, grain, 2, 7)
    assert s["n_tokens"].tolist() == [2 + 4, 8]
    coarse = [codes[0, 0, 0], codes[0, 2, 2], codes[1, 0, 0], codes[1, 0, 2], codes[1, 2, 0], codes[1, 2, 2]]
    fine = list(codes[0, 0:2, 2:4].reshape(-1)) + list(codes[0, 2:4, 0:2].reshape(-1))
    assert np.array_equal(s["counts"][0], np.bincount(coarse, minlength=7)) and np.array_equal(s["counts"][1], np.bincount(fine, minlength=7))
    # the permuter's sequences without specials (content < 1024: pad 1024, eos 1025)
    g = C.load("permuter_reference_selftest")
    idx, gr = g["indices"].astype(np.int64), g["grain"].astype(np.int64)
    s = R.grain_stats(idx, gr, 2, 1024)
    cc, fc = g["region_coarse_content"].astype(np.int64), g["region_fine_content"].astype(np.int64)
    assert s["n_tokens"].tolist() == [int((cc < 1024).sum()), int((fc < 1024).sum())]
    assert np.array_equal(s["counts"][0], np.bincount(cc[cc < 1024], minlength=1024))
    assert np.array_equal(s["counts"][1], np.bincount(fc[fc < 1024], minlength=1024))


# ---------------------------------------------------------------------------------------------
# GPU: the flat kernel against the restatement
# ---------------------------------------------------------------------------------------------
_FLAT = None


def _flat_cases():
    global _FLAT
    if _FLAT is None:
        _FLAT = R.flat_cases()
    return _FLAT


FLAT_NAMES = ["1x1", "257x5", "1024x1024", "4099x16384", "3000x40000", "513x1023", "all_equal", "zipf", "out_of_range", "empty"]
SENTINEL = 7.0


def _run_flat(codes_t, K, with_onehot=True, misalign=0):
    """the ABI entry point itself -> (counts, n_used, perplexity, onehot or None); the one-hot buffer is pre-filled with a
    sentinel and carries guard elements on both sides"""
    from dynamicvectorquantization_amd import _lib
    dev = codes_t.device
    N = codes_t.numel()
    counts = torch.full((K + 8,), -5, dtype=torch.int64, device=dev)
    small = torch.full((2,), -5, dtype=torch.int64, device=dev)
    perp = torch.full((1,), -5.0, dtype=torch.float32, device=dev)
    buf = oh = None
    if with_onehot:
        buf = torch.full((N * K + 64 + misalign,), SENTINEL, dtype=torch.float32, device=dev)
        oh = buf[32 + misalign:32 + misalign + N * K].view(N, K)
    _lib.check(_lib.lib.dvq_code_stats_f32(codes_t.data_ptr(), N, K, counts.data_ptr(), small.data_ptr(), perp.data_ptr(),
                                           _lib.ptr(oh), _lib.stream_ptr(dev)), "dvq_code_stats_f32")
    torch.cuda.synchronize(dev)
    assert bool((counts[K:] == -5).all()) and int(small[1]) == -5                       # nothing past the outputs
    if with_onehot:
        assert bool((buf[:32 + misalign] == SENTINEL).all()) and bool((buf[32 + misalign + N * K:] == SENTINEL).all())
    return counts[:K], small[0], perp[0], oh


def _onehot_gpu(codes_t, K):
    ref = torch.zeros((codes_t.numel(), K), dtype=torch.float32, device=codes_t.device)
    ok = (codes_t >= 0) & (codes_t < K)
    ref[ok.nonzero().reshape(-1), codes_t[ok]] = 1.0
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLAT_NAMES)
def test_flat_kernel(dev, name):
    codes, K = _flat_cases()[name]
    want = R.flat_stats(codes, K)
    ct = torch.from_numpy(codes).to(dev)
    counts, n_used, perp, oh = _run_flat(ct, K)
    print("%s: perplexity %.9g (float64 %.9g, fp32 recipe %.9g) n_used %d" % (name, float(perp), want["perplexity"],
                                                                             want["perplexity_f32"], int(n_used)))
    assert np.array_equal(counts.cpu().numpy(), want["counts"])
    assert int(n_used) == want["n_used"]
    assert abs(float(perp) - want["perplexity"]) <= 1e-5 * want["perplexity"]
    if codes.size == 0:
        assert float(perp) == 1.0 and int(counts.abs().sum()) == 0
    else:
        assert torch.equal(oh, _onehot_gpu(ct, K))                                      # every element written, exactly the one-hot
        if codes.size * K <= (1 << 22):
            assert np.array_equal(oh.cpu().numpy(), R.onehot(codes, K))
    # a second run, without the one-hot: the same counts, the same perplexity bits
    counts2, n_used2, perp2, none = _run_flat(ct, K, with_onehot=False)
    assert none is None and torch.equal(counts2, counts) and int(n_used2) == int(n_used)
    assert np.array_equal(_bits(perp2.cpu().numpy()), _bits(perp.cpu().numpy()))


@pytest.mark.gpu
def test_flat_kernel_unaligned_buffer(dev):
    """K % 4 == 0 but the one-hot buffer starts 4 bytes off a 16-byte boundary: the 4-byte store path"""
    codes, K = _flat_cases()["1024x1024"]
    ct = torch.from_numpy(codes).to(dev)
    counts, n_used, perp, oh = _run_flat(ct, K, misalign=1)
    assert oh.data_ptr() % 16 == 4
    assert torch.equal(oh, _onehot_gpu(ct, K)) and np.array_equal(counts.cpu().numpy(), R.flat_stats(codes, K)["counts"])


@pytest.mark.gpu
def test_code_usage_flat(dev):
    from dynamicvectorquantization_amd.quantize import code_usage
    codes, K = _flat_cases()["out_of_range"]
    want = R.flat_stats(codes, K)
    u = code_usage(torch.from_numpy(codes.reshape(10, 100)).to(dev), K, want_encodings=True)
    assert u.counts.dtype == torch.int64 and tuple(u.counts.shape) == (K,) and u.perplexity.dim() == 0 and u.n_used.dim() == 0
    assert np.array_equal(u.counts.cpu().numpy(), want["counts"]) and int(u.n_used) == want["n_used"] and int(u.n_tokens) == codes.size
    assert abs(float(u.perplexity) - want["perplexity"]) <= 1e-5 * want["perplexity"]
    assert np.array_equal(u.encodings.cpu().numpy(), R.onehot(codes, K))
    assert code_usage(torch.from_numpy(codes).to(dev), K).encodings is None
    with pytest.raises(TypeError):
        code_usage(torch.zeros(4, dtype=torch.int32, device=dev), K)
    with pytest.raises(ValueError):
        code_usage(torch.zeros((2, 4, 4), dtype=torch.int64, device=dev), K,
                   grain_indices=torch.zeros((2, 2, 2), dtype=torch.int64, device=dev), want_encodings=True)


# ---------------------------------------------------------------------------------------------
# GPU: the grain kernel
# ---------------------------------------------------------------------------------------------
def _grain_case(name):
    B, H = 2, 32
    if name == "dual":
        G, hc, K, gm = 2, 16, 1024, R.grain_map(8401, B, 16, 16, 2)
    elif name == "triple":
        G, hc, K, gm = 3, 8, 1024, R.grain_map(8402, B, 8, 8, 3, [0.3, 0.3, 0.4])
    elif name == "absent":                                            # no cell of grain 1
        G, hc, K, gm = 3, 8, 200, R.grain_map(8403, B, 8, 8, 3, [0.5, 0.0, 0.5])
        assert not (gm == 1).any()
    elif name == "out_of_range":
        G, hc, K, gm = 2, 16, 96, R.grain_map(8404, B, 16, 16, 2)
        gm.reshape(-1)[::5] = 2
        gm.reshape(-1)[1::9] = -1
    elif name == "lds_128k":                                          # 64 KiB < counters <= 144 KiB of LDS (K = 16384 dual)
        G, hc, K, gm = 2, 16, 16384, R.grain_map(8406, B, 16, 16, 2)
    elif name == "lds_108k":                                          # the same region, triple
        G, hc, K, gm = 3, 8, 9000, R.grain_map(8407, B, 8, 8, 3)
    elif name == "global":                                            # G * K counters beyond the LDS: global atomics
        G, hc, K, gm = 2, 16, 20000, R.grain_map(8405, B, 16, 16, 2)
    codes = synth.randint(8410 + G, (B, H, H), K)
    if name == "out_of_range":
        codes.reshape(-1)[::13] = K
        codes.reshape(-1)[4::17] = -1
    return codes, gm, G, K


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dual", "triple", "absent", "out_of_range", "lds_128k", "lds_108k", "global"])
def test_grain_kernel(dev, name):
    from dynamicvectorquantization_amd.quantize import code_usage
    if name.startswith("lds_"):
        # the order seam: a small-K call first in this process (the parametrised cases before this one are small too), so the
        # kernel's LDS opt-in was first applied by a call that needed a few KiB
        small = code_usage(torch.zeros((1, 4, 4), dtype=torch.int64, device=dev), 8,
                           grain_indices=torch.zeros((1, 2, 2), dtype=torch.int64, device=dev))
        assert small.n_tokens.tolist() == [4, 0]
    codes, gm, G, K = _grain_case(name)
    want = R.grain_stats(codes, gm, G, K)
    ct, gt = torch.from_numpy(codes).to(dev), torch.from_numpy(gm).to(dev)
    u = code_usage(ct, K, grain_indices=gt)
    u2 = code_usage(ct, K, grain_indices=gt)
    torch.cuda.synchronize(dev)
    print(name, "n_tokens", u.n_tokens.tolist(), "perplexity", u.perplexity.tolist(), "float64", want["perplexity"].tolist())
    assert tuple(u.counts.shape) == (G, K) and u.encodings is None
    assert np.array_equal(u.counts.cpu().numpy(), want["counts"])
    assert np.array_equal(u.n_tokens.cpu().numpy(), want["n_tokens"]) and np.array_equal(u.n_used.cpu().numpy(), want["n_used"])
    p = u.perplexity.cpu().numpy()
    assert np.isfinite(p).all() and (np.abs(p - want["perplexity"]) <= 1e-5 * want["perplexity"]).all()
    assert np.array_equal(_bits(p), _bits(u2.perplexity.cpu().numpy())) and torch.equal(u.counts, u2.counts)
    if name == "absent":
        assert int(u.n_tokens[1]) == 0 and float(u.perplexity[1]) == 1.0 and int(u.n_used[1]) == 0


@pytest.mark.gpu
def test_grain_kernel_counts_the_permuter_sequences(dev):
    """the kernel against the permuter's own sequences (the reference's known-answer self-test), directly"""
    from dynamicvectorquantization_amd.quantize import code_usage
    g = C.load("permuter_reference_selftest")
    idx, gr = g["indices"].astype(np.int64), g["grain"].astype(np.int64)
    u = code_usage(torch.from_numpy(idx).to(dev), 1024, grain_indices=torch.from_numpy(gr).to(dev))
    cc, fc = g["region_coarse_content"].astype(np.int64), g["region_fine_content"].astype(np.int64)
    assert u.n_tokens.tolist() == [int((cc < 1024).sum()), int((fc < 1024).sum())]
    counts = u.counts.cpu().numpy()
    assert np.array_equal(counts[0], np.bincount(cc[cc < 1024], minlength=1024))
    assert np.array_equal(counts[1], np.bincount(fc[fc < 1024], minlength=1024))


@pytest.mark.gpu
def test_grain_kernel_shape_mismatch(dev):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import code_usage
    codes = torch.zeros((2, 32, 32), dtype=torch.int64, device=dev)
    gm = torch.zeros((2, 16, 16), dtype=torch.int64, device=dev)
    out = torch.zeros(64, dtype=torch.int64, device=dev)
    perp = torch.zeros(4, dtype=torch.float32, device=dev)
    rc = _lib.lib.dvq_code_stats_grain_f32(codes.data_ptr(), gm.data_ptr(), 2, 32, 32, 16, 16, 3, 8, out.data_ptr(), out[32:].data_ptr(),
                                           out[40:].data_ptr(), perp.data_ptr(), _lib.stream_ptr(dev))
    assert rc == EINVAL
    with pytest.raises(ValueError):
        code_usage(codes, 8, grain_indices=gm[:, :, :15].contiguous())


# ---------------------------------------------------------------------------------------------
# GPU: the classes against the goldens
# ---------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def _check_stats(g, tag, K, perp, enc, idx):
    codes = idx.cpu().numpy().reshape(-1)
    assert np.array_equal(codes, g[tag + "_codes"].astype(np.int64))                    # all of them: the assign is exact
    ref = float(g[tag + "_perplexity"])
    assert perp.dim() == 0 and abs(float(perp) - ref) <= 1e-5 * ref
    assert tuple(enc.shape) == (codes.size, K) and enc.dtype == torch.float32
    assert C.crc(enc.cpu().numpy()) == g[tag + "_onehot_crc"]
    return codes


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_vector_quantizer_forward_backward(dev, name):
    from dynamicvectorquantization_amd.quantize import VectorQuantizer, VectorQuantizer2
    g, z, E, gw, _ = _case(name)
    B, D, H, W, K = R.CASES[name]
    m = VectorQuantizer(K, D, R.BETA).to(dev)
    m.embedding.weight.data.copy_(_t(E, dev))
    zt = _t(z, dev).requires_grad_(True)
    zq, loss, (perp, enc, idx) = m(zt)
    ((zq * _t(gw, dev)).sum() + 5.0 * loss).backward()
    assert tuple(idx.shape) == (B * H * W, 1) and idx.dtype == torch.int64 and not perp.requires_grad and not enc.requires_grad
    _check_stats(g, "vq", K, perp, enc, idx)
    o = _oracle().vq_assign_nchw(z, E, None)
    assert np.array_equal(_bits(zq.detach().cpu().numpy()), _bits(o["zq"])) and C.crc(zq.detach().cpu().numpy()) == g["vq_zq_crc"]
    assert C.loss_close(float(loss.detach()), g["vq_loss"])
    zg, wg = zt.grad.cpu().numpy(), m.embedding.weight.grad.cpu().numpy()
    assert _close(zg, g["vq_z_grad"], 1e-6) and _close(wg, g["vq_w_grad"], 1e-5)
    # the op VectorQuantizer2(legacy=True) runs: the same bits
    m2 = VectorQuantizer2(K, D, R.BETA, legacy=True).to(dev)
    m2.embedding.weight.data.copy_(_t(E, dev))
    zt2 = _t(z, dev).requires_grad_(True)
    zq2, loss2, (_, _, idx2) = m2(zt2)
    ((zq2 * _t(gw, dev)).sum() + 5.0 * loss2).backward()
    assert torch.equal(zq2, zq) and torch.equal(loss2, loss) and torch.equal(idx2.reshape(-1), idx.reshape(-1))
    assert np.array_equal(_bits(zt2.grad.cpu().numpy()), _bits(zg))
    assert np.array_equal(_bits(m2.embedding.weight.grad.cpu().numpy()), _bits(wg))
    # want_encodings = False: None, everything else the same
    m.want_encodings = False
    with torch.no_grad():
        zq3, loss3, (perp3, enc3, idx3) = m(_t(z, dev))
    assert enc3 is None and torch.equal(zq3, zq) and torch.equal(idx3, idx) and torch.equal(loss3, loss.detach())
    assert np.array_equal(_bits(perp3.cpu().numpy()), _bits(perp.cpu().numpy()))
    entry = m.get_codebook_entry(idx.reshape(-1), (B, H, W, D))
    assert torch.equal(entry, _t(np.moveaxis(E[idx.cpu().numpy().reshape(B, H, W)], 3, 1), dev))


def _make_ema(dev, K, D, E, cs0):
    from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer
    e = EMAVectorQuantizer(K, D, R.BETA, decay=R.DECAY, eps=R.EPS).to(dev)
    with torch.no_grad():
        e.embedding.weight.copy_(_t(E, dev))
        e.embedding.cluster_size.copy_(_t(cs0, dev))
        e.embedding.embed_avg.copy_(_t(E * cs0[:, None], dev))
    e.invalidate_codebook_cache()
    return e


def _params(e):
    emb = e.embedding
    return [p.detach().clone() for p in (emb.weight, emb.cluster_size, emb.embed_avg)]


def _ema_forward(e, z, gw, dev):
    zt = _t(z, dev).requires_grad_(True)
    zq, loss, (perp, enc, idx) = e(zt)
    ((zq * _t(gw, dev)).sum() + 5.0 * loss).backward()
    return zq.detach(), loss.detach(), perp, enc, idx, zt.grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_ema_vector_quantizer(dev, name):
    g, z, E, gw, cs0 = _case(name)
    B, D, H, W, K = R.CASES[name]
    N = B * H * W
    oracle = _oracle()
    o = oracle.vq_assign_nchw(z, E, None)
    # ---- eval: the reference's outputs, the parameters untouched
    e = _make_ema(dev, K, D, E, cs0).eval()
    before = _params(e)
    zq, loss, perp, enc, idx, zgrad = _ema_forward(e, z, gw, dev)
    assert tuple(idx.shape) == (N,)
    _check_stats(g, "ema", K, perp, enc, idx)
    assert np.array_equal(_bits(zq.cpu().numpy()), _bits(o["zq"])) and C.crc(zq.cpu().numpy()) == g["ema_zq_crc"]
    assert C.loss_close(float(loss), g["ema_loss"])
    assert _close(zgrad.cpu().numpy(), g["ema_z_grad"], 1e-6)
    assert all(torch.equal(a, b) for a, b in zip(before, _params(e)))
    # ---- training with update = False: the same outputs, the parameters untouched
    e2 = _make_ema(dev, K, D, E, cs0).train()
    e2.embedding.update = False
    zq2, loss2, perp2, enc2, idx2, _ = _ema_forward(e2, z, gw, dev)
    assert torch.equal(zq2, zq) and torch.equal(loss2, loss) and torch.equal(idx2, idx) and torch.equal(enc2, enc)
    assert all(torch.equal(a, b) for a, b in zip(before, _params(e2)))
    # ---- one training step: outputs from the OLD weight, parameters against the float64 restatement on the returned codes
    e3 = _make_ema(dev, K, D, E, cs0).train()
    e3.want_encodings = False
    zq3, loss3, perp3, enc3, idx3, zgrad3 = _ema_forward(e3, z, gw, dev)
    assert enc3 is None and torch.equal(zq3, zq) and torch.equal(loss3, loss) and torch.equal(idx3, idx)
    assert np.array_equal(_bits(zgrad3.cpu().numpy()), _bits(zgrad.cpu().numpy()))    # backward reads the forward-time rows, not the updated weight
    assert np.array_equal(_bits(perp3.cpu().numpy()), _bits(perp.cpu().numpy()))
    cs, avg, w = R.ema_step(z, idx3.cpu().numpy(), cs0, E * cs0[:, None])
    w_new, cs_new, avg_new = (p.cpu().numpy() for p in _params(e3))
    for what, got, ref in (("cluster_size", cs_new, cs), ("embed_avg", avg_new, avg), ("weight", w_new, w)):
        err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
        print("%s %s: max |got - ref| / max |ref| = %.3g" % (name, what, err))
        assert err < 1e-5, (what, err)
    rows = g["step_rows"].astype(np.int64)                                             # and the reference's own step, where recorded
    assert _close(cs_new, g["step_cluster_size"], 1e-5) and _close(avg_new[rows], g["step_embed_avg"], 1e-5)
    assert _close(w_new[rows], g["step_weight"], 1e-5)
    # ---- the next forward uses the updated weight
    e3.eval()
    with torch.no_grad():
        zq4, _, (_, _, idx4) = e3(_t(z, dev))
    assert not np.array_equal(w_new, E)
    o2 = oracle.vq_assign_nchw(z, w_new, None)
    assert np.array_equal(idx4.cpu().numpy(), o2["codes"].reshape(-1))
    assert np.array_equal(_bits(zq4.cpu().numpy()), _bits(o2["zq"])) and not torch.equal(zq4, zq)      # rows of the NEW weight


@pytest.mark.gpu
def test_ema_training_step_at_three_channels(dev):
    """D = 3 runs the assign at 4 channels (one zero channel) but the EMA kernels at 3: codes and z_q against the oracle (pinned
    for this fixture by tests/test_narrow_width.py), the step against the float64 restatement, the gradient against its formula"""
    from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer
    g = np.load(os.path.join(C.GOLDEN, "narrow_D3.npz"))
    z, E = g["trained_z"], g["trained_E"]
    B, D, K = z.shape[0], z.shape[1], E.shape[0]
    assert D == 3
    cs0 = synth.uniform(8500, (K,), 0.5, 4.0)
    gw = synth.normal(8501, z.shape)
    o = _oracle().vq_assign_nchw(z, E, None)
    assert np.array_equal(o["codes"], g["trained_vqg_codes"].reshape(B, -1))
    e = _make_ema(dev, K, D, E, cs0).train()
    zq, loss, perp, enc, idx, zgrad = _ema_forward(e, z, gw, dev)
    codes = idx.cpu().numpy()
    assert np.array_equal(codes, o["codes"].reshape(-1)) and np.array_equal(_bits(zq.cpu().numpy()), _bits(o["zq"]))
    assert C.loss_close(float(loss), R.BETA * o["sqerr"] / o["numel"])
    assert np.array_equal(enc.cpu().numpy(), R.onehot(codes, K))
    rows = np.moveaxis(E[o["codes"]], 2, 1).reshape(z.shape)
    want = gw.astype(np.float64) + 5.0 * R.BETA * 2.0 / z.size * (z.astype(np.float64) - rows)
    assert _close(zgrad.cpu().numpy(), want, 1e-6)
    cs, avg, w = R.ema_step(z, codes, cs0, E * cs0[:, None])
    w_new, cs_new, avg_new = (p.cpu().numpy() for p in _params(e))
    for what, got, ref in (("cluster_size", cs_new, cs), ("embed_avg", avg_new, avg), ("weight", w_new, w)):
        err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
        print("D=3 %s: max |got - ref| / max |ref| = %.3g" % (what, err))
        assert err < 1e-5, (what, err)
    e.eval()
    with torch.no_grad():
        zq2, _, (_, _, idx2) = e(_t(z, dev))
    o2 = _oracle().vq_assign_nchw(z, w_new, None)
    assert np.array_equal(idx2.cpu().numpy(), o2["codes"].reshape(-1)) and np.array_equal(_bits(zq2.cpu().numpy()), _bits(o2["zq"]))


@pytest.mark.gpu
def test_ema_eval_forward_in_a_graph(dev):
    g, z, E, gw, cs0 = _case("b")
    B, D, H, W, K = R.CASES["b"]
    e = _make_ema(dev, K, D, E, cs0).eval()
    static_z = _t(z, dev)
    with torch.no_grad():
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                e(static_z)                                                            # warm-up on the capturing stream
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            zq, loss, (perp, enc, idx) = e(static_z)
        z2 = _t(synth.z_tokens(E, B, H, W, 8777), dev)
        static_z.copy_(z2)
        graph.replay()
        torch.cuda.synchronize(dev)
        zq_e, loss_e, (perp_e, enc_e, idx_e) = e(z2)
    assert torch.equal(zq, zq_e) and torch.equal(idx, idx_e) and torch.equal(enc, enc_e)
    assert np.array_equal(_bits(perp.cpu().numpy()), _bits(perp_e.cpu().numpy())) and C.loss_close(float(loss), float(loss_e))
    assert not torch.equal(idx_e, _t(g["ema_codes"].astype(np.int64), dev))            # (the replay saw the new input)


@pytest.mark.gpu
def test_sequence_quantizer(dev):
    from dynamicvectorquantization_amd.quantize import VectorQuantizer2Seq
    g = _golden("seq")
    B, D, L, K = R.SEQ
    z, E = R.seq_inputs()
    assert C.crc(z) == g["z_crc"] and C.crc(E) == g["E_crc"]
    o = _oracle().vq_assign_nchw(z, E, None)
    for legacy in (True, False):
        s = "_legacy%d" % int(legacy)
        m = VectorQuantizer2Seq(K, D, R.BETA, legacy=legacy).to(dev).eval()
        m.embedding.weight.data.copy_(_t(E, dev))
        with torch.no_grad():
            zq, loss, (p, e, idx) = m(_t(z, dev))
        assert p is None and e is None and tuple(idx.shape) == (B * L,) and tuple(zq.shape) == (B, D, L)
        assert np.array_equal(idx.cpu().numpy(), g["codes" + s].astype(np.int64))
        assert np.array_equal(_bits(zq.cpu().numpy()), _bits(o["zq"])) and C.crc(zq.cpu().numpy()) == g["zq_crc" + s]
        assert C.loss_close(float(loss), g["loss" + s])
    entry = m.get_codebook_entry(idx, (B, L, D))
    assert tuple(entry.shape) == (B, D, L) and C.crc(entry.cpu().numpy()) == g["entry_crc"]
