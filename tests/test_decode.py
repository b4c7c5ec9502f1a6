"""The fused decode head (codes -> the input of the decoder's conv_in): golden data of the reference's own decode_to_img chain
(tools/gen_golden_decode.py), the numpy restatement in tests/_decode_ref.py, and the kernels through module -> ctypes -> ABI.

Bounds.  conv: 1e-5 * M with M = |E||W|^T + |b| against the float64 conv, the contract include/dvq.h states for every 1x1 conv of
this project; two float32 convs compared with each other get 2e-5 * M.  adds: 4 * 2^-24 * (|T| + |F| + |L|), the four roundings of
the two adds on both sides.  DELTA_F: the fourier table is sin() of a 2-term conv, evaluated on the device here and on the CPU in
the golden; measured max |F_gpu - F_golden| = 4.81e-07 (tools/decode_time.py -> profiles/decode.json), asserted at four times
that, capped at the latent tolerance 1e-5.
"""
import numpy as np
import pytest
import torch
from torch import nn

from dynamicvectorquantization_amd import _lib, synth
from tests import _decode_ref as R

DELTA_F_MEASURED = 4.81e-07
DELTA_F = min(4.0 * DELTA_F_MEASURED, 1e-5)
SMALL = ("decode_head_fourier", "decode_head_toy")


def _params(name, g):
    """codebook rows (as get_codebook_entry indexes them), conv weight [C, D, 1, 1], bias -- regenerated from the fixture's seeds"""
    s = g["meta"]["seeds"]
    if name == "decode_head_dual":
        E = synth.codebook_trained(1024, 256)
        assert R.crc(E) == int(g["cb_crc"])
        E = np.concatenate([E, np.zeros((1, 256), np.float32)])          # VQEmbedding's padding row: no fixture code uses it
        C, D = 256, 256
        cw, cb = synth.normal(s["conv_w"], (C, D, 1, 1), 0.0, 1.0 / 16.0), synth.normal(s["conv_b"], (C,), 0.0, 0.1)
    else:
        rows, D, C = int(g["rows"]), int(g["D"]), int(g["C"])
        E = synth.normal(s["codebook"], (rows, D), 0.0, 1.0)
        assert R.crc(E) == int(g["cb_crc"])
        cw, cb = synth.normal(s["conv_w"], (C, D, 1, 1), 0.0, 1.0 / 16.0), synth.normal(s["conv_b"], (C,), 0.0, 0.1)
    assert R.crc(cw) == int(g["conv_w_crc"]) and R.crc(cb) == int(g["conv_b_crc"])
    return E, cw, cb


@pytest.mark.parametrize("name", ("decode_head_dual",) + SMALL)
def test_restatement_matches_golden(name):
    """|h_in_golden - head(T64 -> f32, F, L, codes)| <= 1e-5 * M[code] + 4 * 2^-24 * (|T| + |F| + |L|).  Measured when the fixtures
    were made: the reference's CPU conv sits at 2.9e-7 * M."""
    g = R.load(name)
    E, cw, cb = _params(name, g)
    codes = g["codes"].astype(np.int64)
    F, L = g.get("pos_first"), g.get("pos_second")
    assert (F is not None, L is not None) == {"fourier+learned": (True, True), "fourier": (True, False),
                                               "learned": (False, False)}[str(g["position_type"])]
    if name == "decode_head_dual":
        assert R.crc(F) == int(g["pos_first_crc"]) and R.crc(L) == int(g["pos_second_crc"]) and R.crc(g["h_in"]) == int(g["h_in_crc"])
        assert codes.min() >= 0 and codes.max() <= 1023
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    ref = R.head(T64.astype(np.float32), F, L, codes)
    err = np.abs(g["h_in"].astype(np.float64) - ref)
    tol = R.bound(M, T64, F, L, codes, 1e-5)
    print(name, "max err / bound %.3g" % float((err / tol).max()))
    assert (err <= tol).all()


def test_head_restatement_rules():
    T = np.arange(12, dtype=np.float32).reshape(3, 4)
    F = np.full((4, 1, 2), 0.5, np.float32)
    h = R.head(T, F, None, np.array([[[2, -1]], [[3, 0]]]))
    assert h.shape == (2, 4, 1, 2)
    assert np.array_equal(h[0, :, 0, 0], T[2] + 0.5) and np.isnan(h[0, :, 0, 1]).all()
    assert np.isnan(h[1, :, 0, 0]).all() and np.array_equal(h[1, :, 0, 1], T[0] + 0.5)


def test_module_and_abi_surface():
    """fails on a build without the feature: the module, the three entry points and ABI 0.10.0"""
    import dynamicvectorquantization_amd.decode as decode
    L = _lib.lib
    for name in ("dvq_decode_table_bytes", "dvq_decode_table_prepare_f32", "dvq_decode_head_f32"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.dvq_version() >= 1000
    assert L.dvq_decode_table_bytes(1025, 256) >= 1025 * 256 * 4 and L.dvq_decode_table_bytes(0, 256) == 0
    # validation that needs no device
    assert L.dvq_decode_head_f32(0, 1, 1, 0, 1, 4, 0, 0, 0, 0) == -1 and b"null" in L.dvq_last_error_string()
    assert L.dvq_decode_head_f32(16, 1, 1, 16, 1, 6, 0, 0, 16, 0) == -1                      # C % 4
    assert L.dvq_decode_head_f32(16, 1, 1, 16, 1, 1028, 0, 0, 16, 0) == -1                   # C > 1024
    assert L.dvq_decode_head_f32(16, 1, 0, 16, 1, 4, 0, 0, 16, 0) == -1                      # HW < 1
    assert L.dvq_decode_head_f32(16, 1, 1, 20, 1, 4, 0, 0, 16, 0) == -1                      # table alignment
    assert L.dvq_decode_table_prepare_f32(16, 4, 8, 16, 0, 4, 16, 16, 0) == -3               # table buffer too small
    assert L.dvq_decode_table_prepare_f32(16, 4, 8, 0, 0, 4, 0, 0, 0) == -1                  # no conv: C must equal D
    assert L.dvq_decode_table_prepare_f32(16, 4, 8, 0, 0, 8, 0, 0, 0) == 0                   # no conv: nothing to build
    S = R.stub_modules()
    emb = nn.Embedding(17, 8)
    conv = nn.Conv2d(8, 4, 1)
    head = decode.DecodeHead(emb, conv, S.Decoder(4, 2, "fourier+learned"))
    codes = torch.zeros((1, 2, 2), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="inference only"):
        head.from_codes(codes)
    with torch.no_grad(), pytest.raises(_lib.DvqError, match="GPU only"):
        head.from_codes(codes)
    with pytest.raises(NotImplementedError):
        decode.DecodeHead(emb, conv, S.Decoder(4, 2, "relative"))
    with pytest.raises(NotImplementedError):
        decode.DecodeHead(emb, conv, S.Decoder(4, 2, "full"))
    assert decode.DecodeHead(emb, conv, S.Decoder(4, 2, "learned"))._positions == ()
    assert decode.DecodeHead(emb, conv, S.Decoder(4, 2, "learned-relative"))._positions == ()
    assert [k for k, _ in decode.DecodeHead(emb, conv, S.Decoder(4, 2, "fourier"))._positions] == ["fourier"]
    assert [k for k, _ in head._positions] == ["fourier", "learned"]
    assert decode.DecodeHead(emb, conv, nn.Conv2d(4, 4, 3))._positions == ()                  # a decoder without position attributes
    with pytest.raises(TypeError):
        decode.DecodeHead(emb, nn.Conv2d(8, 4, 3))


# ------------------------------------------------------------------------------------------------------------- GPU
def _raw_head(codes, T, F, L):
    """the kernel through ctypes: codes [B, H, W] int64, T [rows, C], F / L [C, H, W] or None (device tensors)"""
    B, H, W = codes.shape
    rows, C = T.shape
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=codes.device)
    _lib.check(_lib.lib.dvq_decode_head_f32(codes.data_ptr(), B, H * W, T.data_ptr(), rows, C, _lib.ptr(F), _lib.ptr(L),
                                            out.data_ptr(), _lib.stream_ptr(codes.device)), "dvq_decode_head_f32")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 256, 32, 32), (3, 128, 8, 8), (2, 64, 5, 13), (1, 4, 1, 1)])
@pytest.mark.parametrize("tables", ["FL", "F", "L", "none"])
def test_kernel_exact(dev, shape, tables):
    B, C, H, W = shape
    rows = 1025
    seed = 4100 + C + H
    T = synth.normal(seed, (rows, C), 0.0, 1.0)
    F = synth.normal(seed + 1, (C, H, W), 0.0, 1.0) if "F" in tables else None
    L = synth.normal(seed + 2, (C, H, W), 0.0, 0.02) if "L" in tables else None
    codes = synth.randint(seed + 3, (B, H, W), rows).astype(np.int64)
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    out = _raw_head(t(codes), t(T), t(F), t(L))
    assert torch.equal(out.cpu(), torch.from_numpy(R.head(T, F, L, codes)))


@pytest.mark.gpu
def test_kernel_exact_unaligned_tables(dev):
    """position tables and output at a 4-byte offset: the 4-byte form, the same values"""
    B, C, H, W = 2, 64, 8, 8
    T = synth.normal(4201, (33, C), 0.0, 1.0)
    F, L = synth.normal(4202, (C, H, W), 0.0, 1.0), synth.normal(4203, (C, H, W), 0.0, 0.02)
    codes = synth.randint(4204, (B, H, W), 33).astype(np.int64)
    off = lambda a: torch.cat([torch.zeros(1), torch.from_numpy(a).reshape(-1)]).to(dev)[1:].view(a.shape)
    Fd, Ld = off(F), off(L)
    assert Fd.data_ptr() % 16 == 4
    buf = torch.empty(B * C * H * W + 1, device=dev)
    out = buf[1:].view(B, C, H, W)
    cd, Td = torch.from_numpy(codes).to(dev), torch.from_numpy(T).to(dev)
    _lib.check(_lib.lib.dvq_decode_head_f32(cd.data_ptr(), B, H * W, Td.data_ptr(), 33, C, Fd.data_ptr(), Ld.data_ptr(),
                                            out.data_ptr(), _lib.stream_ptr(dev)), "decode_head")
    assert torch.equal(out.cpu(), torch.from_numpy(R.head(T, F, L, codes)))


@pytest.mark.gpu
def test_kernel_exact_large_batch_crc(dev):
    B, C, H, W, rows = 256, 256, 32, 32, 1025
    T = synth.normal(4301, (rows, C), 0.0, 1.0)
    F, L = synth.normal(4302, (C, H, W), 0.0, 1.0), synth.normal(4303, (C, H, W), 0.0, 0.02)
    codes = synth.randint(4304, (B, H, W), rows).astype(np.int64)
    t = lambda a: torch.from_numpy(a).to(dev)
    out = _raw_head(t(codes), t(T), t(F), t(L)).cpu().numpy()
    for b in range(B):
        assert R.crc(out[b]) == R.crc(R.head(T, F, L, codes[b:b + 1])[0]), b


@pytest.mark.gpu
def test_kernel_out_of_range_codes(dev):
    B, C, H, W, rows = 1, 128, 8, 8, 513
    T = synth.normal(4401, (rows, C), 0.0, 1.0)
    F = synth.normal(4402, (C, H, W), 0.0, 1.0)
    codes = synth.randint(4403, (B, H, W), rows).astype(np.int64)
    codes[0, 0, 0], codes[0, 3, 5], codes[0, 7, 7] = -1, rows, rows - 1
    t = lambda a: torch.from_numpy(a).to(dev)
    out = _raw_head(t(codes), t(T), t(F), None).cpu().numpy()
    ref = R.head(T, F, None, codes)
    assert np.isnan(out[0, :, 0, 0]).all() and np.isnan(out[0, :, 3, 5]).all()
    assert np.array_equal(out[0, :, 7, 7], (T[rows - 1] + F[:, 7, 7]).astype(np.float32))
    assert np.array_equal(out, ref, equal_nan=True) and int(np.isnan(out).sum()) == 2 * C


def _table_gpu(dev, E, cw, cb):
    rows, D = E.shape
    C = cw.shape[0]
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    Ed, Wd, bd = t(E), t(cw.reshape(C, D)), t(cb)
    n = _lib.lib.dvq_decode_table_bytes(rows, C)
    buf = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.dvq_decode_table_prepare_f32(Ed.data_ptr(), rows, D, Wd.data_ptr(), _lib.ptr(bd), C, buf.data_ptr(), n,
                                                     _lib.stream_ptr(dev)), "dvq_decode_table_prepare_f32")
    return buf[:rows * C * 4].view(torch.float32).view(rows, C).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("rdc", [(1025, 256, 256), (16385, 256, 256), (513, 64, 128)])
@pytest.mark.parametrize("bias", [True, False])
def test_table(dev, rdc, bias):
    rows, D, C = rdc
    E = synth.normal(4500 + rows, (rows, D), 0.0, 1.0)
    cw = synth.normal(4501 + rows, (C, D, 1, 1), 0.0, 1.0 / 16.0)
    cb = synth.normal(4502 + rows, (C,), 0.0, 0.1) if bias else None
    T = _table_gpu(dev, E, cw, cb)
    err = np.abs(T.astype(np.float64) - R.table64(E, cw, cb))
    M = R.magnitude(E, cw, cb)
    print(rdc, bias, "max err / M %.3g" % float((err / M).max()))
    assert (err <= 1e-5 * M).all()
    assert np.array_equal(T, _table_gpu(dev, E, cw, cb))                 # a fixed summation order: the same bits


def _vq(dev, kind, rows_arg, D, E):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2
    if kind == "VectorQuantize2":
        q = VectorQuantize2(rows_arg, D).to(dev).eval()
        w = q.codebook.weight
    else:
        q = VectorQuantizer2(rows_arg, D, beta=0.25).to(dev).eval()
        w = q.embedding.weight
    with torch.no_grad():
        w.copy_(torch.from_numpy(E).to(dev))
    return q


def _conv(dev, cw, cb):
    conv = nn.Conv2d(cw.shape[1], cw.shape[0], 1).to(dev).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(cw).to(dev))
        conv.bias.copy_(torch.from_numpy(cb).to(dev))
    return conv


def _decoder(dev, g, C, hw):
    S = R.stub_modules()
    dec = S.Decoder(C, hw, str(g["position_type"])).to(dev).eval()
    sd = {k[6:]: torch.from_numpy(g[k]) for k in g if k.startswith("param/")}
    missing, unexpected = dec.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("conv_in") for k in missing)
    return dec


@pytest.mark.gpu
def test_no_conv_table_is_the_codebook(dev):
    from dynamicvectorquantization_amd.decode import DecodeHead
    E = synth.normal(4601, (17, 64), 0.0, 1.0)
    q = _vq(dev, "VectorQuantize2", 16, 64, E)
    head = DecodeHead(q)
    with torch.no_grad():
        assert torch.equal(head.table(), q.codebook.weight)
        codes = torch.from_numpy(synth.randint(4602, (2, 5, 7), 17).astype(np.int64)).to(dev)
        out = head.from_codes(codes)
    assert torch.equal(out.cpu(), torch.from_numpy(R.head(E, None, None, codes.cpu().numpy())))


@pytest.mark.gpu
def test_golden_end_to_end(dev, golden_dir):
    """DecodeHead.from_tokens on the fixture's token streams against the h_in the reference's decode_to_img chain fed to conv_in:
    <= 2e-5 * M + 4 * 2^-24 * (|T| + |F| + |L|) + DELTA_F"""
    import os
    from dynamicvectorquantization_amd.decode import DecodeHead
    from dynamicvectorquantization_amd.permuter import DualGrainSeperatePermuter
    g = R.load("decode_head_dual")
    E, cw, cb = _params("decode_head_dual", g)
    q = _vq(dev, "VectorQuantize2", 1024, 256, E)
    head = DecodeHead(q, _conv(dev, cw, cb), _decoder(dev, g, 256, 32))
    p = np.load(os.path.join(golden_dir, "permuter_reference_selftest.npz"))
    streams = [torch.from_numpy(p["region_" + k][:1].astype(np.int64)).to(dev)
               for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]
    with torch.no_grad():
        out = head.from_tokens(DualGrainSeperatePermuter(), *streams).cpu().numpy()
        Fg, Lg = [t.cpu().numpy().reshape(256, 32, 32) for t in head.position_tables(32, 32, dev)]
    dF = float(np.abs(Fg - g["pos_first"]).max())
    print("max |F_gpu - F_golden| = %.3g" % dF)
    assert np.array_equal(Lg, g["pos_second"])                           # one float32 add per element: the same bits everywhere
    assert dF <= DELTA_F
    codes = g["codes"].astype(np.int64)
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    err = np.abs(out.astype(np.float64) - g["h_in"])
    tol = R.bound(M, T64, g["pos_first"], g["pos_second"], codes, 2e-5) + DELTA_F
    print("max err / bound %.3g" % float((err / tol).max()))
    assert (err <= tol).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_golden_small_dispatch(dev, name):
    from dynamicvectorquantization_amd.decode import DecodeHead
    g = R.load(name)
    E, cw, cb = _params(name, g)
    rows, D, C = int(g["rows"]), int(g["D"]), int(g["C"])
    kind = str(g["quantizer"])
    q = _vq(dev, kind, rows - 1 if kind == "VectorQuantize2" else rows, D, E)
    head = DecodeHead(q, _conv(dev, cw, cb), _decoder(dev, g, C, 8))
    codes = g["codes"].astype(np.int64)
    with torch.no_grad():
        out = head.from_codes(torch.from_numpy(codes).to(dev)).cpu().numpy()
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    err = np.abs(out.astype(np.float64) - g["h_in"])
    assert (err <= R.bound(M, T64, g.get("pos_first"), g.get("pos_second"), codes, 2e-5) + DELTA_F).all()


def _toy_head(dev, seed=4700, position_type="fourier+learned", C=64, D=32, rows=33, hw=8):
    from dynamicvectorquantization_amd.decode import DecodeHead
    S = R.stub_modules()
    torch.manual_seed(seed)
    E = synth.normal(seed + 1, (rows, D), 0.0, 1.0)
    cw, cb = synth.normal(seed + 2, (C, D, 1, 1), 0.0, 1.0 / 16.0), synth.normal(seed + 3, (C,), 0.0, 0.1)
    q = _vq(dev, "VectorQuantize2", rows - 1, D, E)
    conv = _conv(dev, cw, cb)
    dec = S.Decoder(C, hw, position_type).to(dev).eval()
    return DecodeHead(q, conv, dec), q, conv, dec


def _expect(head, q, conv, dec, codes):
    """head() over the float64 table of the CURRENT parameters and the decoder's own position tables: (reference, tolerance)"""
    E = q.codebook.weight.detach().cpu().numpy()
    cw, cb = conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy()
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    H, W = codes.shape[1:]
    with torch.no_grad():
        z = torch.zeros((1, conv.out_channels, H, W), device=codes.device)
        F = dec.position_bias_fourier(z)[0].cpu().numpy()
        L = dec.position_bias_learned(z)[0].cpu().numpy()
    c = codes.cpu().numpy()
    return R.head(T64.astype(np.float32), F, L, c), R.bound(M, T64, F, L, c, 1e-5)


def _close(out, ref_tol):
    ref, tol = ref_tol
    return bool((np.abs(out.cpu().numpy().astype(np.float64) - ref) <= tol).all())


@pytest.mark.gpu
def test_cache_follows_parameters(dev):
    head, q, conv, dec = _toy_head(dev)
    codes = torch.from_numpy(synth.randint(4710, (3, 8, 8), 33).astype(np.int64)).to(dev)
    with torch.no_grad():
        first = head.from_codes(codes)
        assert _close(first, _expect(head, q, conv, dec, codes))
        assert torch.equal(head.from_codes(codes), first)                 # the cached tables
        # load_state_dict copies in place: the parameters' versions change, the tables follow
        conv.load_state_dict({"weight": conv.weight * 1.5, "bias": conv.bias + 0.25})
        dec.load_state_dict({k: v * 0.5 for k, v in dec.state_dict().items()})
        second = head.from_codes(codes)
        assert not torch.equal(second, first) and _close(second, _expect(head, q, conv, dec, codes))
        # a write through .data is invisible to the key: stale until invalidate()
        q.codebook.weight.data.mul_(2.0)
        dec.position_bias_learned.row_embed.weight.data.add_(0.125)
        assert torch.equal(head.from_codes(codes), second)
        head.invalidate()
        third = head.from_codes(codes)
        assert not torch.equal(third, second) and _close(third, _expect(head, q, conv, dec, codes))


@pytest.mark.gpu
def test_second_stream_and_graph(dev):
    from dynamicvectorquantization_amd.encode import StreamSlots
    head, q, conv, dec = _toy_head(dev, seed=4800)
    codes = torch.from_numpy(synth.randint(4810, (4, 8, 8), 33).astype(np.int64)).to(dev)
    with torch.no_grad():
        slots = StreamSlots(2, dev)
        outs = []
        for _ in range(3):                                                # the first slot builds the tables, the second waits for them
            with slots.next():
                outs.append(head.from_codes(codes))
        slots.join()
        torch.cuda.synchronize(dev)
        ref = _expect(head, q, conv, dec, codes)
        assert all(_close(o, ref) for o in outs) and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        # graph capture: one launch, no allocation inside but the output, no parallel branches
        static_codes = codes.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            head.from_codes(static_codes)                                 # warm-up on the capturing stream
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            static_out = head.from_codes(static_codes)
        new_codes = torch.from_numpy(synth.randint(4811, (4, 8, 8), 33).astype(np.int64)).to(dev)
        static_codes.copy_(new_codes)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(static_out, head.from_codes(new_codes))


@pytest.mark.gpu
def test_fused_decode_to_img(dev):
    """FusedDecode.decode_to_img against the torch-op chain of the stub Dualformer on the GPU: the tensors conv_in reads differ by
    at most 2e-5 * M + 4 * 2^-24 * (...) (both position tables come from the same modules on the same device), and the images
    by conv_in applied to that difference"""
    from dynamicvectorquantization_amd.decode import FusedDecode
    from dynamicvectorquantization_amd.permuter import DualGrainSeperatePermuter
    S = R.stub_modules()
    head, q, conv, dec = _toy_head(dev, seed=4900, C=64, D=32, rows=1025, hw=32)
    fs = S.FirstStage(q, conv, dec).to(dev).eval()

    class Fused(FusedDecode, S.Dualformer):
        pass

    perm = DualGrainSeperatePermuter()
    plain, fused = S.Dualformer(fs, perm), Fused(fs, perm)
    import os
    from tests.conftest import GOLDEN
    p = np.load(os.path.join(GOLDEN, "permuter_reference_selftest.npz"))
    streams = [torch.from_numpy(p["region_" + k].astype(np.int64)).to(dev)
               for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]
    cap = {}
    hook = dec.conv_in.register_forward_pre_hook(lambda m, a: cap.setdefault("h", []).append(a[0].detach().clone()))
    img_ref = plain.decode_to_img(*streams)
    img = fused.decode_to_img(*streams)
    hook.remove()
    h_ref, h = cap["h"]
    codes = perm.forward_back(*streams)
    E, cw, cb = q.codebook.weight.detach().cpu().numpy(), conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy()
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    with torch.no_grad():
        F, L = [t.cpu().numpy().reshape(64, 32, 32) for t in fused.decode_head().position_tables(32, 32, dev)]
    tol = R.bound(M, T64, F, L, codes.cpu().numpy(), 2e-5)
    err = np.abs(h.cpu().numpy().astype(np.float64) - h_ref.cpu().numpy())
    print("max err / bound %.3g" % float((err / tol).max()))
    assert (err <= tol).all()
    # the images: conv_in is linear, so they differ by at most |W_in| applied to the bound above, plus the conv's own float32
    # error on both sides (2 x 1e-5 * sum |w||x|, the conv contract again)
    w_abs = dec.conv_in.weight.detach().abs().double().cpu()
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    tol_img = nn.functional.conv2d(as_t(tol), w_abs, padding=1) + 2e-5 * (
        nn.functional.conv2d(as_t(np.abs(h_ref.cpu().numpy())), w_abs, padding=1) + dec.conv_in.bias.detach().abs().double().cpu()[None, :, None, None])
    assert img.shape == img_ref.shape and bool(((img.double().cpu() - img_ref.double().cpu()).abs() <= tol_img).all())
