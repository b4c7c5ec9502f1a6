"""The fused decode head (csrc/decode_head.hip: decode_head_kernel<VEC>, decode_table_kernel), the embedding gather whose NaN rule
it cites (csrc/route_select.hip: embed_gather_kernel) and decode.DecodeHead / FusedDecode, at the shapes, codes and values that
tests/test_decode.py never ran.  The case table, the restated launch dispatch and the guarded buffers are in tests/_decode_ref.py;
a CPU test asserts that the table reaches both forms of the head (and each single cause of the 4-byte form), every token and
channel edge of the 64 x 64 block, so a dropped case is noticed here and not on the device.

Head.  Every case with the position tables FL, F, L and none, against R.head (float32 numpy fl(fl(T[code] + F) + L)), compared on
the uint32 view wherever the reference is not NaN, with the NaNs in the same places.  The output is a slice of a device buffer
pre-filled with a NaN of a payload no result can have: 4 KiB on each side stay untouched, no word inside keeps the filling.
Codes -1, rows, 2^32, 2^32 + 5, 2^40, INT64_MIN and INT64_MAX at token 0, N - 1, 63, 64 and inside a 4-token group of valid
codes: C NaNs per such token, the reference's bits elsewhere; rows = 1, 3 and 70000.  -0.0, +-Inf, NaN and subnormals in T, F, L.
Table.  |T - T64| <= min(1e-5, (D + 2) 2^-24) M against the float64 conv (R.table_rel), the same bits twice, a row's bits do not
depend on its place in the 8-row group, nothing written past rows C words, a NaN / Inf stays in its row / column.
Gather.  dvq_embed_gather_f32 against E[idx] on bits, up to the second trip of its grid-stride loop (n = 4100, D = 1024).
Not covered: rows * C >= 2^31, the size_t offset arithmetic of the row gather -- it needs an 8 GiB table.

DecodeHead, class by class (every nn.Module class that quantize.py, lucid.py and rq.py define, and a bare nn.Embedding):
  decodes, bit for bit its own get_codebook_entry laid out NCHW: nn.Embedding, VQEmbedding, VectorQuantize2 and VectorQuantize2List
    (the padding row K included), VectorQuantizer2, VectorQuantizer2Seq, VectorQuantizer, MaskVectorQuantize, VectorQuantize (L2 and
    cosine: both gather the raw rows);
  refuses with NotImplementedError: VectorQuantizer2 / VectorQuantizer2Seq with a remap;
  refuses with TypeError: GumbelQuantize, GumbelQuantizeFused, EmbeddingEMA, EMAVectorQuantizer, lucid.EuclideanCodebook,
    lucid.CosineSimCodebook, lucid.VectorQuantize, rq.RQBottleneck (none keeps its rows in a `codebook` / `embedding` nn.Embedding).

What the cases see.  Five one-line variants of the kernels, built apart and never committed, every read and write of each inside
the buffers; the tests of this module that fail for each (all others pass):
  1 the code range test made after narrowing the code to int (2^32, 2^32 + 5 and INT64_MIN then name rows 0, 5 and 0):
    test_head_codes_out_of_range, all three cases; nothing else.
  2 vec write phase, image index taken from the block's first token instead of the group's: test_head_bits at every vec case
    whose block holds more than one image -- (3,68,2,2), (5,60,4,3), (2,132,6,6), (17,64,2,2), and (3,68,2,6) where a NULL table
    leaves the other two bases aligned -- with every table set; test_head_codes_out_of_range at the two vec cases,
    test_head_rows[1] and [3], test_head_special_values[vec], every decoding class of test_decode_head_every_quantizer_class,
    test_position_types at 6x6, test_other_inputs and test_fused_decode_head_follows_the_first_stage.  The scalar cases and the
    one-image cases (1,4,2,2), (1,1024,2,4) pass, as they must.
  3 the two position adds applied in the other order: test_head_bits[*-FL] at all fourteen cases, test_head_codes_out_of_range,
    test_head_rows and test_head_special_values (their FL runs).  The module tests compare within a bound and pass.
  4 the table kernel's k loop stops at D - 1: test_table_bound at all twelve cases, test_table_special_values, test_convs,
    test_position_types and test_fused_decode_head_follows_the_first_stage.  (Row independence holds for it, and passes.)
  5 the table kernel adds the bias for o < 256 only: test_table_bound[9-1024-260-bias] and [17-24-1024-bias],
    test_table_special_values and test_convs[260-24-bias].
"""
import inspect

import numpy as np
import pytest
import torch
from torch import nn

from dynamicvectorquantization_amd import _lib, synth
from tests import _decode_ref as R

ROWS = 1025
TABLE_SETS = ("FL", "F", "L", "none")
CASE_IDS = ["%dx%dx%dx%d+%d.%d.%d" % c for c in R.HEAD_CASES]
_T_CACHE = {}


def _T(rows, C):
    """the table of a head case, made once per (rows, C) and never written"""
    if (rows, C) not in _T_CACHE:
        _T_CACHE[rows, C] = synth.normal(5100 + C + rows, (rows, C), 0.0, 1.0)
        _T_CACHE[rows, C].setflags(write=False)
    return _T_CACHE[rows, C]


def _head_inputs(case, tables, rows=ROWS):
    B, C, H, W = case[:4]
    seed = 5200 + 8 * R.HEAD_CASES.index(tuple(case))
    F = synth.normal(seed + 1, (C, H, W), 0.0, 1.0) if "F" in tables else None
    L = synth.normal(seed + 2, (C, H, W), 0.0, 0.02) if "L" in tables else None
    codes = synth.randint(seed + 3, (B, H, W), rows).astype(np.int64)
    return _T(rows, C), F, L, codes


# ------------------------------------------------------------------------------------------------------------- CPU
def test_case_table_covers_every_form():
    got = set().union(*(R.case_items(c) for c in R.HEAD_CASES))
    missing = [i for i in R.FORM_ITEMS + R.TOKEN_ITEMS + R.CHANNEL_ITEMS if i not in got]
    assert not missing, missing
    forms = [R.form(*c) for c in R.HEAD_CASES]
    assert forms == ["vec"] * 6 + ["scalar"] * 8
    for c in R.HEAD_CASES[6:11]:                                          # scalar by shape: aligned bases
        assert (c[2] * c[3]) % 4 != 0 and c[4:] == (0, 0, 0)
    assert sorted(c[4:] for c in R.HEAD_CASES[11:]) == [(0, 0, 4), (0, 4, 0), (4, 0, 0)]
    for c in R.HEAD_CASES[11:]:                                           # scalar by alignment alone
        assert R.form(*c[:4]) == "vec"
    for c in R.HEAD_CASES:
        assert c[1] % 4 == 0 and c[0] * c[1] * c[2] * c[3] * 4 <= 1 << 20          # the ABI's C % 4; every output under 1 MiB


def test_restatement_rules():
    assert R.form(1, 4, 2, 2) == "vec" and R.form(1, 4, 1, 3) == "scalar" and R.form(1, 4, 1, 4, 16, 32, 48) == "vec"
    for k in range(3):
        for off in (4, 8, 12):
            offs = [0, 0, 0]
            offs[k] = off
            assert R.form(1, 4, 2, 2, *offs) == "scalar"
    assert R.blocks(1, 4, 2, 2) == (1, 1) and R.blocks(5, 60, 1, 13) == (2, 1) and R.blocks(2, 132, 6, 6) == (2, 3)
    assert R.blocks(1, 1024, 8, 8) == (1, 16) and R.blocks(1, 1028, 8, 8)[1] == 17
    # the bit comparison: signed zeros and subnormals differ, NaNs of any payload agree, a NaN against a number does not
    z = np.array([0.0, 1.0, np.nan], np.float32)
    assert R.same_bits(R.bits(z), z)
    assert not R.same_bits(R.bits(np.array([-0.0, 1.0, np.nan], np.float32)), z)
    assert not R.same_bits(R.bits(np.array([0.0, 1.0, 2.0], np.float32)), z)
    assert not R.same_bits(R.bits(np.array([0.0, np.nan, np.nan], np.float32)), z)
    assert R.same_bits(np.array([0, 0x3F800000, R.SENTINEL], np.uint32), z)
    assert not R.same_bits(R.bits(np.array([1e-45], np.float32)), np.array([0.0], np.float32))
    assert np.isnan(np.array([R.SENTINEL], np.uint32).view(np.float32)[0]) and R.SENTINEL != int(R.bits(np.float32(np.nan))[0])
    bad = R.bad_codes(7)
    assert len(bad) == 7 and ((bad < 0) | (bad >= 7)).all() and 7 in bad
    assert (bad.astype(np.int32)[[2, 3, 5]] == [0, 5, 0]).all()             # what a 32-bit comparison would take for rows
    # the guarded buffer notices a write on either side and a word that was never written
    dev = torch.device("cpu")
    g = R.Guarded(dev, 10, off=4)
    g.view.fill_(1.0)
    assert (g.result() == 0x3F800000).all()
    for where in (g.front - 1, g.front + 10):
        g = R.Guarded(dev, 10, off=4)
        g.view.fill_(1.0)
        g.whole[where] = 0
        with pytest.raises(AssertionError, match="a write"):
            g.result()
    g = R.Guarded(dev, 10)
    g.view[:9].fill_(1.0)
    with pytest.raises(AssertionError, match="never written"):
        g.result()
    g = R.Guarded(dev, 10, tail_words=6)
    g.view.fill_(1.0)
    g.whole[g.front + 12] = 0
    with pytest.raises(AssertionError, match="past the output"):
        g.result()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rdc", R.TABLE_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_table_chain_meets_bound(rdc, bias):
    """the bound of test_table_bound is one the arithmetic the kernel documents keeps on its own: the float32 chain on the CPU"""
    E, W, b = R.table_inputs(rdc, bias)
    err = np.abs(R.table_chain32(E, W, b).astype(np.float64) - R.table64(E, W, b))
    M = R.magnitude(E, W, b)
    rel = R.table_rel(rdc[1])
    print(rdc, "bias" if bias else "nobias", "cpu chain: max err / M %.3g, max err / bound %.3g" % (float((err / M).max()), float((err / (rel * M)).max())))
    assert rel <= 1e-5 and (err <= rel * M).all()


def _module_classes():
    from dynamicvectorquantization_amd import lucid, quantize, rq
    out = {}
    for mod in (quantize, lucid, rq):
        short = mod.__name__.rsplit(".", 1)[1]
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if issubclass(cls, nn.Module) and cls.__module__ == mod.__name__ and not name.startswith("_"):
                out["%s.%s" % (short, name)] = cls
    return out


K_Q, D_Q = 16, 8
_nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
_flat = lambda q, c: q.get_codebook_entry(c.reshape(-1), tuple(c.shape) + (D_Q,))


def _quantizers(used_path):
    """name -> (constructor, number of valid codes, the class's own decode of codes [B, H, W] to NCHW | the refusal's type)"""
    from dynamicvectorquantization_amd import lucid, quantize as Q, rq
    return {
        "nn.Embedding": (lambda: nn.Embedding(K_Q + 1, D_Q), K_Q + 1, lambda q, c: _nchw(q(c))),
        "quantize.VQEmbedding": (lambda: Q.VQEmbedding(K_Q, D_Q), K_Q + 1, lambda q, c: _nchw(q.embed(c))),
        "quantize.VectorQuantize2": (lambda: Q.VectorQuantize2(K_Q, D_Q), K_Q + 1, lambda q, c: _nchw(q.get_codebook_entry(c))),
        "quantize.VectorQuantize2List": (lambda: Q.VectorQuantize2List(K_Q, D_Q), K_Q + 1, lambda q, c: _nchw(q.get_codebook_entry(c))),
        "quantize.VectorQuantizer2": (lambda: Q.VectorQuantizer2(K_Q, D_Q, 0.25), K_Q, _flat),
        "quantize.VectorQuantizer2+remap": (lambda: Q.VectorQuantizer2(K_Q, D_Q, 0.25, remap=used_path), 7, NotImplementedError),
        "quantize.VectorQuantizer2Seq": (lambda: Q.VectorQuantizer2Seq(K_Q, D_Q, 0.25), K_Q,
                                         lambda q, c: q.get_codebook_entry(c.reshape(-1), (c.shape[0], c.shape[1] * c.shape[2], D_Q))
                                         .reshape(c.shape[0], D_Q, c.shape[1], c.shape[2])),
        "quantize.VectorQuantizer2Seq+remap": (lambda: Q.VectorQuantizer2Seq(K_Q, D_Q, 0.25, remap=used_path), 7, NotImplementedError),
        "quantize.VectorQuantizer": (lambda: Q.VectorQuantizer(K_Q, D_Q, 0.25), K_Q, _flat),
        "quantize.MaskVectorQuantize": (lambda: Q.MaskVectorQuantize(K_Q, D_Q), K_Q, _flat),
        "quantize.VectorQuantize": (lambda: Q.VectorQuantize(K_Q, D_Q), K_Q, lambda q, c: _nchw(q.get_codebook_entry(c))),
        "quantize.VectorQuantize+cosine": (lambda: Q.VectorQuantize(K_Q, D_Q, use_cosine_sim=True), K_Q,
                                           lambda q, c: _nchw(q.get_codebook_entry(c))),
        "quantize.GumbelQuantize": (lambda: Q.GumbelQuantize(64, D_Q, K_Q), K_Q, TypeError),
        "quantize.GumbelQuantizeFused": (lambda: Q.GumbelQuantizeFused(64, D_Q, K_Q), K_Q, TypeError),
        "quantize.EmbeddingEMA": (lambda: Q.EmbeddingEMA(K_Q, D_Q), K_Q, TypeError),
        "quantize.EMAVectorQuantizer": (lambda: Q.EMAVectorQuantizer(K_Q, D_Q, 0.25), K_Q, TypeError),
        "lucid.EuclideanCodebook": (lambda: lucid.EuclideanCodebook(D_Q, K_Q), K_Q, TypeError),
        "lucid.CosineSimCodebook": (lambda: lucid.CosineSimCodebook(D_Q, K_Q), K_Q, TypeError),
        "lucid.VectorQuantize": (lambda: lucid.VectorQuantize(K_Q, D_Q), K_Q, TypeError),
        "rq.RQBottleneck": (lambda: rq.RQBottleneck((4, 4, D_Q), (4, 4, 2), K_Q), K_Q, TypeError),
    }


QUANTIZER_NAMES = tuple(_quantizers(None))


@pytest.fixture
def used_path(tmp_path):
    path = str(tmp_path / "used.npy")
    np.save(path, np.array([3, 1, 4, 5, 9, 2, 6], dtype=np.int64))
    return path


def test_dispatch_names_every_class_and_refusals_raise(used_path):
    """the table above holds every nn.Module class the three modules define; the classes DecodeHead does not decode raise
    TypeError / NotImplementedError when it is constructed (no device needed), the others construct"""
    from dynamicvectorquantization_amd.decode import DecodeHead
    table = _quantizers(used_path)
    assert {n.split("+")[0] for n in table} - {"nn.Embedding"} == set(_module_classes())
    torch.manual_seed(5300)
    for name, (make, _, own) in table.items():
        q = make()
        if isinstance(own, type):
            with pytest.raises(own):
                DecodeHead(q)
        else:
            assert DecodeHead(q).channels == D_Q, name


# ------------------------------------------------------------------------------------------------------------- GPU: the head
def _run_head(dev, case, T, F, L, codes):
    """the kernel through ctypes into a guarded output; -> uint32 [B, C, H, W]"""
    B, C, H, W, off_out, off_F, off_L = case
    rows = T.shape[0]
    g = R.Guarded(dev, B * C * H * W, off_out)
    Fd, Ld = R.at_offset(dev, F, off_F), R.at_offset(dev, L, off_L)
    cd, Td = torch.tensor(np.ascontiguousarray(codes), device=dev), torch.tensor(np.ascontiguousarray(T), device=dev)
    assert cd.dtype == torch.int64 and tuple(cd.shape) == (B, H, W) and Td.data_ptr() % 16 == 0
    _lib.check(_lib.lib.dvq_decode_head_f32(cd.data_ptr(), B, H * W, Td.data_ptr(), rows, C, _lib.ptr(Fd), _lib.ptr(Ld),
                                            g.view.data_ptr(), _lib.stream_ptr(dev)), "dvq_decode_head_f32")
    return g.result().reshape(B, C, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("tables", TABLE_SETS)
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=CASE_IDS)
def test_head_bits(dev, case, tables):
    T, F, L, codes = _head_inputs(case, tables)
    assert R.same_bits(_run_head(dev, case, T, F, L, codes), R.head(T, F, L, codes))


def _planted(N):
    """token 0, N - 1, 63 and 64 where they exist, position 1 of the 4-token group 4..7 (its other three codes stay valid), and
    tokens far from those up to seven in all, so that one launch holds every bad code"""
    where = [0, N - 1, 5] + [t for t in (63, 64) if t < N - 1]
    extra = [t for t in (17, 30, 42, 11, 23) if t < N - 1 and t not in where]
    where += extra[:7 - len(where)]
    assert len(set(where)) == 7 and not {4, 6, 7} & set(where)
    return np.array(where)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [R.HEAD_CASES[3], R.HEAD_CASES[2], R.HEAD_CASES[8]], ids=["vec-2blocks", "vec-small", "scalar"])
def test_head_codes_out_of_range(dev, case):
    """each bad code at each planted token in turn (seven rotations): exactly C NaNs per planted token, the reference's bits at
    every other one.  rows = 1025 > 5, so 2^32, 2^32 + 5 and INT64_MIN would name the valid rows 0, 5 and 0 after a narrowing."""
    B, C, H, W = case[:4]
    N = B * H * W
    assert (R.form(*case), N > 64) == {3: ("vec", True), 2: ("vec", False), 8: ("scalar", True)}[R.HEAD_CASES.index(case)]
    where, bad = _planted(N), R.bad_codes(ROWS)
    for tables in ("FL", "none"):
        T, F, L, good = _head_inputs(case, tables)
        for rot in range(7):
            codes = good.copy()
            codes.reshape(-1)[where] = np.roll(bad, rot)
            out = _run_head(dev, case, T, F, L, codes)
            assert R.same_bits(out, R.head(T, F, L, codes)), (tables, rot)
            nan = np.isnan(out.view(np.float32))
            per_token = np.moveaxis(nan, 1, 3).reshape(N, C)
            assert int(nan.sum()) == 7 * C and per_token[where].all() and not np.delete(per_token, where, axis=0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 3, 70000])
def test_head_rows(dev, rows):
    """rows = 1 (every code 0), rows = 3, and rows = 70000 at C = 4 with codes above 65535"""
    if rows == 70000:
        case = R.HEAD_CASES[0]                                            # (1, 4, 2, 2)
        codes = np.array([[[69999, 65536], [3, 66000]]], dtype=np.int64)
    else:
        case = R.HEAD_CASES[1]                                            # (3, 68, 2, 2)
        codes = synth.randint(5400 + rows, (3, 2, 2), rows).astype(np.int64)
        codes[2, 1, 1] = rows - 1
    T, F, L, _ = _head_inputs(case, "FL", rows)
    assert R.same_bits(_run_head(dev, case, T, F, L, codes), R.head(T, F, L, codes))
    codes = codes.copy()
    codes.reshape(-1)[1] = rows                                           # one past the last row, whatever the row count
    out = _run_head(dev, case, T, F, L, codes)
    assert R.same_bits(out, R.head(T, F, L, codes)) and int(np.isnan(out.view(np.float32)).sum()) == case[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [R.HEAD_CASES[1], R.HEAD_CASES[6]], ids=["vec", "scalar"])
def test_head_special_values(dev, case):
    """-0.0, +-Inf, NaN and subnormals in T, F and L, channel by channel: -0.0 + -0.0 + -0.0 (stays -0.0), -0.0 + 0.0, Inf + -Inf
    (a NaN), Inf + Inf, subnormal + 0 + 0 and subnormal + subnormal (no flush to zero), a NaN from each of the three operands;
    the last rows of T hold -Inf and subnormals throughout"""
    B, C, H, W = case[:4]
    rows = 9
    T, F, L, _ = _head_inputs(case, "FL", rows)
    T, F, L = T.copy(), F.copy(), L.copy()
    sub = np.array([1, 2, 0x7FFFFF, 0x80000001], np.uint32).view(np.float32)          # subnormals, one negative
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    T[:7, 0], F[0], L[0] = -0.0, -0.0, -0.0
    T[:7, 1], F[1], L[1] = -0.0, 0.0, -0.0
    T[:7, 2], F[2], L[2] = inf, -inf, 0.0
    T[:7, 3], F[3], L[3] = inf, inf, 1.0
    T[:7, 4], F[4], L[4] = sub[0], 0.0, 0.0
    T[:7, 5], F[5], L[5] = sub[1], sub[2], sub[3]
    T[:7, 6], F[7], L[8] = nan, nan, nan
    T[:7, 9], F[9], L[9] = 0.0, sub[3], -0.0
    T[7], T[8] = -inf, np.resize(sub, C)
    codes = synth.randint(5500 + W, (B, H, W), rows).astype(np.int64)
    codes.reshape(-1)[:3] = [7, 8, 0]
    for tables in TABLE_SETS:
        Fx, Lx = (F if "F" in tables else None), (L if "L" in tables else None)
        with np.errstate(invalid="ignore"):                               # Inf + -Inf is meant
            ref = R.head(T, Fx, Lx, codes)
        assert R.same_bits(_run_head(dev, case, T, Fx, Lx, codes), ref), tables
        if tables == "FL":
            u = np.moveaxis(R.bits(ref), 1, 3).reshape(-1, C)[2]          # token 2 has code 0: the reference itself holds the edge values
    assert u[0] == 0x80000000 and u[1] == 0 and np.isnan(u[2:3].view(np.float32))[0] and u[3] == 0x7F800000 and u[4] == 1


# ------------------------------------------------------------------------------------------------------------- GPU: the table
def _run_table(dev, E, W, b):
    """dvq_decode_table_prepare_f32 into a guarded buffer of dvq_decode_table_bytes -> float32 [rows, C]"""
    rows, D = E.shape
    C = W.shape[0]
    nbytes = _lib.lib.dvq_decode_table_bytes(rows, C)
    assert nbytes >= rows * C * 4 and nbytes % 4 == 0
    g = R.Guarded(dev, rows * C, 0, tail_words=nbytes // 4 - rows * C)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ed, Wd, bd = t(E), t(W), t(b)
    _lib.check(_lib.lib.dvq_decode_table_prepare_f32(Ed.data_ptr(), rows, D, Wd.data_ptr(), _lib.ptr(bd), C, g.view.data_ptr(), nbytes,
                                                     _lib.stream_ptr(dev)), "dvq_decode_table_prepare_f32")
    return g.result().view(np.float32).reshape(rows, C)


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rdc", R.TABLE_CASES, ids=lambda c: "%d-%d-%d" % c)
def test_table_bound(dev, rdc, bias):
    E, W, b = R.table_inputs(rdc, bias)
    T = _run_table(dev, E, W, b)
    err = np.abs(T.astype(np.float64) - R.table64(E, W, b))
    M = R.magnitude(E, W, b)
    rel = R.table_rel(rdc[1])
    same = float((R.bits(T) == R.bits(R.table_chain32(E, W, b))).mean())
    print(rdc, "bias" if bias else "nobias", "kernel: max err / M %.3g, max err / bound %.3g; %.4f of the words equal the CPU chain's"
          % (float((err / M).max()), float((err / (rel * M)).max()), same))
    assert (err <= rel * M).all()
    assert np.array_equal(R.bits(T), R.bits(_run_table(dev, E, W, b)))    # a fixed summation order: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_table_rows_do_not_depend_on_their_group(dev, bias):
    """rows 5..13 of the table of all 17 rows against the table of E[5:14] alone: another place in the 8-row group, another
    workgroup, the same bits"""
    E, W, b = R.table_inputs((17, 24, 1024), bias)
    whole, part = _run_table(dev, E, W, b), _run_table(dev, E[5:14], W, b)
    assert np.array_equal(R.bits(whole[5:14]), R.bits(part))


@pytest.mark.gpu
def test_table_special_values(dev):
    """a NaN in one codebook row: that row of T is NaN throughout, every other row finite and inside the bound.  An Inf in one
    weight row: that column is the infinity of the product's sign in every row (E[:, 3] holds no zero), every other column finite
    and inside the bound.  (9, 1024, 260): the column is one of the four of the channel loop's second trip."""
    rdc = (9, 1024, 260)
    E, W, b = R.table_inputs(rdc, True)
    rel = R.table_rel(rdc[1])
    assert (E[:, 3] != 0).all()
    En = E.copy()
    En[8, 700] = np.nan
    T = _run_table(dev, En, W, b)
    assert np.isnan(T[8]).all() and np.isfinite(T[:8]).all()
    assert (np.abs(T[:8].astype(np.float64) - R.table64(E, W, b)[:8]) <= rel * R.magnitude(E, W, b)[:8]).all()
    Wi = W.copy()
    Wi[257, 3] = np.inf
    T = _run_table(dev, E, Wi, b)
    keep = np.arange(260) != 257
    assert np.array_equal(T[:, 257], np.where(E[:, 3] > 0, np.float32(np.inf), np.float32(-np.inf)))
    assert np.isfinite(T[:, keep]).all()
    assert (np.abs(T[:, keep].astype(np.float64) - R.table64(E, W, b)[:, keep]) <= rel * R.magnitude(E, W, b)[:, keep]).all()


# ------------------------------------------------------------------------------------------------------------- GPU: the gather
def _run_gather(dev, E, idx):
    K, D = E.shape
    n = idx.size
    g = R.Guarded(dev, n * D)
    Ed, idxd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    _lib.check(_lib.lib.dvq_embed_gather_f32(Ed.data_ptr(), K, D, idxd.data_ptr(), n, g.view.data_ptr(), _lib.stream_ptr(dev)),
               "dvq_embed_gather_f32")
    return g.result().reshape(n, D)


def _gather_ref(E, idx):
    ok = (idx >= 0) & (idx < E.shape[0])
    return np.where(ok[:, None], E[np.where(ok, idx, 0)], np.float32(np.nan)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("ndk", [(1, 4, 1), (5, 12, 3), (4100, 1024, 7)], ids=lambda c: "%d-%d-%d" % c)
def test_embed_gather_bits(dev, ndk):
    """E[idx] bit for bit; a bad index gives a NaN row and leaves its neighbours alone.  (4100, 1024, 7): 1,049,600 four-float
    items against the grid's 4096 x 256, so rows 4096.. are the second trip of the grid-stride loop; bad indices sit on both sides"""
    n, D, K = ndk
    assert (n * (D // 4) > 4096 * 256) == (n == 4100)
    E = synth.normal(5600 + n, (K, D), 0.0, 1.0)
    E[0, 0], E[K - 1, D - 1] = -0.0, np.array([1], np.uint32).view(np.float32)[0]       # copied, not computed: bits survive
    idx = synth.randint(5601 + n, (n,), K).astype(np.int64)
    assert R.same_bits(_run_gather(dev, E, idx), _gather_ref(E, idx))
    bad = R.bad_codes(K)
    if n == 1:
        trials = [(np.array([0]), bad[i:i + 1]) for i in range(7)]
    elif n == 5:
        trials = [(np.array([0, 2, 4]), np.roll(bad, r)[:3]) for r in range(7)]
    else:
        trials = [(np.array([0, 2, 2000, 4095, 4096, 4098, 4099]), bad)]
    for where, vals in trials:
        j = idx.copy()
        j[where] = vals
        out = _run_gather(dev, E, j)
        assert R.same_bits(out, _gather_ref(E, j))
        nan_rows = np.isnan(out.view(np.float32)).all(axis=1)
        assert np.array_equal(np.flatnonzero(nan_rows), where) and int(np.isnan(out.view(np.float32)).sum()) == len(where) * D


# ------------------------------------------------------------------------------------------------------------- GPU: the modules
@pytest.mark.gpu
@pytest.mark.parametrize("name", QUANTIZER_NAMES)
def test_decode_head_every_quantizer_class(dev, name, used_path):
    """DecodeHead(q).from_codes(codes) is the class's own get_codebook_entry laid out NCHW, bit for bit, or the construction
    raises TypeError / NotImplementedError: never a third outcome"""
    from dynamicvectorquantization_amd.decode import DecodeHead
    torch.manual_seed(5700)
    make, nvalid, own = _quantizers(used_path)[name]
    q = make().to(dev).eval()
    if isinstance(own, type):
        with pytest.raises((TypeError, NotImplementedError)) as info:
            DecodeHead(q)
        assert info.type is own
        return
    codes = synth.randint(5701, (2, 3, 4), nvalid).astype(np.int64)
    codes[0, 0, 0], codes[1, 2, 3] = nvalid - 1, 0                        # the last valid code: VQEmbedding's padding row K
    cd = torch.from_numpy(codes).to(dev)
    with torch.no_grad():
        out = DecodeHead(q).from_codes(cd)
        want = own(q, cd)
    assert tuple(out.shape) == (2, D_Q, 3, 4) and tuple(want.shape) == (2, D_Q, 3, 4)
    assert R.same_bits(R.bits(out.cpu().numpy()), want.cpu().numpy()) and not bool(torch.isnan(out).any())


def _parts(dev, seed, C, D, rows, bias=True):
    """(nn.Embedding, post_quant_conv) on the device with synth parameters"""
    emb = nn.Embedding(rows, D).to(dev).eval()
    conv = nn.Conv2d(D, C, 1, bias=bias).to(dev).eval()
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(synth.normal(seed, (rows, D), 0.0, 1.0)).to(dev))
        conv.weight.copy_(torch.from_numpy(synth.normal(seed + 1, (C, D, 1, 1), 0.0, 1.0 / 16.0)).to(dev))
        if bias:
            conv.bias.copy_(torch.from_numpy(synth.normal(seed + 2, (C,), 0.0, 0.1)).to(dev))
    return emb, conv


def _expect(emb, conv, F, L, codes):
    """R.head over the float64 table of the CURRENT parameters and the given position tables: (reference, tolerance), as _expect of
    tests/test_decode.py"""
    E, cw = emb.weight.detach().cpu().numpy(), conv.weight.detach().cpu().numpy()
    cb = None if conv.bias is None else conv.bias.detach().cpu().numpy()
    T64, M = R.table64(E, cw, cb), R.magnitude(E, cw, cb)
    c = codes.cpu().numpy()
    return R.head(T64.astype(np.float32), F, L, c), R.bound(M, T64, F, L, c, 1e-5)


def _close(out, ref_tol):
    ref, tol = ref_tol
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    return tuple(out.shape) == ref.shape and bool((err <= tol).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("CD", [(68, 8), (260, 24)], ids=lambda c: "%d-%d" % c)
def test_convs(dev, CD, bias):
    from dynamicvectorquantization_amd.decode import DecodeHead
    C, D = CD
    emb, conv = _parts(dev, 5800 + C, C, D, 33, bias)
    codes = torch.from_numpy(synth.randint(5803, (2, 5, 7), 33).astype(np.int64)).to(dev)
    with torch.no_grad():
        out = DecodeHead(emb, conv).from_codes(codes)
    assert _close(out, _expect(emb, conv, None, None, codes))


@pytest.mark.gpu
def test_conv_with_unsupported_width_names_it(dev):
    from dynamicvectorquantization_amd.decode import DecodeHead
    emb, conv = _parts(dev, 5810, 6, 8, 33)
    codes = torch.zeros((1, 2, 2), dtype=torch.int64, device=dev)
    with torch.no_grad(), pytest.raises(_lib.DvqError, match="C=6"):
        DecodeHead(emb, conv).from_codes(codes)


def _positions(dec, C, hw, dev):
    """the decoder's own position tables as Decoder.forward applies them"""
    if dec is None or dec.position_type == "learned":
        return None, None
    z = torch.zeros((1, C, hw, hw), device=dev)
    with torch.no_grad():
        if dec.position_type == "fourier":
            return dec.position_bias(z)[0].cpu().numpy(), None
        return dec.position_bias_fourier(z)[0].cpu().numpy(), dec.position_bias_learned(z)[0].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [6, 5], ids=["6x6-vec", "5x5-scalar"])
@pytest.mark.parametrize("position_type", ["fourier", "fourier+learned", "learned", None])
def test_position_types(dev, position_type, hw):
    from dynamicvectorquantization_amd.decode import DecodeHead
    C, D, rows = 68, 8, 33
    torch.manual_seed(5900 + hw)
    emb, conv = _parts(dev, 5900, C, D, rows)
    dec = None if position_type is None else R.stub_modules().Decoder(C, hw, position_type).to(dev).eval()
    head = DecodeHead(emb, conv, dec)
    codes = torch.from_numpy(synth.randint(5903 + hw, (3, hw, hw), rows).astype(np.int64)).to(dev)
    F, L = _positions(dec, C, hw, dev)
    assert (F is not None, L is not None) == {"fourier": (True, False), "fourier+learned": (True, True)}.get(position_type, (False, False))
    with torch.no_grad():
        assert _close(head.from_codes(codes), _expect(emb, conv, F, L, codes))
        if F is not None:                        # a grid that is not the decoder's latent_size (a smaller one: no module indexes past its rows)
            with pytest.raises(ValueError, match="position bias"):
                head.from_codes(codes[:, :4, :4])
            with pytest.raises(ValueError, match="position bias"):
                head.from_codes(codes[:, :, :4])


@pytest.mark.gpu
def test_other_inputs(dev):
    """int32 codes and a non-contiguous view give the bits of their int64 / contiguous copy; B = 0 gives an empty (0, C, H, W)"""
    from dynamicvectorquantization_amd.decode import DecodeHead
    C, D, rows, hw = 68, 8, 33, 6
    torch.manual_seed(6000)
    emb, conv = _parts(dev, 6000, C, D, rows)
    head = DecodeHead(emb, conv, R.stub_modules().Decoder(C, hw, "fourier+learned").to(dev).eval())
    big = torch.from_numpy(synth.randint(6003, (2, 7, 6), rows).astype(np.int64)).to(dev)
    view = big.transpose(1, 2)[:, :, :6]
    assert tuple(view.shape) == (2, 6, 6) and not view.is_contiguous()
    with torch.no_grad():
        ref = head.from_codes(view.contiguous())
        assert not bool(torch.isnan(ref).any())
        assert torch.equal(head.from_codes(view).view(torch.int32), ref.view(torch.int32))
        assert torch.equal(head.from_codes(view.contiguous().to(torch.int32)).view(torch.int32), ref.view(torch.int32))
        assert torch.equal(head.from_codes(view.to(torch.int32)).view(torch.int32), ref.view(torch.int32))
        empty = head.from_codes(view[:0])
    assert tuple(empty.shape) == (0, C, hw, hw) and empty.dtype == torch.float32 and empty.device == view.device


@pytest.mark.gpu
def test_fused_decode_head_follows_the_first_stage(dev):
    """decode_head() is one object until a module of first_stage_model is replaced; the new head reads the new module's weights"""
    from dynamicvectorquantization_amd.decode import FusedDecode
    S = R.stub_modules()
    C, D, rows, hw = 68, 8, 33, 6
    torch.manual_seed(6100)
    emb, conv = _parts(dev, 6100, C, D, rows)
    dec = S.Decoder(C, hw, "fourier+learned").to(dev).eval()
    fs = S.FirstStage(emb, conv, dec).to(dev).eval()

    class Fused(FusedDecode, S.Dualformer):
        pass

    model = Fused(fs, None)
    codes = torch.from_numpy(synth.randint(6103, (2, hw, hw), rows).astype(np.int64)).to(dev)
    F, L = _positions(dec, C, hw, dev)
    head = model.decode_head()
    assert model.decode_head() is head and head.post_quant_conv is conv
    with torch.no_grad():
        first = head.from_codes(codes)
    assert _close(first, _expect(emb, conv, F, L, codes))
    _, conv2 = _parts(dev, 6110, C, D, rows)
    fs.post_quant_conv = conv2
    head2 = model.decode_head()
    assert head2 is not head and model.decode_head() is head2 and head2.post_quant_conv is conv2
    with torch.no_grad():
        second = head2.from_codes(codes)
    assert _close(second, _expect(emb, conv2, F, L, codes)) and not _close(second, _expect(emb, conv, F, L, codes))
