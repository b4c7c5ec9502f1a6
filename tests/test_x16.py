"""fp16 / bf16 latents in the dense assign, its backward and the EMA step (`dvq_vq_assign_nchw_x16`, `dvq_vq_backward_nchw_x16`,
`dvq_ema_accumulate_nchw_x16`; include/dvq.h 0.17.0).

The contract, with zf = float32(z) (exact): codes are those of the float32 op on zf bit for bit, the loss is that op's (1e-5),
z_q is that op's value narrowed ONCE to z's dtype round-to-nearest-even (the bits of torch's `.to(dtype)`), the backward is the
float32 expression on the widened inputs narrowed once, the EMA statistics are float32 sums over zf.  Expected values: the CPU
oracle on the upcast input, z_q narrowed by torch on the host; the backward from a float64 evaluation narrowed by torch."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from . import _cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 0.25
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
NAMES = ("dvq_vq_assign_nchw_x16", "dvq_vq_backward_nchw_x16", "dvq_ema_accumulate_nchw_x16")
# the backward's share of elements that may land on a NEIGHBOUR of the float64 value rounded to the dtype: the float32 chain errs
# by a few 2^-24 of its largest term against rounding midpoints 2^-8 (bf16) / 2^-11 (fp16) apart, relative: 1e-4 .. 1e-3 expected
NEIGHBOUR_CAP = 0.01


# ---------------------------------------------------------------------------------------------
# host-side helpers
# ---------------------------------------------------------------------------------------------
def _narrow_np(x, name):
    """float32 ndarray -> the 16 bits of `name` as uint16, round to nearest even.  bf16: the integer statement (add 0x7FFF + the
    kept LSB, NaN kept quiet); fp16: IEEE binary16 conversion (numpy's: subnormals, overflow to inf, NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if name == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def _bits(t):
    """a 16-bit torch tensor's words as int32 ndarray (0 .. 65535)"""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int32) & 0xFFFF


def _order_key(bits):
    """sign-magnitude words -> integers ordered like the values (+-0 both 0): neighbours in the dtype differ by 1"""
    mag = bits & 0x7FFF
    return np.where(bits & 0x8000, -mag, mag)


def _narrow_host(a, dtype):
    """float32 ndarray -> torch CPU tensor of `dtype` (what a caller's `.to(dtype)` gives)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def _zq_equal(got, want):
    """raw 16-bit words where the expected value is not NaN, NaN-ness where it is"""
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    wn = torch.isnan(want.float()).reshape(-1).numpy()
    gn = torch.isnan(got.detach().cpu().float()).reshape(-1).numpy()
    bad = np.where(wn, ~gn, g != w)
    return int(bad.sum()), (np.flatnonzero(bad)[:5].tolist() if bad.any() else [])


def _mask(seed, B, HW):
    from dynamicvectorquantization_amd import synth
    return np.where(synth.bernoulli(seed, (B, HW), 0.5), np.float32(1.0), np.float32(0.25))


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    """inputs of a named case narrowed to dtype `dt` on the host, and the oracle's outputs for the upcast input: computed once,
    shared by the tests, never modified"""
    from dynamicvectorquantization_amd import synth
    from oracle import oracle
    oracle.build()
    dtype = DTYPES[dt]
    mask = None
    if name == "ragged":                                 # B = 3, D = 64, 5 x 5, K = 200, masked
        E = synth.codebook_trained(200, 64, seed=9101)
        z = synth.z_tokens(E, 3, 5, 5, 9102)
        mask = _mask(9103, 3, 25)
    elif name == "block_plus_one":                       # one token over a 128-token block
        E = synth.codebook_trained(1024, 128, seed=9111)
        z = synth.z_tokens(E, 1, 1, 129, 9112).reshape(1, 128, 129)
    elif name == "ref_tiestress":                        # the reference shape on the default-init codebook (ties: the resolver)
        E = synth.codebook_default_init(1024, 256, seed=9121)
        z = synth.z_tokens(E, 2, 32, 32, 9122)
        if dt == "f16":                                  # hand-placed fp16 subnormals (|v| < 2^-14)
            z[0, :4, 0, 0] = np.float32([2.0 ** -15, -(2.0 ** -20), 3 * 2.0 ** -24, 2.0 ** -24])
            z[1, 100:104, 31, 31] = np.float32([-(2.0 ** -16), 2.0 ** -17, 5 * 2.0 ** -24, -(2.0 ** -23)])
    elif name == "ref_trained":                          # the reference shape, trained-like codebook, masked
        E = synth.codebook_trained(1024, 256, seed=9131)
        z = synth.z_tokens(E, 2, 32, 32, 9132)
        mask = _mask(9133, 2, 1024)
    elif name == "k16384":                               # per-tile seed form (more than 32 code tiles per workgroup)
        E = synth.codebook_trained(16384, 256, seed=9141)
        z = synth.z_tokens(E, 2, 16, 16, 9142)
    elif name == "exact_list":                           # tokens the fp16 filter cannot score
        E = synth.codebook_trained(1024, 256, seed=9151)
        z = synth.z_tokens(E, 1, 32, 32, 9152)
        z[0, 3, 0, 5] = np.nan
        z[0, 200, 7, 7] = np.inf
        z[0, 17, 31, 31] = -np.inf
        z[0, :, 16, 16] = np.nan
        if dt == "bf16":
            z[0, 9, 20, 1] = 1e30
            z[0, 250, 20, 2] = -1e30
    elif name == "rows":                                 # row-major [N, D]
        E = synth.codebook_trained(512, 128, seed=9161)
        z = synth.z_tokens(E, 130, 1, 1, 9162).reshape(130, 128)
    elif name == "d96":                                  # a zero-padded width
        E = synth.codebook_trained(256, 96, seed=9171)
        z = synth.z_tokens(E, 2, 8, 8, 9172)
    else:
        raise KeyError(name)
    z16 = _narrow_host(z, dtype)
    zf = z16.float().numpy()
    if name == "ref_tiestress" and dt == "f16":
        sub = (np.abs(zf) > 0) & (np.abs(zf) < 2.0 ** -14)
        assert int(sub.sum()) >= 8, "the fp16 tie-stress input holds fp16 subnormals"
    zo = zf if zf.ndim > 2 else zf.reshape(zf.shape[0], zf.shape[1], 1)
    o = oracle.vq_assign_nchw(zo, E, mask)
    zq16 = _narrow_host(o["zq"].reshape(zf.shape), dtype)
    mean = np.float32(o["sqerr"] / o["numel"])
    return dict(E=E, z16=z16, zf=zf, mask=mask, codes=o["codes"], zq16=zq16, loss0=float(mean),
                loss1=float(oracle.vq_loss(o["sqerr"], o["numel"], BETA)))


def _run(dev, c, mode, prep=None, z=None):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    prep = _CodebookPrep() if prep is None else prep
    z = c["z16"].to(dev) if z is None else z
    m = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(dev)
    zq, codes, loss = vq_assign(z, torch.from_numpy(c["E"]).to(dev), prep, m, beta=BETA, mode=mode)
    torch.cuda.synchronize()
    return zq, codes, loss, prep


def _check(c, zq, codes, loss):
    assert zq.dtype == c["z16"].dtype and tuple(zq.shape) == tuple(c["z16"].shape)
    got = codes.cpu().numpy().reshape(c["codes"].shape)
    assert np.array_equal(got, c["codes"]), "%d of %d codes differ from the oracle" % (int((got != c["codes"]).sum()), got.size)
    nbad, first = _zq_equal(zq, c["zq16"])
    assert nbad == 0, "%d z_q words differ from the narrowed oracle value, first at %s" % (nbad, first)
    assert loss.dtype == torch.float32
    print("loss %.9g / %.9g vs %.9g / %.9g" % (float(loss[0]), float(loss[1]), c["loss0"], c["loss1"]))
    assert C.loss_close(float(loss[0]), c["loss0"]) and C.loss_close(float(loss[1]), c["loss1"])


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_symbols_version_and_abi_validation_without_gpu():
    """the three entry points are declared, exported and bound; validation needs no GPU (fake aligned "pointers")"""
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    header = open(os.path.join(ROOT, "include", "dvq.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert "DVQ_API" in header and n + "(" in header, n
        assert hasattr(raw, n) and n in _lib.EXPORTS and hasattr(_lib.checked, n)
    assert "#define DVQ_DTYPE_F16 1" in " ".join(header.split()) and "#define DVQ_DTYPE_BF16 2" in " ".join(header.split())
    assert (_lib.DTYPE_F16, _lib.DTYPE_BF16) == (1, 2)
    assert L.dvq_version() >= 1700
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    a = 256
    need = L.dvq_vq_assign_workspace_bytes(2, 64, 63, 200, _lib.MODE_FILTER)
    assert need > 0

    def assign(z=a, dtype=2, E=a, prep=a, mask=0, B=2, D=64, HW=63, K=200, zq=a, codes=a, loss=0, ws=a, wsb=need, mode=_lib.MODE_FILTER):
        return L.dvq_vq_assign_nchw_x16(z, dtype, E, prep, mask, B, D, HW, K, BETA, zq, codes, loss, ws, wsb, mode, 0)

    for dtype in (0, 3, -1):
        assert assign(dtype=dtype) == EINVAL and b"dtype" in L.dvq_last_error_string()
    for null in ("z", "E", "prep", "codes"):
        assert assign(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert assign(z=a + 1) == EINVAL and b"2-byte" in L.dvq_last_error_string()
    assert assign(zq=a + 1) == EINVAL and b"2-byte" in L.dvq_last_error_string()
    for D in (16, 100, 4, 8, 3):
        assert assign(D=D) == EUNSUPPORTED
        msg = L.dvq_last_error_string()
        assert ("D=%d" % D).encode() in msg and b"narrow widths" in msg
    assert assign(mode=_lib.MODE_FILTER_WIDE) == EUNSUPPORTED and assign(mode=_lib.MODE_FILTER_PASS1) == EUNSUPPORTED
    assert assign(mode=_lib.MODE_FILTER_WIDE | _lib.MODE_WS_CLEAN) == EUNSUPPORTED
    assert assign(mode=7) == EINVAL
    assert assign(B=0) == EINVAL and assign(HW=0) == EINVAL and assign(K=0) == EINVAL
    assert assign(wsb=need - 1) == EWORKSPACE and b"workspace" in L.dvq_last_error_string()
    assert assign(ws=0, wsb=0) == EWORKSPACE
    assert assign(ws=a + 8) == EINVAL
    assert assign(loss=a, ws=0, wsb=0, mode=_lib.MODE_EXACT) == EINVAL

    def backward(z=a, dtype=1, E=a, codes=a, mask=0, g_zq=a, g_loss=a, B=2, D=64, HW=63, K=200, g_z=a):
        return L.dvq_vq_backward_nchw_x16(z, dtype, E, codes, mask, g_zq, g_loss, 0.5, B, D, HW, K, g_z, 0)

    assert backward(dtype=0) == EINVAL and backward(dtype=3) == EINVAL
    for null in ("z", "E", "codes", "g_z"):
        assert backward(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert backward(g_zq=0, g_loss=0) == EINVAL
    assert backward(D=100) == EUNSUPPORTED and backward(D=0) == EINVAL and backward(B=0) == EINVAL
    assert backward(E=a + 8) == EINVAL
    assert backward(z=a + 1) == EINVAL and backward(g_zq=a + 1) == EINVAL and backward(g_z=a + 1) == EINVAL

    def accumulate(z=a, dtype=2, codes=a, B=2, D=64, HW=63, K=200, cs=a, vs=a):
        return L.dvq_ema_accumulate_nchw_x16(z, dtype, codes, B, D, HW, K, cs, vs, 0)

    assert accumulate(dtype=0) == EINVAL and accumulate(dtype=3) == EINVAL
    for null in ("z", "codes", "cs", "vs"):
        assert accumulate(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert accumulate(z=a + 1) == EINVAL and accumulate(B=0) == EINVAL and accumulate(K=0) == EINVAL


def test_latent_checker_accepts_the_three_dtypes_only():
    from dynamicvectorquantization_amd import _lib
    assert _lib.X16 == {torch.float16: 1, torch.bfloat16: 2}
    with pytest.raises(TypeError):
        _lib.require_cuda_latents(np.zeros(3), "z")
    with pytest.raises(_lib.DvqError):                   # CPU tensors: no fallback, whatever the dtype
        _lib.require_cuda_latents(torch.zeros(3, dtype=torch.bfloat16), "z")
    for dtype in DTYPES.values():
        with pytest.raises(TypeError, match="must be float32, got"):
            _lib.refuse_x16(torch.zeros(3, dtype=dtype), "z")
    _lib.refuse_x16(torch.zeros(3), "z")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_numpy_narrowing_is_torchs(dt):
    """what the GPU tests' expected values rest on: f32 -> 16 bit, round to nearest even, subnormals, overflow, NaN -- the numpy
    statement and torch.Tensor.to agree word for word (NaN: NaN-ness)"""
    from dynamicvectorquantization_amd import synth
    rnd = synth.normal(9001, (4096,), 0.0, 1.0) * np.exp2(synth.randint(9002, (4096,), 60).astype(np.float32) - 40.0).astype(np.float32)
    raw = (synth.bits(9003, 4096) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)      # every exponent, NaNs and infs
    f16_mid = np.float32([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25,
                          65504.0, 65519.9, 65520.0, 65536.0, 1e30])
    bf_mid = np.float32([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.3895314e38, 3.4e38, 1e-40, 2.0 ** -133, 2.0 ** -134])
    edge = np.concatenate([f16_mid, -f16_mid, bf_mid, -bf_mid, np.float32([0.0, -0.0, np.inf, -np.inf, np.nan])])
    x = np.concatenate([rnd, raw, edge]).astype(np.float32)
    mine = _narrow_np(x, dt).astype(np.int32)
    t = torch.from_numpy(x).to(DTYPES[dt])
    theirs = _bits(t)
    nan = np.isnan(x)
    assert np.array_equal(mine[~nan], theirs[~nan])
    assert bool(torch.isnan(t[torch.from_numpy(nan)]).all())
    back = torch.from_numpy(mine[nan].astype(np.uint16).view(np.int16)).view(DTYPES[dt]).float()
    assert bool(torch.isnan(back).all())
    # widening is exact: the 16-bit value, widened and narrowed again, is itself
    assert np.array_equal(_bits(t.float().to(DTYPES[dt]))[~nan], theirs[~nan])


def _backward_inputs(name, dt):
    """(zf, e rows gathered by the oracle's codes, mask, g_zq of the dtype, g_loss) of a backward case"""
    from dynamicvectorquantization_amd import synth
    c = _case(name, dt)
    zf = c["zf"]
    B, D = zf.shape[0], zf.shape[1]
    e = np.moveaxis(c["E"][c["codes"]], 2, 1).reshape(zf.shape)           # [B, HW, D] -> [B, D, H, W]
    m = np.ones((B, 1) + zf.shape[2:], np.float32) if c["mask"] is None else c["mask"].reshape((B, 1) + zf.shape[2:])
    g16 = _narrow_host(synth.normal(9201 + len(name), zf.shape, 0.0, 1.0), DTYPES[dt])
    return zf, e, m, g16, np.float32(0.75)


@functools.lru_cache(maxsize=None)
def _backward_expected(name, dt, with_g):
    """float64 evaluation of g_zq + (g_loss fl(2 c / numel)) ((zf - e) m), narrowed (through float32: a value exactly on a 16-bit
    rounding midpoint after the float32 step is a 2^-29 event per element, far below the cap it would count against)"""
    zf, e, m, g16, gl = _backward_inputs(name, dt)
    coef = np.float64(np.float32(BETA * (2.0 / zf.size)))
    g = g16.float().numpy().astype(np.float64) if with_g else 0.0
    x = g + (np.float64(gl) * coef) * ((zf.astype(np.float64) - e.astype(np.float64)) * m.astype(np.float64))
    return torch.from_numpy(x).to(torch.float32).to(DTYPES[dt])


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["ragged", "ref_trained"])
def test_backward_cap_is_met_by_the_float32_reference_arithmetic(name, dt):
    """the float32 torch expression of the backward, rounded to the dtype, against the float64 restatement rounded to the dtype,
    on the GPU test's inputs: every element equal or a neighbour, and the share of neighbours under the cap the GPU test applies"""
    zf, e, m, g16, gl = _backward_inputs(name, dt)
    coef = np.float32(BETA * (2.0 / zf.size))
    t = torch.from_numpy
    for with_g in (True, False):
        want = _backward_expected(name, dt, with_g)
        f32 = (torch.tensor(gl) * torch.tensor(coef)) * ((t(zf) - t(e)) * t(np.broadcast_to(m, zf.shape).copy()))
        if with_g:
            f32 = g16.float() + f32
        d = np.abs(_order_key(_bits(f32.to(DTYPES[dt]))) - _order_key(_bits(want)))
        share = float((d == 1).mean())
        print("%s %s g_zq=%s: neighbour share %.3g" % (name, dt, with_g, share))
        assert int(d.max()) <= 1 and share <= NEIGHBOUR_CAP


# ---------------------------------------------------------------------------------------------
# GPU: the assign
# ---------------------------------------------------------------------------------------------
def _modes():
    from dynamicvectorquantization_amd import _lib
    return {"filter": _lib.MODE_FILTER, "exact": _lib.MODE_EXACT}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["filter", "exact"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_ragged_tail_and_odd_positions(dev, dt, mode):
    """HW = 25: every second channel row starts at an address that is 2-byte aligned only; N = 75: 53 lanes of the last wave have
    no token; K = 200 is no multiple of the code tile; masked"""
    c = _case("ragged", dt)
    zq, codes, loss, _ = _run(dev, c, _modes()[mode])
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_one_token_over_a_block(dev, dt):
    c = _case("block_plus_one", dt)
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"])
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_reference_shape_tiestress_goes_through_the_resolver(dev, dt):
    """default-init codebook: many tokens are undecided by the filter, the resolver rewrites rows of z_q (narrowed)"""
    c = _case("ref_tiestress", dt)
    zq, codes, loss, prep = _run(dev, c, _modes()["filter"])
    queued, _ = prep.fallback_count()
    print("queued for the resolver: %d" % queued)
    assert queued > 0
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_reference_shape_trained_masked(dev, dt):
    c = _case("ref_trained", dt)
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"])
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_per_tile_seed_form_at_K16384(dev, dt):
    c = _case("k16384", dt)
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"])
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_list_takes_nonfinite_and_unscalable_tokens(dev, dt):
    c = _case("exact_list", dt)
    assert np.isnan(c["zf"]).any() and np.isinf(c["zf"]).any()
    zq, codes, loss, prep = _run(dev, c, _modes()["filter"])
    _, nexact = prep.fallback_count()
    print("exact list: %d tokens" % nexact)
    assert nexact >= (6 if dt == "bf16" else 4)
    _check(c, zq, codes, loss)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_row_major_fresh_and_offset_by_one_element(dev, dt):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantize2List
    c = _case("rows", dt)
    N, D = c["z16"].shape
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"])
    _check(c, zq, codes, loss)
    base = torch.zeros(N * D + 1, dtype=DTYPES[dt], device=dev)
    view = base[1:].view(N, D)
    view.copy_(c["z16"].to(dev))
    assert view.is_contiguous() and view.data_ptr() % 4 == 2
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"], z=view)
    _check(c, zq, codes, loss)
    K = c["E"].shape[0]
    for cls, kw in ((VectorQuantize2, dict(accept_image_fmap=False, channel_last=True)), (VectorQuantize2List, {})):
        m = cls(K, D, **kw).to(dev).eval()
        m.codebook.weight.data[:-1].copy_(torch.from_numpy(c["E"]))
        m.invalidate_codebook_cache()
        x = c["z16"].to(dev).view(2, 65, D)
        with torch.no_grad():
            if cls is VectorQuantize2List:
                xq, l, (_, _, code) = m([x[0], x[1]])
                xq, code = torch.stack(xq), torch.stack(code)
            else:
                xq, l, (_, _, code) = m(x)
        assert xq.dtype == DTYPES[dt] and l.dtype == torch.float32
        assert np.array_equal(code.cpu().numpy().reshape(-1), c["codes"].reshape(-1))
        assert _zq_equal(xq.reshape(N, D), c["zq16"])[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_zero_padded_width_96(dev, dt):
    c = _case("d96", dt)
    zq, codes, loss, _ = _run(dev, c, _modes()["filter"])
    _check(c, zq, codes, loss)


@pytest.mark.gpu
def test_modules_take_bf16_and_float32_only_ops_still_refuse(dev):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2, _CodebookPrep, vq_assign
    K, D = 1024, 256
    E = torch.from_numpy(synth.codebook_trained(K, D, seed=9301)).to(dev)
    x = torch.from_numpy(synth.z_tokens(E.cpu().numpy(), 2, 16, 16, 9302)).to(dev).to(torch.bfloat16)
    mods = [VectorQuantize2(K, D).to(dev).eval()]
    mods[0].codebook.weight.data[:-1].copy_(E)
    for legacy in (True, False):
        q = VectorQuantizer2(K, D, beta=0.25, legacy=legacy, sane_index_shape=True).to(dev).eval()
        q.embedding.weight.data.copy_(E)
        mods.append(q)
    for m in mods:
        m.invalidate_codebook_cache()
        with torch.no_grad():
            xq, loss, (_, _, codes) = m(x)
            xq32, loss32, (_, _, codes32) = m(x.float())
        assert xq.dtype == torch.bfloat16 and loss.dtype == torch.float32
        assert torch.equal(codes, codes32)
        assert torch.equal(xq.view(torch.int16), xq32.to(torch.bfloat16).view(torch.int16))
        assert C.loss_close(float(loss), float(loss32))
    narrow = VectorQuantize2(64, 8).to(dev).eval()
    with pytest.raises(TypeError, match="float32"):
        narrow(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16, device=dev))
    conv = torch.nn.Conv2d(D, D, 1).to(dev).eval()
    for kw in (dict(conv=conv), dict(conv=conv, fold=True, want_loss=False)):
        with pytest.raises(TypeError, match="float32"):
            vq_assign(x, E, _CodebookPrep(), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_workspace_hand_over_between_float32_and_16_bit_calls(dev, dt):
    """one workspace, DVQ_MODE_WS_CLEAN from the second call on, float32 and 16-bit calls of the same shape alternating"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    c = _case("ref_tiestress", dt)
    E = torch.from_numpy(c["E"]).to(dev)
    z16, z32 = c["z16"].to(dev), torch.from_numpy(c["zf"]).to(dev)
    prep = _CodebookPrep()
    first = {}
    for i in range(6):
        z = z32 if i % 2 == 0 else z16
        if i > 0:
            assert prep._last_ws[1].clean and len(prep._ws) == 1
        zq, codes, loss = vq_assign(z, E, prep, None, beta=BETA, mode=_lib.MODE_FILTER)
        torch.cuda.synchronize()
        assert prep.fallback_count()[0] > 0
        if i < 2:
            first[i] = (zq.clone(), codes.clone(), loss.clone())
            if i == 1:
                _check(c, zq, codes, loss)
        else:
            for got, want in zip((zq, codes, loss), first[i % 2]):
                assert torch.equal(got, want), i
    assert torch.equal(first[0][1], first[1][1])
    assert torch.equal(first[0][0].to(DTYPES[dt]).view(torch.int16), first[1][0].view(torch.int16))


# ---------------------------------------------------------------------------------------------
# GPU: backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["ragged", "ref_trained"])
def test_backward_kernel(dev, name, dt):
    from dynamicvectorquantization_amd import _lib
    c = _case(name, dt)
    zf, e, m, g16, gl = _backward_inputs(name, dt)
    B, D = zf.shape[0], zf.shape[1]
    HW = zf[0, 0].size
    K = c["E"].shape[0]
    z = c["z16"].to(dev)
    E = torch.from_numpy(c["E"]).to(dev)
    codes = torch.from_numpy(c["codes"]).to(dev)
    mask = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(dev)
    g = g16.to(dev)
    gloss = torch.tensor([float(gl)], device=dev)
    coef = float(BETA * (2.0 / zf.size))

    def run(gq, gls):
        out = torch.full_like(z, float("nan"))
        with _lib.on_device(dev):
            _lib.checked.dvq_vq_backward_nchw_x16(z.data_ptr(), _lib.X16[z.dtype], E.data_ptr(), codes.data_ptr(), _lib.ptr(mask), _lib.ptr(gq),
                                                  _lib.ptr(gls), coef, B, D, HW, K, out.data_ptr(), _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        return out

    for with_g in (True, False):
        got = run(g if with_g else None, gloss)
        d = np.abs(_order_key(_bits(got)) - _order_key(_bits(_backward_expected(name, dt, with_g))))
        share = float((d == 1).mean())
        print("%s %s g_zq=%s: neighbour share %.3g, worst distance %d" % (name, dt, with_g, share, int(d.max())))
        assert int(d.max()) <= 1 and share <= NEIGHBOUR_CAP
    assert torch.equal(run(g, None).view(torch.int16), g.view(torch.int16))         # no loss term: the identity, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_backward_through_autograd(dev, dt):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    name = "ref_trained"
    c = _case(name, dt)
    zf, e, m, g16, gl = _backward_inputs(name, dt)
    K, D = c["E"].shape
    vq = VectorQuantize2(K, D).to(dev).eval()
    vq.codebook.weight.data[:-1].copy_(torch.from_numpy(c["E"]))
    vq.invalidate_codebook_cache()
    x = c["z16"].to(dev).requires_grad_(True)
    xq, loss, _ = vq(x, codebook_mask=torch.from_numpy(c["mask"]).to(dev).reshape(2, 1, 32, 32))
    assert xq.dtype == DTYPES[dt] and loss.dtype == torch.float32
    torch.autograd.backward([xq, loss], [g16.to(dev), torch.tensor(float(gl), device=dev)])
    assert x.grad is not None and x.grad.dtype == DTYPES[dt]
    d = np.abs(_order_key(_bits(x.grad)) - _order_key(_bits(_backward_expected(name, dt, True))))
    assert int(d.max()) <= 1 and float((d == 1).mean()) <= NEIGHBOUR_CAP


# ---------------------------------------------------------------------------------------------
# GPU: the EMA step
# ---------------------------------------------------------------------------------------------
def _tokens64(z):
    B, D = z.shape[0], z.shape[1]
    return z.double().reshape(B, D, -1).permute(0, 2, 1).reshape(-1, D)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ["ragged", "ref_trained"])
def test_ema_step_matches_the_float32_module(dev, name, dt):
    """one training forward of a 16-bit module and of a float32 module fed x.float(), from equal state, no restarts: equal counts;
    embed_ema and weight within the 1e-5 (of the largest entry) that tests/test_ema_stats.py asks of the float32 kernel, against the
    reference's expressions in float64 on the codes the forward returned -- float atomics add in arrival order"""
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    c = _case(name, dt)
    K, D = c["E"].shape
    x16 = c["z16"].to(dev)
    E = torch.from_numpy(c["E"]).to(dev)
    cs0 = (torch.rand(K, generator=torch.Generator().manual_seed(9401)) * 100.0).to(dev)
    mods = []
    for x in (x16, x16.float()):
        m = VectorQuantize2(K, D, restart_unused_codes=False).to(dev)
        m.codebook.weight.data[:-1].copy_(E)
        m.codebook.embed_ema.copy_(E)
        m.codebook.cluster_size_ema.copy_(cs0)
        m.train()
        xq, _, (_, _, codes) = m(x)
        assert xq.dtype == x.dtype
        mods.append((m, codes.reshape(-1)))
    torch.cuda.synchronize()
    (m16, codes16), (m32, codes32) = mods
    assert torch.equal(codes16, codes32) and np.array_equal(codes16.cpu().numpy(), c["codes"].reshape(-1))
    assert torch.equal(m16.codebook.cluster_size_ema, m32.codebook.cluster_size_ema)
    decay, eps = float(m16.codebook.decay), float(m16.codebook.eps)
    n = torch.bincount(codes16, minlength=K).double()
    S = torch.zeros((K, D), dtype=torch.float64, device=dev).index_add_(0, codes16, _tokens64(x16))
    cs_r = cs0.double() * decay + (1 - decay) * n
    emb_r = E.double() * decay + (1 - decay) * S
    tot = cs_r.sum()
    w_r = emb_r / (tot * (cs_r + eps) / (tot + K * eps)).reshape(-1, 1)
    for m in (m16, m32):
        for what, got, ref in (("cluster_size_ema", m.codebook.cluster_size_ema, cs_r), ("embed_ema", m.codebook.embed_ema, emb_r),
                               ("weight", m.codebook.weight.data[:K], w_r)):
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            print("%s: max |got - ref| / max |ref| = %.3g" % (what, err))
            assert err < 1e-5, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_ema_restart_rows_are_upcast_latents(dev, dt):
    """restart_unused_codes=True from cluster_size_ema = 0: a code with fewer than 100 tokens this step is dead (0.01 n < 1) and
    restarts from a token of the batch: its embed_ema row is the widened latent vector of some token, bit for bit"""
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    c = _case("ref_trained", dt)
    K, D = c["E"].shape
    m = VectorQuantize2(K, D, restart_unused_codes=True).to(dev)
    m.codebook.weight.data[:-1].copy_(torch.from_numpy(c["E"]))
    m.codebook.embed_ema.copy_(torch.from_numpy(c["E"]))
    m.train()
    x = c["z16"].to(dev)
    m(x)
    torch.cuda.synchronize()
    n = np.bincount(c["codes"].reshape(-1), minlength=K)
    assert n.max() < 100
    assert bool((m.codebook.cluster_size_ema == 1.0).all())              # every code was dead and restarted
    toks = {r.tobytes() for r in c["zf"].reshape(2, D, -1).transpose(0, 2, 1).reshape(-1, D)}
    rows = m.codebook.embed_ema.cpu().numpy()
    missing = [j for j in range(K) if rows[j].tobytes() not in toks]
    assert not missing, "%d restarted rows are no token of the batch, first %s" % (len(missing), missing[:5])


@pytest.mark.gpu
def test_codebook_gradient_of_16_bit_latents_is_float32(dev):
    """VectorQuantizer2 trains its codebook by back-propagation: with bf16 latents the codebook gradient is the torch expression on
    z.float() -- float32, the values the float32 module gets on x.float() up to the summation order (1e-5 of the largest entry),
    and x.grad is that module's, narrowed (equal or a neighbour)"""
    from dynamicvectorquantization_amd.quantize import VectorQuantizer2
    c = _case("ragged", "bf16")
    K, D = c["E"].shape
    out = []
    for x in (c["z16"].to(dev), c["z16"].to(dev).float()):
        q = VectorQuantizer2(K, D, beta=0.25, legacy=False).to(dev).train()
        q.embedding.weight.data.copy_(torch.from_numpy(c["E"]))
        x = x.clone().requires_grad_(True)
        zq, loss, _ = q(x)
        assert zq.dtype == x.dtype and loss.dtype == torch.float32
        loss.backward()
        out.append((q.embedding.weight.grad, x.grad))
    (gw16, gx16), (gw32, gx32) = out
    assert gw16.dtype == torch.float32 and gx16.dtype == torch.bfloat16 and gx32.dtype == torch.float32
    assert float(gw32.abs().max()) > 0
    assert float((gw16 - gw32).abs().max()) <= 1e-5 * float(gw32.abs().max())
    d = np.abs(_order_key(_bits(gx16)) - _order_key(_bits(gx32.to(torch.bfloat16))))
    assert int(d.max()) <= 1 and float((d == 1).mean()) <= NEIGHBOUR_CAP
