"""Row-major [N, D] and channels_last latents on the training side (include/dvq.h 0.18.0, csrc/train_rows.hip):
`dvq_vq_backward_nchw_f32` / `_x16`, `dvq_vq_backward_codebook_nchw_f32` and `dvq_ema_accumulate_nchw_f32` / `_x16` called with B = N, HW = 1
(the row-major form: kernels whose accesses follow the rows), the modules that train through them and channels_last image maps served in place.

Tolerances: the backward is the NCHW kernel's fp32 expression in its operation order, so it is compared BIT FOR BIT with the torch
expression evaluated op by op in float32 and with `dvq_vq_backward_nchw_*` on the transposed data.  The two scatter kernels add in
another order than a float64 scatter-add: 1e-5 of the largest entry, the criterion of tests/test_autograd_and_training.py and
tests/test_train_step.py for reordered fp32 sums.  Counts are exact."""
import contextlib
import copy
import subprocess

import pytest
import torch

# position of the HW argument of the entry points that take a layout: a call is in the row-major form iff HW == 1
HW_ARG = {"dvq_vq_backward_nchw_f32": 9, "dvq_vq_backward_nchw_x16": 10, "dvq_vq_backward_codebook_nchw_f32": 8, "dvq_ema_accumulate_nchw_f32": 4,
          "dvq_ema_accumulate_nchw_x16": 5, "dvq_vq_assign_nchw_f32": 6, "dvq_vq_assign_nchw_x16": 7, "dvq_vq_assign_narrow_nchw_f32": 5}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Trace(list):
    """the names of the calls, in order; .calls has their arguments too"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def strided(self):
        """the calls that took a layout and were NOT in the row-major form (HW > 1)"""
        return [(n, a[HW_ARG[n]]) for n, a in self.calls if n in HW_ARG and a[HW_ARG[n]] != 1]


@contextlib.contextmanager
def recording():
    """the names of the entry points the package calls (every call site goes through `_lib.checked`), in order"""
    from dynamicvectorquantization_amd import _lib
    names, saved = _Trace(), {}
    for n in _lib.EXPORTS:
        saved[n] = getattr(_lib.checked, n)
        setattr(_lib.checked, n, (lambda fn, n: lambda *a: (names.append(n), names.calls.append((n, a)), fn(*a))[2])(saved[n], n))
    try:
        yield names
    finally:
        for n, fn in saved.items():
            setattr(_lib.checked, n, fn)


@contextlib.contextmanager
def no_torch_scatter(monkeypatch):
    """torch.bincount / Tensor.index_add_ -- the path row-major latents took -- count their calls"""
    calls = []
    bincount, index_add_ = torch.bincount, torch.Tensor.index_add_
    with monkeypatch.context() as m:
        m.setattr(torch, "bincount", lambda *a, **k: (calls.append("bincount"), bincount(*a, **k))[1])
        m.setattr(torch.Tensor, "index_add_", lambda *a, **k: (calls.append("index_add_"), index_add_(*a, **k))[1])
        yield calls


# ---------------------------------------------------------------------------------------------------------------------------
# 1. ABI (no GPU: nothing here gets past argument validation)
# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_0_18_serves_rows_through_the_entry_points_it_had():
    """the row-major form is HW = 1 of the existing entry points: the version says so, and the header declares no new symbol for it"""
    from dynamicvectorquantization_amd import _lib
    header = open(_lib.HEADER).read()
    assert _lib.lib.dvq_version() >= 1800 and " 0.18.0 " in header
    assert all(n in _lib.EXPORTS for n in HW_ARG) and not [n for n in _lib.EXPORTS if "backward" in n and "flat" in n]


P = 256                                                      # a fake pointer that passes every null and alignment check
#                 entry point, arguments (HW = 1: the row-major form), status, words of the message
_REFUSALS = [
    #                           z  E  codes mask gzq gl coef  B   D  HW K  gz stream
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, P, P, 1.0, 8, 100, 1, 8, P, 0), -2, "D=100 must be a multiple of 16"),
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, P, P, 1.0, 8, 8, 1, 8, P, 0), -2, "D=8 must be a multiple of 16"),
    ("dvq_vq_backward_nchw_f32", (P, 8, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "codebook must be 16-byte aligned"),
    ("dvq_vq_backward_nchw_f32", (0, P, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    ("dvq_vq_backward_nchw_f32", (P, 0, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    ("dvq_vq_backward_nchw_f32", (P, P, 0, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, P, P, 1.0, 8, 64, 1, 8, 0, 0), -1, "null pointer"),
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, 0, 0, 1.0, 8, 64, 1, 8, P, 0), -1, "neither g_zq nor g_loss given"),
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, P, P, 1.0, 0, 64, 1, 8, P, 0), -1, "sizes must be positive"),
    ("dvq_vq_backward_nchw_f32", (P, P, P, 0, P, P, 1.0, 8, 64, 1, 0, P, 0), -1, "sizes must be positive"),
    #                           z dtype E codes mask gzq gl coef B  D  HW K  gz stream
    ("dvq_vq_backward_nchw_x16", (P, 0, P, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "dtype 0"),
    ("dvq_vq_backward_nchw_x16", (P, 2, P, P, 0, P, P, 1.0, 8, 72, 1, 8, P, 0), -2, "D=72 must be a multiple of 16"),
    ("dvq_vq_backward_nchw_x16", (P, 2, 8, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "codebook must be 16-byte aligned"),
    ("dvq_vq_backward_nchw_x16", (1, 1, P, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "must be 2-byte aligned"),
    ("dvq_vq_backward_nchw_x16", (P, 1, P, P, 0, P, P, 1.0, 8, 64, 1, 8, 1, 0), -1, "must be 2-byte aligned"),
    ("dvq_vq_backward_nchw_x16", (0, 1, P, P, 0, P, P, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    #                                    z  E  codes mask gl coef B  D  HW  K    gw stream
    ("dvq_vq_backward_codebook_nchw_f32", (P, P, P, 0, P, 1.0, 8, 64, 1, 8193, P, 0), -2, "K=8193 > 8192"),
    ("dvq_vq_backward_codebook_nchw_f32", (0, P, P, 0, P, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    ("dvq_vq_backward_codebook_nchw_f32", (P, P, P, 0, 0, 1.0, 8, 64, 1, 8, P, 0), -1, "null pointer"),
    ("dvq_vq_backward_codebook_nchw_f32", (P, P, P, 0, P, 1.0, 8, 64, 1, 8, 0, 0), -1, "null pointer"),
    ("dvq_vq_backward_codebook_nchw_f32", (P, P, P, 0, P, 1.0, 8, 0, 1, 8, P, 0), -1, "sizes must be positive"),
    #                              z  codes B  D  HW K  cs vs stream
    ("dvq_ema_accumulate_nchw_f32", (0, P, 8, 64, 1, 8, P, P, 0), -1, "null pointer"),
    ("dvq_ema_accumulate_nchw_f32", (P, 0, 8, 64, 1, 8, P, P, 0), -1, "null pointer"),
    ("dvq_ema_accumulate_nchw_f32", (P, P, 8, 64, 1, 8, 0, P, 0), -1, "null pointer"),
    ("dvq_ema_accumulate_nchw_f32", (P, P, 8, 64, 1, 8, P, 0, 0), -1, "null pointer"),
    ("dvq_ema_accumulate_nchw_f32", (P, P, 0, 64, 1, 8, P, P, 0), -1, "sizes must be positive"),
    ("dvq_ema_accumulate_nchw_f32", (P, P, 8, 64, 1, 0, P, P, 0), -1, "sizes must be positive"),
    ("dvq_ema_accumulate_nchw_x16", (P, 3, P, 8, 64, 1, 8, P, P, 0), -1, "dtype 3"),
    ("dvq_ema_accumulate_nchw_x16", (1, 1, P, 8, 64, 1, 8, P, P, 0), -1, "z must be 2-byte aligned"),
    ("dvq_ema_accumulate_nchw_x16", (0, 2, P, 8, 64, 1, 8, P, P, 0), -1, "null pointer"),
]


@pytest.mark.parametrize("fn,args,rc,words", _REFUSALS, ids=["%s-%d" % (r[0][4:], i) for i, r in enumerate(_REFUSALS)])
def test_row_major_form_refuses_with_the_documented_code(fn, args, rc, words):
    """the row-major form (HW = 1) of each training entry point: a width that is no multiple of 16, a base off its alignment, K over
    the limit, sizes that are not positive and null required pointers return the status include/dvq.h documents, with a message that
    names the entry point, before anything is launched (the pointers are fake: a call that got through would come back as DVQ_EHIP
    or fault).  z / g_zq / g_z off 16 bytes are no refusal for the float32 backward: it runs the strided kernel (same bits, tested below)."""
    from dynamicvectorquantization_amd import _lib
    assert getattr(_lib.lib, fn)(*args) == rc
    msg = _lib.lib.dvq_last_error_string().decode()
    assert msg.startswith(fn + ":") and words in msg, msg


def test_row_major_entry_points_are_declared_and_exported():
    """the entry points whose HW = 1 form serves rows are in the header, bound, and in the dynamic symbol table (that a plain-C program
    links every declared symbol is tests/test_abi_and_host.py's check)"""
    from dynamicvectorquantization_amd import _lib
    header = " ".join(open(_lib.HEADER).read().split())
    dynsyms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in HW_ARG:
        assert "DVQ_API int " + n + "(" in header and n in _lib.EXPORTS and hasattr(_lib.checked, n), n
        assert " T " + n + "\n" in dynsyms, n
    assert "HW == 1" in header and "ROW-MAJOR form" in header


def test_channels_last_predicate():
    """channels_last AND not contiguous: C = 1 or H = W = 1 satisfy both predicates and stay on the NCHW path"""
    from dynamicvectorquantization_amd import _lib
    x = torch.randn(2, 64, 5, 3)
    cl = x.to(memory_format=torch.channels_last)
    assert _lib.is_channels_last(cl) and not _lib.is_channels_last(x) and not _lib.is_channels_last(x[:, :, 0])
    rows = _lib.channels_last_rows(cl)
    assert rows.shape == (30, 64) and rows.is_contiguous() and rows.data_ptr() == cl.data_ptr()          # a view of the same bytes
    assert torch.equal(rows, x.permute(0, 2, 3, 1).reshape(30, 64))
    back = _lib.rows_channels_last(rows, cl.shape)
    assert back.data_ptr() == cl.data_ptr() and back.stride() == cl.stride() and torch.equal(back, x)
    for shape in ((2, 1, 5, 3), (2, 64, 1, 1)):
        t = torch.randn(*shape).to(memory_format=torch.channels_last)
        assert t.is_contiguous() and not _lib.is_channels_last(t)
    assert not _lib.is_channels_last(cl[:, :32])                                                        # a channel slice is neither


# ---------------------------------------------------------------------------------------------------------------------------
# 2. backward, bit-exact
# ---------------------------------------------------------------------------------------------------------------------------
NS = (1, 63, 64, 65, 127, 129, 1000)


def _backward_inputs(dev, N, D, K, dt, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    z = torch.randn(N, D, generator=g).to(dev).to(dt)
    gq = torch.randn(N, D, generator=g).to(dev).to(dt)
    E = (0.5 * torch.randn(K, D, generator=g)).to(dev)
    codes = torch.randint(0, K, (N,), generator=g).to(dev)
    codes[0] = -1                                            # codes outside [0, K) at the first and the last token
    codes[N - 1] = K
    mask = torch.where(torch.rand(N, generator=g) < 0.5, 1.0, 0.25).to(dev)
    return z, gq, E, codes, mask


def _backward_flat(_lib, z, E, codes, mask, gq, gl, cs, K):
    """the row-major form: B = N, HW = 1"""
    N, D = z.shape
    gz = torch.full_like(z, float("nan"))
    x16 = _lib.X16.get(z.dtype, 0)
    a = (E.data_ptr(), codes.data_ptr(), _lib.ptr(mask), _lib.ptr(gq), _lib.ptr(gl), float(cs), N, D, 1, K, gz.data_ptr(), _lib.stream_ptr(z.device))
    if x16:
        _lib.checked.dvq_vq_backward_nchw_x16(z.data_ptr(), x16, *a)
    else:
        _lib.checked.dvq_vq_backward_nchw_f32(z.data_ptr(), *a)
    return gz


def _backward_nchw(_lib, z, E, codes, mask, gq, gl, cs, K):
    """the strided form on the transposed data [1, D, N] (B = 1, HW = N) -> back as rows"""
    N, D = z.shape
    zt = z.t().contiguous()
    gqt = None if gq is None else gq.t().contiguous()
    gz = torch.empty_like(zt)
    x16 = _lib.X16.get(z.dtype, 0)
    a = (E.data_ptr(), codes.data_ptr(), _lib.ptr(mask), _lib.ptr(gqt), _lib.ptr(gl), float(cs), 1, D, N, K, gz.data_ptr(), _lib.stream_ptr(z.device))
    if x16:
        _lib.checked.dvq_vq_backward_nchw_x16(zt.data_ptr(), x16, *a)
    else:
        _lib.checked.dvq_vq_backward_nchw_f32(zt.data_ptr(), *a)
    return gz.t().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f16", "bf16"))
@pytest.mark.parametrize("D", (16, 64, 96, 256))
def test_backward_rows_is_the_torch_expression_bit_for_bit(dev, D, dt):
    """g_z = g_zq + (g_loss coef) ((z - E[codes]) m) op by op in float32 (16-bit latents: on the widened inputs, rounded once), and the
    NCHW entry point on the transposed data; codes -1 and K sit at token 0 and token N - 1 and give no loss term"""
    from dynamicvectorquantization_amd import _lib
    gl = torch.tensor([3.0], device=dev)
    for K in (3, 1024):
        for N in NS:
            z, gq, E, codes, mask = _backward_inputs(dev, N, D, K, dt, 9100 + N + D + K)
            cs = 0.25 * (2.0 / z.numel())
            ok = (codes >= 0) & (codes < K)
            e = E[torch.where(ok, codes, 0)]
            c_tok = torch.where(ok, gl * cs, torch.zeros((), device=dev)).reshape(N, 1)      # fl(g_loss coef), 0 for a code out of range
            for m_ in (None, mask):
                for gq_ in (None, gq):
                    got = _backward_flat(_lib, z, E, codes, m_, gq_, gl, cs, K)
                    diff = z.float() - e
                    if m_ is not None:
                        diff = diff * m_.reshape(N, 1)
                    want = ((gq_.float() if gq_ is not None else torch.zeros_like(diff)) + c_tok * diff).to(dt)
                    what = (N, D, K, m_ is not None, gq_ is not None)
                    assert same_bits(got, want), what
                    assert same_bits(got, _backward_nchw(_lib, z, E, codes, m_, gq_, gl, cs, K)), what
                    bad = (gq_ if gq_ is not None else torch.zeros_like(z))[~ok]
                    assert torch.equal(got[~ok], bad), what                                  # no loss term
            if N > 1:                                        # rows one float off 16-byte alignment take the strided kernel: the same bits
                off = lambda t: torch.empty(t.numel() + (2 if t.dtype != torch.float32 else 1), dtype=t.dtype, device=dev)[(2 if t.dtype != torch.float32 else 1):].view(t.shape).copy_(t)
                assert same_bits(_backward_flat(_lib, off(z), E, codes, mask, off(gq), gl, cs, K), _backward_flat(_lib, z, E, codes, mask, gq, gl, cs, K)), (N, D, K)
            # z_q alone was used (no g_loss): the gradient passes through
            got = _lib_call_no_loss(_lib, z, E, codes, gq, K)
            assert same_bits(got, gq), (N, D, K)


def _lib_call_no_loss(_lib, z, E, codes, gq, K):
    return _backward_flat(_lib, z, E, codes, None, gq, None, 1.0, K)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. codebook gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", (16, 64, 96, 256))
def test_codebook_gradient_rows_vs_float64_scatter_add(dev, D):
    """-(g_loss coef) sum over a code's tokens of (z - E[j]) m against a float64 index_add_: 1e-5 of the largest entry; K = 8192 is the
    entry point's limit; accumulates; the padding row stays as it was"""
    from dynamicvectorquantization_amd import _lib
    gl = torch.tensor([1.7], device=dev)
    for K in (3, 1024, 8192):
        for N in NS:
            z, _, E, codes, mask = _backward_inputs(dev, N, D, K, torch.float32, 9300 + N + D + K)
            if N >= 64:
                codes[8:40] = codes[8]                       # a run of equal codes inside one tile: summed before the atomics
            cs = 2.0 / z.numel()
            ok = (codes >= 0) & (codes < K)
            for m_ in (None, mask):
                gw = torch.zeros((K + 1, D), device=dev)
                gw[K] = 0.5
                run = lambda: _lib.checked.dvq_vq_backward_codebook_nchw_f32(
                    z.data_ptr(), E.data_ptr(), codes.data_ptr(), _lib.ptr(m_), gl.data_ptr(), float(cs), N, D, 1, K, gw.data_ptr(),
                    _lib.stream_ptr(dev))
                run()
                diff = z.double()[ok] - E.double()[codes[ok]]
                if m_ is not None:
                    diff = diff * m_.double()[ok].reshape(-1, 1)
                want = torch.zeros((K, D), dtype=torch.float64, device=dev).index_add_(0, codes[ok], -(gl.double() * cs) * diff)
                scale = max(float(want.abs().max()), 1e-30)
                what = (N, D, K, m_ is not None)
                assert float((gw[:K].double() - want).abs().max()) <= 1e-5 * scale, what
                assert torch.equal(gw[K], torch.full((D,), 0.5, device=dev)), what
                run()
                assert float((gw[:K].double() - 2 * want).abs().max()) <= 2e-5 * scale, what


# ---------------------------------------------------------------------------------------------------------------------------
# 4. EMA statistics
# ---------------------------------------------------------------------------------------------------------------------------
def _accumulate(_lib, z, codes, K):
    N, D = z.shape
    buf = torch.full((K * D + K + 64,), 7.0, device=z.device)               # both outputs are OVERWRITTEN; the guard behind them is not
    vs, cs = buf[:K * D].view(K, D), buf[K * D:K * D + K]
    x16 = _lib.X16.get(z.dtype, 0)
    a = (codes.data_ptr(), N, D, 1, K, cs.data_ptr(), vs.data_ptr(), _lib.stream_ptr(z.device))      # B = N, HW = 1
    if x16:
        _lib.checked.dvq_ema_accumulate_nchw_x16(z.data_ptr(), x16, *a)
    else:
        _lib.checked.dvq_ema_accumulate_nchw_f32(z.data_ptr(), *a)
    assert torch.equal(buf[K * D + K:], torch.full((64,), 7.0, device=z.device))
    return cs, vs


def _check_stats(cs, vs, z, codes, K, what):
    ok = (codes >= 0) & (codes < K)
    assert torch.equal(cs, torch.bincount(codes[ok], minlength=K).float()), what                          # exact
    want = torch.zeros((K, z.shape[1]), dtype=torch.float64, device=z.device).index_add_(0, codes[ok], z.double()[ok])
    assert float((vs.double() - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-30), what


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f16", "bf16"))
@pytest.mark.parametrize("D", (16, 96, 256))
def test_ema_statistics_rows_vs_float64(dev, D, dt):
    """counts equal bincount exactly; sums within 1e-5 (max-norm) of a float64 index_add_ of the widened rows; K = 8200 is above the NCHW
    kernel's LDS-table limit (rows combine equal codes at every K); every token on one code; codes outside [0, K) ignored"""
    from dynamicvectorquantization_amd import _lib
    for K in (3, 1024, 8200):
        for N in (1, 63, 64, 65, 1000):
            z, _, _, codes, _ = _backward_inputs(dev, N, D, K, dt, 9500 + N + D + K)                       # codes -1 and K included
            _check_stats(*_accumulate(_lib, z, codes, K), z, codes, K, (N, D, K, "spread"))
            one = torch.full_like(codes, K - 1)
            _check_stats(*_accumulate(_lib, z, one, K), z, one, K, (N, D, K, "one code"))
            out = torch.where(torch.arange(N, device=dev) % 2 == 0, torch.full_like(codes, K + 5), torch.full_like(codes, -3))
            cs, vs = _accumulate(_lib, z, out, K)
            assert not cs.any() and not vs.any(), (N, D, K, "all out of range")


@pytest.mark.gpu
@pytest.mark.parametrize("D,K", ((16, 1000), (48, 4096)))
def test_ema_statistics_rows_sorted_form(dev, D, K):
    """N >= 65536 float32 tokens, K <= 4096, D % 16 == 0 select the big sorted tile (ema_update.hip) in its row-major form: a token
    count that is no multiple of the 2048-token tile, spread codes, 10 % and all of the tokens on one code (its long-run path),
    codes out of range; and one float off 16-byte alignment, which takes the 64-token kernel again"""
    from dynamicvectorquantization_amd import _lib
    N = 65536 + 2048 + 37
    z, _, _, codes, _ = _backward_inputs(dev, N, D, K, torch.float32, 9700 + D)
    _check_stats(*_accumulate(_lib, z, codes, K), z, codes, K, (D, K, "spread"))
    skew = codes.clone()
    skew[torch.arange(N, device=dev) % 10 == 3] = 5
    _check_stats(*_accumulate(_lib, z, skew, K), z, skew, K, (D, K, "10 % on one code"))
    one = torch.full_like(codes, K - 1)
    one[0], one[N - 1] = -1, K
    _check_stats(*_accumulate(_lib, z, one, K), z, one, K, (D, K, "one code"))
    off = torch.empty(N * D + 1, device=dev)[1:].view(N, D).copy_(z)
    assert off.data_ptr() % 16 == 4
    _check_stats(*_accumulate(_lib, off, codes, K), off, codes, K, (D, K, "off alignment"))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. modules
# ---------------------------------------------------------------------------------------------------------------------------
STEP = {"dvq_ema_update_f32"}


def _close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), what


def _buffers_close(cb, ref, what):
    for name in ("cluster_size_ema", "embed_ema", "weight"):
        _close(getattr(cb, name), getattr(ref, name), (what, name))


def _trained_like(vq, dev, seed):
    """a codebook spread like the data, EMA counts above the restart threshold"""
    g = torch.Generator().manual_seed(seed)
    K, D = vq.codebook.n_embed, vq.codebook.weight.shape[1]
    with torch.no_grad():
        vq.codebook.weight[:-1].copy_(torch.randn(K, D, generator=g))
        vq.codebook.embed_ema.copy_(vq.codebook.weight[:-1] * 3.0)
        vq.codebook.cluster_size_ema.fill_(3.0)
    return vq.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=("f32", "f16", "bf16"))
def test_vq2_channel_last_trains_through_the_row_kernels(dev, dt, monkeypatch):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    B, H, W, K, D = 2, 16, 16, 64, 64
    rows_mod = _trained_like(VectorQuantize2(K, D, channel_last=True, accept_image_fmap=False, restart_unused_codes=False), dev, 1).train()
    nchw_mod = VectorQuantize2(K, D, accept_image_fmap=True, restart_unused_codes=False).to(dev).train()
    nchw_mod.load_state_dict(rows_mod.state_dict())
    x = torch.randn(B, H, W, D, generator=torch.Generator().manual_seed(2)).to(dev).to(dt)
    xr = x.clone().requires_grad_(True)
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    R = torch.randn(B, H, W, D, generator=torch.Generator().manual_seed(3)).to(dev).to(dt)
    with recording() as names, no_torch_scatter(monkeypatch) as scatter:
        q, loss, (_, _, codes) = rows_mod(xr)
        ((q * R).sum() + 3.0 * loss).backward()
    x16 = dt != torch.float32
    assert {"dvq_ema_accumulate_nchw_x16" if x16 else "dvq_ema_accumulate_nchw_f32",
            "dvq_vq_backward_nchw_x16" if x16 else "dvq_vq_backward_nchw_f32"} | STEP <= set(names), names
    assert not names.strided() and not scatter, (names, scatter)
    qn, lossn, (_, _, codesn) = nchw_mod(xn)
    ((qn * R.permute(0, 3, 1, 2)).sum() + 3.0 * lossn).backward()
    assert torch.equal(codes.reshape(-1), codesn.reshape(-1)) and same_bits(q.detach(), qn.detach().permute(0, 2, 3, 1).contiguous())
    assert xr.grad.shape == xr.shape and xr.grad.dtype == dt and xr.grad.is_contiguous()
    assert same_bits(xr.grad, xn.grad.permute(0, 2, 3, 1).contiguous())
    _buffers_close(rows_mod.codebook, nchw_mod.codebook, dt)


@pytest.mark.gpu
def test_vq_embedding_forward_trains_through_the_row_kernels(dev, monkeypatch):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    K, D, N = 64, 64, 300
    emb = _trained_like(VectorQuantize2(K, D, restart_unused_codes=False), dev, 4).codebook.train()
    ref = copy.deepcopy(emb)
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(5)).to(dev)
    w0 = emb.weight.detach().clone()
    with recording() as names, no_torch_scatter(monkeypatch) as scatter:
        e, idx = emb(x)
    assert {"dvq_ema_accumulate_nchw_f32"} | STEP <= set(names) and not names.strided() and not scatter, (names, scatter)
    assert torch.equal(e, w0[idx])                            # the rows of the weight the search used, not of the updated one
    zn = x.t().contiguous().reshape(1, D, N, 1)               # the same tokens as NCHW latents through the NCHW kernels
    ref._ema_step(zn.reshape(1, D, N).permute(0, 2, 1), idx, nchw=zn)
    _buffers_close(emb, ref, "VQEmbedding")


def _rq(dev, restart, seed):
    from dynamicvectorquantization_amd.rq import RQBottleneck
    rq = RQBottleneck(latent_shape=(8, 8, 64), code_shape=(8, 8, 2), n_embed=64, restart_unused_codes=restart).to(dev).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for cb in rq.codebooks:
            cb.weight[:-1].copy_(torch.randn(64, 64, generator=g))
            cb.embed_ema.copy_(cb.weight[:-1] * 3.0)
            cb.cluster_size_ema.fill_(3.0)
    return rq


@pytest.mark.gpu
def test_rq_bottleneck_trains_through_the_row_kernels(dev, monkeypatch):
    """N = 128 tokens, K = 64, depth 2.  The module has no straight-through assign op: its backward is `dvq_rq_backward_f32`, so of the
    three entry points only the two of the EMA step apply, once per depth.
    Reference: the same module with every codebook on the torch path (bincount, index_add_, the element-wise EMA chain).  Depth 1
    searches the codebook depth 0's update wrote, and the two updates agree to 1e-5 only, so a near tie could send the runs apart;
    the reference therefore CHECKS each depth's buffers against the kernel run's (same residual rows, same codes: asserted) and then
    continues from the kernel run's bits, which makes codes, output and x.grad comparable bit for bit at every depth."""
    x = torch.randn(2, 8, 8, 64, generator=torch.Generator().manual_seed(7)).to(dev)
    rq, ref = _rq(dev, False, 6), _rq(dev, False, 6)
    state = lambda cb: {n: getattr(cb, n).detach().clone() for n in ("cluster_size_ema", "embed_ema", "weight")}
    seen = []                                                 # per depth of the kernel run: (rows, codes, buffers after the step)
    for cb in rq.codebooks:
        def step(vectors, idxs, nchw=None, cb=cb, inner=cb._ema_step):
            inner(vectors, idxs, nchw=nchw)
            seen.append((vectors.detach().clone(), idxs.detach().clone(), state(cb)))
        monkeypatch.setattr(cb, "_ema_step", step)
    xr = x.clone().requires_grad_(True)
    with recording() as names, no_torch_scatter(monkeypatch) as scatter:
        out, loss, codes = rq(xr)
        (out.sum() + 3.0 * loss).backward()
    assert names.count("dvq_ema_accumulate_nchw_f32") == 2 and names.count("dvq_ema_update_f32") == 2, names
    assert "dvq_rq_backward_f32" in names and not names.strided() and not scatter, (names, scatter)
    assert len(seen) == 2
    checked_depths = []
    for i, cb in enumerate(ref.codebooks):
        monkeypatch.setattr(cb, "_kernel_latents", lambda vectors, nchw: None)          # the torch path

        def step(vectors, idxs, nchw=None, cb=cb, i=i, inner=cb._ema_step):
            rows, idx, after = seen[i]
            assert same_bits(vectors.detach(), rows) and torch.equal(idxs, idx), "depth %d: other inputs" % i
            inner(vectors, idxs, nchw=nchw)
            for name, want in after.items():
                _close(want, getattr(cb, name), ("RQ depth %d" % i, name))
            with torch.no_grad():
                for name, want in after.items():
                    getattr(cb, name).copy_(want)
            cb.invalidate_codebook_cache()
            checked_depths.append(i)
        monkeypatch.setattr(cb, "_ema_step", step)
    xt = x.clone().requires_grad_(True)
    with no_torch_scatter(monkeypatch) as scatter:
        out_t, loss_t, codes_t = ref(xt)
        (out_t.sum() + 3.0 * loss_t).backward()
    assert scatter.count("index_add_") == 2 and checked_depths == [0, 1]              # the reference run did take the torch path
    assert torch.equal(codes, codes_t) and same_bits(out.detach(), out_t.detach())
    assert same_bits(xr.grad, xt.grad)


@pytest.mark.gpu
def test_restarted_rows_are_the_picked_tokens(dev):
    """restart_unused_codes=True, a fixed seed: every code whose EMA count fell below 1 restarts from the token the seeded pick names
    (fresh modules: all counts are 0, so all K rows restart).  n < 16 K: the pick is torch.randperm(n)[:K] under torch.manual_seed."""
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    K, D = 64, 64
    x = torch.randn(2, 16, 16, D, generator=torch.Generator().manual_seed(8)).to(dev)        # 512 tokens < 16 K
    for dt in DTYPES:
        vq = VectorQuantize2(K, D, channel_last=True, accept_image_fmap=False, restart_unused_codes=True).to(dev).train()
        torch.manual_seed(1234)
        with recording() as names:
            vq(x.to(dt))
        assert "dvq_ema_update_f32" in names
        torch.manual_seed(1234)
        pick = torch.randperm(512, device=dev)[:K]
        rows = x.to(dt).reshape(-1, D)[pick].float()
        assert torch.equal(vq.codebook.embed_ema, rows), dt
        assert torch.equal(vq.codebook.cluster_size_ema, torch.ones(K, device=dev)), dt
    # residual quantization, depth 0: the picked rows of x itself
    rq = _rq(dev, True, 9)
    for cb in rq.codebooks:
        cb.cluster_size_ema.zero_()
    xr = torch.randn(2, 8, 8, 64, generator=torch.Generator().manual_seed(10)).to(dev)
    torch.manual_seed(4321)
    rq(xr)
    torch.manual_seed(4321)
    pick = torch.randperm(128, device=dev)[:64]
    assert torch.equal(rq.codebooks[0].embed_ema, xr.reshape(128, 64)[pick])


@pytest.mark.gpu
def test_vq2_list_items_train_through_the_row_kernels(dev, monkeypatch):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2List
    K, D = 64, 64
    vq = _trained_like(VectorQuantize2List(K, D, restart_unused_codes=False), dev, 11).train()
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(n, D, generator=g).to(dev).requires_grad_(True) for n in (70, 129)]
    with recording() as names, no_torch_scatter(monkeypatch) as scatter:
        qs, loss, _ = vq(xs)
        (sum(q.sum() for q in qs) + loss).backward()
    assert names.count("dvq_ema_accumulate_nchw_f32") == 2 and names.count("dvq_ema_update_f32") == 2, names
    assert names.count("dvq_vq_backward_nchw_f32") == 2 and not names.strided() and not scatter, (names, scatter)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. channels_last
# ---------------------------------------------------------------------------------------------------------------------------
def _quantizer(kind, K, D, dev):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2
    torch.manual_seed(20)
    if kind == "vq2":
        m = _trained_like(VectorQuantize2(K, D, accept_image_fmap=True, restart_unused_codes=False), dev, 21)
    else:
        m = VectorQuantizer2(K, D, beta=0.25, legacy=False, sane_index_shape=True)
        with torch.no_grad():
            m.embedding.weight.copy_(torch.randn(K, D, generator=torch.Generator().manual_seed(22)))
        m = m.to(dev)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("train", (False, True), ids=("eval", "train"))
@pytest.mark.parametrize("D,dt", ((64, torch.float32), (4, torch.float32), (64, torch.bfloat16), (64, torch.float16)),
                         ids=("D64", "D4narrow", "D64bf16", "D64fp16"))
@pytest.mark.parametrize("kind", ("vq2", "vqgan"))
def test_channels_last_is_served_in_place(dev, kind, D, dt, train):
    """x [2, D, 5, 3] channels_last (HW = 15, odd): codes and z_q bit-equal to the module on x.contiguous(), the loss within 1e-5, z_q
    and x.grad channels_last, only row-major entry points in the trace"""
    K = 32
    x = torch.randn(2, D, 5, 3, generator=torch.Generator().manual_seed(23)).to(dev).to(dt)
    xc = x.to(memory_format=torch.channels_last).requires_grad_(True)
    xn = x.clone().requires_grad_(True)
    assert xc.is_contiguous(memory_format=torch.channels_last) and not xc.is_contiguous() and xn.is_contiguous()
    R = torch.randn(2, D, 5, 3, generator=torch.Generator().manual_seed(24)).to(dev).to(dt)
    mc = _quantizer(kind, K, D, dev).train(train)
    mn = copy.deepcopy(mc)
    with recording() as names:
        qc, lc, (_, _, cc) = mc(xc)
        ((qc * R).sum() + 3.0 * lc).backward()
    qn, ln, (_, _, cn) = mn(xn)
    ((qn * R).sum() + 3.0 * ln).backward()
    assert cc.shape == (2, 5, 3) and torch.equal(cc, cn)
    assert qc.shape == qn.shape and qc.dtype == dt and torch.equal(_bits(qc.detach().contiguous()), _bits(qn.detach()))
    assert abs(float(lc.detach()) - float(ln.detach())) <= 1e-5 * abs(float(ln.detach()))
    assert qc.is_contiguous(memory_format=torch.channels_last) and not qc.is_contiguous()
    g = xc.grad
    assert g.is_contiguous(memory_format=torch.channels_last) and not g.is_contiguous() and g.dtype == dt
    assert torch.equal(_bits(g.contiguous()), _bits(xn.grad))
    assert not names.strided(), names
    x16 = dt != torch.float32
    assign = "dvq_vq_assign_narrow_flat_f32" if D == 4 else "dvq_vq_assign_nchw_x16" if x16 else "dvq_vq_assign_flat_f32"
    assert assign in names, names
    if D % 16 == 0:
        assert ("dvq_vq_backward_nchw_x16" if x16 else "dvq_vq_backward_nchw_f32") in names, names
    if kind == "vqgan" and not x16 and D % 16 == 0:
        assert "dvq_vq_backward_codebook_nchw_f32" in names, names
        gc, gn = mc.embedding.weight.grad.double(), mn.embedding.weight.grad.double()
        assert float((gc - gn).abs().max()) <= 1e-5 * float(gn.abs().max())
    if kind == "vq2" and train:
        assert {"dvq_ema_accumulate_nchw_x16" if x16 else "dvq_ema_accumulate_nchw_f32", "dvq_ema_update_f32"} <= set(names), names
        _buffers_close(mc.codebook, mn.codebook, (kind, D, dt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
def test_channels_last_with_a_codebook_mask(dev, dt):
    """a mask [B, 1, H, W] is [N] in memory: through the channels_last assign, its backward and its EMA step the results are those of
    the module on x.contiguous() with the same mask"""
    K, D = 32, 64
    x = torch.randn(2, D, 5, 3, generator=torch.Generator().manual_seed(26)).to(dev).to(dt)
    mask = torch.where(torch.rand(2, 1, 5, 3, generator=torch.Generator().manual_seed(27)) < 0.5, 1.0, 0.25).to(dev)
    xc = x.to(memory_format=torch.channels_last).requires_grad_(True)
    xn = x.clone().requires_grad_(True)
    R = torch.randn(2, D, 5, 3, generator=torch.Generator().manual_seed(28)).to(dev).to(dt)
    mc = _quantizer("vq2", K, D, dev).train()
    mn = copy.deepcopy(mc)
    with recording() as names:
        qc, lc, (_, _, cc) = mc(xc, codebook_mask=mask)
        ((qc * R).sum() + 3.0 * lc).backward()
    qn, ln, (_, _, cn) = mn(xn, codebook_mask=mask)
    ((qn * R).sum() + 3.0 * ln).backward()
    assert not names.strided(), names
    assert torch.equal(cc, cn) and torch.equal(_bits(qc.detach().contiguous()), _bits(qn.detach()))
    assert abs(float(lc.detach()) - float(ln.detach())) <= 1e-5 * abs(float(ln.detach()))
    assert xc.grad.is_contiguous(memory_format=torch.channels_last) and torch.equal(_bits(xc.grad.contiguous()), _bits(xn.grad))
    _buffers_close(mc.codebook, mn.codebook, ("masked", dt))
    me = _quantizer("vq2", K, D, dev).eval()                  # the mask does enter the loss
    with torch.no_grad():
        lm, lu = me(xc.detach(), codebook_mask=mask)[1], me(xc.detach())[1]
    assert abs(float(lm) - float(lu)) > 1e-3 * abs(float(lu))


@pytest.mark.gpu
def test_channels_last_into_preallocated_outputs(dev):
    """vq_assign(out=...) on a channels_last z: z_q must be a channels_last tensor of z's shape and is written in place, as are codes
    and loss; an NCHW z_q buffer is refused"""
    from dynamicvectorquantization_amd.quantize import vq_assign
    m = _quantizer("vq2", 32, 64, dev).eval()
    E, prep = m.codebook.codes.detach(), m.codebook._prep
    x = torch.randn(2, 64, 5, 3, generator=torch.Generator().manual_seed(29)).to(dev)
    xc = x.to(memory_format=torch.channels_last)
    want = vq_assign(x, E, prep)
    zq = torch.full_like(xc, float("nan"))
    codes = torch.full((2, 5, 3), -7, dtype=torch.int64, device=dev)
    loss = torch.full((2,), float("nan"), device=dev)
    assert zq.is_contiguous(memory_format=torch.channels_last) and not zq.is_contiguous()
    with recording() as names:
        got = vq_assign(xc, E, prep, out=(zq, codes, loss))
    assert got[0] is zq and got[1] is codes and got[2] is loss and not names.strided()
    assert same_bits(zq.contiguous(), want[0]) and torch.equal(codes, want[1])
    assert float((loss - want[2]).abs().max()) <= 1e-5 * float(want[2].abs().max())
    with pytest.raises(ValueError):
        vq_assign(xc, E, prep, out=(torch.empty_like(x), codes, loss))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((2, 64, 1, 1),))
def test_both_predicates_keep_the_nchw_path(dev, shape):
    """H = W = 1: channels_last and contiguous at once -- the tensor is handled as before (C = 1 has no kernel width either way)"""
    from dynamicvectorquantization_amd import _lib
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(25)).to(dev).to(memory_format=torch.channels_last)
    assert t.is_contiguous() and not _lib.is_channels_last(t)
    m = _quantizer("vq2", 32, 64, dev).eval()
    with torch.no_grad():
        q, loss, (_, _, c) = m(t)
        q2, loss2, (_, _, c2) = m(t.clone(memory_format=torch.contiguous_format))
    assert q.shape == t.shape and same_bits(q, q2) and torch.equal(c, c2) and float(loss) == float(loss2)
    one = torch.randn(2, 1, 5, 3).to(dev).to(memory_format=torch.channels_last)
    with pytest.raises(_lib.DvqError):                        # codebook_dim 1: no kernel serves it, in any layout
        _quantizer("vq2", 32, 1, dev).eval()(one)
